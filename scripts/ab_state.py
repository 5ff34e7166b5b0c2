"""A/B helper: the state a workload reaches after some fused launches, saved for a bitwise comparison between two builds of the library
(FMJ_SO=<path> python scripts/ab_state.py walk out.npz [launches] [steps per launch]; scripts/ab_state.py --diff a.npz b.npz).
The workloads f64_plain, f64_limits, f64_rk4, f64_contacts and f64_terrain are the five kernel families of the fp64 step (fmj_step under
a sine ctrl tape, the walkers' a trot; FMJ_ENVS envs of eel(48), eel(48) limited to +-0.1, the RK4 salamander, the limited walking salamander, the salamander
on the heightfield)."""
import os
import sys
sys.path.insert(0, os.environ.get('GRAFT_REPO_ROOT', os.path.join(os.path.dirname(os.path.abspath(__file__)), '..')))
import numpy as np

if sys.argv[1] == '--diff':
    a, b = np.load(sys.argv[2]), np.load(sys.argv[3])
    for k in a.files:
        same = np.array_equal(a[k], b[k], equal_nan=True)
        d = np.abs(a[k].astype(np.float64) - b[k].astype(np.float64))
        print(f'{k}: {"bitwise equal" if same else "DIFFERENT"}  max abs diff {np.nanmax(d):.3e}  envs differing {int((d.reshape(d.shape[0], -1) > 0).any(1).sum())} of {d.shape[0]}')
    sys.exit(0)
import torch
import bench
wl, out = sys.argv[1], sys.argv[2]
launches = int(sys.argv[3]) if len(sys.argv) > 3 else 3
L = int(sys.argv[4]) if len(sys.argv) > 4 else 100
n = int(os.environ.get('FMJ_ENVS', '4096'))


def f64_family(wl):
    """The context of one fp64 kernel family on the synthetic batch, and a launch of L steps under a sine ctrl tape."""
    import farms_mujoco_amd.model as mm
    from farms_mujoco_amd.physics import BatchedPhysics
    m, kw = {'f64_plain': lambda: (mm.eel(n_joints=48), {}), 'f64_limits': lambda: (mm.eel(n_joints=48), dict(fp64_limits=True)),
             'f64_rk4': lambda: (mm.salamander33(), dict(fp64_rk4=True)),
             'f64_contacts': lambda: (mm.salamander33(contacts=True, limits=True, spawn_z=0.045), dict(fp64_contacts=True, fp64_limits=True)),
             'f64_terrain': lambda: (mm.salamander33(contacts=True, terrain='hfield'), dict(fp64_contacts=True, fp64_terrain=True))}[wl]()
    if wl == 'f64_limits':
        m.jnt_limited = (m.jnt_type != 0).astype(m.jnt_limited.dtype); m.jnt_range = np.tile([-0.1, 0.1], (m.njnt, 1)).astype(float)
    if wl == 'f64_rk4':
        m.integrator = mm.INTEGRATORS['rk4']
    qpos, qvel, psi = mm.synthetic_batch(m, n, seed=0)
    phys = BatchedPhysics(m, n, precision='fp64', **kw)
    phys.data.qpos[:] = torch.as_tensor(qpos, dtype=torch.float32); phys.data.qvel[:] = torch.as_tensor(qvel, dtype=torch.float32)
    amp, lag = mm.trot_controller_params(m) if 'contacts' in kw else (np.full(m.nu, 0.3), 2*np.pi*np.arange(m.nu)/m.nu)      # (the walkers trot)
    tape = amp[None, None, :]*np.sin(2*np.pi*(1.0 if 'contacts' in kw else 2.0)*np.arange(L)[:, None, None]*m.timestep + psi[None, :, None] - lag[None, None, :])
    tape = torch.as_tensor(tape, dtype=torch.float32, device='cuda:0').contiguous()
    print(wl, phys.kernel_info())
    return phys, lambda: phys.step(L, tape)


if wl.startswith('f64_'):
    phys, launch = f64_family(wl)
else:
    sim, m, _ = bench.build_sim(n, 1 << 30, L, 0, 'cuda:0', wl)
    phys, launch = sim.physics, lambda: sim.step_fused(L)
for _ in range(launches):
    launch()
torch.cuda.synchronize()
d = phys.data
print('envs with a warning bit:', int((d.status != 0).sum()), 'of', n, '; mean contacts per env', float(d.ncon.float().mean()))
np.savez(out, **{k: getattr(d, k).cpu().numpy() for k in ('qpos', 'qvel', 'sensordata', 'contact', 'ncon')})
print('saved', out)
