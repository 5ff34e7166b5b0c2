"""Rate (env-steps/s) of RK4 inside the fp64 step kernel (fp64_rk4=True: fmj_step_f64_rk4_kernel of csrc/fmj_f64_step.inc) on 4096 envs
of salamander33 and centipede(20, 25), plain (fmj_step in launches of 100 steps) and fused (Simulation(fp64_rk4=True, fp64_fused=True):
fmj_step_fused_f64 in launches of 100 iterations with drag, buoyancy and the wave controller), beside fp64 Euler on contexts of the same
size and, for the salamander (the fp32 RK4 path stops at 64 bodies and dofs), the fp32 RK4 per-iteration path (fmj_step: eight launches
per step).  usage: python scripts/f64_rk4_rates.py [n_envs] [samples] [repeats]

The runs of a model are sampled in turn, ``samples`` times (default 5) after one warm-up pass each; the whole measurement is repeated
``repeats`` times (default 3) on fresh contexts.  Printed per model and repeat: the median rate of each run and its spread (min .. max
over the samples) and the ratios of RK4 to Euler; then per model the spread of the medians over the repeats."""
import sys

import numpy as np

from f64_rates_common import context, sample, over_repeats


def with_integrator(make, name):
    import farms_mujoco_amd.model as mm
    m = make()
    m.integrator = mm.INTEGRATORS[name]
    return m


def plain(m, n, **kw):
    return context(m, n, **kw)[0]


def swim(m, n, iterations, rk4):
    """A swimming Simulation (drag, buoyancy, wave controller) on an fp64 context that fuses, ready for step_fused()."""
    import torch
    import farms_mujoco_amd.model as mm
    from farms_mujoco_amd.control import WaveController
    from farms_mujoco_amd.options import SimulationOptions, ArenaOptions, AnimatOptions, WaterOptions
    from farms_mujoco_amd.simulation.simulation import Simulation
    qpos, qvel, psi = mm.synthetic_batch(m, n, seed=0)
    sim = Simulation.from_sdf(SimulationOptions(timestep=m.timestep, n_iterations=iterations, integrator='RK4' if rk4 else 'Euler'),
                              AnimatOptions.from_model(m), ArenaOptions(water=WaterOptions()), model=m, n_envs=n,
                              controller=WaveController(m, psi, frequency=1.5), buffer_size=100, precision='fp64', fp64_fused=True, fp64_rk4=rk4)
    sim.reset()
    sim.physics.data.qpos[:] = torch.as_tensor(qpos, dtype=torch.float32)
    sim.physics.data.qvel[:] = torch.as_tensor(qvel, dtype=torch.float32)
    sim.physics.forward(disable_actuation=True)
    assert sim.task.fusable()
    return sim


def rates(name, make, n, samples, fp32_rk4, chunk=100):
    total = (samples + 1)*chunk
    euler, rk4 = with_integrator(make, 'euler'), with_integrator(make, 'rk4')
    p_eu, p_rk = plain(euler, n, precision='fp64'), plain(rk4, n, precision='fp64', fp64_rk4=True)
    s_eu, s_rk = swim(euler, n, total, False), swim(rk4, n, total, True)
    assert p_rk.kernel_info()['threads_per_env'] == 128
    runs = {'fp64 Euler': lambda _: p_eu.step(chunk), 'fp64 RK4': lambda _: p_rk.step(chunk),
            'fp64 Euler fused': lambda _: s_eu.step_fused(chunk), 'fp64 RK4 fused': lambda _: s_rk.step_fused(chunk)}
    checked = [p_eu, p_rk, s_eu.physics, s_rk.physics]
    if fp32_rk4:
        p32 = plain(rk4, n, precision='fp32')
        runs['fp32 RK4 (8 launches per step)'] = lambda _: p32.step(chunk)
        checked.append(p32)
    out = sample(runs, n, chunk, samples)
    for phys in checked:
        assert int(phys.data.status.abs().sum()) == 0
    med = {k: float(np.median(v)) for k, v in out.items()}
    print(f'{name} nbody {rk4.nbody} nv {rk4.nv} envs {n}: ' +
          '; '.join(f'{k} {med[k]/1e6:.3f} M env-steps/s ({min(v)/1e6:.3f} .. {max(v)/1e6:.3f})' for k, v in out.items()) +
          f'; RK4 / Euler {med["fp64 RK4"]/med["fp64 Euler"]:.3f}; fused RK4 / fused Euler {med["fp64 RK4 fused"]/med["fp64 Euler fused"]:.3f}' +
          (f'; fp64 RK4 / fp32 RK4 {med["fp64 RK4"]/med["fp32 RK4 (8 launches per step)"]:.3f}' if fp32_rk4 else ''), flush=True)
    return med


if __name__ == '__main__':
    import farms_mujoco_amd.model as mm
    n = int(sys.argv[1]) if len(sys.argv) > 1 else 4096
    samples = int(sys.argv[2]) if len(sys.argv) > 2 else 5
    repeats = int(sys.argv[3]) if len(sys.argv) > 3 else 3
    for name, make, fp32_rk4 in (('salamander33', mm.salamander33, True), ('centipede(20, 25)', lambda: mm.centipede(20, 25), False)):
        over_repeats(name, lambda: rates(name, make, n, samples, fp32_rk4), repeats, 3)
