"""Fused swimming rate (env-steps/s) of the two-wave step kernel (csrc/fmj_wide.inc): centipede(20, 25) (107 bodies, nv 111) at 2048 and
4096 envs, and centipede() (nv 61) on its one-wave kernel against the same model under FMJ_WIDE=1 (what the second wave costs).
Each case runs in a fresh process (FMJ_WIDE is read at fmj_create).  usage: python scripts/wide_rates.py"""
import os
import subprocess
import sys
import time

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), '..')


def one(shape, n):
    sys.path.insert(0, ROOT)
    import torch
    import farms_mujoco_amd.model as mm
    from farms_mujoco_amd.options import SimulationOptions, ArenaOptions, AnimatOptions, WaterOptions
    from farms_mujoco_amd.control import WaveController
    from farms_mujoco_amd.simulation.simulation import Simulation
    m = mm.centipede(*shape)
    qpos, qvel, psi = mm.synthetic_batch(m, n, seed=0)
    T, ring = 1500, 100
    sim = Simulation.from_sdf(SimulationOptions(timestep=m.timestep, n_iterations=T), AnimatOptions.from_model(m),
                              ArenaOptions(water=WaterOptions(height=0.0)), model=m, n_envs=n,
                              controller=WaveController(m, psi, frequency=1.5), buffer_size=ring)
    sim.reset()
    sim.physics.data.qpos[:] = torch.as_tensor(qpos, dtype=torch.float32)
    sim.physics.data.qvel[:] = torch.as_tensor(qvel, dtype=torch.float32)
    sim.physics.forward(disable_actuation=True)
    for _ in range(3):
        sim.step_fused(ring)
    torch.cuda.synchronize(); t0 = time.time()
    for _ in range(10):
        sim.step_fused(ring)
    torch.cuda.synchronize(); dt = time.time() - t0
    assert int(sim.physics.data.status.abs().sum()) == 0
    print(f'centipede{shape} nbody {m.nbody} nv {m.nv} envs {n} FMJ_WIDE={os.environ.get("FMJ_WIDE", "-")}: '
          f'{n*10*ring/dt/1e6:.2f} M env-steps/s {sim.physics.kernel_info()}', flush=True)


if __name__ == '__main__':
    if len(sys.argv) > 1:
        a, b, n = (int(x) for x in sys.argv[1:4])
        one((a, b), n)
        sys.exit(0)
    cases = [((20, 25), 2048, None), ((20, 25), 4096, None), ((10, 15), 2048, None), ((10, 15), 2048, '1')]
    for shape, n, wide in cases:
        env = dict(os.environ)
        env.pop('FMJ_WIDE', None)
        if wide:
            env['FMJ_WIDE'] = wide
        subprocess.run([sys.executable, os.path.abspath(__file__), str(shape[0]), str(shape[1]), str(n)], env=env, check=True, timeout=600)
