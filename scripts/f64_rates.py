"""Rate (env-steps/s) of fmj_step on 4096 envs with the fp32 step kernels and with the fp64 step kernel (csrc/fmj_f64.inc,
BatchedPhysics(precision='fp64')) for salamander33, eel(48) and centipede(20, 25), and the fp64 oracle's rate on 16 threads for the
same models: what the fp64 kernel is measured against.  usage: python scripts/f64_rates.py

python scripts/f64_rates.py fused [samples]: the fused fp64 launch (Simulation(precision='fp64', fp64_fused=True).run() in chunks of
100) against the per-iteration path of the default fp64 simulation and against plain fmj_step(100), for eel(48) and centipede(20, 25)
at 64, 512 and 4096 envs (the per-iteration path as run() steps it, without its status checks).  The three are sampled in turn, ``samples`` times (default 5) after one warm-up pass each; printed per
configuration: the median rate of each and its spread (min .. max over the samples), in env-steps/s."""
import os
import sys
import time

import numpy as np

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), '..')
sys.path.insert(0, ROOT)


def device_rate(m, n, precision, steps=100, launches=5):
    import torch
    import farms_mujoco_amd.model as mm
    from farms_mujoco_amd.physics import BatchedPhysics
    qpos, qvel, _ = mm.synthetic_batch(m, n, seed=0)
    phys = BatchedPhysics(m, n, precision=precision)
    phys.data.qpos[:] = torch.as_tensor(qpos, dtype=torch.float32)
    phys.data.qvel[:] = torch.as_tensor(qvel, dtype=torch.float32)
    phys.step(steps)
    torch.cuda.synchronize(); t0 = time.time()
    for _ in range(launches):
        phys.step(steps)
    torch.cuda.synchronize(); dt = time.time() - t0
    assert int(phys.data.status.abs().sum()) == 0
    return n*steps*launches/dt, phys.kernel_info()


def oracle_rate(m, n=256, steps=20, threads=16):
    import farms_mujoco_amd.model as mm
    from oracle import oracle
    oracle.build()
    qpos, qvel, _ = mm.synthetic_batch(m, n, seed=0)
    q = qpos.astype(np.float32).astype(np.float64); v = qvel.astype(np.float32).astype(np.float64)
    oracle.step(m, q, v, n_steps=1, n_threads=threads)
    t0 = time.time()
    oracle.step(m, q, v, n_steps=steps, n_threads=threads)
    return n*steps/(time.time() - t0)


def swim_run(m, n, fused, iterations):
    """A swimming Simulation of ``iterations`` iterations (drag, buoyancy, wave controller) on an fp64 context, ready to run()."""
    import torch
    import farms_mujoco_amd.model as mm
    from farms_mujoco_amd.control import WaveController
    from farms_mujoco_amd.options import SimulationOptions, ArenaOptions, AnimatOptions, WaterOptions
    from farms_mujoco_amd.simulation.simulation import Simulation
    qpos, qvel, psi = mm.synthetic_batch(m, n, seed=0)
    sim = Simulation.from_sdf(SimulationOptions(timestep=m.timestep, n_iterations=iterations), AnimatOptions.from_model(m),
                              ArenaOptions(water=WaterOptions()), model=m, n_envs=n, controller=WaveController(m, psi, frequency=1.5),
                              buffer_size=100, precision='fp64', fp64_fused=fused)
    sim.reset()
    sim.physics.data.qpos[:] = torch.as_tensor(qpos, dtype=torch.float32)
    sim.physics.data.qvel[:] = torch.as_tensor(qvel, dtype=torch.float32)
    sim.physics.forward(disable_actuation=True)
    return sim


def fused_rates(samples=5, chunk=100):
    import torch
    import farms_mujoco_amd.model as mm
    from farms_mujoco_amd.physics import BatchedPhysics
    for name, make in (('eel(48)', lambda: mm.eel(n_joints=48)), ('centipede(20, 25)', lambda: mm.centipede(20, 25))):
        for n in (64, 512, 4096):
            m = make()
            total = (samples + 1)*chunk
            fused, host = swim_run(m, n, True, total), swim_run(m, n, False, total)
            assert fused.task.fusable() and not host.task.fusable()
            phys = BatchedPhysics(m, n, precision='fp64')
            phys.data.qpos[:] = host.physics.data.qpos

            def advance(sim):      # the next `chunk` iterations of the run, as run() takes them
                if sim.task.fusable():
                    sim.step_fused(chunk)
                else:
                    for _ in range(chunk):
                        sim._env_step()
            runs = {'fused': lambda: advance(fused), 'per-iteration': lambda: advance(host), 'fmj_step': lambda: phys.step(chunk)}
            rates = {k: [] for k in runs}
            for s in range(samples + 1):      # alternating samples; the first pass warms up
                for k, go in runs.items():
                    torch.cuda.synchronize(); t0 = time.perf_counter()
                    go()
                    torch.cuda.synchronize(); dt = time.perf_counter() - t0
                    if s:
                        rates[k].append(n*chunk/dt)
            for sim in (fused, host):
                assert int(sim.physics.data.status.abs().sum()) == 0
            med = {k: float(np.median(v)) for k, v in rates.items()}
            print(f'{name} envs {n}: ' + '; '.join(f'{k} {med[k]/1e6:.3f} M env-steps/s ({min(v)/1e6:.3f} .. {max(v)/1e6:.3f})' for k, v in rates.items()) +
                  f'; fused / per-iteration {med["fused"]/med["per-iteration"]:.2f}; fused / fmj_step {med["fused"]/med["fmj_step"]:.3f}', flush=True)


if __name__ == '__main__':
    import farms_mujoco_amd.model as mm
    if len(sys.argv) > 1 and sys.argv[1] == 'fused':
        fused_rates(int(sys.argv[2]) if len(sys.argv) > 2 else 5)
        sys.exit(0)
    n = 4096
    for name, make in (('salamander33', mm.salamander33), ('eel(48)', lambda: mm.eel(n_joints=48)), ('centipede(20, 25)', lambda: mm.centipede(20, 25))):
        m = make()
        r32, i32 = device_rate(m, n, 'fp32')
        r64, i64 = device_rate(m, n, 'fp64')
        ro = oracle_rate(m)
        print(f'{name} nbody {m.nbody} nv {m.nv} envs {n}: fp32 {r32/1e6:.2f} M env-steps/s {i32}; fp64 {r64/1e6:.2f} M env-steps/s {i64}; '
              f'fp64 / fp32 {r64/r32:.3f}; fp64 oracle on 16 threads {ro/1e6:.3f} M env-steps/s; fp64 kernel / oracle {r64/ro:.1f}', flush=True)
