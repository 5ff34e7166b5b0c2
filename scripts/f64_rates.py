"""Rate (env-steps/s) of fmj_step on 4096 envs with the fp32 step kernels and with the fp64 step kernel (csrc/fmj_f64.inc,
BatchedPhysics(precision='fp64')) for salamander33, eel(48) and centipede(20, 25), and the fp64 oracle's rate on 16 threads for the
same models: what the fp64 kernel is measured against.  usage: python scripts/f64_rates.py"""
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


if __name__ == '__main__':
    import farms_mujoco_amd.model as mm
    n = 4096
    for name, make in (('salamander33', mm.salamander33), ('eel(48)', lambda: mm.eel(n_joints=48)), ('centipede(20, 25)', lambda: mm.centipede(20, 25))):
        m = make()
        r32, i32 = device_rate(m, n, 'fp32')
        r64, i64 = device_rate(m, n, 'fp64')
        ro = oracle_rate(m)
        print(f'{name} nbody {m.nbody} nv {m.nv} envs {n}: fp32 {r32/1e6:.2f} M env-steps/s {i32}; fp64 {r64/1e6:.2f} M env-steps/s {i64}; '
              f'fp64 / fp32 {r64/r32:.3f}; fp64 oracle on 16 threads {ro/1e6:.3f} M env-steps/s; fp64 kernel / oracle {r64/ro:.1f}', flush=True)
