"""What the fp64 rate scripts (f64_limits_rates.py, f64_rk4_rates.py, f64_contacts_rates.py, f64_terrain_rates.py,
f64_elliptic_rates.py, f64_mesh_rates.py, f64_contacts_rk4_rates.py) share: a context on
the synthetic batch, a sine ctrl tape, the walking centipede's stance, the alternating-sample loop and the line of medians over repeats."""
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), '..'))


def context(m, n, **kw):
    import torch
    import farms_mujoco_amd.model as mm
    from farms_mujoco_amd.physics import BatchedPhysics
    qpos, qvel, psi = mm.synthetic_batch(m, n, seed=0)
    phys = BatchedPhysics(m, n, **kw)
    phys.data.qpos[:] = torch.as_tensor(qpos, dtype=torch.float32)
    phys.data.qvel[:] = torch.as_tensor(qvel, dtype=torch.float32)
    return phys, psi


def tape_of(m, psi, amp, lag, chunk, offset=None, f=1.0):
    """ctrl[t, env, a] = offset_a + amp_a sin(2 pi f t + psi_env - lag_a) over one launch (the same tape every launch)."""
    import torch
    t = np.arange(chunk)[:, None, None]*m.timestep
    tape = amp[None, None, :]*np.sin(2*np.pi*f*t + psi[None, :, None] - lag[None, None, :])
    if offset is not None:
        tape = tape + offset[None, None, :]
    return torch.as_tensor(tape, dtype=torch.float32, device='cuda:0').contiguous()


def centipede_stance(w):
    """ctrl offsets that hold the walking centipede's legs down."""
    stance = np.zeros(w.nu)
    for a in range(w.nu):
        name = w.joint_names[int(w.actuator_jntid[a])]
        if name.startswith('joint_leg_') and name.endswith('_1'):
            stance[a] = -0.25 if '_L_' in name else 0.25
    return stance


def sample(runs, n, chunk, samples, warmup=1, pass_input=None, each_pass=None):
    """``runs``: {name: go(x)}, each a launch of ``chunk`` steps on ``n`` envs.  They are sampled in turn, ``samples`` times after
    ``warmup`` passes; x is ``pass_input(s)`` of the pass, made before its runs are timed (None without one); ``each_pass(s)`` runs
    after every pass.  Returns {name: [env-steps/s per sample]}."""
    import torch
    out = {k: [] for k in runs}
    for s in range(samples + warmup):
        x = pass_input(s) if pass_input else None
        for k, go in runs.items():
            torch.cuda.synchronize(); t0 = time.perf_counter()
            go(x)
            torch.cuda.synchronize(); dt = time.perf_counter() - t0
            if s >= warmup:
                out[k].append(n*chunk/dt)
        if each_pass:
            each_pass(s)
    return out


def stepping(runs, chunk):
    """{name: (phys, tape)} as ``sample`` takes it: every pass steps the context under its tape."""
    return {k: (lambda _, p=p, tape=tape: p.step(chunk, tape)) for k, (p, tape) in runs.items()}


def over_repeats(name, measure, repeats, digits):
    meds = [measure() for _ in range(repeats)]
    print(f'{name}: medians over {repeats} runs: ' +
          '; '.join(f'{k} {min(m[k] for m in meds)/1e6:.{digits}f} .. {max(m[k] for m in meds)/1e6:.{digits}f}' for k in meds[0]), flush=True)
