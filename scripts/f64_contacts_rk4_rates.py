"""Rate (env-steps/s) of RK4 inside the fp64 contact solve (fp64_contacts=True, fp64_contacts_rk4=True: fmj_step_f64_terrain_rk4_kernel of
csrc/fmj_f64_step.inc) on 4096 envs, fmj_step in launches of 100 steps under a ctrl tape, beside the same model integrating with Euler
on contexts of the same size: on the terrain kernels (fmj_step_f64_terrain_kernel, fp64_terrain=True: the text the RK4 kernels are built
from, so the ratio is the cost of the four passes) and on the flat-ground contact kernels (fmj_step_f64_contacts_kernel: what a user
of planes runs today):
  salamander33 walking (bench.py's walk_newton model: contacts, limits, Newton x 100, a trot tape);
  centipede(20, 25, contacts=True) walking (a travelling wave on the spine, the legs held down) at a timestep of 0.25 ms, both
    integrators: at the model's 1 ms explicit RK4, which has no implicit damping, diverges on this animal within 100 steps - in the fp64
    oracle as on the device, whose envs then freeze - while Euler is stable; at 0.5 ms and below RK4 is stable too.
usage: python scripts/f64_contacts_rk4_rates.py [n_envs] [samples] [repeats]

The runs of a model are sampled in turn, ``samples`` times (default 5) after two warm-up passes each (the animal settles on the
ground); the whole measurement is repeated ``repeats`` times (default 3) on fresh contexts.  Printed per model and repeat: the median
rate of each run, its spread (min .. max over the samples), the mean contacts per env at the end and the ratios RK4 / Euler; then per
model the spread of the medians over the repeats."""
import sys

import numpy as np

from f64_rates_common import context, tape_of, centipede_stance, sample, stepping, over_repeats


def _pair(make, n, chunk, tape_args, **kw):
    """The RK4 model on the new kernels and its Euler twin on the terrain and on the contact kernels, under one tape.  ``tape_args``:
    amplitude, phase lag and ctrl offset (or None) of the model's tape."""
    import farms_mujoco_amd.model as mm
    rk, eu, eu_t = make(), make(), make()
    rk.integrator = mm.INTEGRATORS['rk4']
    p_rk, psi = context(rk, n, precision='fp64', fp64_contacts=True, fp64_contacts_rk4=True, **kw)
    p_eu, _ = context(eu, n, precision='fp64', fp64_contacts=True, **kw)
    p_eu_t, _ = context(eu_t, n, precision='fp64', fp64_contacts=True, fp64_terrain=True, **kw)
    assert p_rk.kernel_info()['fp64_step_kernel'] == 'fmj_step_f64_terrain_rk4_kernel' and p_eu.kernel_info()['fp64_step_kernel'] == 'fmj_step_f64_contacts_kernel'
    assert p_eu_t.kernel_info()['fp64_step_kernel'] == 'fmj_step_f64_terrain_kernel'
    amp, lag, offset = tape_args(rk)
    tape = tape_of(rk, psi, amp, lag, chunk, offset)
    return rk, {'RK4': (p_rk, tape), 'Euler, terrain kernels': (p_eu_t, tape), 'Euler, contact kernels': (p_eu, tape)}


def salamander_runs(n, chunk):
    import farms_mujoco_amd.model as mm

    def walker():
        m = mm.salamander33(contacts=True, limits=True, spawn_z=0.045)
        m.solver = mm.SOLVERS['newton']; m.solver_iterations = 100
        return m
    return _pair(walker, n, chunk, lambda m: (*mm.trot_controller_params(m), None), fp64_limits=True)


CENTIPEDE_TIMESTEP = 2.5e-4      # (see the module's text)


def centipede_runs(n, chunk):
    import farms_mujoco_amd.model as mm

    def walker():
        w = mm.centipede(20, 25, contacts=True, timestep=CENTIPEDE_TIMESTEP)
        w.solver = mm.SOLVERS['newton']; w.solver_iterations = 100
        return w
    return _pair(walker, n, chunk, lambda w: (*mm.wave_controller_params(w, amplitude=0.1), centipede_stance(w)))


def rates(name, make_runs, n, samples, chunk=100):
    m, runs = make_runs(n, chunk)
    out = sample(stepping(runs, chunk), n, chunk, samples, warmup=2)      # (the animal settles on the ground)
    for phys, _ in runs.values():
        assert int((phys.data.status & 7).abs().sum()) == 0      # (a full contact list is reported, not an error)
    med = {k: float(np.median(v)) for k, v in out.items()}
    ncon = {k: float(p.data.ncon.float().mean()) for k, (p, _) in runs.items()}
    a, b, c = list(runs)
    print(f'{name} nbody {m.nbody} nv {m.nv} envs {n}: ' +
          '; '.join(f'{k} {med[k]/1e6:.4f} M env-steps/s ({min(v)/1e6:.4f} .. {max(v)/1e6:.4f}), {ncon[k]:.1f} contacts per env' for k, v in out.items()) +
          f'; {a} / {b} {med[a]/med[b]:.3f}; {a} / {c} {med[a]/med[c]:.3f}', flush=True)
    return med


if __name__ == '__main__':
    n = int(sys.argv[1]) if len(sys.argv) > 1 else 4096
    samples = int(sys.argv[2]) if len(sys.argv) > 2 else 5
    repeats = int(sys.argv[3]) if len(sys.argv) > 3 else 3
    for name, make_runs in (('salamander33 walking', salamander_runs), ('centipede(20, 25) walking', centipede_runs)):
        over_repeats(name, lambda: rates(name, make_runs, n, samples), repeats, 4)
