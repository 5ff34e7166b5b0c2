"""Rate (env-steps/s) of ground contacts inside the fp64 step kernel (fp64_contacts=True: fmj_step_f64_contacts_kernel of
csrc/fmj_f64_step.inc) on 4096 envs, fmj_step in launches of 100 steps under a ctrl tape:
  salamander33 walking (bench.py's walk_newton model: contacts, limits, Newton x 100, a trot tape) on this path, beside the fp32
    constraint path on a context of the same size;
  centipede(20, 25, contacts=True) walking (a travelling wave on the spine, the legs held down), beside centipede(20, 25) swimming on a
    plain fp64 context - the model only this path can put on the ground.
usage: python scripts/f64_contacts_rates.py [n_envs] [samples] [repeats]

The runs of a model are sampled in turn, ``samples`` times (default 5) after two warm-up passes each (the animal settles on the
ground); the whole measurement is repeated ``repeats`` times (default 3) on fresh contexts.  Printed per model and repeat: the median
rate of each run, its spread (min .. max over the samples), the mean contacts per env at the end and the ratio of the two runs; then
per model the spread of the medians over the repeats."""
import sys

import numpy as np

from f64_rates_common import context, tape_of, centipede_stance, sample, stepping, over_repeats


def salamander_runs(n, chunk):
    import farms_mujoco_amd.model as mm

    def walker():
        m = mm.salamander33(contacts=True, limits=True, spawn_z=0.045)
        m.solver = mm.SOLVERS['newton']; m.solver_iterations = 100
        return m
    m = walker()
    amp, lag = mm.trot_controller_params(m)
    p64, psi = context(m, n, precision='fp64', fp64_contacts=True, fp64_limits=True)
    p32, _ = context(walker(), n)
    tape = tape_of(m, psi, amp, lag, chunk)
    return m, {'fp64 contacts': (p64, tape), 'fp32 constraint path (Newton)': (p32, tape)}


def centipede_runs(n, chunk):
    import farms_mujoco_amd.model as mm
    w, s = mm.centipede(20, 25, contacts=True), mm.centipede(20, 25)
    w.solver = mm.SOLVERS['newton']; w.solver_iterations = 100
    amp, lag = mm.wave_controller_params(w, amplitude=0.1)
    stance = centipede_stance(w)
    pw, psi = context(w, n, precision='fp64', fp64_contacts=True)
    ps, _ = context(s, n, precision='fp64')
    amp_s, lag_s = mm.wave_controller_params(s, amplitude=0.3)
    return w, {'fp64 contacts, walking': (pw, tape_of(w, psi, amp, lag, chunk, stance)), 'fp64, swimming': (ps, tape_of(s, psi, amp_s, lag_s, chunk))}


def rates(name, make_runs, n, samples, chunk=100):
    m, runs = make_runs(n, chunk)
    out = sample(stepping(runs, chunk), n, chunk, samples, warmup=2)      # (the animal settles on the ground)
    for phys, _ in runs.values():
        assert int((phys.data.status & 7).abs().sum()) == 0      # (a full contact list is reported, not an error)
    med = {k: float(np.median(v)) for k, v in out.items()}
    ncon = {k: float(p.data.ncon.float().mean()) for k, (p, _) in runs.items()}
    a, b = list(runs)
    print(f'{name} nbody {m.nbody} nv {m.nv} envs {n}: ' +
          '; '.join(f'{k} {med[k]/1e6:.4f} M env-steps/s ({min(v)/1e6:.4f} .. {max(v)/1e6:.4f}), {ncon[k]:.1f} contacts per env' for k, v in out.items()) +
          f'; {a} / {b} {med[a]/med[b]:.3f}', flush=True)
    return med


if __name__ == '__main__':
    n = int(sys.argv[1]) if len(sys.argv) > 1 else 4096
    samples = int(sys.argv[2]) if len(sys.argv) > 2 else 5
    repeats = int(sys.argv[3]) if len(sys.argv) > 3 else 3
    for name, make_runs in (('salamander33 walking', salamander_runs), ('centipede(20, 25)', centipede_runs)):
        over_repeats(name, lambda: rates(name, make_runs, n, samples), repeats, 4)
