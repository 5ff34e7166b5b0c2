"""Rate (env-steps/s) of the fp64 contact solve under the elliptic cone (fp64_contacts=True, fp64_elliptic=True:
fmj_step_f64_elliptic_kernel of csrc/fmj_f64_step.inc) on 4096 envs, fmj_step in launches of 100 steps under a ctrl tape.  The walking
centipede(20, 25) on its plane (a travelling wave on the spine, the legs held down: the tape of scripts/f64_contacts_rates.py):
  under the pyramidal cone through the contacts kernel (fp64_contacts=True alone);
  under the elliptic cone through the elliptic kernel;
  under the elliptic cone with friction 0 on every geom (1e-5 after the clamp) - the feet the pyramid refuses.
usage: python scripts/f64_elliptic_rates.py [n_envs] [samples] [repeats]

The three runs are sampled in turn, ``samples`` times (default 5) after two warm-up passes each (the animal settles on the ground);
the whole measurement is repeated ``repeats`` times (default 3) on fresh contexts.  Printed per repeat: the median rate of each run,
its spread (min .. max over the samples), the mean contacts per env at the end and each run's ratio to the first; then the spread of
the medians over the repeats."""
import sys

import numpy as np

from f64_rates_common import context, tape_of, centipede_stance, sample, stepping, over_repeats


def centipede_runs(n, chunk):
    import farms_mujoco_amd.model as mm

    def walker(cone, friction0=False):
        w = mm.centipede(20, 25, contacts=True)
        w.solver = mm.SOLVERS['newton']; w.solver_iterations = 100
        w.cone = mm.CONES[cone]
        if friction0:
            w.geom_friction = np.zeros_like(w.geom_friction)
        return w
    w = walker('pyramidal')
    amp, lag = mm.wave_controller_params(w, amplitude=0.1)
    stance = centipede_stance(w)
    runs = {}
    for key, cone, friction0 in (('pyramidal, contacts kernel', 'pyramidal', False), ('elliptic, elliptic kernel', 'elliptic', False),
                                 ('elliptic, friction 0', 'elliptic', True)):
        p, psi = context(walker(cone, friction0), n, precision='fp64', fp64_contacts=True, fp64_elliptic=cone == 'elliptic')
        assert p.kernel_info()['fp64_step_kernel'] == ('fmj_step_f64_elliptic_kernel' if cone == 'elliptic' else 'fmj_step_f64_contacts_kernel')
        runs[key] = (p, tape_of(w, psi, amp, lag, chunk, stance))
    return w, runs


def rates(name, n, samples, chunk=100):
    m, runs = centipede_runs(n, chunk)
    out = sample(stepping(runs, chunk), n, chunk, samples, warmup=2)      # (the animal settles on the ground)
    for phys, _ in runs.values():
        assert int((phys.data.status & 7).abs().sum()) == 0      # (a full contact list is reported, not an error)
    med = {k: float(np.median(v)) for k, v in out.items()}
    ncon = {k: float(p.data.ncon.float().mean()) for k, (p, _) in runs.items()}
    first = list(runs)[0]
    print(f'{name} nbody {m.nbody} nv {m.nv} envs {n}: ' +
          '; '.join(f'{k} {med[k]/1e6:.4f} M env-steps/s ({min(v)/1e6:.4f} .. {max(v)/1e6:.4f}), {ncon[k]:.1f} contacts per env, '
                    f'{med[k]/med[first]:.3f} of the first' for k, v in out.items()), flush=True)
    return med


if __name__ == '__main__':
    n = int(sys.argv[1]) if len(sys.argv) > 1 else 4096
    samples = int(sys.argv[2]) if len(sys.argv) > 2 else 5
    repeats = int(sys.argv[3]) if len(sys.argv) > 3 else 3
    over_repeats('centipede(20, 25) walking', lambda: rates('centipede(20, 25) walking', n, samples), repeats, 4)
