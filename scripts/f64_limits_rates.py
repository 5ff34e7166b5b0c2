"""Rate (env-steps/s) of fmj_step on an fp64 context for eel(48) and centipede(20, 25) in three settings: without limits
(BatchedPhysics(precision='fp64'), the unconstrained instantiation of csrc/fmj_f64.inc), with limits that never engage (every joint
limited to +-10 under fp64_limits=True: the LIMITS instantiation, whose every step takes the no-candidate branch) and with limits
engaged (every joint limited to +-0.1, margin 0.01 on the even joints: most steps run the Newton solve).  All three start from rest
and step under the same ctrl tape, 0.3 sin(2 pi 2 Hz t + 0.7 env - 2 pi a / nu), in launches of 100 steps.
usage: python scripts/f64_limits_rates.py [n_envs] [samples]

The three are sampled in turn, ``samples`` times (default 5) after one warm-up pass each; printed per model: the median rate of each
and its spread (min .. max over the samples), the share of the engaged run's env-steps that ended with a limit force, and the two
ratios to the rate without limits."""
import sys

import numpy as np

from f64_rates_common import sample


def limited(make, lim, margin_even):
    m = make()
    m.jnt_limited = (m.jnt_type != 0).astype(m.jnt_limited.dtype)
    m.jnt_range = np.tile([-lim, lim], (m.njnt, 1)).astype(float)
    margin = np.zeros(m.njnt); margin[::2] = margin_even
    m.jnt_margin = margin
    return m


def tape(m, n, step0, steps, device):
    import torch
    t = (step0 + torch.arange(steps, device=device, dtype=torch.float64))[:, None, None]*m.timestep
    env = torch.arange(n, device=device, dtype=torch.float64)[None, :, None]
    a = torch.arange(m.nu, device=device, dtype=torch.float64)[None, None, :]
    return (0.3*torch.sin(2*np.pi*2.0*t + 0.7*env - 2*np.pi*a/m.nu)).to(torch.float32).contiguous()


def rates(name, make, n, samples, chunk=100):
    import torch
    from farms_mujoco_amd.physics import BatchedPhysics
    runs = {'no limits': BatchedPhysics(make(), n, precision='fp64'),
            'limits, never engaged': BatchedPhysics(limited(make, 10.0, 0.0), n, precision='fp64', fp64_limits=True),
            'limits engaged': BatchedPhysics(limited(make, 0.1, 0.01), n, precision='fp64', fp64_limits=True)}
    m = runs['no limits'].model
    engaged = []
    nl, njs = 6*(m.nbody - 1), m.n_sensor_joints
    out = sample({k: (lambda ctrl, p=p: p.step(chunk, ctrl)) for k, p in runs.items()}, n, chunk, samples,
                 pass_input=lambda s: tape(m, n, s*chunk, chunk, runs['no limits'].device),
                 each_pass=lambda s: engaged.append(float((runs['limits engaged'].data.sensordata[:, nl + 2:nl + 3*njs:3] != 0).any(dim=1).float().mean())))
    for phys in runs.values():
        assert int(phys.data.status.abs().sum()) == 0
    assert float(runs['limits, never engaged'].data.sensordata[:, nl + 2:nl + 3*njs:3].abs().max()) == 0
    assert torch.equal(runs['no limits'].data.qpos, runs['limits, never engaged'].data.qpos)      # the same steps, bit for bit
    med = {k: float(np.median(v)) for k, v in out.items()}
    print(f'{name} nbody {m.nbody} nv {m.nv} envs {n}: ' +
          '; '.join(f'{k} {med[k]/1e6:.3f} M env-steps/s ({min(v)/1e6:.3f} .. {max(v)/1e6:.3f})' for k, v in out.items()) +
          f'; envs with a limit force where a launch ends {min(engaged[1:]):.2f} .. {max(engaged[1:]):.2f}' +
          f'; never engaged / no limits {med["limits, never engaged"]/med["no limits"]:.3f}; engaged / no limits {med["limits engaged"]/med["no limits"]:.3f}',
          flush=True)


if __name__ == '__main__':
    import farms_mujoco_amd.model as mm
    n = int(sys.argv[1]) if len(sys.argv) > 1 else 4096
    samples = int(sys.argv[2]) if len(sys.argv) > 2 else 5
    for name, make in (('eel(48)', lambda: mm.eel(n_joints=48)), ('centipede(20, 25)', lambda: mm.centipede(20, 25))):
        rates(name, make, n, samples)
