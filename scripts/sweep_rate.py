"""Rate (env-steps/s) of a gait sweep: 4096 x salamander33, fused launches of 1000 steps, in four configurations run alternately on
one box (each run a fresh process, as scripts/ab.sh does):
  a  shared wave parameters, the lean build of the two-env kernel (the headline)
  b  shared wave parameters, FMJ_DUAL_LEAN=0 (the generic build)
  c  per-env frequency, amplitude and phase lag (fmj_step_fused_ex: the generic build reads the env's rows)
  d  the same sweep through a ctrl tape [n_steps, n_envs, nu] built by torch kernels (controller = 0): the only route before
With csrc/libfmj_hip_base.so present (scripts/build_base.sh <rev>) a and b are also run on that build (base_a, base_b): the
yardstick for b is the base's generic build, for a the base's lean build.
usage: python scripts/sweep_rate.py [REPS]          (one run: python scripts/sweep_rate.py --config c)"""
import json
import math
import os
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), '..')
sys.path.insert(0, ROOT)
N, STEPS, LAUNCHES = 4096, 1000, 4
BASE_SO = os.path.join(ROOT, 'farms_mujoco_amd', 'csrc', 'libfmj_hip_base.so')


def sweep(m, n, seed=0):
    rng = np.random.default_rng(seed)
    pos = np.array([t == 'position' for t in m.actuator_tags[:m.nu]])
    axial = np.array([m.joint_names[m.actuator_jntid[a]].startswith('joint_body_') for a in range(m.nu)])
    return (rng.uniform(0.5, 2.0, n), rng.uniform(0.1, 0.4, (n, m.nu))*(pos & axial), rng.uniform(-2*np.pi, 2*np.pi, (n, m.nu))*(pos & axial))


def run_one(config):
    import torch
    import bench
    from farms_mujoco_amd.control import WaveController
    sim, m, (_, _, psi) = bench.build_sim(N, STEPS*(LAUNCHES + 1), STEPS, 0, 'cuda:0')
    if config in ('c', 'd'):
        freq, amp, lag = sweep(m, N)
        wave = ctl = WaveController(m, psi, frequency=freq, amplitude_env=amp, phase_lag_env=lag)
        if config == 'd':
            class TapeSweep:      # what a user had to write: the sweep's commands for a whole launch, evaluated by torch
                fusable, tape, joints_names, it = True, True, wave.joints_names, 0

                def ctrl_tape(self, n_steps):
                    t = (self.it + torch.arange(n_steps, device='cuda:0', dtype=torch.float64))*m.timestep
                    cyc = torch.remainder(wave.frequency.to(torch.float64)[None, :]*t[:, None], 1.0).to(torch.float32)
                    arg = (2*math.pi*cyc + wave.env_phase[None, :])[:, :, None] - wave.phase_lag[None]
                    self.it += n_steps
                    return (wave.amplitude[None]*torch.sin(arg)).contiguous()
            ctl = TapeSweep()
        sim.task._controller = ctl
    sim.step_fused(STEPS)
    torch.cuda.synchronize(); t0 = time.time()
    for _ in range(LAUNCHES):
        sim.step_fused(STEPS)
    torch.cuda.synchronize(); dt = time.time() - t0
    assert int(sim.physics.data.status.abs().sum()) == 0
    print(json.dumps(dict(config=config, rate=N*STEPS*LAUNCHES/dt, last_launch=sim.physics.kernel_info().get('dual_last_launch'))), flush=True)


if __name__ == '__main__':
    if len(sys.argv) > 2 and sys.argv[1] == '--config':
        run_one(sys.argv[2][-1])
        sys.exit(0)
    reps = int(sys.argv[1]) if len(sys.argv) > 1 else 3
    configs = ['a', 'b', 'c', 'd'] + (['base_a', 'base_b'] if os.path.exists(BASE_SO) else [])
    rates = {c: [] for c in configs}
    for _ in range(reps):
        for c in configs:
            env = dict(os.environ)
            env.pop('FMJ_DUAL_LEAN', None)
            if c.endswith('b'):
                env['FMJ_DUAL_LEAN'] = '0'
            if c.startswith('base_'):
                env['FMJ_SO'] = BASE_SO
            out = subprocess.run([sys.executable, os.path.abspath(__file__), '--config', c], env=env, capture_output=True, text=True, timeout=300)
            if out.returncode != 0:      # nothing more is started on the device after a failure
                sys.exit(f'{c}: exit status {out.returncode}\n{out.stderr[-2000:]}')
            r = json.loads(out.stdout.strip().splitlines()[-1])
            rates[c].append(r['rate'])
            print(c, f"{r['rate']/1e6:.2f} M env-steps/s", r['last_launch'], flush=True)
    med = {c: float(np.median(v)) for c, v in rates.items()}
    for c, v in rates.items():
        print(f'{c}: median {med[c]/1e6:.2f} M env-steps/s, spread {(max(v) - min(v))/med[c]*100:.2f} % over {len(v)} runs')
    print(f"c / d = {med['c']/med['d']:.2f}; c / a = {med['c']/med['a']:.3f}" +
          (f"; b / base_b = {med['b']/med['base_b']:.4f}; a / base_a = {med['a']/med['base_a']:.4f}" if 'base_b' in med else ''))
