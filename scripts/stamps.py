"""Diagnostic: per-phase cycle shares of the fused step kernel (a -DFMJ_STAMPS build of the library, made on demand:
``python -c "from farms_mujoco_amd import _lib; _lib.build(defines=['-DFMJ_STAMPS'], out='libfmj_hip_stamps.so')"``).
usage: python scripts/stamps.py [batch ...]      a batch is an env count, or ``N:p0`` for that count with FMJ_DUAL_PRIO=0 at fmj_create
(the two-env kernel without its priority code).  With more than one batch the phases of every later batch are also set against the
first one, cycles and ratio - ``FMJ_WPS=2 python scripts/stamps.py 2048 4096 4096:p0`` is a wave alone on its SIMD against a wave
with a partner, with the priority policy and without."""
import sys, os
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from farms_mujoco_amd import _lib
_lib.SO_PATH = os.path.join(_lib.CSRC, os.environ.get('FMJ_STAMPS_SO', 'libfmj_hip_stamps.so'))
import torch, bench
names = ['emit+drag', 'joints row', 'K', 'C', 'V', 'F+carry', 'S', 'Q', 'M', 'L', 'X', 'Euler', 'facM', 'collide', 'Jrows', 'rowprm', 'Y',
         'A|nwt-start', 'warm|nwt-H', 'PGS|nwt-update', 'qfrc_c', 'nwt-factor', 'nwt-solve', 'nwt-linesearch']
workload = os.environ.get('FMJ_WORKLOAD', 'swim')
prio_env = os.environ.get('FMJ_DUAL_PRIO')
taken = []
for arg in sys.argv[1:] or ['256', '4096']:
    n = int(arg.split(':')[0])
    if arg.endswith(':p0'):
        os.environ['FMJ_DUAL_PRIO'] = '0'
    elif prio_env is None:
        os.environ.pop('FMJ_DUAL_PRIO', None)
    else:
        os.environ['FMJ_DUAL_PRIO'] = prio_env
    sim, m, _ = bench.build_sim(n, 1 << 30, 100, 0, 'cuda:0', workload, **({'morphology': os.environ['FMJ_MORPHOLOGY']} if 'FMJ_MORPHOLOGY' in os.environ else {}))
    print('lds bytes per env', sim.physics.kernel_info())
    for _ in range(int(os.environ.get('FMJ_STAMP_WARM', '100')) // 100 + 1):
        sim.step_fused(100)
    torch.cuda.synchronize()
    st = sim.physics.data.qacc[0, :24].cpu().numpy()/100.0
    tot = st.sum()
    print(f'n_envs={arg}: cycles/step {tot:.0f}')
    print('  ' + '  '.join(f'{k}:{v:.0f}({100*v/tot:.0f}%)' for k, v in zip(names, st)))
    if workload.startswith('walk'):
        nc = sim.physics.data.ncon.float()
        print(f'  ncon mean {nc.mean().item():.1f} max {nc.max().item():.0f} env0 {nc[0].item():.0f}')
    taken.append((arg, st))
    del sim
if len(taken) > 1:      # every later batch against the first: cycles per step of env 0's wave, ratio, share of the difference
    a0, s0 = taken[0]
    for a1, s1 in taken[1:]:
        d = s1.sum() - s0.sum()
        print(f'{a1} against {a0}: phase, cycles, cycles, ratio, share of the difference')
        for k, x, y in zip(names, s0, s1):
            if x > 0 or y > 0:
                print(f'  {k:12s} {x:8.0f} {y:8.0f}  {y/x if x > 0 else float("nan"):6.3f}  {100*(y - x)/d if d else float("nan"):6.1f} %')
        print(f'  {"step":12s} {s0.sum():8.0f} {s1.sum():8.0f}  {s1.sum()/s0.sum():6.3f}  (difference) / (second) = {100*d/s1.sum():.1f} %')
