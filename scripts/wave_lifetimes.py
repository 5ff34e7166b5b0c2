"""Diagnostic (-DFMJ_STAMPS build): lifetime and placement of every wave of one 1000-step launch of the two-env swim kernel
(csrc/fmj_dual2.inc).  Every wave of the headline batch is resident from the launch's first cycle, so the launch lasts as long as its
slowest wave: the script prints how far the mean wave is from the slowest one, and splits the lifetimes by the waves that share a SIMD
(first against second to enter), by XCC and by wave slot.
usage: python scripts/wave_lifetimes.py [envs] [steps per launch]      (FMJ_STAMPS_SO names another stamps build in csrc/;
FMJ_DUAL_PRIO=0 runs it without the priority code)"""
import os, sys
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from farms_mujoco_amd import _lib
_lib.SO_PATH = os.path.join(_lib.CSRC, os.environ.get('FMJ_STAMPS_SO', 'libfmj_hip_stamps.so'))
import numpy as np, torch, bench

n = int(sys.argv[1]) if len(sys.argv) > 1 else 4096
T = int(sys.argv[2]) if len(sys.argv) > 2 else 1000
sim, m, _ = bench.build_sim(n, 1 << 30, T, 0, 'cuda:0')
info = sim.physics.kernel_info()
print(f'{n} envs, launches of {T} steps, library {os.path.basename(_lib.SO_PATH)} build {_lib.build_id()}, kernel_info {info}')


def stats(t):
    return (f'n {len(t):5d}  mean {t.mean()/1e6:7.3f} M  p10 {np.percentile(t, 10)/1e6:7.3f}  p50 {np.median(t)/1e6:7.3f}  p90 {np.percentile(t, 90)/1e6:7.3f}  '
            f'max {t.max()/1e6:7.3f}') if len(t) else 'n     0'


for k in range(4):      # three warm launches, then the one that is reported
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record(); sim.step_fused(T); e1.record()
    torch.cuda.synchronize()
ms = e0.elapsed_time(e1)
# the last six qacc slots of an env: entry lo / hi, exit lo / hi (s_memtime), HW_REG_HW_ID, HW_REG_XCC_ID - raw words
w = sim.physics.data.qacc[:, m.nv - 6:].contiguous().view(torch.int32).cpu().numpy().view(np.uint32).astype(np.uint64)
w = w[0::2]      # one record per wave (both halves of a wave write the same words)
t0 = w[:, 0] | (w[:, 1] << np.uint64(32)); t1 = w[:, 2] | (w[:, 3] << np.uint64(32))
hw = w[:, 4].astype(np.int64); xcc = (w[:, 5].astype(np.int64)) & 15
slot, simd, pipe, cu, sh, se = hw & 15, (hw >> 4) & 3, (hw >> 6) & 3, (hw >> 8) & 15, (hw >> 12) & 1, (hw >> 13) & 7
life = (t1 - t0).astype(np.float64)
# s_memtime counters are not aligned between the SIMDs' clock domains (entry times of one launch differ by far more than the launch
# lasts): only differences taken by one wave, or between the waves of one SIMD, mean anything
print(f'launch {ms:.3f} ms by events; {len(life)} waves; longest lifetime {life.max()/1e6:.3f} M ticks = {life.max()/ms/1e3:.1f} ticks per us of the launch')
print(f'all waves   {stats(life)}  mean/max {life.mean()/life.max():.3f}')
# waves that share a SIMD
key = (((xcc * 8 + se) * 2 + sh) * 16 + cu) * 4 + simd
order = np.lexsort((t0, key))
ks, ls, ss, t0s, t1s = key[order], life[order], slot[order], t0[order], t1[order]
starts = np.flatnonzero(np.r_[True, ks[1:] != ks[:-1]]); counts = np.diff(np.r_[starts, len(ks)])
print(f'SIMDs in use {len(starts)}; waves per SIMD: ' + ', '.join(f'{c}: {int((counts == c).sum())} SIMDs' for c in np.unique(counts)))
for rank in range(int(counts.max())):
    sel = starts[counts > rank] + rank
    print(f'wave {rank + 1} to enter its SIMD   {stats(ls[sel])}  slots {sorted(set(ss[sel].tolist()))}')
two = starts[counts == 2]
if len(two):
    a, b = ls[two], ls[two + 1]
    print(f'pairs (SIMDs with two waves): {len(two)};  second entered {np.median((t0s[two + 1] - t0s[two]).astype(np.float64)):.0f} ticks after the first (median);  '
          f'first shorter than second in {100*(a < b).mean():.1f} %;  lifetime second - first: mean {np.mean(b - a)/1e6:+.3f} M  p10 {np.percentile(b - a, 10)/1e6:+.3f}  p90 {np.percentile(b - a, 90)/1e6:+.3f}')
    print(f'  shorter of a pair  {stats(np.minimum(a, b))}')
    print(f'  longer of a pair   {stats(np.maximum(a, b))}')
    print(f'  time the longer wave ran alone: mean {np.mean(np.abs((t1s[two + 1]).astype(np.float64) - (t1s[two]).astype(np.float64)))/1e6:.3f} M ticks '
          f'({100*np.mean(np.abs((t1s[two + 1]).astype(np.float64) - (t1s[two]).astype(np.float64)))/life.max():.1f} % of the longest lifetime)')
    sa, sb = ss[two], ss[two + 1]
    print(f'  slot pairs (first, second): ' + ', '.join(f'({x}, {y}): {c}' for (x, y), c in sorted(
        {p: int(((sa == p[0]) & (sb == p[1])).sum()) for p in set(zip(sa.tolist(), sb.tolist()))}.items())) +
          f';  slots differ in parity in {100*((sa ^ sb) & 1).mean():.1f} % of the pairs')
    hi = (sb & 1) == 1
    print(f'  odd-slot wave is the second to enter in {100*hi.mean():.1f} % of the pairs')
for x in np.unique(xcc):
    s_ = xcc == x
    print(f'XCC {x}   {stats(life[s_])}  mean/max {life[s_].mean()/life[s_].max():.3f}')
print('slot ids in use:', {int(s_): int((slot == s_).sum()) for s_ in np.unique(slot)})
