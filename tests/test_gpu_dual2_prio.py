"""Issue priority in the two-env step kernel (csrc/fmj_dual2.inc, FMJ_DUAL_PRIO_POLICY): fused launches let the waves that share a SIMD
take turns at s_setprio 1.  That changes which wave wins arbitration and nothing a wave computes, so a run with it must agree BITWISE
with a run of a context created with KernelOptions(prio=False), in every register tier and on the per-iteration host path.
Only the builds of the WPS = 2 and 3 tiers carry the policy (FMJ_DUAL_PRIO_MAX_WPS): kernel_info() reports it there and False in the other
tier, whose cases check the plumbing only - the switch must change nothing where there is nothing to switch."""
import pytest

from farms_mujoco_amd.options import KernelOptions
from support_sims import dual2_run, assert_bitwise

pytestmark = pytest.mark.gpu

N, T, RING = 7, 120, 40      # odd batch: the last wave has an idle half; more steps than ring rows: the ring wraps
PRIO_TIERS = ('2', '3')      # register tiers whose builds carry the policy: wps <= FMJ_DUAL_PRIO_MAX_WPS of csrc/fmj_dual2.inc (keep in step)


def _run(fused=True, **kernel):
    """The workload in a context created with KernelOptions(**kernel): its outputs and the context's kernel_info after the run."""
    return dual2_run(N, T, RING, KernelOptions(**kernel), fused)[:2]


@pytest.mark.parametrize('wps', ['2', '3', '4'])
def test_priority_policy_is_bitwise_the_plain_run(wps):
    on, info = _run(wps=int(wps))
    assert info['threads_per_env'] == 32 and info['dual_wps'] == int(wps)
    assert info['dual_prio'] is (wps in PRIO_TIERS) and info['dual_last_launch'] == 'lean', info          # the default, on the kernel of the headline
    off, oinfo = _run(wps=int(wps), prio=False)
    assert oinfo['dual_prio'] is False and oinfo['dual_last_launch'] == 'lean', oinfo
    assert oinfo['dual_wps'] == int(wps) and oinfo['dual_build'] == info['dual_build'] == 'lean'      # the switch moved nothing else
    assert_bitwise(on, off, f'WPS={wps} priority on vs prio=False')


@pytest.mark.parametrize('wps', ['2', '3', '4'])
def test_priority_policy_in_the_generic_build(wps):
    on, info = _run(wps=int(wps), lean=False)
    assert info['dual_prio'] is (wps in PRIO_TIERS) and info['dual_last_launch'] == 'generic', info
    off, oinfo = _run(wps=int(wps), lean=False, prio=False)
    assert oinfo['dual_prio'] is False and oinfo['dual_last_launch'] == 'generic', oinfo
    assert_bitwise(on, off, f'WPS={wps} generic build, priority on vs prio=False')


def test_host_path_is_bitwise_with_and_without_the_switch():
    a, info = _run(fused=False, wps=2)      # (seven envs would pick this tier anyway)
    assert info['dual_prio'] is True and info['dual_last_launch'] == 'generic', info
    b, oinfo = _run(fused=False, wps=2, prio=False)
    assert oinfo['dual_prio'] is False and oinfo['dual_last_launch'] == 'generic', oinfo
    assert_bitwise(a, b, 'host path, priority on vs prio=False')
