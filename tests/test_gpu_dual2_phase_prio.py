"""Issue priority by phase in the two-env step kernel (csrc/fmj_dual2.inc, FMJ_DUAL_PRIO_PHASE): a fused launch may execute s_setprio at
the top of a step and at phase boundaries inside it.  Whatever policy the library was built with, it decides which wave wins
arbitration and nothing a wave computes: a run with it must agree BITWISE with a run of a context created with KernelOptions(prio=False),
which executes no s_setprio at all - on the lean and on the generic build, in the register tiers that carry the policy (wps = 2, 3) and in
the one that does not (4), which must report policy 0.  kernel_info() names the build that ran and the policy id it carries."""
import pytest

from farms_mujoco_amd.options import KernelOptions
from support_sims import dual2_run, assert_bitwise

pytestmark = pytest.mark.gpu

N, T, RING = 5, 20, 7        # odd batch: the last wave has an empty half; 20 fused steps over a ring of 7 rows, which wraps twice
PRIO_TIERS = ('2', '3')      # wps <= FMJ_DUAL_PRIO_MAX_WPS of csrc/fmj_dual2.inc (keep in step)


def _run(**kernel):
    return dual2_run(N, T, RING, KernelOptions(**kernel))[:2]


@pytest.mark.parametrize('build', ['lean', 'generic'])
@pytest.mark.parametrize('wps', ['2', '3', '4'])
def test_phase_priority_is_bitwise_the_plain_run(wps, build):
    on, info = _run(wps=int(wps), lean=build == 'lean')
    assert info['threads_per_env'] == 32 and info['dual_wps'] == int(wps) and info['dual_last_launch'] == build, info
    if wps in PRIO_TIERS:
        assert info['dual_prio'] is True and info['dual_prio_policy'] >= 1, info      # the policy id the library's builds carry
    else:
        assert info['dual_prio'] is False and info['dual_prio_policy'] == 0, info     # a tier without a policy
    off, oinfo = _run(wps=int(wps), lean=build == 'lean', prio=False)
    assert oinfo['dual_prio'] is False and oinfo['dual_prio_policy'] == 0, oinfo       # no s_setprio at all
    assert oinfo['dual_wps'] == int(wps) and oinfo['dual_last_launch'] == build, oinfo  # the switch moved nothing else
    assert_bitwise(on, off, f'WPS={wps} {build} build, priority policy {info["dual_prio_policy"]} vs prio=False')
