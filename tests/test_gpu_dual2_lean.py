"""The lean build of the two-env step kernel (csrc/fmj_dual2.inc, LEAN): a fused launch of the flagship shape runs an instantiation
with its launch options folded in at compile time.  It removes tests, not arithmetic, so it must agree BITWISE with the generic
build (KernelOptions(lean=False)) in every register tier, and a launch shape it does not cover must still run the generic build."""
import pytest

from farms_mujoco_amd.options import KernelOptions
from support_sims import dual2_swim, dual2_finish, dual2_run, assert_bitwise as _assert_bitwise

pytestmark = pytest.mark.gpu

N, T, RING = 7, 120, 40      # odd batch: the last wave has an idle half; more steps than ring rows: the ring wraps


def _run(fused=True, **kernel):
    return dual2_run(N, T, RING, KernelOptions(**kernel), fused)


@pytest.mark.parametrize('wps', ['2', '3', '4'])
def test_lean_build_is_bitwise_the_generic_build(wps):
    lean, info, _ = _run(wps=int(wps))
    assert info['threads_per_env'] == 32 and info['dual_wps'] == int(wps)
    assert info['dual_build'] == 'lean' and info['dual_last_launch'] == 'lean', info      # the default, and the fused run really took it
    generic, ginfo, _ = _run(wps=int(wps), lean=False)
    assert ginfo['dual_build'] == 'generic' and ginfo['dual_last_launch'] == 'generic', ginfo
    _assert_bitwise(lean, generic, f'WPS={wps} lean vs generic')


def test_launch_shape_the_lean_build_refuses_runs_the_generic_build():
    """The per-iteration host path: one-step launches with rows_ahead (and a last one without readout), none of which the lean
    build covers.  A context with the lean build enabled runs the generic build for every one of them, to the same bits as a
    context that has it turned off."""
    a, info, launches = _run(fused=False)
    assert info['dual_build'] == 'lean' and launches == {'generic'}, (info, launches)
    b, ginfo, glaunches = _run(fused=False, lean=False)
    assert ginfo['dual_build'] == 'generic' and glaunches == {'generic'}, (ginfo, glaunches)
    _assert_bitwise(a, b, 'host path, lean enabled vs forced generic')


def test_register_tiers_agree_bitwise():
    """The three register tiers compute the same bits on the fused workload (the property the per-tier instruction orders - resident
    constants, the order of independent chains - have to keep)."""
    w2, i2, _ = _run(wps=2)
    w4, i4, _ = _run(wps=4)
    assert i2['dual_wps'] == 2 and i4['dual_wps'] == 4
    _assert_bitwise(w2, w4, 'WPS=2 vs WPS=4')
    w3, _, _ = _run(wps=3)
    _assert_bitwise(w3, w4, 'WPS=3 vs WPS=4')


def test_register_tiers_agree_bitwise_with_both_contexts_alive():
    """The tier is a property of the context: two simulations that differ in it are constructed first, then run one after the other."""
    s2, s4 = (dual2_swim(N, T, RING, KernelOptions(wps=w)) for w in (2, 4))
    assert s2.physics.kernel_info()['dual_wps'] == 2 and s4.physics.kernel_info()['dual_wps'] == 4
    w2, i2, _ = dual2_finish(s2)
    w4, i4, _ = dual2_finish(s4)
    assert i2['dual_wps'] == 2 and i4['dual_wps'] == 4
    assert i2['threads_per_env'] == i4['threads_per_env'] == 32 and i2['dual_last_launch'] == i4['dual_last_launch'] == 'lean', (i2, i4)
    _assert_bitwise(w2, w4, 'WPS=2 vs WPS=4, both contexts alive')
