"""Kernel selection per context on the device (include/fmj.h, "Kernel selection" at fmj_create_ex): the FMJ_* variables speak for a
caller who passes no kernel options, and a caller who passes them has said everything.  Contexts are created, none is stepped: what the
options select computes is checked by the tests that compare kernels.  This is the only test that sets one of the variables."""
import pytest

pytestmark = pytest.mark.gpu


def test_environment_is_the_fallback_and_options_take_precedence(monkeypatch):
    from farms_mujoco_amd.model import salamander33
    from farms_mujoco_amd.options import KernelOptions
    from farms_mujoco_amd.physics import BatchedPhysics
    for k in ('FMJ_WIDE', 'FMJ_DUAL', 'FMJ_WPS', 'FMJ_DUAL_LEAN', 'FMJ_DUAL_PRIO'):
        monkeypatch.delenv(k, raising=False)
    m = salamander33()
    info = lambda kernel: BatchedPhysics(m, 3, kernel=kernel).kernel_info()
    monkeypatch.setenv('FMJ_DUAL', '0')
    assert info(None)['threads_per_env'] == 64                  # no options: the variable is heard
    assert info(KernelOptions())['threads_per_env'] == 32       # options, all at their defaults: it is not
    monkeypatch.delenv('FMJ_DUAL')
    monkeypatch.setenv('FMJ_WPS', '4')
    assert info(None)['dual_wps'] == 4
    assert info(KernelOptions(wps=2))['dual_wps'] == 2
