"""Kernel selection per context (include/fmj.h, "Kernel selection" at fmj_create_ex; farms_mujoco_amd.options.KernelOptions) as far
as it can be checked without a GPU: the kernel fields of fmj_create_options are validated before the device lookup, the 8-byte struct
from before them is still accepted, and the Python option class is strict.  What the options select is checked on the device, by
the tests that compare kernels (tests/test_gpu_dual2_lean.py and the others that pass ``kernel=``)."""
import ctypes
import inspect

import pytest

from support_capi import lib as _lib, create_ex as _create_ex, no_gpu as _no_gpu, F32, FMJ_ERR_ARG, FMJ_ERR_NODEVICE


def test_struct_and_flags_mirror_the_header():
    L, _ = _lib()
    assert ctypes.sizeof(L.CCreateOptions) == 16
    assert [n for n, _ in L.CCreateOptions._fields_] == ['size', 'precision', 'kernel_flags', 'dual_wps']
    assert (L.KERNEL_TWO_WAVE, L.KERNEL_ONE_ENV_PER_WAVE, L.KERNEL_NO_LEAN, L.KERNEL_NO_PRIO) == (1, 2, 4, 8)


def test_unknown_flag_bit_is_an_argument_error():
    from farms_mujoco_amd.model import salamander33
    for flags in (16, 1 | 32, -1):
        rc, msg, _ = _create_ex(salamander33(), precision=F32, kernel_flags=flags)
        assert rc == FMJ_ERR_ARG and 'kernel_flags' in msg, (flags, rc, msg)


@pytest.mark.parametrize('wps', [5, 1, -2])
def test_bad_dual_wps_is_an_argument_error(wps):
    from farms_mujoco_amd.model import salamander33
    rc, msg, _ = _create_ex(salamander33(), precision=F32, dual_wps=wps)
    assert rc == FMJ_ERR_ARG and 'dual_wps' in msg, (rc, msg)


@pytest.mark.parametrize('opts', [dict(size=8), dict(size=8, kernel_flags=-1, dual_wps=5), dict(), dict(kernel_flags=15, dual_wps=3)],
                         ids=['size8', 'size8_tail_not_read', 'zeros', 'every_flag'])
def test_valid_options_pass_every_model_check(opts):
    """The struct of the header before the kernel fields (size 8: whatever lies behind it is not read), a full struct of zeros and one
    with every flag.  On a machine without a GPU the first thing that fails is the device lookup; with one the context is created."""
    from farms_mujoco_amd.model import salamander33
    rc, msg, prec = _create_ex(salamander33(), precision=F32, **opts)
    if _no_gpu():
        assert rc == FMJ_ERR_NODEVICE, (rc, msg)
    else:
        assert rc == 0 and prec == F32, (rc, msg, prec)


def test_kernel_options_are_strict():
    from farms_mujoco_amd.options import KernelOptions
    k = KernelOptions()
    assert (k.two_wave, k.two_env, k.wps, k.lean, k.prio) == (False, True, None, True, True)
    k = KernelOptions(two_wave=True, two_env=False, wps=3, lean=False, prio=False)
    assert (k.two_wave, k.two_env, k.wps, k.lean, k.prio) == (True, False, 3, False, False)
    with pytest.raises(AssertionError):
        KernelOptions(wide=True)
    with pytest.raises(ValueError, match='wps'):
        KernelOptions(wps=5)


def test_python_takes_kernel():
    from farms_mujoco_amd.physics import BatchedPhysics
    from farms_mujoco_amd.simulation.simulation import Simulation
    from farms_mujoco_amd.model import salamander33
    p = inspect.signature(BatchedPhysics.__init__).parameters
    assert 'kernel' in p and p['kernel'].default is None
    assert "kwargs.pop('kernel', None)" in inspect.getsource(Simulation.__init__)
    with pytest.raises(TypeError, match='KernelOptions'):        # before any device use: no GPU is needed to get here
        BatchedPhysics(salamander33(), 2, kernel=dict(wps=2))
