"""Shims around the C ABI (include/fmj.h) for the tests that call libfmj_hip.so directly: fmj_create validates a model before it
looks for a device, so most of them run without a GPU."""
import ctypes
import os

import pytest

FMJ_ERR_ARG, FMJ_ERR_UNSUPPORTED, FMJ_ERR_NODEVICE = 1, 2, 4      # include/fmj.h
F32, F64 = 0, 1                                                   # FMJ_PRECISION_*


def lib():
    """The ctypes mirror module and the loaded library."""
    try:
        import torch  # noqa: F401  (before the library, as in the package: loaded after it, torch and the library each find no device once the other has looked)
    except Exception:
        pass
    from farms_mujoco_amd import _lib
    if not os.path.exists(_lib.SO_PATH):
        pytest.skip('libfmj_hip.so not built')
    return _lib, _lib.load()


def no_gpu():
    try:
        import torch
        return not torch.cuda.is_available()
    except Exception:
        return True


def create(m):
    """fmj_create(m, 4 envs) and destroy: the return code and the library's message."""
    _, so = lib()
    c = m.as_c(); ctx = ctypes.c_void_p()
    rc = so.fmj_create(ctypes.byref(c), 4, 0, ctypes.byref(ctx))
    if rc == 0:
        so.fmj_destroy(ctx)
    return rc, so.fmj_last_error().decode()


def create_ex(m, precision=F64, size=None, kernel_flags=0, dual_wps=0):
    """fmj_create_ex(m, 4 envs, options) and destroy: the return code, the message and the precision the context reports."""
    L, so = lib()
    c = m.as_c(); ctx = ctypes.c_void_p()
    opts = L.CCreateOptions(ctypes.sizeof(L.CCreateOptions) if size is None else size, precision, kernel_flags, dual_wps)
    rc = so.fmj_create_ex(ctypes.byref(c), 4, 0, ctypes.byref(opts), ctypes.byref(ctx))
    prec = None
    if rc == 0:
        prec = so.fmj_precision(ctx)
        so.fmj_destroy(ctx)
    return rc, so.fmj_last_error().decode(), prec
