"""Joint limits on the fp64 step (fmj_create_ex2 with FMJ_CREATE_F64_LIMITS, the LIMITS instantiations of csrc/fmj_f64.inc) as far as
it can be checked without a GPU: the entry point and its extension struct, the argument errors (decided before the device lookup),
what stays refused, the Python arguments, and the compiler's resource remarks for the two new instantiations."""
import ctypes
import inspect
import os
import re
import shutil

import numpy as np
import pytest

from support_capi import lib as _lib, create_ex as _create_ex, no_gpu as _no_gpu, F32, F64, FMJ_ERR_ARG, FMJ_ERR_UNSUPPORTED, FMJ_ERR_NODEVICE
from support_f64_interface import (create_ex2 as _create_ex2, limited_eel48 as _limited_eel48, LIMITS, SRC, lds_bytes, resource_remarks,
                                   within_resources)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_entry_point_and_struct_sizes():
    L, lib = _lib()
    assert hasattr(lib, 'fmj_create_ex2') and 'fmj_create_ex2' in L.SYMBOLS
    assert lib.fmj_abi_version() == 6 and L.ABI_VERSION == 6
    assert ctypes.sizeof(L.CCreateOptions) == 16 and ctypes.sizeof(L.CCreateExt) == 8
    assert [n for n, _ in L.CCreateExt._fields_] == ['size', 'flags'] and L.CREATE_F64_LIMITS == 1
    hdr = open(os.path.join(ROOT, 'include', 'fmj.h')).read()
    assert 'fmj_create_ex2' in hdr and 'FMJ_CREATE_F64_LIMITS = 1' in hdr and '#define FMJ_ABI_VERSION 6' in hdr


def test_argument_errors_come_before_the_device_lookup():
    m = _limited_eel48()
    rc, msg, _, _ = _create_ex2(m, size=12)
    assert rc == FMJ_ERR_ARG and 'size' in msg, (rc, msg)
    rc, msg, _, _ = _create_ex2(m, flags=2)
    assert rc == FMJ_ERR_ARG and 'flags' in msg, (rc, msg)
    rc, msg, _, _ = _create_ex2(m, flags=LIMITS | 4)
    assert rc == FMJ_ERR_ARG and 'flags' in msg, (rc, msg)
    rc, msg, _, _ = _create_ex2(m, precision=F32)
    assert rc == FMJ_ERR_ARG and 'FMJ_PRECISION_F64' in msg, (rc, msg)


def test_limited_eel48_passes_every_model_check():
    """48 dofs in one chain: past the fp32 constraint path's chain of 32.  Without a GPU the first thing that fails is the device lookup."""
    rc, msg, prec, solver = _create_ex2(_limited_eel48())
    if _no_gpu():
        assert rc == FMJ_ERR_NODEVICE, (rc, msg)
    else:
        assert rc == 0 and prec == F64, (rc, msg, prec)
        assert solver[1] == 2 and solver[2] == _limited_eel48().solver_iterations, solver      # Newton runs, with the model's budget


def test_a_limited_tree_past_64_dofs_passes_every_model_check():
    from farms_mujoco_amd.model import centipede
    m = centipede(20, 25)
    assert m.nv > 64
    m.jnt_limited = (m.jnt_type != 0).astype(m.jnt_limited.dtype)
    m.jnt_range = np.tile([-0.1, 0.1], (m.njnt, 1)).astype(float)
    rc, msg, prec, _ = _create_ex2(m)
    assert (rc == FMJ_ERR_NODEVICE) if _no_gpu() else (rc == 0 and prec == F64), (rc, msg)


def test_without_the_flag_the_refusal_stays():
    m = _limited_eel48()
    rc, msg, _ = _create_ex(m)
    assert rc == FMJ_ERR_UNSUPPORTED and 'fp64' in msg and 'limit' in msg, (rc, msg)
    for kw in (dict(flags=0), dict(ext=False)):
        rc, msg2, _, _ = _create_ex2(m, **kw)
        assert rc == FMJ_ERR_UNSUPPORTED and msg2 == msg, (kw, rc, msg2)


def test_contacts_and_rk4_stay_refused_with_the_flag():
    from farms_mujoco_amd.model import salamander33, INTEGRATORS
    rc, msg, _, _ = _create_ex2(salamander33(contacts=True))
    assert rc == FMJ_ERR_UNSUPPORTED and 'fp64' in msg and 'contact' in msg, (rc, msg)
    m = _limited_eel48()
    m.integrator = INTEGRATORS['rk4']
    rc, msg, _, _ = _create_ex2(m)
    assert rc == FMJ_ERR_UNSUPPORTED and 'fp64' in msg and 'RK4' in msg, (rc, msg)


def test_python_takes_fp64_limits():
    from farms_mujoco_amd.physics import BatchedPhysics
    from farms_mujoco_amd.simulation.simulation import Simulation
    from farms_mujoco_amd.options import SimulationOptions, ArenaOptions, AnimatOptions
    p = inspect.signature(BatchedPhysics.__init__).parameters
    assert 'fp64_limits' in p and p['fp64_limits'].default is False
    m = _limited_eel48()
    for precision in ('fp32', 'fp16'):       # before any device use: no GPU is needed to get here
        with pytest.raises(ValueError):
            BatchedPhysics(m, 2, precision=precision, fp64_limits=True)
    with pytest.raises(ValueError, match='fp64_limits'):
        BatchedPhysics(m, 2, fp64_limits=True)
    with pytest.raises(ValueError, match='fp64_limits'):
        Simulation.from_sdf(SimulationOptions(timestep=m.timestep, n_iterations=2), AnimatOptions.from_model(m), ArenaOptions(),
                            model=m, n_envs=2, fp64_limits=True)


@pytest.mark.skipif(shutil.which('hipcc') is None, reason='hipcc not on PATH')
def test_limits_instantiations_compile_without_scratch(tmp_path):
    """The translation unit of the LIMITS instantiations (-DFMJ_TU_F64=2) with the flags of _lib.build() holds two kernels, the plain
    step and the fused loop; both keep out of scratch, spill no VGPR, and their LDS at the size limits (ldsd_total_bytes of
    fmj_f64.inc: F64_LIMITS_LDS_DOUBLES = 20 doubles past ldsd_layout) is within 160 KB."""
    res = resource_remarks('-DFMJ_TU_F64=2', tmp_path)
    lim = {k: v for k, v in res.items() if re.search(r'fmj_step_f64_kernelILb[01]ELb1EE', k)}      # <FUSED, LIMITS = true>
    assert len(res) == 2 and len(lim) == 2, sorted(res)
    from farms_mujoco_amd import _lib as L
    assert "'-DFMJ_TU_F64=2'" in inspect.getsource(L.build) and 'F64_LIMITS_LDS_DOUBLES 20' in open(os.path.join(os.path.dirname(SRC), 'fmj_f64.inc')).read()
    within_resources(lim, lds_bytes('limits', 128, 128, 129, 64))
