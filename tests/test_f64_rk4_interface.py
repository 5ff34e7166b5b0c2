"""RK4 inside the fp64 step kernel (fmj_create_ex2 with FMJ_CREATE_F64_RK4, csrc/fmj_f64_step.inc compiled as fmj_step_f64_rk4_kernel) as
far as it can be checked without a GPU: the flag and what it leaves alone, the argument errors (decided before the device lookup), what
stays refused, the Python arguments, and the compiler's resource remarks for the four new kernels."""
import ctypes
import inspect
import os
import re
import shutil

import pytest

from support_capi import lib as _lib, create_ex as _create_ex, F32, FMJ_ERR_ARG, FMJ_ERR_UNSUPPORTED
from support_f64_interface import (create_ex2 as _create_ex2, limited_eel48 as _limited_eel48, accepted as _accepted, LIMITS, RK4, SRC,
                                   lds_bytes, resource_remarks, within_resources)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _rk4(m):
    from farms_mujoco_amd.model import INTEGRATORS
    m.integrator = INTEGRATORS['rk4']
    return m


def test_the_flag_is_8_and_the_abi_stays():
    L, lib = _lib()
    assert L.CREATE_F64_RK4 == 8 and L.CREATE_F64_LIMITS == 1
    assert lib.fmj_abi_version() == 6 and L.ABI_VERSION == 6 and ctypes.sizeof(L.CCreateExt) == 8
    hdr = open(os.path.join(ROOT, 'include', 'fmj.h')).read()
    assert 'FMJ_CREATE_F64_RK4 = 8' in hdr and 'FMJ_CREATE_F64_LIMITS = 1' in hdr and '#define FMJ_ABI_VERSION 6' in hdr
    assert 'Bits 2 and 4' in hdr      # the header says that they stay unknown


def test_an_rk4_salamander_passes_every_model_check():
    from farms_mujoco_amd.model import salamander33
    rc, msg, prec, _ = _create_ex2(_rk4(salamander33()), flags=RK4)
    assert _accepted(rc, msg, prec), (rc, msg)


def test_an_rk4_tree_past_64_dofs_passes_every_model_check():
    from farms_mujoco_amd.model import centipede
    m = _rk4(centipede(20, 25))
    assert m.nv > 64
    rc, msg, prec, _ = _create_ex2(m, flags=RK4)
    assert _accepted(rc, msg, prec), (rc, msg)


def test_a_limited_rk4_eel48_passes_with_both_flags():
    rc, msg, prec, _ = _create_ex2(_rk4(_limited_eel48()), flags=LIMITS | RK4)
    assert _accepted(rc, msg, prec), (rc, msg)
    rc, msg, _, _ = _create_ex2(_rk4(_limited_eel48()), flags=RK4)      # RK4 alone does not take the limits
    assert rc == FMJ_ERR_UNSUPPORTED and 'fp64' in msg and 'limit' in msg, (rc, msg)


def test_argument_errors_come_before_the_device_lookup():
    from farms_mujoco_amd.model import salamander33
    m = _rk4(salamander33())
    rc, msg, _, _ = _create_ex2(m, precision=F32, flags=RK4)
    assert rc == FMJ_ERR_ARG and 'FMJ_CREATE_F64_RK4' in msg and 'FMJ_PRECISION_F64' in msg, (rc, msg)
    for flags in (2, 4, RK4 | 2, RK4 | 4, 16):
        rc, msg, _, _ = _create_ex2(m, flags=flags)
        assert rc == FMJ_ERR_ARG and 'flags' in msg, (flags, rc, msg)


def test_contacts_stay_refused_with_the_flag():
    from farms_mujoco_amd.model import salamander33
    for flags in (RK4, RK4 | LIMITS):
        rc, msg, _, _ = _create_ex2(_rk4(salamander33(contacts=True)), flags=flags)
        assert rc == FMJ_ERR_UNSUPPORTED and 'fp64' in msg and 'contact' in msg, (flags, rc, msg)


def test_without_the_flag_the_refusal_stays_word_for_word():
    from farms_mujoco_amd.model import salamander33
    m = _rk4(salamander33())
    rc, msg, _ = _create_ex(m)
    assert rc == FMJ_ERR_UNSUPPORTED and msg == 'fmj_create_ex: the fp64 step integrates with Euler or implicitfast, not RK4', (rc, msg)
    for kw in (dict(flags=0), dict(flags=LIMITS), dict(ext=False)):
        rc, msg2, _, _ = _create_ex2(m, **kw)
        assert rc == FMJ_ERR_UNSUPPORTED and msg2 == msg, (kw, rc, msg2)


def test_python_takes_fp64_rk4():
    from farms_mujoco_amd.model import salamander33
    from farms_mujoco_amd.physics import BatchedPhysics
    from farms_mujoco_amd.simulation.simulation import Simulation
    from farms_mujoco_amd.options import SimulationOptions, ArenaOptions, AnimatOptions
    p = inspect.signature(BatchedPhysics.__init__).parameters
    assert 'fp64_rk4' in p and p['fp64_rk4'].default is False
    m = _rk4(salamander33())
    for precision in ('fp32', 'fp16'):       # before any device use: no GPU is needed to get here
        with pytest.raises(ValueError):
            BatchedPhysics(m, 2, precision=precision, fp64_rk4=True)
    with pytest.raises(ValueError, match='fp64_rk4'):
        BatchedPhysics(m, 2, fp64_rk4=True)
    with pytest.raises(ValueError, match='fp64_rk4'):
        Simulation(m, m.body_names[1], SimulationOptions(timestep=m.timestep, n_iterations=2, integrator='RK4'), n_envs=2, fp64_rk4=True)
    with pytest.raises(ValueError, match='fp64_rk4'):
        Simulation.from_sdf(SimulationOptions(timestep=m.timestep, n_iterations=2, integrator='RK4'), AnimatOptions.from_model(m), ArenaOptions(),
                            model=m, n_envs=2, fp64_rk4=True)


@pytest.mark.skipif(shutil.which('hipcc') is None, reason='hipcc not on PATH')
def test_rk4_kernels_compile_without_scratch(tmp_path):
    """The translation unit of the RK4 kernels (-DFMJ_TU_F64=3) with the flags of _lib.build() holds exactly four kernels,
    fmj_step_f64_rk4_kernel<FUSED, LIMITS>; all keep out of scratch, spill no VGPR, and their LDS at the size limits (ldsd_total_bytes
    with limits + F64_RK4_LDS_DOUBLES(nu) of fmj_f64.inc, nu = 128: 2 nu doubles and 12 rows of one double per lane) is within 160 KB."""
    res = resource_remarks('-DFMJ_TU_F64=3', tmp_path)
    rk = {k: v for k, v in res.items() if re.search(r'fmj_step_f64_rk4_kernelILb[01]ELb[01]EE', k)}
    assert len(res) == 4 and len(rk) == 4, sorted(res)
    from farms_mujoco_amd import _lib as L
    inc = open(os.path.join(os.path.dirname(SRC), 'fmj_f64.inc')).read()
    assert "'-DFMJ_TU_F64=3'" in inspect.getsource(L.build) and 'F64_RK4_LDS_DOUBLES(nu) (2 * (nu) + F64_RK4_ROWS * FMJ_F64_LANES)' in inc and 'F64_RK4_ROWS = 12' in inc and 'F64_LIMITS_LDS_DOUBLES 20' in inc
    within_resources(rk, lds_bytes('rk4', 128, 128, 129, 64, nu=128))
