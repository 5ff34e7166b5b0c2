"""The opt-in fp64 step (fmj_create_ex with FMJ_PRECISION_F64, csrc/fmj_f64.inc) as far as it can be checked without a GPU: the two
new entry points, what an fp64 context refuses (before the device lookup, with 'fp64' in the message), the Python arguments, and the
compiler's resource remarks for the kernel (hipcc cross-compiles)."""
import inspect
import os
import shutil

import numpy as np
import pytest

from support_capi import (lib as _lib, create_ex as _create_ex, no_gpu as _no_gpu, F32, F64, FMJ_ERR_ARG, FMJ_ERR_UNSUPPORTED,
                          FMJ_ERR_NODEVICE)
from support_f64_interface import lds_bytes, resource_remarks, within_resources

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_entry_points_are_exported_and_the_abi_version_stays():
    L, lib = _lib()
    assert hasattr(lib, 'fmj_create_ex') and hasattr(lib, 'fmj_precision')
    assert lib.fmj_abi_version() == 6 and L.ABI_VERSION == 6
    hdr = open(os.path.join(ROOT, 'include', 'fmj.h')).read()
    assert 'fmj_create_ex' in hdr and 'FMJ_PRECISION_F64 = 1' in hdr and '#define FMJ_ABI_VERSION 6' in hdr


def test_fp64_refuses_limits():
    from farms_mujoco_amd.model import eel
    m = eel(n_joints=48)
    m.jnt_limited = np.ones_like(m.jnt_limited)
    m.jnt_range = np.tile([-1.0, 1.0], (m.njnt, 1)).astype(float)
    rc, msg, _ = _create_ex(m)
    assert rc == FMJ_ERR_UNSUPPORTED and 'fp64' in msg and 'limit' in msg, (rc, msg)


def test_fp64_refuses_contact_geoms():
    from farms_mujoco_amd.model import salamander33
    rc, msg, _ = _create_ex(salamander33(contacts=True))
    assert rc == FMJ_ERR_UNSUPPORTED and 'fp64' in msg and 'contact' in msg, (rc, msg)


def test_fp64_refuses_rk4():
    from farms_mujoco_amd.model import salamander33, INTEGRATORS
    m = salamander33()
    m.integrator = INTEGRATORS['rk4']
    rc, msg, _ = _create_ex(m)
    assert rc == FMJ_ERR_UNSUPPORTED and 'fp64' in msg and 'RK4' in msg, (rc, msg)


@pytest.mark.parametrize('name', ['eel48', 'centipede_20_25', 'salamander33'])
def test_fp64_models_pass_every_model_check(name):
    """On a machine without a GPU the first thing that fails is the device lookup; with one the context is created and reports fp64."""
    import farms_mujoco_amd.model as mm
    m = {'eel48': lambda: mm.eel(n_joints=48), 'centipede_20_25': lambda: mm.centipede(20, 25), 'salamander33': mm.salamander33}[name]()
    rc, msg, prec = _create_ex(m)
    if _no_gpu():
        assert rc == FMJ_ERR_NODEVICE, (rc, msg)
    else:
        assert rc == 0 and prec == F64, (rc, msg, prec)


def test_bad_precision_and_bad_size_are_argument_errors():
    from farms_mujoco_amd.model import salamander33
    m = salamander33()
    rc, msg, _ = _create_ex(m, precision=2)
    assert rc == FMJ_ERR_ARG and 'precision' in msg, (rc, msg)
    rc, msg, _ = _create_ex(m, precision=-1)
    assert rc == FMJ_ERR_ARG, (rc, msg)
    rc, msg, _ = _create_ex(m, precision=F64, size=4)
    assert rc == FMJ_ERR_ARG and 'size' in msg, (rc, msg)
    rc, msg, _ = _create_ex(m, precision=F32, size=12)
    assert rc == FMJ_ERR_ARG and 'size' in msg, (rc, msg)


def test_the_size_limits_keep_their_messages():
    from farms_mujoco_amd.model import centipede, eel
    rc, msg, _ = _create_ex(centipede(25, 30))
    assert rc == FMJ_ERR_UNSUPPORTED and '128' in msg, (rc, msg)
    rc, msg, _ = _create_ex(eel(n_joints=70))
    assert rc == FMJ_ERR_UNSUPPORTED and 'chain longer than 64' in msg, (rc, msg)


def test_python_takes_precision():
    from farms_mujoco_amd.physics import BatchedPhysics
    from farms_mujoco_amd.simulation.simulation import Simulation
    from farms_mujoco_amd.model import salamander33
    p = inspect.signature(BatchedPhysics.__init__).parameters
    assert 'precision' in p and p['precision'].default == 'fp32'
    assert 'precision' in inspect.getsource(Simulation.__init__)
    with pytest.raises(ValueError, match='fp16'):        # before any device use: no GPU is needed to get here
        BatchedPhysics(salamander33(), 2, precision='fp16')
    from farms_mujoco_amd.options import SimulationOptions, ArenaOptions, AnimatOptions
    m = salamander33()
    with pytest.raises(ValueError, match='fp16'):
        Simulation.from_sdf(SimulationOptions(timestep=m.timestep, n_iterations=2), AnimatOptions.from_model(m), ArenaOptions(),
                            model=m, n_envs=2, precision='fp16')


@pytest.mark.skipif(shutil.which('hipcc') is None, reason='hipcc not on PATH')
def test_fp64_kernel_compiles_without_scratch(tmp_path):
    """The fp64 translation unit with the flags of _lib.build(): every fp64 step kernel keeps out of scratch (no private array is
    indexed at run time), spills no VGPR, and its LDS - the largest dynamic request of the size limits plus the static part the
    compiler reports - is within gfx950's 160 KB per workgroup."""
    res = resource_remarks('-DFMJ_TU_F64', tmp_path)
    f64 = {k: v for k, v in res.items() if 'f64' in k}
    assert f64 and all('fmj_step_wide_kernel' not in k for k in res), sorted(res)
    assert sorted(res) == sorted(f64), sorted(res)          # the translation unit holds nothing else
    # the kernel's dynamic LDS at the size limits: 128 bodies, 128 dofs (nq 129), rows of 64 doubles (ldsd_layout of fmj_f64.inc)
    within_resources(f64, lds_bytes('plain', 128, 128, 129, 64))
