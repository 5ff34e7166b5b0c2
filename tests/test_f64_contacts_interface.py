"""Ground contacts on the fp64 step (fmj_create_ex2 with FMJ_CREATE_F64_CONTACTS, csrc/fmj_f64_step.inc compiled as
fmj_step_f64_contacts_kernel) as far as it can be checked without a GPU: the flag and what it leaves alone, every acceptance and every
refusal (decided before the device lookup), the Python arguments, the centipede's walking variant, and the compiler's resource remarks
for the two new kernels."""
import ctypes
import inspect
import os
import re
import shutil

import numpy as np
import pytest

from support_capi import lib as _lib, create_ex as _create_ex, F32, FMJ_ERR_ARG, FMJ_ERR_UNSUPPORTED
from support_f64_interface import create_ex2 as _create_ex2, accepted as _accepted, SRC, F64_CT, lds_bytes, resource_remarks, within_resources
from support_f64_contacts import CONTACTS, LIMITS, RK4, GEOM_PLANE, make, boxfoot, set_geoms

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _walker():
    from farms_mujoco_amd.model import salamander33
    return salamander33(contacts=True)


def test_the_flag_is_32_and_the_abi_stays():
    L, lib = _lib()
    assert L.CREATE_F64_CONTACTS == 32 and L.CREATE_F64_RK4 == 8 and L.CREATE_F64_LIMITS == 1
    assert lib.fmj_abi_version() == 6 and L.ABI_VERSION == 6 and ctypes.sizeof(L.CCreateExt) == 8
    hdr = open(os.path.join(ROOT, 'include', 'fmj.h')).read()
    assert 'FMJ_CREATE_F64_CONTACTS = 32' in hdr and '#define FMJ_ABI_VERSION 6' in hdr and 'Bits 2 and 4' in hdr


@pytest.mark.parametrize('integrator', ['euler', 'implicitfast'])
def test_walking_models_pass_every_model_check(integrator):
    for name in ('salamander33', 'centipede_20_25', 'boxfoot6'):
        m = make(name, integrator)
        flags = CONTACTS | (LIMITS if np.any(m.jnt_limited) else 0)
        rc, msg, prec, solver = _create_ex2(m, flags=flags)
        assert _accepted(rc, msg, prec), (name, rc, msg)
    m = make('centipede_20_25')
    assert m.nbody == 107 and m.nv == 111      # past every other path's 64
    rc, msg, _ = _create_ex(m, precision=F32)
    assert rc == FMJ_ERR_UNSUPPORTED, (rc, msg)


def test_a_limited_walker_needs_both_flags():
    m = make('salamander33')
    rc, msg, _, _ = _create_ex2(m, flags=CONTACTS)
    assert rc == FMJ_ERR_UNSUPPORTED and 'fp64' in msg and 'limit' in msg, (rc, msg)
    rc, msg, _, _ = _create_ex2(m, flags=LIMITS)
    assert rc == FMJ_ERR_UNSUPPORTED and 'fp64' in msg and 'contact' in msg, (rc, msg)
    rc, msg, prec, _ = _create_ex2(m, flags=LIMITS | CONTACTS)
    assert _accepted(rc, msg, prec), (rc, msg)


def test_argument_errors_come_before_the_device_lookup():
    m = _walker()
    rc, msg, _, _ = _create_ex2(m, precision=F32, flags=CONTACTS)
    assert rc == FMJ_ERR_ARG and 'FMJ_CREATE_F64_CONTACTS' in msg and 'FMJ_PRECISION_F64' in msg, (rc, msg)
    for flags in (2, 4, 16, CONTACTS | 2, CONTACTS | 4, CONTACTS | 16, 64):
        rc, msg, _, _ = _create_ex2(m, flags=flags)
        assert rc == FMJ_ERR_ARG and 'flags' in msg, (flags, rc, msg)


def _refused(m, *words, flags=CONTACTS):
    rc, msg, _, _ = _create_ex2(m, flags=flags)
    assert rc == FMJ_ERR_UNSUPPORTED and 'fp64' in msg and all(w in msg for w in words), (words, rc, msg)
    return msg


def test_what_the_contact_solve_does_not_take_is_refused_by_name():
    import farms_mujoco_amd.model as mm
    _refused(mm.salamander33(contacts=True, self_collisions=True), 'pair')
    _refused(mm.salamander33(contacts=True, terrain='hfield'), 'heightfield')
    _refused(mm.salamander33(contacts=True, mesh_feet=True), 'mesh')
    m = _walker(); m.geom_type = np.where(m.geom_type == 2, 5, m.geom_type).astype(np.int32)      # spheres -> cylinders
    _refused(m, 'cylinder')
    m = _walker(); m.cone = mm.CONES['elliptic']
    _refused(m, 'elliptic')
    m = _walker(); m.noslip_iterations = 3
    _refused(m, 'noslip')
    m = _walker(); m.integrator = mm.INTEGRATORS['rk4']
    _refused(m, 'RK4')
    _refused(m, 'RK4', flags=CONTACTS | RK4)
    m = _walker(); m.max_contacts = 129
    _refused(m, 'max_contacts', '128')
    m = _walker(); m.geom_friction = np.zeros_like(m.geom_friction)      # friction 1e-5 after the clamp: below 1e-3
    _refused(m, 'friction', '1e-3')
    m = _walker(); m.impratio = 4e6                                      # 1 / sqrt(impratio) = 5e-4
    _refused(m, 'friction', '1e-3')


def test_the_lds_corner():
    """nbody = nv = 128 with a dof chain of 64 and 128 contacts is within 160 KB; a map past it is refused with its bytes named."""
    from wide_trees import shape_tree
    m = shape_tree(1)
    assert (m.nbody, m.nv, m.nq) == (128, 128, 129)
    unit = (1.0, 0.0, 0.0, 0.0)
    geoms = [(GEOM_PLANE, 0, (0, 0, 0), (0, 0, 0), unit, 0.0)] + [(2, b, (0.02, 0, 0), (0, 0, 0), unit, 1.0) for b in range(1, 128)]
    set_geoms(m, geoms, 128)
    need = lds_bytes('contacts', 128, 128, 129, 64, 128)
    assert need <= 160*1024, need
    rc, msg, prec, _ = _create_ex2(m, flags=CONTACTS)
    assert _accepted(rc, msg, prec), (rc, msg)
    assert lds_bytes('contacts', 107, 111, 112, 36, 92) <= 160*1024      # centipede(20, 25, contacts=True)


def test_without_the_flag_the_refusals_stay_word_for_word():
    import farms_mujoco_amd.model as mm
    for m, what in ((_walker(), 'contact geoms'), (mm.salamander33(contacts=True, self_collisions=True), 'explicit contact pairs'),
                    (mm.salamander33(contacts=True, limits=True), 'joint limits')):
        want = 'fmj_create_ex: the fp64 step has no constraint solver: the model has ' + what
        rc, msg, _ = _create_ex(m)
        assert rc == FMJ_ERR_UNSUPPORTED and msg == want, (rc, msg)
        for kw in (dict(flags=0), dict(ext=False), dict(flags=RK4)):
            rc, msg2, _, _ = _create_ex2(m, **kw)
            assert rc == FMJ_ERR_UNSUPPORTED and msg2 == want, (kw, rc, msg2)
    rc, msg, _, _ = _create_ex2(_walker(), flags=LIMITS)
    assert rc == FMJ_ERR_UNSUPPORTED and msg == 'fmj_create_ex: the fp64 step has no constraint solver: the model has contact geoms', (rc, msg)


def test_python_takes_fp64_contacts():
    from farms_mujoco_amd.physics import BatchedPhysics
    from farms_mujoco_amd.simulation.simulation import Simulation
    from farms_mujoco_amd.options import SimulationOptions, ArenaOptions, AnimatOptions
    p = inspect.signature(BatchedPhysics.__init__).parameters
    assert 'fp64_contacts' in p and p['fp64_contacts'].default is False
    m = _walker()
    for kw in (dict(precision='fp32'), dict(), dict(precision='fp64', fp64_fused=True), dict(precision='fp64', fp64_rk4=True)):
        with pytest.raises(ValueError, match='fp64_contacts'):      # before any device use: no GPU is needed to get here
            BatchedPhysics(m, 2, fp64_contacts=True, **kw)
    with pytest.raises(ValueError, match='fp64_contacts'):
        Simulation(m, m.body_names[1], SimulationOptions(timestep=m.timestep, n_iterations=2), n_envs=2, fp64_contacts=True)
    with pytest.raises(ValueError, match='fp64_contacts'):
        Simulation.from_sdf(SimulationOptions(timestep=m.timestep, n_iterations=2), AnimatOptions.from_model(m), ArenaOptions(),
                            model=m, n_envs=2, fp64_contacts=True)


def test_the_swimming_centipede_is_what_it_was():
    from farms_mujoco_amd.model import centipede, centipede_touch_height
    a, b = centipede(20, 25), centipede(20, 25, contacts=False)
    assert sorted(vars(a)) == sorted(vars(b))
    for k, v in vars(a).items():
        w = vars(b)[k]
        if isinstance(v, np.ndarray):
            assert v.dtype == w.dtype and v.tobytes() == w.tobytes(), k
        elif not isinstance(v, (list, dict)):
            assert v == w or (v is None and w is None), k
    assert a.ngeom == 0 and a.max_contacts == 0
    w = centipede(20, 25, contacts=True)
    assert (w.nbody, w.nv) == (a.nbody, a.nv) and w.ngeom == 1 + 26 + 40 and w.max_contacts == 2*26 + 40 <= 96
    assert w.geom_type[0] == GEOM_PLANE and np.all(w.geom_friction[0] == 0) and np.all(w.geom_friction[1:, 0] == 1.0)
    assert abs(w.key_qpos[2] - (centipede_touch_height() - 2e-4)) < 1e-15      # the feet touch: 0.2 mm into the ground
    from support_f64_contacts import lowest_point
    assert abs(lowest_point(w, w.key_qpos) + 2e-4) < 1e-12


@pytest.mark.skipif(shutil.which('hipcc') is None, reason='hipcc not on PATH')
def test_contacts_kernels_compile_without_scratch(tmp_path):
    """The translation unit of the contacts kernels (-DFMJ_TU_F64=4) with the flags of _lib.build() holds exactly two kernels,
    fmj_step_f64_contacts_kernel<LIMITS>; both keep out of scratch, spill no VGPR, and their LDS at the size limits (nbody = nv = 128,
    dof chain 64, 128 contacts: ldsd_contacts_bytes of fmj_f64.inc) is within 160 KB."""
    res = resource_remarks('-DFMJ_TU_F64=4', tmp_path)
    ck = {k: v for k, v in res.items() if re.search(r'fmj_step_f64_contacts_kernelILb[01]EE', k)}
    assert len(res) == 2 and len(ck) == 2, sorted(res)
    from farms_mujoco_amd import _lib as L
    inc = open(os.path.join(os.path.dirname(SRC), 'fmj_f64.inc')).read()
    assert "'-DFMJ_TU_F64=4'" in inspect.getsource(L.build) and f'#define F64_CT {F64_CT} ' in inc and 'F64_LIMITS_LDS_DOUBLES 20' in inc
    within_resources(ck, lds_bytes('contacts', 128, 128, 129, 64, 128))
