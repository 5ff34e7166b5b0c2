"""Heightfield ground and cylinder geoms on the fp64 contact solve (fmj_create_ex2 with FMJ_CREATE_F64_CONTACTS |
FMJ_CREATE_F64_TERRAIN, csrc/fmj_f64_step.inc compiled as fmj_step_f64_terrain_kernel) as far as it can be checked without a GPU: the
flag and what it leaves alone, every acceptance and every refusal (decided before the device lookup), the Python arguments, the
centipede's terrain keyword, and the compiler's resource remarks for the two new kernels."""
import ctypes
import inspect
import os
import re
import shutil

import numpy as np
import pytest

from support_capi import lib as _lib, F32, FMJ_ERR_ARG, FMJ_ERR_UNSUPPORTED
from support_f64_interface import (create_ex2 as _create_ex2, accepted as _accepted, SRC, BUILD_FLAGS, F64_CT, F64_TN, lds_bytes, resource_remarks,
                                   within_resources)
from support_f64_contacts import CONTACTS, LIMITS, RK4, GEOM_PLANE, GEOM_SPHERE, set_geoms
from support_f64_terrain import TERRAIN, GEOM_CYLINDER, GEOM_HFIELD, make, flags_of

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _three():
    """The models a contacts context refuses and a terrain context takes, with the word of today's refusal."""
    import farms_mujoco_amd.model as mm
    cyl = mm.salamander33(contacts=True)
    cyl.geom_type = np.where(cyl.geom_type == GEOM_SPHERE, GEOM_CYLINDER, cyl.geom_type).astype(np.int32)      # spheres -> cylinders
    return ((mm.salamander33(contacts=True, terrain='hfield'), 'heightfield'), (cyl, 'cylinder'),
            (mm.centipede(20, 25, contacts=True, terrain='hfield'), 'heightfield'))


def test_the_flag_is_128_and_the_abi_stays():
    L, lib = _lib()
    assert L.CREATE_F64_TERRAIN == 128 == TERRAIN and L.CREATE_F64_CONTACTS == 32
    assert lib.fmj_abi_version() == 6 and L.ABI_VERSION == 6 and ctypes.sizeof(L.CCreateExt) == 8
    hdr = open(os.path.join(ROOT, 'include', 'fmj.h')).read()
    assert 'FMJ_CREATE_F64_TERRAIN = 128' in hdr and '#define FMJ_ABI_VERSION 6' in hdr and 'bit 64 is not assigned' in hdr


def test_argument_errors_come_before_the_device_lookup():
    m = _three()[0][0]
    for kw in (dict(flags=TERRAIN), dict(flags=TERRAIN, precision=F32), dict(flags=TERRAIN | CONTACTS, precision=F32), dict(flags=TERRAIN | LIMITS)):
        rc, msg, _, _ = _create_ex2(m, **kw)
        assert rc == FMJ_ERR_ARG and 'FMJ_CREATE_F64_' in msg, (kw, rc, msg)
        if kw.get('precision') != F32 or kw['flags'] == TERRAIN:
            assert 'FMJ_CREATE_F64_TERRAIN' in msg and 'FMJ_CREATE_F64_CONTACTS' in msg and 'FMJ_PRECISION_F64' in msg, (kw, msg)
    for flags in (CONTACTS | TERRAIN | 64, 64, TERRAIN | 64, CONTACTS | TERRAIN | 2, CONTACTS | TERRAIN | 256):
        rc, msg, _, _ = _create_ex2(m, flags=flags)
        assert rc == FMJ_ERR_ARG and 'flags' in msg, (flags, rc, msg)


def test_terrain_models_pass_every_model_check_and_stay_refused_without_the_flag():
    for m, word in _three():
        limited = LIMITS if np.any(m.jnt_limited) else 0
        rc, msg, prec, _ = _create_ex2(m, flags=CONTACTS | TERRAIN | limited)
        assert _accepted(rc, msg, prec), (word, rc, msg)
        rc, msg, _, _ = _create_ex2(m, flags=CONTACTS | limited)
        assert rc == FMJ_ERR_UNSUPPORTED and 'fp64' in msg and 'FMJ_CREATE_F64_CONTACTS' in msg and word in msg, (word, rc, msg)
    import farms_mujoco_amd.model as mm
    m = mm.salamander33(contacts=True, limits=True, terrain='hfield')      # a limited model needs LIMITS too, as on flat ground
    rc, msg, _, _ = _create_ex2(m, flags=CONTACTS | TERRAIN)
    assert rc == FMJ_ERR_UNSUPPORTED and 'fp64' in msg and 'limit' in msg, (rc, msg)
    rc, msg, prec, _ = _create_ex2(m, flags=CONTACTS | TERRAIN | LIMITS)
    assert _accepted(rc, msg, prec), (rc, msg)
    for name in ('salamander_hfield_cyl', 'centipede_hfield_cyl', 'boxfoot_hfield', 'salamander_tilted_cyl'):      # the GPU tests' models
        for integrator in ('euler', 'implicitfast'):
            m = make(name, integrator)
            rc, msg, prec, _ = _create_ex2(m, flags=flags_of(m))
            assert _accepted(rc, msg, prec), (name, rc, msg)
    rc, msg, prec, _ = _create_ex2(mm.centipede(20, 25, contacts=True), flags=CONTACTS | TERRAIN)      # flat ground under the flag
    assert _accepted(rc, msg, prec), (rc, msg)


def _refused(m, *words, flags=CONTACTS | TERRAIN):
    rc, msg, _, _ = _create_ex2(m, flags=flags)
    assert rc == FMJ_ERR_UNSUPPORTED and 'fp64' in msg and all(w in msg for w in words), (words, rc, msg)
    rc0, msg0, _, _ = _create_ex2(m, flags=flags & ~TERRAIN)      # the same words as without the flag
    assert rc0 == rc and msg0 == msg, (msg0, msg)
    return msg


def test_what_stays_out_of_scope_is_refused_by_name_with_the_flag_set():
    import farms_mujoco_amd.model as mm
    walker = lambda: mm.salamander33(contacts=True)
    _refused(mm.salamander33(contacts=True, mesh_feet=True), 'mesh')
    _refused(mm.salamander33(contacts=True, self_collisions=True), 'pair')
    m = walker(); m.cone = mm.CONES['elliptic']
    _refused(m, 'elliptic')
    m = walker(); m.noslip_iterations = 3
    _refused(m, 'noslip')
    m = walker(); m.integrator = mm.INTEGRATORS['rk4']
    _refused(m, 'RK4')
    _refused(m, 'RK4', flags=CONTACTS | TERRAIN | RK4)
    m = walker(); m.max_contacts = 129
    _refused(m, 'max_contacts', '128')
    m = walker(); m.geom_friction = np.zeros_like(m.geom_friction)      # friction 1e-5 after the clamp: below 1e-3
    _refused(m, 'friction', '1e-3')
    # a heightfield that is no ground: too few samples, no table, not on the world (fmj_create's own words, whatever the flags)
    for edit, word in ((lambda m: setattr(m, 'hfield_ncol', 1), 'nrow, ncol >= 2'), (lambda m: setattr(m, 'hfield_data', None), 'data'),
                       (lambda m: m.geom_bodyid.__setitem__(int(np.nonzero(m.geom_type == GEOM_HFIELD)[0][0]), 1), 'world')):
        m = mm.salamander33(contacts=True, terrain='hfield')
        m.geom_bodyid = m.geom_bodyid.copy()
        edit(m)
        rc, msg, _, _ = _create_ex2(m, flags=CONTACTS | TERRAIN)
        assert rc in (FMJ_ERR_ARG, FMJ_ERR_UNSUPPORTED) and 'heightfield' in msg and word in msg, (word, rc, msg)


def test_the_lds_corner_names_its_bytes():
    """nbody = nv = 128 with a dof chain of 64: the terrain kernels' map fits up to 120 contacts; 128 are refused with the bytes named,
    where the contacts kernels' map still fits."""
    from wide_trees import shape_tree
    unit = (1.0, 0.0, 0.0, 0.0)
    for max_contacts, fits in ((120, True), (121, False), (128, False)):
        m = shape_tree(1)
        assert (m.nbody, m.nv, m.nq) == (128, 128, 129)
        set_geoms(m, [(GEOM_PLANE, 0, (0, 0, 0), (0, 0, 0), unit, 0.0)] + [(GEOM_SPHERE, b, (0.02, 0, 0), (0, 0, 0), unit, 1.0) for b in range(1, 128)],
                  max_contacts)
        need = lds_bytes('terrain', 128, 128, 129, 64, max_contacts)
        assert (need <= 160*1024) == fits, (max_contacts, need)
        rc, msg, prec, _ = _create_ex2(m, flags=CONTACTS | TERRAIN)
        if fits:
            assert _accepted(rc, msg, prec), (rc, msg)
        else:
            assert rc == FMJ_ERR_UNSUPPORTED and 'FMJ_CREATE_F64_TERRAIN' in msg and str(need) in msg and 'LDS' in msg, (rc, msg, need)
            rc, msg, prec, _ = _create_ex2(m, flags=CONTACTS)
            assert _accepted(rc, msg, prec), (rc, msg)
    assert lds_bytes('terrain', 107, 111, 112, 36, 92) <= 160*1024      # centipede(20, 25, contacts=True, terrain='hfield')


def test_python_takes_fp64_terrain():
    from farms_mujoco_amd.physics import BatchedPhysics
    from farms_mujoco_amd.simulation.simulation import Simulation
    from farms_mujoco_amd.options import SimulationOptions, ArenaOptions, AnimatOptions
    p = inspect.signature(BatchedPhysics.__init__).parameters
    assert 'fp64_terrain' in p and p['fp64_terrain'].default is False
    m = _three()[2][0]
    for kw in (dict(precision='fp32'), dict(), dict(precision='fp64'), dict(precision='fp32', fp64_contacts=True)):
        with pytest.raises(ValueError, match='fp64_terrain|fp64_contacts'):      # before any device use: no GPU is needed to get here
            BatchedPhysics(m, 2, fp64_terrain=True, **kw)
    with pytest.raises(ValueError, match='fp64_terrain'):
        BatchedPhysics(m, 2, fp64_terrain=True, precision='fp64')
    with pytest.raises(ValueError, match='fp64_terrain'):
        Simulation(m, m.body_names[1], SimulationOptions(timestep=m.timestep, n_iterations=2), n_envs=2, precision='fp64', fp64_terrain=True)
    with pytest.raises(ValueError, match='fp64_terrain'):
        Simulation.from_sdf(SimulationOptions(timestep=m.timestep, n_iterations=2), AnimatOptions.from_model(m), ArenaOptions(),
                            model=m, n_envs=2, precision='fp64', fp64_terrain=True)


def _same(a, b):
    assert sorted(vars(a)) == sorted(vars(b))
    for k, v in vars(a).items():
        w = vars(b)[k]
        if isinstance(v, np.ndarray):
            assert v.dtype == w.dtype and v.tobytes() == w.tobytes(), k
        elif not isinstance(v, (list, dict)):
            assert v == w or (v is None and w is None), k


def test_the_default_centipede_is_what_it_was_and_the_terrain_one_stands_on_its_ground():
    from farms_mujoco_amd.model import centipede, centipede_touch_height, CENTIPEDE_HFIELD
    from support_f64_contacts import lowest_point
    from support_f64_terrain import lowest
    assert inspect.signature(centipede).parameters['terrain'].default == 'plane'
    _same(centipede(20, 25), centipede(20, 25, terrain='plane'))
    _same(centipede(20, 25, contacts=True), centipede(20, 25, contacts=True, terrain='plane'))
    _same(centipede(20, 25), centipede(20, 25, terrain='hfield'))      # no contacts, no ground
    w = centipede(20, 25, contacts=True)
    assert abs(w.key_qpos[2] - (centipede_touch_height() - 2e-4)) < 1e-15 and abs(lowest_point(w, w.key_qpos) + 2e-4) < 1e-12
    h = centipede(20, 25, contacts=True, terrain='hfield')
    assert (h.nbody, h.nv, h.ngeom, h.max_contacts) == (w.nbody, w.nv, w.ngeom, w.max_contacts)
    assert h.geom_type[0] == GEOM_HFIELD and np.all(h.geom_friction[0] == 0) and np.array_equal(h.geom_type[1:], w.geom_type[1:])
    assert (h.hfield_nrow, h.hfield_ncol) == (CENTIPEDE_HFIELD['n'],)*2 and h.hfield_size[0] == h.hfield_size[1] == CENTIPEDE_HFIELD['radius']
    elev = h.hfield_data*h.hfield_size[2]
    assert 0.8*CENTIPEDE_HFIELD['amplitude'] < elev.max() <= CENTIPEDE_HFIELD['amplitude'] and elev.min() >= -CENTIPEDE_HFIELD['amplitude']      # millimetres
    low = lowest(h, h.key_qpos)      # the feet touch: the foot on the highest ground 0.2 mm into it (along the normal: to 1e-7 m)
    assert abs(low + 2e-4) < 1e-6, low
    assert 0.78 + 0.1 < CENTIPEDE_HFIELD['radius']      # the animal is 0.78 m long: a walk of the tests' lengths stays on the patch


@pytest.mark.skipif(shutil.which('hipcc') is None, reason='hipcc not on PATH')
def test_terrain_kernels_compile_without_scratch(tmp_path):
    """The translation unit of the terrain kernels (-DFMJ_TU_F64=5) with the flags of _lib.build() holds exactly two kernels,
    fmj_step_f64_terrain_kernel<LIMITS>; both keep out of scratch, spill no VGPR, and their LDS at the largest model the create check
    admits (nbody = nv = 128, dof chain 64, 120 contacts: ldsd_terrain_bytes of fmj_f64.inc) is within 160 KB."""
    res = resource_remarks('-DFMJ_TU_F64=5', tmp_path)
    ck = {k: v for k, v in res.items() if re.search(r'fmj_step_f64_terrain_kernelILb[01]EE', k)}
    assert len(res) == 2 and len(ck) == 2, sorted(res)
    from farms_mujoco_amd import _lib as L
    inc = open(os.path.join(os.path.dirname(SRC), 'fmj_f64.inc')).read()
    assert repr(BUILD_FLAGS)[:-1] in inspect.getsource(L.build) and "'-DFMJ_TU_F64=5'" in inspect.getsource(L.build)
    assert f'#define F64_CT {F64_CT} ' in inc and f'#define F64_TN {F64_TN} ' in inc and 'F64_LIMITS_LDS_DOUBLES 20' in inc
    assert 'kf64t:-DFMJ_TU_F64=5' in open(os.path.join(ROOT, 'scripts', 'device_listing.sh')).read()
    dyn = lds_bytes('terrain', 128, 128, 129, 64, 120)
    assert dyn <= 160*1024 < lds_bytes('terrain', 128, 128, 129, 64, 121)
    within_resources(ck, dyn)
