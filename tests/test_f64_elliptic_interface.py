"""The elliptic cone on the fp64 contact solve (fmj_create_ex2 with FMJ_CREATE_F64_CONTACTS | FMJ_CREATE_F64_ELLIPTIC,
csrc/fmj_f64_step.inc compiled as fmj_step_f64_elliptic_kernel) as far as it can be checked without a GPU: the flag and what it leaves
alone, every acceptance and every refusal (decided before the device lookup), the Python arguments, and the compiler's resource remarks
for the two new kernels."""
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
from support_f64_contacts import CONTACTS, LIMITS, RK4
from support_f64_terrain import TERRAIN
import support_f64_elliptic as E
from support_f64_elliptic import ELLIPTIC

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _walker(**kw):
    import farms_mujoco_amd.model as mm
    m = mm.salamander33(contacts=True, **kw)
    m.cone = mm.CONES['elliptic']
    return m


def test_the_flag_is_512_and_the_abi_stays():
    L, lib = _lib()
    assert L.CREATE_F64_ELLIPTIC == 512 == ELLIPTIC and L.CREATE_F64_TERRAIN == 128 and L.CREATE_F64_CONTACTS == 32
    assert lib.fmj_abi_version() == 6 and L.ABI_VERSION == 6 and ctypes.sizeof(L.CCreateExt) == 8
    hdr = open(os.path.join(ROOT, 'include', 'fmj.h')).read()
    assert 'FMJ_CREATE_F64_ELLIPTIC = 512' in hdr and '#define FMJ_ABI_VERSION 6' in hdr
    for sentence in ('Bits 2 and 4', 'bit 16 is not assigned', 'bit 64 is not assigned', 'bit 256 is not assigned'):
        assert sentence in hdr, sentence


def test_argument_errors_come_before_the_device_lookup():
    m = _walker()
    for kw in (dict(flags=ELLIPTIC), dict(flags=ELLIPTIC, precision=F32), dict(flags=ELLIPTIC | CONTACTS, precision=F32), dict(flags=ELLIPTIC | LIMITS),
               dict(flags=ELLIPTIC | TERRAIN)):
        rc, msg, _, _ = _create_ex2(m, **kw)
        assert rc == FMJ_ERR_ARG and 'FMJ_CREATE_F64_' in msg, (kw, rc, msg)
        if kw.get('precision') != F32 or kw['flags'] == ELLIPTIC:
            assert 'FMJ_CREATE_F64_CONTACTS' in msg and 'FMJ_PRECISION_F64' in msg, (kw, msg)
            if not kw['flags'] & TERRAIN:      # (the terrain flag's own sentence comes first)
                assert 'FMJ_CREATE_F64_ELLIPTIC' in msg, (kw, msg)
    for flags in (2, 64, 256, CONTACTS | ELLIPTIC | 2, CONTACTS | ELLIPTIC | 64, CONTACTS | ELLIPTIC | 256, CONTACTS | ELLIPTIC | 1024):
        rc, msg, _, _ = _create_ex2(m, flags=flags)
        assert rc == FMJ_ERR_ARG and msg == 'fmj_create_ex2: unknown bits in fmj_create_ext.flags', (flags, rc, msg)


def test_elliptic_models_are_accepted_with_the_flag_and_refused_without_it():
    import farms_mujoco_amd.model as mm
    m = _walker()
    rc, msg, prec, _ = _create_ex2(m, flags=CONTACTS | ELLIPTIC)
    assert _accepted(rc, msg, prec), (rc, msg)
    for flags in (CONTACTS, CONTACTS | TERRAIN):      # today's refusal, verbatim
        rc, msg, _, _ = _create_ex2(m, flags=flags)
        assert rc == FMJ_ERR_UNSUPPORTED and msg == 'fmj_create_ex2: the fp64 contact solve (FMJ_CREATE_F64_CONTACTS) has no elliptic cone (pyramidal only)', (rc, msg)
    m = _walker(limits=True)      # a limited model needs LIMITS too, as under the pyramid
    rc, msg, _, _ = _create_ex2(m, flags=CONTACTS | ELLIPTIC)
    assert rc == FMJ_ERR_UNSUPPORTED and 'fp64' in msg and 'limit' in msg, (rc, msg)
    rc, msg, prec, _ = _create_ex2(m, flags=CONTACTS | ELLIPTIC | LIMITS)
    assert _accepted(rc, msg, prec), (rc, msg)
    cases = [(n, False, 1.0) for n in E.ONE_STEP] + list(E.FURTHER) + [('centipede_hfield', False, 1.0)]      # the GPU tests' models
    for name, friction0, impratio in cases:
        for integrator in ('euler', 'implicitfast'):
            m = E.make(name, integrator, friction0=friction0, impratio=impratio)
            rc, msg, prec, _ = _create_ex2(m, flags=E.flags_of(name, m))
            assert _accepted(rc, msg, prec), (name, rc, msg)
    pyr = mm.centipede(20, 25, contacts=True)      # a pyramidal model under the flag: what the context may take, not what it must
    rc, msg, prec, _ = _create_ex2(pyr, flags=CONTACTS | ELLIPTIC)
    assert _accepted(rc, msg, prec), (rc, msg)


LOW_FRICTION = ('fmj_create_ex2: the fp64 contact solve (FMJ_CREATE_F64_CONTACTS) has no primal solve for a ground contact whose friction / sqrt(impratio) can '
                'fall below 1e-3 (rows too stiff for it: the fp32 constraint path solves such a model on the dual problem)')


def test_low_friction_feet_are_accepted_under_the_elliptic_cone_only():
    import farms_mujoco_amd.model as mm
    m = mm.centipede(20, 25, contacts=True)
    m.geom_friction = np.zeros_like(m.geom_friction)      # friction 1e-5 after the clamp
    for flags in (CONTACTS, CONTACTS | ELLIPTIC):         # pyramidal: refused with today's words, flag or not
        rc, msg, _, _ = _create_ex2(m, flags=flags)
        assert rc == FMJ_ERR_UNSUPPORTED and msg == LOW_FRICTION, (flags, rc, msg)
    m.cone = mm.CONES['elliptic']
    rc, msg, prec, _ = _create_ex2(m, flags=CONTACTS | ELLIPTIC)
    assert _accepted(rc, msg, prec), (rc, msg)
    m.impratio = 1e-4      # mu = friction / sqrt(impratio) is no part of the elliptic rule either
    rc, msg, prec, _ = _create_ex2(m, flags=CONTACTS | ELLIPTIC)
    assert _accepted(rc, msg, prec), (rc, msg)


def _refused(m, *words, flags=CONTACTS | ELLIPTIC):
    """Refused with the flag, in the words a pyramidal twin of the model is refused with when the flag is absent."""
    import copy
    import farms_mujoco_amd.model as mm
    rc, msg, _, _ = _create_ex2(m, flags=flags)
    assert rc == FMJ_ERR_UNSUPPORTED and 'fp64' in msg and all(w in msg for w in words), (words, rc, msg)
    twin = copy.copy(m); twin.cone = mm.CONES['pyramidal']
    rc0, msg0, _, _ = _create_ex2(twin, flags=flags & ~ELLIPTIC)
    assert rc0 == rc and msg0 == msg, (msg0, msg)
    return msg


def test_what_stays_out_of_scope_is_refused_with_todays_words():
    import farms_mujoco_amd.model as mm
    _refused(_walker(mesh_feet=True), 'mesh')
    _refused(_walker(self_collisions=True), 'pair')
    m = _walker(); m.noslip_iterations = 3
    _refused(m, 'noslip')
    m = _walker(); m.integrator = mm.INTEGRATORS['rk4']
    _refused(m, 'RK4')
    _refused(m, 'RK4', flags=CONTACTS | ELLIPTIC | RK4)
    m = _walker(); m.max_contacts = 129
    _refused(m, 'max_contacts', '128')
    _refused(_walker(terrain='hfield'), 'heightfield')      # a heightfield without the terrain flag
    rc, msg, prec, _ = _create_ex2(_walker(terrain='hfield'), flags=CONTACTS | ELLIPTIC | TERRAIN)
    assert _accepted(rc, msg, prec), (rc, msg)
    cyl = _walker()
    cyl.geom_type = np.where(cyl.geom_type == 2, 5, cyl.geom_type).astype(np.int32)      # spheres -> cylinders
    _refused(cyl, 'cylinder')


def test_a_fused_launch_stays_refused_in_the_library_text():
    """fmj_step_fused_f64 refuses every contacts family through one table entry: the elliptic row has no fused builds."""
    src = open(SRC).read()
    row = re.search(r'\{fmj_tu_f64_elliptic, (\w+), (\w+),', src)
    assert row and row.groups() == ('false', 'true'), row
    assert 'FMJ_CREATE_F64_ELLIPTIC, FMJ_CREATE_F64_CONTACTS,' in src      # its row of f64_flags[]


def test_the_lds_is_the_terrain_contexts():
    """nbody = nv = 128 with a dof chain of 64: 120 contacts fit, 121 are refused with the bytes named (ldsd_terrain_bytes)."""
    import farms_mujoco_amd.model as mm
    from wide_trees import shape_tree
    from support_f64_contacts import GEOM_PLANE, GEOM_SPHERE, set_geoms
    unit = (1.0, 0.0, 0.0, 0.0)
    for max_contacts, fits in ((120, True), (121, False)):
        m = shape_tree(1)
        set_geoms(m, [(GEOM_PLANE, 0, (0, 0, 0), (0, 0, 0), unit, 0.0)] + [(GEOM_SPHERE, b, (0.02, 0, 0), (0, 0, 0), unit, 1.0) for b in range(1, 128)],
                  max_contacts)
        m.cone = mm.CONES['elliptic']
        need = lds_bytes('terrain', 128, 128, 129, 64, max_contacts)
        rc, msg, prec, _ = _create_ex2(m, flags=CONTACTS | ELLIPTIC)
        if fits:
            assert _accepted(rc, msg, prec), (rc, msg)
        else:
            assert rc == FMJ_ERR_UNSUPPORTED and 'FMJ_CREATE_F64_ELLIPTIC' in msg and str(need) in msg and 'LDS' in msg, (rc, msg, need)


def test_python_takes_fp64_elliptic():
    from farms_mujoco_amd.physics import BatchedPhysics, FP64_OPTIONS
    from farms_mujoco_amd.simulation.simulation import Simulation
    from farms_mujoco_amd.options import SimulationOptions, ArenaOptions, AnimatOptions
    from farms_mujoco_amd import _lib as L
    p = inspect.signature(BatchedPhysics.__init__).parameters
    assert 'fp64_elliptic' in p and p['fp64_elliptic'].default is False
    flag, needs, _, excludes = FP64_OPTIONS['fp64_elliptic']
    assert flag == L.CREATE_F64_ELLIPTIC and needs == ('fp64_contacts',) and excludes == FP64_OPTIONS['fp64_contacts'][3]
    assert list(FP64_OPTIONS)[-1] == 'fp64_elliptic'
    m = E.make('centipede_20_25')
    for kw in (dict(precision='fp32'), dict(), dict(precision='fp64'), dict(precision='fp32', fp64_contacts=True)):
        with pytest.raises(ValueError, match='fp64_elliptic|fp64_contacts'):      # before any device use: no GPU is needed to get here
            BatchedPhysics(m, 2, fp64_elliptic=True, **kw)
    with pytest.raises(ValueError, match='fp64_elliptic'):
        BatchedPhysics(m, 2, fp64_elliptic=True, precision='fp64')
    for other in ('fp64_fused', 'fp64_rk4'):
        with pytest.raises(ValueError, match='does not go with'):
            BatchedPhysics(m, 2, precision='fp64', fp64_contacts=True, fp64_elliptic=True, **{other: True})
    with pytest.raises(ValueError, match='fp64_elliptic'):
        Simulation(m, m.body_names[1], SimulationOptions(timestep=m.timestep, n_iterations=2), n_envs=2, precision='fp64', fp64_elliptic=True)
    with pytest.raises(ValueError, match='fp64_elliptic'):
        Simulation.from_sdf(SimulationOptions(timestep=m.timestep, n_iterations=2), AnimatOptions.from_model(m), ArenaOptions(),
                            model=m, n_envs=2, precision='fp64', fp64_elliptic=True)


@pytest.mark.skipif(shutil.which('hipcc') is None, reason='hipcc not on PATH')
def test_elliptic_kernels_compile_without_scratch(tmp_path):
    """The translation unit of the elliptic kernels (-DFMJ_TU_F64=6) with the flags of _lib.build() holds exactly two kernels,
    fmj_step_f64_elliptic_kernel<LIMITS>; both keep out of scratch, spill no VGPR, and their LDS at the largest model the create check
    admits (nbody = nv = 128, dof chain 64, 120 contacts: ldsd_terrain_bytes of fmj_f64.inc) is within 160 KB."""
    res = resource_remarks('-DFMJ_TU_F64=6', tmp_path)
    ck = {k: v for k, v in res.items() if re.search(r'fmj_step_f64_elliptic_kernelILb[01]EE', k)}
    assert len(res) == 2 and len(ck) == 2, sorted(res)
    from farms_mujoco_amd import _lib as L
    inc = open(os.path.join(os.path.dirname(SRC), 'fmj_f64.inc')).read()
    assert repr(BUILD_FLAGS)[:-1] in inspect.getsource(L.build) and "'-DFMJ_TU_F64=6'" in inspect.getsource(L.build)
    assert f'#define F64_CT {F64_CT} ' in inc and f'#define F64_TN {F64_TN} ' in inc      # the record keeps its stride
    listing = open(os.path.join(ROOT, 'scripts', 'device_listing.sh')).read()
    assert 'kf64e:-DFMJ_TU_F64=6' in listing and 'kf64t:-DFMJ_TU_F64=5' in listing
    dyn = lds_bytes('terrain', 128, 128, 129, 64, 120)
    assert dyn <= 160*1024 < lds_bytes('terrain', 128, 128, 129, 64, 121)
    within_resources(ck, dyn)
