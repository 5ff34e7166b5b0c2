"""RK4 on the fp64 contact solve (fmj_create_ex2 with FMJ_CREATE_F64_CONTACTS | FMJ_CREATE_F64_CONTACTS_RK4, csrc/fmj_f64_step.inc
compiled as fmj_step_f64_terrain_rk4_kernel / fmj_step_f64_elliptic_rk4_kernel) as far as it can be checked without a GPU: the flag and
what it leaves alone, every acceptance and every refusal (decided before the device lookup), the Python arguments, and the compiler's
resource remarks for the four new kernels."""
import ctypes
import inspect
import os
import re
import shutil

import numpy as np
import pytest

from support_capi import lib as _lib, F32, FMJ_ERR_ARG, FMJ_ERR_UNSUPPORTED
from support_f64_interface import create_ex2 as _create_ex2, accepted as _accepted, SRC, BUILD_FLAGS, lds_bytes, resource_remarks, within_resources
import support_f64_contacts_rk4 as R
from support_f64_contacts_rk4 import CONTACTS, LIMITS, RK4, TERRAIN, ELLIPTIC, CONTACTS_RK4

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MESH = 2048
NO = 'fmj_create_ex2: the fp64 contact solve (FMJ_CREATE_F64_CONTACTS) has no '
NO_RK4 = NO + 'RK4 (Euler or implicitfast only, also with FMJ_CREATE_F64_RK4)'


def _walker(integrator='rk4', **kw):
    import farms_mujoco_amd.model as mm
    m = mm.salamander33(contacts=True, **kw)
    m.integrator = mm.INTEGRATORS[integrator]
    return m


def test_the_flag_is_8192_and_the_abi_stays():
    L, lib = _lib()
    assert L.CREATE_F64_CONTACTS_RK4 == 8192 == CONTACTS_RK4 and L.CREATE_F64_MESH == 2048 and L.CREATE_F64_RK4 == 8
    assert lib.fmj_abi_version() == 6 and L.ABI_VERSION == 6 and ctypes.sizeof(L.CCreateExt) == 8
    hdr = open(os.path.join(ROOT, 'include', 'fmj.h')).read()
    assert 'FMJ_CREATE_F64_CONTACTS_RK4 = 8192' in hdr and '#define FMJ_ABI_VERSION 6' in hdr and 'bit 4096 is not assigned' in hdr


def test_argument_errors_come_before_the_device_lookup():
    m = _walker()
    for kw in (dict(flags=CONTACTS_RK4), dict(flags=CONTACTS_RK4, precision=F32), dict(flags=CONTACTS_RK4 | CONTACTS, precision=F32),
               dict(flags=CONTACTS_RK4 | RK4), dict(flags=CONTACTS_RK4 | LIMITS)):
        rc, msg, _, _ = _create_ex2(m, **kw)
        assert rc == FMJ_ERR_ARG and 'FMJ_CREATE_F64_' in msg, (kw, rc, msg)
        if kw.get('precision') != F32 or kw['flags'] == CONTACTS_RK4:
            assert 'FMJ_CREATE_F64_CONTACTS_RK4 needs FMJ_CREATE_F64_CONTACTS and precision = FMJ_PRECISION_F64' in msg, (kw, msg)
    for flags in (4096, 16384, CONTACTS | CONTACTS_RK4 | 4096, CONTACTS | CONTACTS_RK4 | 2, CONTACTS | CONTACTS_RK4 | 1024, CONTACTS | CONTACTS_RK4 | 16384):
        rc, msg, _, _ = _create_ex2(m, flags=flags)
        assert rc == FMJ_ERR_ARG and msg == 'fmj_create_ex2: unknown bits in fmj_create_ext.flags', (flags, rc, msg)


def test_rk4_walkers_are_accepted_with_the_flag():
    for case in R.CASES:      # the GPU tests' models: limits, past 64 dofs, heightfield + cylinders with TERRAIN, elliptic with ELLIPTIC
        m = R.make(case)
        rc, msg, prec, _ = _create_ex2(m, flags=R.flags_of(case, m))
        assert _accepted(rc, msg, prec), (case, rc, msg)
    m = R.make('centipede_20_25')
    assert m.nv > 64 and R.flags_of('centipede_20_25', m) == CONTACTS | CONTACTS_RK4
    rc, msg, prec, _ = _create_ex2(m, flags=CONTACTS | CONTACTS_RK4 | TERRAIN)      # planes under the terrain flag: the same family
    assert _accepted(rc, msg, prec), (rc, msg)
    m = R.make('salamander33')
    rc, msg, _, _ = _create_ex2(m, flags=CONTACTS | CONTACTS_RK4)      # a limited model needs LIMITS too, as under Euler
    assert rc == FMJ_ERR_UNSUPPORTED and 'fp64' in msg and 'limit' in msg, (rc, msg)
    for integrator in ('euler', 'implicitfast'):      # what the context may take, not what it must
        m = R.make('centipede_20_25', integrator)
        rc, msg, prec, _ = _create_ex2(m, flags=CONTACTS | CONTACTS_RK4)
        assert _accepted(rc, msg, prec), (integrator, rc, msg)


def test_without_the_flag_an_rk4_walker_is_refused_with_todays_words():
    for m, base in ((_walker(), CONTACTS), (_walker(limits=True), CONTACTS | LIMITS), (R.make('elliptic_salamander33'), CONTACTS | LIMITS | ELLIPTIC),
                    (R.make('salamander_hfield_cyl'), CONTACTS | LIMITS | TERRAIN)):
        for flags in (base, base | RK4):      # FMJ_CREATE_F64_RK4 neither implies the new flag nor stands in for it
            rc, msg, _, _ = _create_ex2(m, flags=flags)
            assert rc == FMJ_ERR_UNSUPPORTED and msg == NO_RK4, (flags, rc, msg)
    import farms_mujoco_amd.model as mm
    plain = mm.salamander33(); plain.integrator = mm.INTEGRATORS['rk4']      # no geoms: the new flag does not admit RK4 by itself
    rc, msg, _, _ = _create_ex2(plain, flags=CONTACTS | CONTACTS_RK4)
    assert rc == FMJ_ERR_UNSUPPORTED and msg == 'fmj_create_ex: the fp64 step integrates with Euler or implicitfast, not RK4', (rc, msg)
    rc, msg, prec, _ = _create_ex2(plain, flags=CONTACTS | CONTACTS_RK4 | RK4)
    assert _accepted(rc, msg, prec), (rc, msg)


def test_what_stays_out_of_scope_is_refused_by_name():
    F = CONTACTS | CONTACTS_RK4
    for flags in (F | MESH, F | MESH | TERRAIN):      # two more families, left out on purpose
        rc, msg, _, _ = _create_ex2(_walker(mesh_feet=True), flags=flags)
        assert rc == FMJ_ERR_UNSUPPORTED and msg.startswith(NO + 'RK4 with mesh geoms'), (rc, msg)
    rc, msg, _, _ = _create_ex2(_walker(mesh_feet=True), flags=F)
    assert rc == FMJ_ERR_UNSUPPORTED and msg == NO + 'mesh geoms', (rc, msg)
    rc, msg, _, _ = _create_ex2(_walker(self_collisions=True), flags=F)
    assert rc == FMJ_ERR_UNSUPPORTED and msg.startswith(NO + 'explicit contact pairs'), (rc, msg)
    m = _walker(); m.noslip_iterations = 3
    rc, msg, _, _ = _create_ex2(m, flags=F)
    assert rc == FMJ_ERR_UNSUPPORTED and msg.startswith(NO + 'noslip'), (rc, msg)
    rc, msg, _, _ = _create_ex2(_walker(terrain='hfield'), flags=F)
    assert rc == FMJ_ERR_UNSUPPORTED and msg == NO + 'heightfield geoms', (rc, msg)
    rc, msg, prec, _ = _create_ex2(_walker(terrain='hfield'), flags=F | TERRAIN)
    assert _accepted(rc, msg, prec), (rc, msg)
    cyl = _walker()
    cyl.geom_type = np.where(cyl.geom_type == 2, 5, cyl.geom_type).astype(np.int32)      # spheres -> cylinders
    rc, msg, _, _ = _create_ex2(cyl, flags=F)
    assert rc == FMJ_ERR_UNSUPPORTED and msg == NO + 'cylinder geoms', (rc, msg)
    low = R.make('centipede_20_25'); low.geom_friction = np.zeros_like(low.geom_friction)      # low-friction feet under the pyramid
    rc, msg, _, _ = _create_ex2(low, flags=F)
    assert rc == FMJ_ERR_UNSUPPORTED and msg.startswith(NO + 'primal solve for a ground contact whose friction'), (rc, msg)
    import farms_mujoco_amd.model as mm
    ell = _walker(); ell.cone = mm.CONES['elliptic']      # an elliptic model still needs its own flag
    rc, msg, _, _ = _create_ex2(ell, flags=F)
    assert rc == FMJ_ERR_UNSUPPORTED and msg == NO + 'elliptic cone (pyramidal only)', (rc, msg)


def test_a_fused_launch_stays_refused_in_the_library_text():
    """fmj_step_fused_f64 refuses every contacts family through one table entry (F64_NO_FUSED): the new rows have no fused builds, and
    their contexts run no stage launches."""
    src = open(SRC).read()
    for getter in ('fmj_tu_f64_terrain_rk4', 'fmj_tu_f64_elliptic_rk4'):
        row = re.search(r'\{%s, (\w+), (\w+),' % getter, src)
        assert row and row.groups() == ('false', 'true'), (getter, row)
    assert 'FMJ_CREATE_F64_CONTACTS_RK4, FMJ_CREATE_F64_CONTACTS,' in src      # its row of f64_flags[]
    assert 'if (fused && !fam.fused) return set_err(FMJ_ERR_UNSUPPORTED, F64_NO_FUSED);' in src
    assert 'c->rk4 = m->integrator == FMJ_INT_RK4 && !f64_rk4_inside(F.f64.family);' in src


def _corner(max_contacts):
    from wide_trees import shape_tree
    from support_f64_contacts import GEOM_PLANE, GEOM_SPHERE, set_geoms
    unit = (1.0, 0.0, 0.0, 0.0)
    m = shape_tree(1)
    set_geoms(m, [(GEOM_PLANE, 0, (0, 0, 0), (0, 0, 0), unit, 0.0)] + [(GEOM_SPHERE, b, (0.02, 0, 0), (0, 0, 0), unit, 1.0) for b in range(1, 128)], max_contacts)
    m.integrator = 1
    return m


def _rk4_lds(nb, nv, nq, rs, max_contacts, nu):
    """ldsd_terrain_bytes + F64_RK4_LDS_DOUBLES(nu) * 8 of csrc/fmj_f64.inc"""
    return lds_bytes('terrain', nb, nv, nq, rs, max_contacts) + 8*(2*nu + 12*128)


def test_the_lds_is_the_terrain_contexts_plus_the_stage_state():
    """nbody = nv = 128 with a dof chain of 64: the stage state takes 8 (2 nu + 1536) bytes past the contacts' normals, so fewer contacts
    fit than the terrain context's 120; the refusal names the bytes and the flags.  The corner tree has 219 actuators: its stage state is
    15 792 bytes and 65 contacts fit (163 744 bytes), held against fmj_create_ex2; with 128 actuators the same formula gives 14 336 bytes
    and 70 contacts (163 728 bytes)."""
    import farms_mujoco_amd.model as mm
    m = _corner(1)
    assert (m.nbody, m.nv, m.nq) == (128, 128, 129)
    fits = max(k for k in range(1, 129) if _rk4_lds(128, 128, 129, 64, k, m.nu) <= 160*1024)
    print('nu', m.nu, 'contacts that fit', fits, 'bytes', _rk4_lds(128, 128, 129, 64, fits, m.nu))
    assert m.nu == 219 and 8*(2*m.nu + 12*128) == 15792 and fits == 65 and _rk4_lds(128, 128, 129, 64, 65, 219) == 163744
    assert _rk4_lds(128, 128, 129, 64, 66, 219) == 164032 > 160*1024
    assert 8*(2*128 + 12*128) == 14336 and _rk4_lds(128, 128, 129, 64, 70, 128) == 163728 <= 160*1024 < _rk4_lds(128, 128, 129, 64, 71, 128) == 164016
    for cone, flags, name in (('pyramidal', CONTACTS | CONTACTS_RK4, 'FMJ_CREATE_F64_CONTACTS | FMJ_CREATE_F64_CONTACTS_RK4)'),
                              ('elliptic', CONTACTS | CONTACTS_RK4 | ELLIPTIC, 'FMJ_CREATE_F64_CONTACTS | FMJ_CREATE_F64_CONTACTS_RK4 | FMJ_CREATE_F64_ELLIPTIC)')):
        for max_contacts, ok in ((fits, True), (fits + 1, False)):
            m = _corner(max_contacts); m.cone = mm.CONES[cone]
            rc, msg, prec, _ = _create_ex2(m, flags=flags)
            if ok:
                assert _accepted(rc, msg, prec), (rc, msg)
            else:
                need = _rk4_lds(128, 128, 129, 64, max_contacts, m.nu)
                assert rc == FMJ_ERR_UNSUPPORTED and name in msg and f'needs {need} bytes of LDS' in msg and 'above 160 KB' in msg, (rc, msg, need)
    m = R.make('centipede_20_25')      # the walker past 64 dofs with its 92 contacts
    from wide_trees import dof_depth
    rs = (int(max(dof_depth(m))) + 1 + 3) & ~3
    need = _rk4_lds(m.nbody, m.nv, m.nq, rs, m.max_contacts, m.nu)
    print('centipede(20, 25): max_contacts', m.max_contacts, 'row length', rs, 'LDS bytes', need)
    assert m.max_contacts == 92 and (m.nu, rs) == (105, 32) and need == 125312


def test_python_takes_fp64_contacts_rk4():
    from farms_mujoco_amd.physics import BatchedPhysics, FP64_OPTIONS
    from farms_mujoco_amd.simulation.simulation import Simulation
    from farms_mujoco_amd.options import SimulationOptions, ArenaOptions, AnimatOptions
    from farms_mujoco_amd import _lib as L
    p = inspect.signature(BatchedPhysics.__init__).parameters
    assert 'fp64_contacts_rk4' in p and p['fp64_contacts_rk4'].default is False
    flag, needs, _, excludes = FP64_OPTIONS['fp64_contacts_rk4']
    assert flag == L.CREATE_F64_CONTACTS_RK4 and needs == ('fp64_contacts',) and excludes == FP64_OPTIONS['fp64_contacts'][3] and 'fp64_fused' in excludes
    m = R.make('centipede_20_25')
    for kw in (dict(precision='fp32'), dict(), dict(precision='fp64'), dict(precision='fp32', fp64_contacts=True)):
        with pytest.raises(ValueError, match='fp64_contacts_rk4|fp64_contacts'):      # before any device use: no GPU is needed to get here
            BatchedPhysics(m, 2, fp64_contacts_rk4=True, **kw)
    with pytest.raises(ValueError, match='fp64_contacts_rk4=True needs'):
        BatchedPhysics(m, 2, fp64_contacts_rk4=True, precision='fp64')
    for other in ('fp64_fused', 'fp64_rk4'):      # fp64_rk4 with fp64_contacts stays an error, with or without the new keyword
        with pytest.raises(ValueError, match='does not go with'):
            BatchedPhysics(m, 2, precision='fp64', fp64_contacts=True, fp64_contacts_rk4=True, **{other: True})
    with pytest.raises(ValueError, match='fp64_contacts=True does not go with fp64_rk4=True'):
        BatchedPhysics(m, 2, precision='fp64', fp64_contacts=True, fp64_rk4=True)
    opts = SimulationOptions(timestep=m.timestep, n_iterations=2, integrator='RK4')      # check_supported_options lets RK4 through
    with pytest.raises(ValueError, match='fp64_contacts_rk4'):
        Simulation(m, m.body_names[1], opts, n_envs=2, precision='fp64', fp64_contacts_rk4=True)
    with pytest.raises(ValueError, match='fp64_contacts_rk4'):
        Simulation.from_sdf(opts, AnimatOptions.from_model(m), ArenaOptions(), model=m, n_envs=2, precision='fp64', fp64_contacts_rk4=True)


@pytest.mark.skipif(shutil.which('hipcc') is None, reason='hipcc not on PATH')
@pytest.mark.parametrize('unit,kernel', [(9, 'fmj_step_f64_terrain_rk4_kernel'), (10, 'fmj_step_f64_elliptic_rk4_kernel')])
def test_contact_rk4_kernels_compile_without_scratch(tmp_path, unit, kernel):
    """The translation units of the new kernels (-DFMJ_TU_F64=9 and =10) with the flags of _lib.build() hold exactly two kernels each,
    <LIMITS> false and true; all keep out of scratch, spill no VGPR, and their LDS at the largest model the create check admits
    (nbody = nv = nu = 128, dof chain 64, 70 contacts) is within 160 KB."""
    res = resource_remarks(f'-DFMJ_TU_F64={unit}', tmp_path)
    ck = {k: v for k, v in res.items() if re.search(kernel + r'ILb[01]EE', k)}
    assert len(res) == 2 and len(ck) == 2, sorted(res)
    print({k: (v['VGPRs'], v['SGPRs Spill']) for k, v in ck.items()})
    from farms_mujoco_amd import _lib as L
    assert repr(BUILD_FLAGS)[:-1] in inspect.getsource(L.build) and f"'-DFMJ_TU_F64={unit}'" in inspect.getsource(L.build)
    listing = open(os.path.join(ROOT, 'scripts', 'device_listing.sh')).read()
    assert 'kf64tr:-DFMJ_TU_F64=9' in listing and 'kf64er:-DFMJ_TU_F64=10' in listing
    dyn = _rk4_lds(128, 128, 129, 64, 70, 128)
    assert dyn <= 160*1024 < _rk4_lds(128, 128, 129, 64, 71, 128)
    within_resources(ck, dyn)
