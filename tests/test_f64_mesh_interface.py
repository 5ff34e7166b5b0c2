"""Convex mesh geoms on the fp64 contact solve (fmj_create_ex2 with FMJ_CREATE_F64_CONTACTS | FMJ_CREATE_F64_MESH, csrc/fmj_f64_step.inc
compiled as fmj_step_f64_mesh_kernel / fmj_step_f64_mesh_elliptic_kernel) as far as it can be checked without a GPU: the flag and what
it leaves alone, every acceptance and every refusal (decided before the device lookup), the Python arguments, and the compiler's
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
from support_f64_contacts import CONTACTS, LIMITS, RK4
from support_f64_terrain import TERRAIN
from support_f64_elliptic import ELLIPTIC
import support_f64_mesh as M
from support_f64_mesh import MESH

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NO_MESH = 'fmj_create_ex2: the fp64 contact solve (FMJ_CREATE_F64_CONTACTS) has no mesh geoms'
LOW_FRICTION = ('fmj_create_ex2: the fp64 contact solve (FMJ_CREATE_F64_CONTACTS) has no primal solve for a ground contact whose friction / sqrt(impratio) can '
                'fall below 1e-3 (rows too stiff for it: the fp32 constraint path solves such a model on the dual problem)')


def _walker(**kw):
    import farms_mujoco_amd.model as mm
    return mm.salamander33(contacts=True, mesh_feet=True, **kw)


def test_the_flag_is_2048_and_the_abi_stays():
    L, lib = _lib()
    assert L.CREATE_F64_MESH == 2048 == MESH and L.CREATE_F64_ELLIPTIC == 512 and L.CREATE_F64_TERRAIN == 128 and L.CREATE_F64_CONTACTS == 32
    assert lib.fmj_abi_version() == 6 and L.ABI_VERSION == 6 and ctypes.sizeof(L.CCreateExt) == 8
    hdr = open(os.path.join(ROOT, 'include', 'fmj.h')).read()
    assert 'FMJ_CREATE_F64_MESH = 2048' in hdr and '#define FMJ_ABI_VERSION 6' in hdr
    for sentence in ('bit 16 is not assigned', 'bit 64 is not assigned', 'bit 256 is not assigned', 'bit 1024 is not assigned'):
        assert sentence in hdr, sentence


def test_argument_errors_come_before_the_device_lookup():
    m = _walker()
    for flags in (1024, CONTACTS | MESH | 1024, CONTACTS | 1024, CONTACTS | MESH | 4096):
        rc, msg, _, _ = _create_ex2(m, flags=flags)
        assert rc == FMJ_ERR_ARG and msg == 'fmj_create_ex2: unknown bits in fmj_create_ext.flags', (flags, rc, msg)
    for kw in (dict(flags=MESH), dict(flags=MESH, precision=F32), dict(flags=MESH | LIMITS), dict(flags=MESH | CONTACTS, precision=F32)):
        rc, msg, _, _ = _create_ex2(m, **kw)
        assert rc == FMJ_ERR_ARG and 'FMJ_CREATE_F64_' in msg, (kw, rc, msg)
        if not (kw['flags'] & CONTACTS):      # (with CONTACTS and fp32 the contacts flag's own sentence comes first)
            assert 'FMJ_CREATE_F64_MESH' in msg and 'FMJ_CREATE_F64_CONTACTS' in msg and 'FMJ_PRECISION_F64' in msg, (kw, msg)


def test_mesh_models_are_accepted_with_the_flag_and_refused_without_it():
    import farms_mujoco_amd.model as mm
    for m, extra in ((_walker(), 0), (_walker(limits=True), LIMITS), (M.make('centipede_mesh'), 0)):
        for flags in (CONTACTS, CONTACTS | TERRAIN, CONTACTS | ELLIPTIC):      # today's refusal, verbatim
            rc, msg, _, _ = _create_ex2(m, flags=flags | extra)
            assert rc == FMJ_ERR_UNSUPPORTED and msg == NO_MESH, (flags, rc, msg)
        for flags in (CONTACTS | MESH, CONTACTS | MESH | TERRAIN, CONTACTS | MESH | ELLIPTIC | TERRAIN):
            rc, msg, prec, _ = _create_ex2(m, flags=flags | extra)
            assert _accepted(rc, msg, prec), (flags, rc, msg)
    for name in M.MODELS:      # the GPU tests' models
        for integrator in ('euler', 'implicitfast'):
            m = M.make(name, integrator)
            rc, msg, prec, _ = _create_ex2(m, flags=M.flags_of(m))
            assert _accepted(rc, msg, prec), (name, rc, msg)
    plain = mm.centipede(20, 25, contacts=True)      # a model without meshes under the flag: what the context may take, not what it must
    rc, msg, prec, _ = _create_ex2(plain, flags=CONTACTS | MESH)
    assert _accepted(rc, msg, prec), (rc, msg)


def _refused(m, *words, flags=CONTACTS | MESH):
    rc, msg, _, _ = _create_ex2(m, flags=flags)
    assert rc == FMJ_ERR_UNSUPPORTED and 'fp64' in msg and all(w in msg for w in words), (words, rc, msg)
    return msg


def test_what_stays_out_of_scope_is_refused_with_todays_words():
    import farms_mujoco_amd.model as mm
    pre = 'fmj_create_ex2: the fp64 contact solve (FMJ_CREATE_F64_CONTACTS) has no '
    assert _refused(_walker(self_collisions=True), 'pair') == pre + 'explicit contact pairs (their rows couple two chains: outside the tree-sparse pattern of M)'
    m = _walker(); m.noslip_iterations = 3
    assert _refused(m, 'noslip') == pre + 'noslip post-pass (noslip_iterations > 0)'
    m = _walker(); m.integrator = mm.INTEGRATORS['rk4']
    assert _refused(m, 'RK4') == pre + 'RK4 (Euler or implicitfast only, also with FMJ_CREATE_F64_RK4)'
    _refused(m, 'RK4', flags=CONTACTS | MESH | RK4)
    assert _refused(_walker(terrain='hfield'), 'heightfield') == pre + 'heightfield geoms'      # a heightfield without the terrain flag
    assert _refused(M.make('centipede_hfield_mixed'), 'heightfield') == pre + 'heightfield geoms'
    m = M.make('centipede_mesh_elliptic')      # an elliptic mesh model without the elliptic flag
    assert _refused(m, 'elliptic') == pre + 'elliptic cone (pyramidal only)'
    m.cone = mm.CONES['pyramidal']             # ... and its friction-0 feet under the pyramid, flag or not
    assert _refused(m, 'friction') == LOW_FRICTION
    assert _refused(m, 'friction', flags=CONTACTS | MESH | ELLIPTIC) == LOW_FRICTION


def test_the_families_have_no_fused_builds_in_the_library_text():
    src = open(SRC).read()
    for getter in ('fmj_tu_f64_mesh', 'fmj_tu_f64_mesh_elliptic'):
        row = re.search(r'\{%s, (\w+), (\w+),' % getter, src)
        assert row and row.groups() == ('false', 'true'), getter
    assert 'FMJ_CREATE_F64_MESH, FMJ_CREATE_F64_CONTACTS,' in src      # its row of f64_flags[]


def test_the_lds_is_the_terrain_contexts():
    """nbody = nv = 128 with a dof chain of 64 and a mesh geom on every body: 120 contacts fit, 121 are refused with the bytes named."""
    from wide_trees import shape_tree
    from support_f64_contacts import GEOM_PLANE, GEOM_SPHERE, set_geoms
    unit = (1.0, 0.0, 0.0, 0.0)
    tet = M.vertex_sets()['tetrahedron']
    for max_contacts, fits in ((120, True), (121, False)):
        m = shape_tree(1)
        set_geoms(m, [(GEOM_PLANE, 0, (0, 0, 0), (0, 0, 0), unit, 0.0)] + [(GEOM_SPHERE, b, (0.02, 0, 0), (0, 0, 0), unit, 1.0) for b in range(1, 128)],
                  max_contacts)
        M.meshes(m, range(1, 128), [tet]*127)
        need = lds_bytes('terrain', 128, 128, 129, 64, max_contacts)
        rc, msg, prec, _ = _create_ex2(m, flags=CONTACTS | MESH)
        if fits:
            assert _accepted(rc, msg, prec), (rc, msg)
        else:
            assert rc == FMJ_ERR_UNSUPPORTED and 'FMJ_CREATE_F64_MESH' in msg and str(need) in msg and 'LDS' in msg, (rc, msg, need)


def test_python_takes_fp64_mesh():
    from farms_mujoco_amd.physics import BatchedPhysics, FP64_OPTIONS
    from farms_mujoco_amd.simulation.simulation import Simulation
    from farms_mujoco_amd.options import SimulationOptions, ArenaOptions, AnimatOptions
    from farms_mujoco_amd import _lib as L
    p = inspect.signature(BatchedPhysics.__init__).parameters
    assert 'fp64_mesh' in p and p['fp64_mesh'].default is False
    flag, needs, _, excludes = FP64_OPTIONS['fp64_mesh']
    assert flag == L.CREATE_F64_MESH and needs == ('fp64_contacts',) and excludes == FP64_OPTIONS['fp64_contacts'][3]
    m = M.make('centipede_mesh')
    for kw in (dict(precision='fp32'), dict(), dict(precision='fp64'), dict(precision='fp32', fp64_contacts=True)):
        with pytest.raises(ValueError, match='fp64_mesh|fp64_contacts'):      # before any device use: no GPU is needed to get here
            BatchedPhysics(m, 2, fp64_mesh=True, **kw)
    with pytest.raises(ValueError, match='fp64_mesh'):
        BatchedPhysics(m, 2, fp64_mesh=True, precision='fp64')
    for other in ('fp64_fused', 'fp64_rk4'):
        with pytest.raises(ValueError, match='does not go with'):
            BatchedPhysics(m, 2, precision='fp64', fp64_contacts=True, fp64_mesh=True, **{other: True})
    with pytest.raises(ValueError, match='fp64_mesh'):
        Simulation(m, m.body_names[1], SimulationOptions(timestep=m.timestep, n_iterations=2), n_envs=2, precision='fp64', fp64_mesh=True)
    with pytest.raises(ValueError, match='fp64_mesh'):
        Simulation.from_sdf(SimulationOptions(timestep=m.timestep, n_iterations=2), AnimatOptions.from_model(m), ArenaOptions(),
                            model=m, n_envs=2, precision='fp64', fp64_mesh=True)


@pytest.mark.skipif(shutil.which('hipcc') is None, reason='hipcc not on PATH')
@pytest.mark.parametrize('unit, kernel', [(7, 'fmj_step_f64_mesh_kernel'), (8, 'fmj_step_f64_mesh_elliptic_kernel')])
def test_mesh_kernels_compile_without_scratch(tmp_path, unit, kernel):
    """Each new translation unit with the flags of _lib.build() holds exactly two kernels, <LIMITS> false and true; both keep out of
    scratch, spill no VGPR, and their LDS at the largest model the create check admits is within 160 KB."""
    res = resource_remarks(f'-DFMJ_TU_F64={unit}', tmp_path)
    ck = {k: v for k, v in res.items() if re.search(r'\d+%sILb[01]EE' % kernel, k)}
    assert len(res) == 2 and len(ck) == 2, sorted(res)
    from farms_mujoco_amd import _lib as L
    assert repr(BUILD_FLAGS)[:-1] in inspect.getsource(L.build) and f"'-DFMJ_TU_F64={unit}'" in inspect.getsource(L.build)
    listing = open(os.path.join(ROOT, 'scripts', 'device_listing.sh')).read()
    assert 'kf64m:-DFMJ_TU_F64=7' in listing and 'kf64me:-DFMJ_TU_F64=8' in listing
    dyn = lds_bytes('terrain', 128, 128, 129, 64, 120)
    assert dyn <= 160*1024 < lds_bytes('terrain', 128, 128, 129, 64, 121)
    within_resources(ck, dyn)
