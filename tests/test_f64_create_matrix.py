"""fmj_create_ex2 over every combination of eleven models, twenty settings of fmj_create_ext.flags and both precisions, held to what
the library answered before the fp64 kernel families were put in one table (tests/golden/f64_create_matrix.json): a refusal's return
code and message verbatim; for an acceptance, FMJ_ERR_NODEVICE without a GPU, and with one what fmj_kernel_info, fmj_constraint_info,
fmj_solver_info and fmj_precision report.  Contexts are 4 envs and destroyed at once.

The fixture is recorded from the library FMJ_SO names (scripts/build_base.sh <revision>):
    FMJ_SO=farms_mujoco_amd/csrc/libfmj_hip_base.so python tests/test_f64_create_matrix.py --record
once without a GPU (the 'cpu' entries) and once with one (the 'gpu' entries of the cases accepted without one)."""
import ctypes
import functools
import itertools
import json
import os
import sys

import pytest

from support_capi import lib, no_gpu, F32, F64
from support_f64_interface import limited_eel48, LIMITS, RK4, CONTACTS, TERRAIN, ROOT

FIXTURE = os.path.join(ROOT, 'tests', 'golden', 'f64_create_matrix.json')


def _rk4(mm, m):
    m.integrator = mm.INTEGRATORS['rk4']
    return m


def _lds_corner(mm):
    """nbody = nv = 128 with a dof chain of 64 and 121 contacts: one past what the terrain kernels' LDS map holds."""
    from wide_trees import shape_tree
    from support_f64_contacts import GEOM_PLANE, GEOM_SPHERE, set_geoms
    unit = (1.0, 0.0, 0.0, 0.0)
    return set_geoms(shape_tree(1), [(GEOM_PLANE, 0, (0, 0, 0), (0, 0, 0), unit, 0.0)] +
                     [(GEOM_SPHERE, b, (0.02, 0, 0), (0, 0, 0), unit, 1.0) for b in range(1, 128)], 121)


# name -> the model, given farms_mujoco_amd.model
MODELS = {'eel48': lambda mm: mm.eel(n_joints=48), 'limited_eel48': lambda mm: limited_eel48(), 'rk4_salamander33': lambda mm: _rk4(mm, mm.salamander33()),
          'limited_rk4_eel48': lambda mm: _rk4(mm, limited_eel48()), 'salamander33_contacts': lambda mm: mm.salamander33(contacts=True),
          'salamander33_contacts_limits': lambda mm: mm.salamander33(contacts=True, limits=True),
          'salamander33_contacts_hfield': lambda mm: mm.salamander33(contacts=True, terrain='hfield'),
          'centipede_20_25_contacts': lambda mm: mm.centipede(20, 25, contacts=True),
          'salamander33_self_collisions': lambda mm: mm.salamander33(contacts=True, self_collisions=True),
          'salamander33_mesh_feet': lambda mm: mm.salamander33(contacts=True, mesh_feet=True), 'lds_corner_121': _lds_corner}
SUBSETS = [sum(s) for r in range(5) for s in itertools.combinations((LIMITS, RK4, CONTACTS, TERRAIN), r)]
FLAGS = SUBSETS + [2, 64 | CONTACTS | TERRAIN, 256, None]      # None: ext = NULL
CASES = [(m, f, p) for m in MODELS for f in FLAGS for p in (F32, F64)]


@functools.lru_cache(maxsize=None)
def _model(name):
    import farms_mujoco_amd.model as mm
    return MODELS[name](mm)


def _key(name, flags, precision):
    return f"{name}|{'null' if flags is None else flags}|{('f32', 'f64')[precision]}"


def _answer(name, flags, precision):
    """['refused', rc, message], or ['accepted', kernel_info + constraint_info + solver_info + [precision]]."""
    L, so = lib()
    c = _model(name).as_c(); ctx = ctypes.c_void_p()
    opts = L.CCreateOptions(ctypes.sizeof(L.CCreateOptions), precision, 0, 0)
    e = L.CCreateExt(ctypes.sizeof(L.CCreateExt), flags or 0)
    rc = so.fmj_create_ex2(ctypes.byref(c), 4, 0, ctypes.byref(opts), None if flags is None else ctypes.byref(e), ctypes.byref(ctx))
    if rc:
        return ['refused', rc, so.fmj_last_error().decode()]
    try:
        return ['accepted', L.ints(so.fmj_kernel_info, ctx) + L.ints(so.fmj_constraint_info, ctx) + L.ints(so.fmj_solver_info, ctx) + [so.fmj_precision(ctx)]]
    finally:
        so.fmj_destroy(ctx)


NODEVICE = ['refused', 4, 'fmj_create: no HIP device visible']


@functools.lru_cache(maxsize=None)
def _fixture():
    return json.load(open(FIXTURE))


@pytest.mark.parametrize('name,flags,precision', CASES, ids=[_key(*c) for c in CASES])
def test_create_answers_what_it_answered(name, flags, precision):
    want = _fixture()[_key(name, flags, precision)]
    got = _answer(name, flags, precision)
    if want['cpu'] != 'accepted':
        assert got == want['cpu']
    elif no_gpu():
        assert got == NODEVICE
    else:
        assert got == want['gpu']


def test_the_fixture_holds_every_case_and_nothing_else():
    fx = _fixture()
    assert sorted(fx) == sorted(_key(*c) for c in CASES) and len(CASES) == 11*20*2
    assert all(v['cpu'] == 'accepted' or v['cpu'][0] == 'refused' for v in fx.values())
    assert all('gpu' in v for v in fx.values() if v['cpu'] == 'accepted')


def _record():
    fx = json.load(open(FIXTURE)) if os.path.exists(FIXTURE) else {}
    gpu = not no_gpu()
    for c in CASES:
        got, e = _answer(*c), fx.setdefault(_key(*c), {})
        if not gpu:
            e['cpu'] = 'accepted' if got == NODEVICE else got
        elif e['cpu'] == 'accepted':
            e['gpu'] = got
        else:
            assert got == e['cpu'], (c, got, e['cpu'])
    with open(FIXTURE, 'w') as f:
        json.dump(fx, f, indent=0, sort_keys=True)
        f.write('\n')
    print(f"recorded {len(fx)} cases ({'gpu' if gpu else 'cpu'}) from {sys.modules['farms_mujoco_amd._lib'].SO_PATH}")


if __name__ == '__main__':
    assert sys.argv[1:] == ['--record'], 'usage: [FMJ_SO=<library>] python tests/test_f64_create_matrix.py --record'
    sys.path.insert(0, ROOT)
    _record()
