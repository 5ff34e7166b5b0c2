"""The recipes of the fp64 mesh GPU tests (support_f64_mesh.py), checked on the CPU oracle alone: at each model's stored seed the
conditions hold in every env, and the reference is converged - a 100 x tighter tolerance and 200 iterations move no field by more
than 0.1 of its one-step bound and leave ncon as it is."""
import numpy as np
import pytest

import support_f64_contacts as C
import support_f64_mesh as M
from support_f64_mesh import N


def test_the_vertex_sets_are_what_they_say():
    vs = M.vertex_sets()
    assert [len(vs[k]) for k in ('vertex', 'triangle', 'tetrahedron', 'hull12', 'hull42')] == [1, 3, 4, 12, 42]
    for k, v in vs.items():
        r = np.linalg.norm(v, axis=1)
        assert r.max() <= 1.0 + 1e-12 and r.min() >= 0.55, (k, r)
    for k in ('hull12', 'hull42'):      # irregular: radii in [0.8, 1], no two equal
        r = np.linalg.norm(vs[k], axis=1)
        assert r.min() >= 0.8 and len(np.unique(r)) == len(r)


@pytest.mark.parametrize('name', M.MODELS)
def test_conditions_hold_and_the_reference_is_converged(oracle, name):
    import support_f64_step as S
    m = M.make(name)
    ins = M.inputs_of(name, m)
    ok, ref, what = M.conditions(oracle, name, m, ins)
    print(name, what)
    assert ok, (name, what)
    if name == 'centipede_mesh':
        assert m.nbody == 107 and m.ngeom == 67 and m.max_contacts == 120 and int((m.geom_type == M.GEOM_MESH).sum()) == 40
        assert max(ref['geoms'][e, :ref['ncon'][e], 1].max() for e in range(N)) >= 64 and ref['ncon'].max() > 64      # the second wave
    tight = C.reference(oracle, m, ins, tighter=True)
    groups = C._groups(m)
    moved = {k: S.ulp_excess(tight[k], ref[k], groups[k]) for k in C.STATE}
    moved['contact'] = C._contact_excess(tight['contact'], ref['ncon'], ref)
    print(name, 'a 100 x tighter tolerance moves the reference by (in bounds):', {k: round(v, 4) for k, v in moved.items()})
    assert max(moved.values()) <= 0.1 and np.array_equal(tight['ncon'], ref['ncon']), moved


@pytest.mark.parametrize('which', M.NARROW)
def test_the_hand_placed_cases_take_their_branches(oracle, which):
    m, ins = M.narrow_case(which)
    ref = C.reference(oracle, m, ins)
    M.narrow_branch(which, m, ins, ref)
