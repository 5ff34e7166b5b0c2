"""The inputs of tests/test_gpu_f64_contact_params.py, checked on the CPU oracle alone (no GPU): at the seeds of
support_f64_contact_params.SEEDS every case has in every env what it is about (support_f64_contact_params.conditions: contacts with
and without a force, contact slots past 64, every impedance branch and every meaning of solref on a contact with a force, both friction
winners, both grounds, a geom past the grid's edge, geoms on welded bodies and past geom 64), no narrow-phase decision grazes (1e-9), the
model passes every check of fmj_create_ex2, and the reference is converged by the project's rule: a 100 x tighter tolerance with 200
iterations moves no field by more than 0.1 of the one-step bound, and the solve ended below its iteration budget.  A seed at which a
condition failed would be replaced by support_f64_contact_params.first_seed's and recorded in SEEDS."""
import numpy as np
import pytest

import support_f64_contacts as C
import support_f64_contact_params as P
from support_f64_interface import create_ex2, accepted


def test_the_branch_helpers_name_every_branch():
    """impedance_branch and solref_form on hand-made parameters, x = |dist| / width worked out by hand (0.4, 0.2, 0.8, 1.2)."""
    assert P.impedance_branch((0.5, 0.5, 0.05, 0.5, 2), -0.02) == 'flat' and P.impedance_branch((0.5, 0.95, 0.0, 0.5, 2), -0.02) == 'flat'
    assert P.impedance_branch((0.5, 0.95, 0.05, 0.5, 1), -0.02) == 'linear' and P.impedance_branch((0.5, 0.95, 0.05, 0.5, 2), -0.01) == 'below_mid'
    assert P.impedance_branch((0.5, 0.95, 0.05, 0.5, 2), -0.04) == 'above_mid' and P.impedance_branch((0.5, 0.95, 0.05, 0.5, 2), -0.06) == 'saturated'
    assert P.impedance_branch((0.5, 0.95, 0.05, 0.3, 3), -0.0125) == 'below_mid' and P.impedance_branch((0.5, 0.95, 0.05, 0.3, 3), -0.02) == 'above_mid'
    h = 1e-3
    assert [P.solref_form(s, h) for s in P.SOLREF_FORMS] == ['time_constant', 'floor_2h', 'time_constant', 'time_constant', 'direct', 'direct']
    assert P.solref_form((0.0, 0.0), h) == 'direct' and P.solref_form((0.002, 1.0), h) == 'time_constant'


def test_recipe_p_differs_per_geom():
    """Every animat geom of a recipe-P model has its own friction, the six solimp and the six solref forms all occur, the ground has
    friction 0.8, and the scaled widths follow the depth of the model's inputs."""
    for name in ('P-salamander-euler', 'P-boxfoot-euler', 'P-centipede-euler', '2planes-salamander', 'hfield+plane-salamander'):
        m = P.make(name)
        an = P.animat(m)
        assert len(np.unique(m.geom_friction[an, 0])) == len(an) and m.geom_friction[an, 0].min() >= 0.3 and m.geom_friction[an, 0].max() <= 1.3
        assert len(np.unique(m.geom_solimp[an], axis=0)) == 6 and len(np.unique(m.geom_solref[an], axis=0)) == 6
        assert m.geom_friction[0, 0] == P.GROUND_FRICTION
        depth = P._inputs_kw(name).get('depth', P.P_DEPTH.get(m.name))
        assert np.isclose(m.geom_solimp[an, 2].max(), P.WIDTH*depth), (name, depth)
    m = P.make('2planes-boxfoot')
    assert P.grounds(m) == [0, 1] and list(m.geom_friction[:2, 0]) == [P.GROUND_FRICTION, P.SECOND_FRICTION] and m.geom_bodyid[1] == 0
    assert m.ngeom == C.make('boxfoot6').ngeom + 1 and m.geom_type[2] == C.GEOM_CAPSULE


def test_the_welded_model_is_what_the_case_says():
    m = P.make('welded-contacts')
    wg = P.welded_geoms(m)
    boxes = [g for g in wg if m.geom_type[g] == C.GEOM_BOX]
    assert (m.nbody, m.nv, m.ngeom) == (72, 64, 1 + 71 + P.WELDED_BOXES) and len(boxes) == P.WELDED_BOXES and len(wg) == 12 + P.WELDED_BOXES
    assert sum(1 for g in P.animat(m) if g >= 64) >= 8 and any(g >= 64 for g in wg)
    for g in boxes:      # the box follows its body's sphere: two geoms on one body
        assert m.geom_bodyid[g - 1] == m.geom_bodyid[g] and m.geom_type[g - 1] == C.GEOM_SPHERE


@pytest.mark.parametrize('name', list(P.CASES))
def test_the_case_has_what_it_is_about_and_the_reference_is_converged(oracle, name):
    m, ins, family = P.case(name)
    rc, msg, prec, _ = create_ex2(m, flags=P.flags_of(m, family))
    assert accepted(rc, msg, prec), (name, rc, msg)
    ok, ref, what = P.conditions(oracle, name, m, ins)
    print(name, what)
    assert ok, (name, what)
    assert ref['iterations'].max() < m.solver_iterations, ref['iterations']      # ended by the tolerance, not by the budget
    moved = P.moved_by_a_tighter_tolerance(oracle, m, ins, ref)
    print(name, 'a 100 x tighter tolerance moves the reference by (in bounds):', {k: round(v, 5) for k, v in moved.items()})
    assert max(moved.values()) <= 0.1, moved


def test_the_seeds_are_the_first_that_satisfy_the_conditions(oracle):
    """first_seed on one case of each kind whose seed is not the first tried (the others are 100: the first)."""
    for name in ('big-terrain', '2planes-salamander', 'P-salamander-euler'):
        assert P.first_seed(oracle, name) == P.SEEDS[name], name
    assert all(P.SEEDS[n] == 100 for n in P.CASES if n not in ('big-terrain', '2planes-salamander') and not n.startswith('P-salamander'))


def test_the_truncation_case_cuts_a_list_past_64(oracle):
    """max_contacts = 70 on the 'big-euler' inputs: every env's full list is longer, the oracle keeps its first 70 and reports
    FMJ_WARN_CONTACTFULL and nothing else."""
    m, ins, _ = P.case('big-euler')
    full = C.reference(oracle, m, ins)
    assert full['ncon'].min() > P.TRUNCATED > 64
    m.max_contacts = P.TRUNCATED
    a = oracle.step(m, ins['qpos'], ins['qvel'], ctrl=ins['ctrl'])
    b = oracle.step_tf(m, ins['qpos'], ins['qvel'], ctrl=ins['ctrl'], want_AR=False)
    assert np.all(b['ncon'] == P.TRUNCATED) and np.all(a['status'] == C.FMJ_WARN_CONTACTFULL)
    for e in range(C.N):
        assert np.array_equal(b['contact'][e, :, :3], full['contact'][e, :P.TRUNCATED, :3])
        assert (b['contact'][e, 64:, 12] > 0).sum() >= 1      # a kept contact past slot 64 carries a force
    rc, msg, prec, _ = create_ex2(m, flags=P.flags_of(m, 'contacts'))
    assert accepted(rc, msg, prec), (rc, msg)


@pytest.mark.parametrize('which', P.NARROW)
def test_the_narrow_phase_cases_take_their_branches(oracle, which):
    m, ins = P.narrow_case(which)
    assert np.array_equal(ins['qpos'], ins['qpos'].astype(np.float32).astype(np.float64))
    rc, msg, prec, _ = create_ex2(m, flags=P.flags_of(m, 'terrain'))
    assert accepted(rc, msg, prec), (which, rc, msg)
    ref = C.reference(oracle, m, ins)
    print(which, 'ncon', ref['ncon'], 'dist', ref['dist'][0, :ref['ncon'][0]])
    P.narrow_branch(which, m, ins, ref)
    assert ref['iterations'].max() < m.solver_iterations
    moved = P.moved_by_a_tighter_tolerance(oracle, m, ins, ref)
    assert max(moved.values()) <= 0.1, moved
