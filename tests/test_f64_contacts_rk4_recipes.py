"""The recipes of test_gpu_f64_contacts_rk4.py, from the oracle and the models alone (no GPU): at the committed seeds every one-step
case meets the conditions of support_f64_contacts_rk4.conditions in every env, the reference does not move under a 100 x tighter
tolerance, the Euler recipes' seeds already give a fourth-pass contact list that differs from the first pass's, and the trajectory's
plain and state-rounded oracle runs see the same ncon sequence."""
import numpy as np
import pytest

import support_f64_contacts as C
import support_f64_contacts_rk4 as R
from support_f64_contacts_rk4 import N


@pytest.mark.parametrize('case', list(R.CASES))
def test_the_one_step_cases_meet_their_conditions(oracle, case):
    import support_f64_step as S
    m = R.make(case)
    assert m.integrator == 1
    ins = R.inputs(case, m)
    ok, ref, st, what = R.conditions(oracle, case, m, ins)
    print(case, what)
    assert ok, (case, what)
    assert what['forced'].min() >= 4 and what['idle'].min() >= 1 and what['clear'] and what['fourth_is_left'] and any(what['lists_differ'])
    assert ref['iterations'].max() < m.solver_iterations
    if np.any(m.jnt_limited):
        assert what['limit_rows_with_force'].min() >= 1
    tight = C.reference(oracle, m, ins, tighter=True)      # the reference is converged
    groups = C._groups(m)
    moved = {k: S.ulp_excess(tight[k], ref[k], groups[k]) for k in C.STATE}
    moved['contact'] = C._contact_excess(tight['contact'], ref['ncon'], ref)
    print(case, 'a 100 x tighter tolerance moves the reference by (in bounds):', {k: round(v, 4) for k, v in moved.items()})
    assert max(moved.values()) <= 0.1 and np.array_equal(tight['ncon'], ref['ncon']), moved


@pytest.mark.parametrize('name', ['salamander33', 'centipede_20_25'])
def test_the_fourth_pass_list_differs_at_the_euler_seeds_too(oracle, name):
    """At the seeds of the Euler recipes (support_f64_contacts.SEEDS) some env's fourth pass already has another contact list than its first."""
    m = C.make(name, 'rk4')
    ins = C.inputs(m, N, C.SEEDS[name])
    first, fourth = [], []
    for e in range(N):
        st = R.stages(oracle, m, ins, e)
        first.append(R.pass_list(st[0][2])); fourth.append(R.pass_list(st[3][2]))
    print(name, 'ncon of the first pass', [a[0] for a in first], 'of the fourth', [b[0] for b in fourth])
    assert any(a[0] != b[0] or not np.array_equal(a[1], b[1]) for a, b in zip(first, fourth))
    ref = C.reference(oracle, m, ins)
    assert [b[0] for b in fourth] == list(ref['ncon'])      # what the step leaves is the fourth pass's


def test_the_first_seed_search_finds_the_committed_seed(oracle):
    assert R.first_seed(oracle, 'salamander33') == R.SEEDS['salamander33']


def test_the_trajectory_sees_one_ncon_sequence(oracle):
    m = R.make('salamander33')
    q0, v0, tape32 = R.trajectory_inputs(m)
    assert min(C.lowest_point(m, q) for q in q0) > 0.5*R.TRAJ_LIFT      # just above touch height (fp32 rounding of the root's height)
    (_, _, plain, share), (_, _, rounded, _) = R.trajectory_runs(oracle, m, q0, v0, tape32)
    print('share of steps with a contact force per env', share, 'largest ncon', plain.max(axis=0))
    assert np.array_equal(plain, rounded)
    assert plain.max() >= 2 and share.max() >= 0.5 and share.min() > 0
