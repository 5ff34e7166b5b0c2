"""The inputs of tests/test_gpu_f64_limit_params.py, checked on the CPU oracle alone: that each recipe of support_limits.py engages what
it says it engages (a floor on what the GPU test exercises, asserted there again), and that the reference is converged on these inputs,
so that an excess on the device cannot be the oracle's.

Seed rule, as in test_gpu_f64_limits.py: the first of 100, 101, ... at which the conditions hold in every env (support_limits.RECIPE_SEEDS; 100 on
every model here).  With it, per env: recipe R gives 1 - 5 joints with both rows candidate and 13 - 59 rows with a force (on shape1 and
shape6 1 - 4 joints with a force on both rows, on the eel and the centipede none), recipe S 7 - 37 rows with a force; the oracle's
Newton takes 2 - 5 iterations."""
import numpy as np
import pytest

import support_limits as L
from support_f64_step import ulp_excess, _field_groups

N, MODELS = L.N, L.RECIPE_MODELS
recipe_inputs, undamped_inputs = L.recipe_inputs, L.undamped_inputs


def test_row_branches_names_every_branch_of_get_impedance():
    """row_branches on one joint, one state per branch, with x = |dist - margin| / width worked out by hand (0.4, 0.2, 0.8, 1.2)."""
    m = L.limited('eel48')
    j = int(np.flatnonzero(m.jnt_type != 0)[0])
    m.jnt_range[j] = (-0.1, 0.3); m.jnt_margin[j] = 0.0
    cases = [((0.5, 0.5, 0.05, 0.5, 2), (0.02, 1), -0.12, 'flat', 'time_constant'),
             ((0.5, 0.95, 0.0, 0.5, 2), (0.02, 1), -0.12, 'flat', 'time_constant'),
             ((0.5, 0.95, 0.05, 0.5, 1), (0.001, 1), -0.12, 'linear', 'floor_2h'),
             ((0.5, 0.95, 0.05, 0.5, 2), (-100, -1), -0.11, 'below_mid', 'direct'),
             ((0.5, 0.95, 0.05, 0.5, 2), (0, 0), -0.14, 'above_mid', 'direct'),
             ((0.5, 0.95, 0.05, 0.5, 2), (0.002, 1), -0.16, 'saturated', 'time_constant')]
    for solimp, solref, q, imp, form in cases:
        m.jnt_solimp[j] = solimp; m.jnt_solref[j] = solref
        qpos = m.qpos0.copy(); qpos[m.jnt_qposadr[j]] = q
        assert L.row_branches(m, qpos) == [(j, -1, imp, form)], (solimp, solref, q, L.row_branches(m, qpos))
    qpos = m.qpos0.copy(); qpos[m.jnt_qposadr[j]] = -0.1
    assert L.row_branches(m, qpos) == []      # dist == margin: no row
    m.jnt_range[j] = (-0.01, 0.01); m.jnt_margin[j] = 0.03
    assert [r[:2] for r in L.row_branches(m, m.qpos0)] == [(j, -1), (j, 1)]      # both rows, the lower one first


@pytest.mark.parametrize('recipe', ['R', 'S'])
@pytest.mark.parametrize('name', MODELS)
def test_recipe_engages_what_it_says(oracle, name, recipe):
    m, ins = recipe_inputs(name, recipe)
    L.assert_recipe_engaged(name, recipe, m, ins, L.step_tf(oracle, m, ins))
    if recipe == 'R':      # ranges and margins differ per joint and are asymmetric: a wrong index into the table cannot go unseen
        on = m.jnt_type != 0
        assert len(np.unique(m.jnt_range[on], axis=0)) > on.sum()*0.7 and len(np.unique(m.jnt_margin[on])) > on.sum()*0.7
        assert np.abs(m.jnt_range[on, 0] + m.jnt_range[on, 1]).max() > 0.05


@pytest.mark.parametrize('name', ['eel48', 'shape6'])
def test_undamped_models_engage_their_limits(oracle, name):
    for integrator in ('euler', 'implicitfast'):
        m, ins = undamped_inputs(name, integrator)
        assert not np.any(m.dof_damping) and not np.any(np.reshape(m.actuator_bias, (m.nu, 3))[:, 2])
        o = L.step_tf(oracle, m, ins)
        forced = np.array([(o['efc'][e, :o['nefc'][e], 0] > 0).sum() for e in range(N)])
        print(name, integrator, 'rows with a force per env', forced, 'iterations', o['iterations'])
        assert forced.min() >= 5 and not o['status'].any() and o['iterations'].max() <= 10, (name, forced, o['status'], o['iterations'])
        assert np.array_equal(o['warmstart'], o['qacc'])      # nothing is damped: the integrator uses the constrained acceleration itself


def test_margin_edge_rows(oracle):
    m, qpos, qvel = L.margin_edge(N)
    ins = L.as_fp32_inputs(m, qpos, qvel)
    sq = L.scalar_q(m)
    assert np.array_equal(ins['qpos'][:, sq], qpos[:, sq])      # the four joint positions are fp32 numbers
    o = L.step_tf(oracle, m, ins)
    forced = [int((o['efc'][e, :o['nefc'][e], 0] > 0).sum()) for e in range(N)]
    print('margin edge: candidate rows per env', o['nefc'], 'with a force', forced)
    assert list(o['nefc']) == [0, 48, 0, 48] and forced[1] >= 5 and forced[3] >= 5, (o['nefc'], forced)
    assert [len(L.row_branches(m, qpos[e])) for e in range(N)] == [0, 48, 0, 48]


def _converged(oracle, m, ins, label):
    """The oracle as the tests configure it (tolerance 1e-8, 100 iterations) against 1e-14 and 500: at most 0.01 of the ulp bound."""
    import copy
    assert m.solver_tolerance == 1e-8 and m.solver_iterations == 100
    tight = copy.deepcopy(m); tight.solver_tolerance = 1e-14; tight.solver_iterations = 500
    kw = dict(ctrl=ins['ctrl'], qpos_spring=ins['qpos_spring'], xfrc_applied=ins['xfrc_applied'])
    a, b = oracle.step(m, ins['qpos'], ins['qvel'], **kw), oracle.step(tight, ins['qpos'], ins['qvel'], **kw)
    wa, wb = L.step_tf(oracle, m, ins)['warmstart'], L.step_tf(oracle, tight, ins)['warmstart']
    groups = _field_groups(m)
    ex = {k: ulp_excess(a[k], b[k], groups[k]) for k in ('qpos', 'qvel', 'qacc', 'sensordata')}
    ex['warmstart'] = ulp_excess(wa, wb, groups['qvel'])
    print(label, 'default against tight oracle, difference / bound:', {k: '%.2g' % v for k, v in ex.items()}, 'max |qacc| %.3g' % np.abs(b['qacc']).max())
    assert max(ex.values()) <= 0.01, (label, ex)


@pytest.mark.parametrize('integrator', ['euler', 'implicitfast'])
@pytest.mark.parametrize('recipe', ['R', 'S'])
@pytest.mark.parametrize('name', MODELS)
def test_the_oracle_is_converged_on_the_recipes(oracle, name, recipe, integrator):
    m, ins = recipe_inputs(name, recipe, integrator)
    _converged(oracle, m, ins, f'{name} {recipe} {integrator}')


def test_the_oracle_is_converged_on_the_undamped_and_edge_inputs(oracle):
    for name in ('eel48', 'shape6'):
        for integrator in ('euler', 'implicitfast'):
            m, ins = undamped_inputs(name, integrator)
            _converged(oracle, m, ins, f'{name} undamped {integrator}')
    m, qpos, qvel = L.margin_edge(N)
    _converged(oracle, m, L.as_fp32_inputs(m, qpos, qvel), 'margin edge')
