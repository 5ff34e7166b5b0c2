"""Joint limits on the fp64 step kernel (the LIMITS instantiations of csrc/fmj_f64.inc) away from the one point of the parameter space
that test_gpu_f64_limits.py visits: ranges and margins that differ per joint and are asymmetric, joints with both rows at once, every
impedance branch of f64_limit_row and every meaning of solref (recipes R and S of support_limits.py), models with nothing damped,
dist == margin exactly, a batch whose workgroups take different branches in one launch, fmj_forward_debug on a limits context, and
qacc_warmstart as a number, not as "non-zero".

The bound is that of test_gpu_f64_step.py everywhere, |got - ref| <= ulp32(ref_i) + ulp32(max |ref| of the component's group in its env)
(ulp_excess <= 1 with _field_groups); qacc_warmstart is compared in the groups of qvel with the oracle's constrained acceleration
(step_tf's 'warmstart').  tests/test_f64_limit_recipes.py shows on the CPU that the oracle is converged on these inputs to 2e-4 of that
bound, max |qacc| of 7e5 notwithstanding.  Every case first asserts, from the oracle, that its inputs engage what the case is about."""
import numpy as np
import pytest

from parity_metrics import relerr
from wide_trees import dof_depth
import support_limits as L
from support_f64_step import ulp_excess, _field_groups

pytestmark = pytest.mark.gpu

N, MODELS = L.N, L.RECIPE_MODELS
recipe_inputs, undamped_inputs = L.recipe_inputs, L.undamped_inputs
FIELDS = ('qpos', 'qvel', 'qacc', 'sensordata')
ALL_FIELDS = FIELDS + ('qacc_warmstart', 'xpos', 'xquat', 'xipos', 'time')


def _phys(m, ins):
    """A limits context holding ``ins`` (already fp32 numbers); checks that the device holds exactly what the oracle is given."""
    phys, held = L.phys(m, N, ins['qpos'], ins['qvel'], ins['ctrl'], ins['xfrc_applied'], ins['qpos_spring'])
    for k, v in held.items():
        assert (v is None and ins[k] is None) or np.array_equal(v, ins[k]), k
    return phys


def _limit_forces(m, sensordata):
    nl = 6*(m.nbody - 1)
    return np.asarray(sensordata)[:, nl + 2:nl + 3*m.n_sensor_joints:3]


def _step_and_forward(oracle, m, ins, label):
    """One step and fmj_forward against the oracle: error / bound per field, qacc_warmstart after the step included; returns the
    context that stepped and the figures."""
    import torch
    out = {}
    stepped = None
    for forward in (False, True):
        phys = _phys(m, ins)
        ex, ref = L.excess(oracle, m, phys, ins, forward)
        assert np.abs(_limit_forces(m, ref['sensordata'])).max() > 0      # the reference has limit forces
        if not forward:
            stepped = phys
            ws = L.step_tf(oracle, m, ins)['warmstart']
            ex['qacc_warmstart'] = ulp_excess(phys.data.qacc_warmstart.cpu().numpy(), ws, _field_groups(m)['qvel'])
        out['forward' if forward else 'step'] = ex
        print(label, 'forward' if forward else 'step', 'error / bound per field:', {k: round(v, 3) for k, v in ex.items()})
    bad = {(w, k): v for w, ex in out.items() for k, v in ex.items() if v > 1.0}
    assert not bad, (label, bad)
    torch.cuda.synchronize()
    return stepped, out


@pytest.mark.parametrize('integrator', ['euler', 'implicitfast'])
@pytest.mark.parametrize('recipe', ['R', 'S'])
@pytest.mark.parametrize('name', MODELS)
def test_recipes_one_step_and_forward_to_the_ulp(oracle, name, recipe, integrator):
    import torch
    m, ins = recipe_inputs(name, recipe, integrator)
    L.assert_recipe_engaged(name, recipe, m, ins, L.step_tf(oracle, m, ins))
    phys, _ = _step_and_forward(oracle, m, ins, f'{name} {recipe} {integrator}')
    assert np.any(m.dof_damping)      # damped dofs: the integrator's acceleration is not the constrained one
    assert not torch.equal(phys.data.qacc_warmstart, phys.data.qacc)


@pytest.mark.parametrize('integrator', ['euler', 'implicitfast'])
@pytest.mark.parametrize('name', ['eel48', 'shape6'])
def test_nothing_damped(oracle, name, integrator):
    """dof_damping zero (and no velocity bias on an actuator, which implicitfast counts as damping): the step ends on the constrained
    acceleration itself, without the last factorisation, and qacc_warmstart and qacc are the fp32 store of the same double."""
    import torch
    m, ins = undamped_inputs(name, integrator)
    forced, _ = L.rows_engaged(oracle, m, ins)
    assert forced.min() >= 5 and not np.any(m.dof_damping) and not np.any(np.reshape(m.actuator_bias, (m.nu, 3))[:, 2]), forced
    phys, _ = _step_and_forward(oracle, m, ins, f'{name} undamped {integrator}')
    assert torch.equal(phys.data.qacc_warmstart.view(torch.int32), phys.data.qacc.view(torch.int32))
    assert float(phys.data.qacc.abs().max()) > 0


def test_margin_edge_in_a_mixed_batch(oracle):
    """support_limits.margin_edge: in one launch, envs 0 and 2 have dist == margin on every joint (no candidate row: the unconstrained
    branch, bit for bit the kernel without limits) and envs 1 and 3 are one fp32 step past it (48 rows each, the Newton branch)."""
    import torch
    m, qpos, qvel = L.margin_edge(N)
    ins = L.as_fp32_inputs(m, qpos, qvel)
    o = L.step_tf(oracle, m, ins)
    forced = [int((o['efc'][e, :o['nefc'][e], 0] > 0).sum()) for e in range(N)]
    assert list(o['nefc']) == [0, 48, 0, 48] and forced[1] >= 5 and forced[3] >= 5, (o['nefc'], forced)
    free, _, _ = L.margin_edge(N)
    free.jnt_limited = np.zeros_like(free.jnt_limited)
    groups = _field_groups(m)
    for forward in (False, True):
        pa = _phys(m, ins)
        pb, _ = L.phys(free, N, ins['qpos'], ins['qvel'], limits=False)
        assert pa.has_constraints and not pb.has_constraints
        ex, ref = L.excess(oracle, m, pa, ins, forward)
        if forward:
            pb.forward()
        else:
            pb.step(1)
        torch.cuda.synchronize()
        assert int(pb.data.status.abs().sum()) == 0
        for k in FIELDS + ('xpos', 'xquat', 'xipos'):
            a, b = getattr(pa.data, k)[[0, 2]], getattr(pb.data, k)[[0, 2]]
            assert torch.equal(a.view(torch.int32), b.view(torch.int32)), (forward, k)
        # envs 1 and 3 alone against the oracle (L.excess has held the whole batch to the bound already; this names the engaged half)
        ex13 = {k: ulp_excess(getattr(pa.data, k).cpu().numpy()[[1, 3]], np.asarray(ref[k])[[1, 3]], groups[k]) for k in FIELDS}
        print('margin edge', 'forward' if forward else 'step', 'error / bound, all envs', {k: round(v, 3) for k, v in ex.items()},
              'envs 1 and 3', {k: round(v, 3) for k, v in ex13.items()})
        assert max(ex.values()) <= 1.0 and max(ex13.values()) <= 1.0, (forward, ex, ex13)
        got_f = _limit_forces(m, pa.data.sensordata.cpu().numpy())
        assert not got_f[[0, 2]].any() and np.all(np.abs(got_f[[1, 3]]).max(axis=1) > 0), got_f
        if not forward:      # (envs 0 and 2 took the step without candidates, whose qacc_warmstart is by design the integrator's qacc)
            ws = ulp_excess(pa.data.qacc_warmstart.cpu().numpy()[[1, 3]], o['warmstart'][[1, 3]], groups['qvel'])
            print('margin edge qacc_warmstart error / bound', round(ws, 3))
            assert ws <= 1.0, ws


@pytest.mark.parametrize('name', ['eel48', 'shape6'])
def test_forward_debug_on_a_limits_context(oracle, name):
    """fmj_forward_debug under recipe R with engaged limits: the rows of H are those of M + h diag(damping) - not of the Newton matrix
    M + D_S that the solve leaves in the same LDS rows - and qfrc_smooth carries no constraint force; bound and row layout of
    test_gpu_f64_step.py::test_stage_outputs_to_the_ulp.  The derived fields are those of fmj_forward."""
    import torch
    m, ins = recipe_inputs(name, 'R')
    L.assert_recipe_engaged(name, 'R', m, ins, L.step_tf(oracle, m, ins))
    phys = _phys(m, ins)
    H, qf = phys.forward_debug()
    torch.cuda.synchronize()
    assert int(phys.data.status.abs().sum()) == 0
    rs, depth = H.shape[2], dof_depth(m)
    assert rs == (int(depth.max()) + 4)//4*4
    Hrows = H.cpu().numpy()
    assert H.shape == (N, m.nv, rs) and np.all(H._base.cpu().numpy()[N*m.nv*rs:] == 0.0)
    Href = np.zeros_like(Hrows, dtype=np.float64); qref = np.zeros((N, m.nv)); qcon = np.zeros((N, m.nv))
    for e in range(N):
        o = oracle.forward_debug(m, ins['qpos'][e], ins['qvel'][e], ctrl=ins['ctrl'][e] if m.nu else None, qpos_spring=ins['qpos_spring'][e],
                                 xfrc_applied=ins['xfrc_applied'][e])
        Hd = o['M'] + np.diag(m.timestep*m.dof_damping)
        for i in range(m.nv):
            j = i
            while j >= 0:
                Href[e, i, depth[j]] = Hd[i, j]; j = m.dof_parentid[j]
        qref[e] = o['qfrc_smooth']; qcon[e] = o['qfrc_constraint']
    assert np.all(np.abs(qcon).max(axis=1) > 0)
    eh, eq = ulp_excess(Hrows, Href), ulp_excess(qf.cpu().numpy(), qref)
    with_force = ulp_excess(qf.cpu().numpy(), qref + qcon)
    print(name, 'limits context: H error / bound', eh, 'qfrc_smooth error / bound', eq, '(against qfrc_smooth + qfrc_constraint:', with_force, ')')
    assert eh <= 1.0 and eq <= 1.0, (name, eh, eq)
    assert with_force > 1.0, with_force      # the comparison tells the two apart
    fw = _phys(m, ins)
    fw.forward()
    torch.cuda.synchronize()
    for k in ('qacc', 'sensordata', 'xpos', 'xquat', 'xipos'):
        assert torch.equal(getattr(phys.data, k).view(torch.int32), getattr(fw.data, k).view(torch.int32)), k


@pytest.mark.parametrize('name', ['eel48', 'shape6'])
def test_the_iteration_budget_does_not_matter_above_what_the_solve_needs(oracle, name):
    """Recipe S, three steps with solver_iterations = 100 and = 50: the oracle needs at most 10 on each of the three steps, and every
    output is the same bit for bit."""
    import torch
    m, ins = recipe_inputs(name, 'S')
    q, v, ws = ins['qpos'], ins['qvel'], None
    for t in range(3):
        o = oracle.step_tf(m, q, v, ctrl=ins['ctrl'], warmstart=ws, qpos_spring=ins['qpos_spring'], xfrc_applied=ins['xfrc_applied'], want_AR=False)
        assert o['iterations'].max() <= 10 and (o['nefc'] > 0).all() and not o['status'].any(), (t, o['iterations'], o['nefc'])
        q, v, ws = o['qpos'], o['qvel'], o['warmstart']
    outs = []
    for budget in (100, 50):
        mb, _ = recipe_inputs(name, 'S')
        mb.solver_iterations = budget
        phys = _phys(mb, ins)
        assert phys.solver_budget == budget
        phys.step(3)
        torch.cuda.synchronize()
        assert int(phys.data.status.abs().sum()) == 0
        outs.append({k: getattr(phys.data, k).clone() for k in ALL_FIELDS})
    assert float(_limit_forces(m, outs[0]['sensordata'].cpu().numpy()).max()) > 0
    for k in ALL_FIELDS:
        assert torch.equal(outs[0][k].view(torch.int32), outs[1][k].view(torch.int32)), k


def test_trajectory_with_both_recipes_against_the_state_rounding_floor(oracle):
    """eel(48) with R's ranges and margins and S's solref and solimp, 300 steps in one fmj_step launch from rest under the ctrl tape of
    test_gpu_f64_limits.py's recipe A (amplitude 0.3, 2 Hz), against floor_state (the oracle's own run with the state rounded to fp32
    every step) as there.  From the step-by-step oracle run: a candidate row in every step and a force in every step of every env
    (shares 1.0, 1.0, 1.0, 1.0; the narrow joints are inside their margin at rest), at most 3 Newton iterations."""
    import torch
    T = 300
    m = L.recipe_model('eel48', 'RS')
    tape32 = L.tape(m, N, T, 2.0)
    tape = tape32.astype(np.float64)
    q0 = np.tile(m.qpos0, (N, 1)); v0 = np.zeros((N, m.nv))
    q, v, ws = q0, v0, None
    with_force = np.zeros(N); with_row = np.zeros(N)
    for t in range(T):
        o = oracle.step_tf(m, q, v, ctrl=tape[t], warmstart=ws, want_AR=False)
        with_row += o['nefc'] > 0
        with_force += np.array([(o['efc'][e, :o['nefc'][e], 0] > 0).any() for e in range(N)])
        q, v, ws = o['qpos'], o['qvel'], o['warmstart']
    print('share of steps with a force', with_force/T, 'with a candidate row', with_row/T)
    assert with_row.min() == T and (with_force/T).min() >= 0.9, (with_force/T, with_row/T)
    ref = oracle.step(m, q0, v0, ctrl=tape, n_steps=T, ctrl_step_stride=N*m.nu, n_threads=4)
    fq, fv = q0, v0
    for t in range(T):      # floor_state
        o = oracle.step(m, fq, fv, ctrl=tape[t], n_steps=1, n_threads=4)
        fq = o['qpos'].astype(np.float32).astype(np.float64); fv = o['qvel'].astype(np.float32).astype(np.float64)
    phys, _ = L.phys(m, N, q0, v0)
    phys.step(T, torch.as_tensor(tape32, device=phys.device).contiguous())
    torch.cuda.synchronize()
    assert int(phys.data.status.abs().sum()) == 0
    for k, fl in (('qpos', fq), ('qvel', fv)):
        err, floor = relerr(getattr(phys.data, k).cpu().numpy(), ref[k]), relerr(fl, ref[k])
        print('R + S', k, 'after', T, 'steps: fp64 kernel %.3g  floor_state %.3g  ratio %.3g' % (err, floor, err/floor))
        assert err <= floor, (k, err, floor)
