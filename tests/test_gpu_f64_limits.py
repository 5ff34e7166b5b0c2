"""Joint limits on the fp64 step kernel (BatchedPhysics(precision='fp64', fp64_limits=True): fmj_create_ex2 with FMJ_CREATE_F64_LIMITS,
the LIMITS instantiations of csrc/fmj_f64.inc) against the fp64 oracle, whose model names Newton with 100 iterations and the default
tolerance - the device runs its primal Newton solve whatever the model names.

One step and fmj_forward are held to the rounding of the fp32 store, the bound of test_gpu_f64_step.py, jointlimitfrc included:
    |got - ref| <= ulp32(ref_i) + ulp32(max |ref| over the component's column group in that env)
The oracle's Newton solve is 1e-10 (relative to the largest acceleration) from the converged solution and the kernel ends on the exact
minimiser of the final active set, so the solve adds nothing visible at the size of one ulp32 (6e-8).  Trajectories are held to the
oracle's own run with the state rounded to fp32 every step (floor_state of test_gpu_f64_step.py): a launch keeps its state in double.
Every case first asserts, from the oracle, that the limits are engaged as it says: rows with a force and candidate rows without one."""
import warnings

import numpy as np
import pytest

from parity_metrics import relerr
from support_sims import swim_sim, wave_at, load_batch
from support_limits import (limited as _limited, scalar_q as _scalar_q, engaged_inputs as _engaged_inputs, phys as _phys,
                            rows_engaged as _rows_engaged, excess as _excess, tape as _tape, ENGAGED_SEEDS as SEEDS)

pytestmark = pytest.mark.gpu

N = 4
FMJ_WARN_BADQVEL = 2
TREES = ('shape1', 'shape4', 'shape6', 'shape10')      # wide_trees.WIDE_SHAPES: 128 / 127 / 68 / 65 dofs, dof chains of 64 / 20 / 40 / 30
MODELS = ('salamander33', 'eel48', 'centipede_20_25') + TREES


@pytest.mark.parametrize('integrator', ['euler', 'implicitfast'])
@pytest.mark.parametrize('name', MODELS)
def test_one_step_and_forward_to_the_ulp(oracle, name, integrator):
    m = _limited(name, integrator=integrator)
    inputs = _engaged_inputs(m, N, SEEDS[name])
    for forward in (False, True):
        phys, ins = _phys(m, N, *inputs)
        if not forward:
            pos, idle = _rows_engaged(oracle, m, ins)
            print(name, 'rows with a force per env', pos, 'candidate rows without', idle)
            assert pos.min() >= 5 and idle.min() >= 1, (name, pos, idle)
        ex, ref = _excess(oracle, m, phys, ins, forward)
        print(name, integrator, 'forward' if forward else 'step', 'error / bound per field:', {k: round(v, 3) for k, v in ex.items()})
        njs, nl = m.n_sensor_joints, 6*(m.nbody - 1)
        assert np.abs(ref['sensordata'][:, nl + 2:nl + 3*njs:3]).max() > 0      # the reference has limit forces
        bad = {k: v for k, v in ex.items() if v > 1.0}
        assert not bad, (name, integrator, forward, bad)
        if name == 'salamander33' and not forward:      # also runs on the fp32 constraint kernel, which is further from the oracle
            p32, i32 = _phys(m, N, *inputs, precision='fp32')
            ex32, _ = _excess(oracle, m, p32, i32, False)
            print(name, integrator, 'fp32 context, error / bound per field:', {k: round(v, 3) for k, v in ex32.items()})
            assert ex32['qvel'] > ex['qvel'] and ex32['qacc'] > ex['qacc'], (ex32, ex)


@pytest.mark.parametrize('name', ['eel48', 'shape6'])
def test_the_solver_the_model_names_does_not_matter(name):
    import torch
    from farms_mujoco_amd.model import SOLVERS
    outs = []
    for solver in ('pgs', 'newton'):
        m = _limited(name)
        m.solver = SOLVERS[solver]
        inputs = _engaged_inputs(m, N, SEEDS[name])
        with warnings.catch_warnings(record=True) as w:
            warnings.simplefilter('always')
            phys, _ = _phys(m, N, *inputs)
        said = [str(x.message) for x in w if 'primal Newton solve' in str(x.message)]
        assert len(said) == (solver == 'pgs'), (solver, [str(x.message) for x in w])      # only when the model asked for another solver
        assert (phys.solver_requested, phys.solver_effective, phys.solver_budget) == ({'pgs': 'PGS', 'newton': 'Newton'}[solver], 'Newton', 100)
        phys.step(3)
        torch.cuda.synchronize()
        assert int(phys.data.status.abs().sum()) == 0
        outs.append({k: getattr(phys.data, k).clone() for k in ('qpos', 'qvel', 'qacc', 'qacc_warmstart', 'sensordata', 'xpos', 'xquat', 'xipos')})
    for k in outs[0]:
        assert torch.equal(outs[0][k], outs[1][k]), k
    assert float(outs[0]['qacc_warmstart'].abs().max()) > 0


@pytest.mark.parametrize('name', ['eel48', 'centipede_20_25'])
def test_limits_that_never_engage_change_no_bit(name):
    """Range +-10: no row is ever a candidate, and every step is the unconstrained kernel's - 50 steps of fmj_step and 10 iterations of
    fmj_step_fused_f64 against an fp64 context of the same model with jnt_limited cleared."""
    import torch
    from support_sims import rows
    a, b = _limited(name, lim=10.0), _limited(name, lim=10.0)
    b.jnt_limited = np.zeros_like(b.jnt_limited)
    qpos, qvel, ctrl, xf, qs = _engaged_inputs(a, N, 5)
    pa, _ = _phys(a, N, qpos, qvel, ctrl, xf, qs)
    pb, _ = _phys(b, N, qpos, qvel, ctrl, xf, qs, limits=False)
    assert pa.has_constraints and not pb.has_constraints
    pa.step(50); pb.step(50)
    torch.cuda.synchronize()
    assert int(pa.data.status.abs().sum()) == 0
    for k in ('qpos', 'qvel', 'qacc', 'sensordata', 'xpos', 'xquat', 'xipos', 'time'):
        assert torch.equal(getattr(pa.data, k), getattr(pb.data, k)), k
    T = 10
    sa = swim_sim(N, T, m=a, seed=9, controller_of=wave_at(1.5), precision='fp64', fp64_fused=True, fp64_limits=True)[0]
    sb = swim_sim(N, T, m=b, seed=9, controller_of=wave_at(1.5), precision='fp64', fp64_fused=True)[0]
    assert sa.task.fusable() and sb.task.fusable()
    sa.run(); sb.run()
    torch.cuda.synchronize()
    assert sa.task.sim_iteration == T and int(sa.physics.data.status.abs().sum()) == 0
    for k in ('qpos', 'qvel', 'sensordata', 'xpos', 'xquat', 'xipos'):
        assert torch.equal(getattr(sa.physics.data, k), getattr(sb.physics.data, k)), k
    ra, rb = rows(sa), rows(sb)
    for k in ra:
        assert np.array_equal(ra[k], rb[k]), k


@pytest.mark.parametrize('recipe', ['A', 'B'])
def test_trajectory_against_the_state_rounding_floor(oracle, recipe):
    """One fmj_step launch from rest under a ctrl tape.  A: eel(48), every joint limited to +-0.1, margin 0.01 on the even joints, 300
    steps: some row carries a force in at least 90 % of the steps of every env.  B: joints 1::4 limited to +-0.25, 600 steps: a
    candidate row exists in 50 % to 90 % of the steps, so both branches of the kernel alternate within the launch."""
    import torch
    m, T = (_limited('eel48', 0.1, 0.01), 300) if recipe == 'A' else (_limited('eel48', 0.25, 0.0, slice(1, None, 4)), 600)
    tape32 = _tape(m, N, T, 2.0)
    tape = tape32.astype(np.float64)
    q0 = np.tile(m.qpos0, (N, 1)); v0 = np.zeros((N, m.nv))
    # the conditions, from a step-by-step oracle run (the warm start carried as mj_step carries it)
    q, v, ws = q0, v0, None
    with_force = np.zeros(N); with_row = np.zeros(N)
    for t in range(T):
        o = oracle.step_tf(m, q, v, ctrl=tape[t], warmstart=ws, want_AR=False)
        with_row += o['nefc'] > 0
        with_force += np.array([(o['efc'][e, :o['nefc'][e], 0] > 0).any() for e in range(N)])
        q, v, ws = o['qpos'], o['qvel'], o['warmstart']
    print(recipe, 'share of steps with a force', with_force/T, 'with a candidate row', with_row/T)
    if recipe == 'A':
        assert (with_force/T).min() >= 0.9, with_force/T
    else:
        assert 0.5 <= (with_row/T).min() and (with_row/T).max() <= 0.9, with_row/T
    ref = oracle.step(m, q0, v0, ctrl=tape, n_steps=T, ctrl_step_stride=N*m.nu, n_threads=4)
    fq, fv = q0, v0
    for t in range(T):      # floor_state: the oracle's own run with the state rounded to fp32 every step
        o = oracle.step(m, fq, fv, ctrl=tape[t], n_steps=1, n_threads=4)
        fq = o['qpos'].astype(np.float32).astype(np.float64); fv = o['qvel'].astype(np.float32).astype(np.float64)
    phys, _ = _phys(m, N, q0, v0)
    phys.step(T, torch.as_tensor(tape32, device=phys.device).contiguous())
    torch.cuda.synchronize()
    assert int(phys.data.status.abs().sum()) == 0
    for k, fl in (('qpos', fq), ('qvel', fv)):
        err, floor = relerr(getattr(phys.data, k).cpu().numpy(), ref[k]), relerr(fl, ref[k])
        print(recipe, k, 'after', T, 'steps: fp64 kernel %.3g  floor_state %.3g  ratio %.3g' % (err, floor, err/floor))
        assert err <= floor, (recipe, k, err, floor)


@pytest.mark.parametrize('fused', [False, True])
def test_through_the_simulation(oracle, fused):
    """eel(48) with recipe A's limits, wave controller and drag, 40 iterations: per-iteration (fp64_limits=True) and in one fused launch
    (fp64_fused=True as well), against oracle.run_fused with the measures and bounds of the unconstrained cases in
    test_gpu_f64_step.py (per-iteration) and test_gpu_f64_fused.py (fused)."""
    import support_f64_fused as F
    T = 40
    m = _limited('eel48', 0.1, 0.01)
    kw = dict(fp64_fused=True) if fused else {}
    sim = swim_sim(N, T, m=m, seed=9, controller_of=wave_at(1.5), water_kwargs=dict(height=F.SURFACE['eel48'], velocity=F.CURRENT),
                   precision='fp64', fp64_limits=True, **kw)[0]
    rng = np.random.default_rng(77)
    qpos = np.tile(m.key_qpos, (N, 1)); qpos[:, _scalar_q(m)] = rng.uniform(-0.12, 0.12, (N, len(_scalar_q(m))))
    load_batch(sim, qpos, np.zeros((N, m.nv)))
    assert sim.physics.has_constraints and sim.task.fusable() == fused
    ref, floor, fst = F._references(oracle, sim, m, T)
    assert np.abs(ref['joints'][..., 9]).max() > 0      # FMJ_JOINT_LIMIT_FORCE
    sim.run()
    got = F._got(sim)
    assert not got['status'].any() and sim.task.sim_iteration == T and sim._env_order is None      # no contact ordering
    assert np.abs(got['joints'][..., 9]).max() > 0
    if fused:
        F._check_one_pass_rows(got, ref, (0, 1), 'limited eel48, fused')
        F._check_run(got, ref, floor, fst, 'limited eel48, fused')
    else:
        err = {k: relerr(got[k], ref[k]) for k in ('qpos', 'links', 'joints', 'xfrc')}; fl = {k: relerr(fst[k], ref[k]) for k in err}
        print('limited eel48, per-iteration: whole-tensor error', err, 'fp32-storage run', fl)
        assert err['qpos'] <= fl['qpos']/10, (err, fl)
        assert err['links'] <= fl['links'] and err['xfrc'] <= fl['xfrc'] and err['joints'] <= fl['joints'], (err, fl)


def test_a_nan_freezes_one_env_and_leaves_the_rest_alone():
    import torch
    m = _limited('eel48')
    qpos, qvel, ctrl, xf, qs = _engaged_inputs(m, N, SEEDS['eel48'])
    clean, _ = _phys(m, N, qpos, qvel, ctrl, xf, qs)
    clean.step(3)
    bad_v = qvel.copy(); bad_v[2, m.nv - 1] = np.nan
    phys, _ = _phys(m, N, qpos, bad_v, ctrl, xf, qs)
    fields = ('qpos', 'qvel', 'qacc', 'qacc_warmstart', 'xpos', 'xquat', 'xipos', 'sensordata', 'time')
    before = {k: getattr(phys.data, k)[2].clone() for k in fields}
    phys.step(3)
    torch.cuda.synchronize()
    st = phys.data.status.cpu().numpy()
    assert st[2] & FMJ_WARN_BADQVEL and not st[[0, 1, 3]].any(), st
    for k, v in before.items():
        assert torch.equal(getattr(phys.data, k)[2].view(torch.int32), v.view(torch.int32)), k
    keep = [0, 1, 3]
    assert float(clean.data.sensordata[keep][:, 6*(m.nbody - 1) + 2::3][:, :m.n_sensor_joints].abs().max()) > 0      # limits engaged
    for k in fields:
        assert torch.equal(getattr(phys.data, k)[keep], getattr(clean.data, k)[keep]), k
