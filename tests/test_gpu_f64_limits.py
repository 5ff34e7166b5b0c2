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
from wide_trees import shape_tree
from support_models import tree_inputs
from support_sims import f64 as _f64, swim_sim, wave_at, load_batch

pytestmark = pytest.mark.gpu

N = 4
FMJ_WARN_BADQVEL = 2
TREES = ('shape1', 'shape4', 'shape6', 'shape10')      # wide_trees.WIDE_SHAPES: 128 / 127 / 68 / 65 dofs, dof chains of 64 / 20 / 40 / 30
MODELS = ('salamander33', 'eel48', 'centipede_20_25') + TREES
# the seed of each model's inputs: the first of 100, 101, ... (0, 1, ... for the larger models) at which the oracle finds, in every
# env, at least 5 rows with a force and a candidate row without one (the test asserts both before it looks at the device)
SEEDS = {'salamander33': 104, 'eel48': 100, 'centipede_20_25': 2, 'shape1': 3, 'shape4': 4, 'shape6': 5, 'shape10': 6}


def _base(name):
    import farms_mujoco_amd.model as mm
    if name.startswith('shape'):
        return shape_tree(int(name[5:]))
    return {'salamander33': lambda: mm.salamander33(limits=True), 'eel48': lambda: mm.eel(n_joints=48),
            'centipede_20_25': lambda: mm.centipede(20, 25)}[name]()


def _newton(m):
    from farms_mujoco_amd.model import SOLVERS
    m.solver = SOLVERS['newton']; m.solver_iterations = 100
    return m


def _limited(name, lim=0.1, margin_even=0.02, which=slice(None), integrator='euler'):
    """The model with joints ``which`` (of its hinge and slide joints) limited to +-lim, ``margin_even`` on the even joints, set after
    the build as test_fp64_refuses_limits does; the solver fields are the reference's: Newton, 100 iterations."""
    import farms_mujoco_amd.model as mm
    m = _base(name)
    assert m.ngeom == 0
    on = np.zeros(m.njnt, bool); on[which] = True
    on &= m.jnt_type != 0
    m.jnt_limited = on.astype(m.jnt_limited.dtype)
    m.jnt_range = np.tile([-lim, lim], (m.njnt, 1)).astype(float)
    margin = np.zeros(m.njnt); margin[::2] = margin_even
    m.jnt_margin = margin
    m.integrator = mm.INTEGRATORS[integrator]
    return _newton(m)


def _scalar_q(m):
    return m.jnt_qposadr[m.jnt_type != 0]


def _engaged_inputs(m, n, seed):
    """tree_inputs with the joint positions uniform in +-0.15, qvel normal x 0.5 and ctrl uniform in +-0.3."""
    qpos, qvel, ctrl, xf, qs = tree_inputs(m, n, seed)
    rng = np.random.default_rng([4242, seed])
    qpos[:, _scalar_q(m)] = rng.uniform(-0.15, 0.15, (n, len(_scalar_q(m))))
    qvel = rng.normal(size=(n, m.nv))*0.5
    ctrl = rng.uniform(-0.3, 0.3, (n, max(m.nu, 1)))[:, :m.nu]
    return qpos, qvel, ctrl, xf, qs


def _phys(m, n, qpos, qvel, ctrl=None, xf=None, qs=None, precision='fp64', limits=True):
    import test_gpu_f64_step as S
    import torch
    from farms_mujoco_amd.physics import BatchedPhysics
    if precision == 'fp32':
        return S._phys(m, n, qpos, qvel, ctrl, xf, qs, precision)
    phys = BatchedPhysics(m, n, precision='fp64', fp64_limits=limits)
    assert phys.precision == 'fp64' and phys.kernel_info()['threads_per_env'] == 128
    d = phys.data
    f32 = lambda a: torch.as_tensor(np.asarray(a), dtype=torch.float32)
    d.qpos[:] = f32(qpos); d.qvel[:] = f32(qvel)
    if xf is not None:
        d.xfrc_applied[:] = f32(xf)
    if qs is not None:
        d.qpos_spring[:] = f32(qs)
    if ctrl is not None and m.nu:
        d.ctrl[:] = f32(ctrl)
    return phys, dict(qpos=_f64(d.qpos), qvel=_f64(d.qvel), ctrl=_f64(d.ctrl) if m.nu else None, xfrc_applied=_f64(d.xfrc_applied),
                      qpos_spring=_f64(d.qpos_spring))


def _rows_engaged(oracle, m, ins):
    """Per env, from oracle.step_tf: the rows with a positive force and the candidate rows with none."""
    o = oracle.step_tf(m, ins['qpos'], ins['qvel'], ctrl=ins['ctrl'], qpos_spring=ins['qpos_spring'], xfrc_applied=ins['xfrc_applied'], want_AR=False)
    pos = np.array([(o['efc'][e, :o['nefc'][e], 0] > 0).sum() for e in range(len(o['nefc']))])
    return pos, o['nefc'] - pos


def _excess(oracle, m, phys, ins, forward):
    import test_gpu_f64_step as S
    import torch
    q0, v0 = phys.data.qpos.clone(), phys.data.qvel.clone()
    if forward:
        phys.forward()
    else:
        phys.step(1)
    torch.cuda.synchronize()
    assert int(phys.data.status.abs().sum()) == 0
    ref = oracle.step(m, ins['qpos'], ins['qvel'], ctrl=ins['ctrl'], qpos_spring=ins['qpos_spring'], xfrc_applied=ins['xfrc_applied'])
    if forward:
        assert torch.equal(phys.data.qpos, q0) and torch.equal(phys.data.qvel, v0)
        ref = dict(ref, qpos=ins['qpos'], qvel=ins['qvel'])
    groups = S._field_groups(m)
    return {k: S.ulp_excess(getattr(phys.data, k).cpu().numpy(), ref[k], groups[k]) for k in ('qpos', 'qvel', 'qacc', 'sensordata')}, ref


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


def _tape(m, n, T, f):
    """ctrl[t, env, a] = 0.3 sin(2 pi f t + 0.7 env - 2 pi a / nu), rounded to fp32 as the device holds it."""
    t = np.arange(T)[:, None, None]*m.timestep
    tape = 0.3*np.sin(2*np.pi*f*t + 0.7*np.arange(n)[None, :, None] - 2*np.pi*np.arange(m.nu)[None, None, :]/m.nu)
    return tape.astype(np.float32)


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
    import test_gpu_f64_fused as F
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
