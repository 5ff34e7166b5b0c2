"""RK4 inside the fp64 step kernel (BatchedPhysics(precision='fp64', fp64_rk4=True): fmj_create_ex2 with FMJ_CREATE_F64_RK4,
fmj_step_f64_rk4_kernel of csrc/fmj_f64_step.inc) against the plain fp64 oracle, whose rk4() restates mj_RungeKutta.

One step and fmj_forward are held to the rounding of the fp32 store, the bound of test_gpu_f64_step.py:
    |got - ref| <= ulp32(ref_i) + ulp32(max |ref| over the component's column group in that env)
Four passes in double add arithmetic noise of the size one pass adds (1e-9 of the group's size at the documented condition numbers),
far below one ulp32.  Trajectories are held to the oracle's own RK4 run with the state rounded to fp32 after every step; the order of
convergence to the window test_oracle_rk4.py holds the oracle to."""
import numpy as np
import pytest

from parity_metrics import relerr
from support_sims import wave_at, load_batch
from support_limits import scalar_q as _scalar_q, engaged_inputs as _engaged_inputs, tape as _tape, as_fp32_inputs
from support_f64_rk4 import (rk4_model, rk4_limited, as_euler, phys as _phys, oracle_kw, first_pass, second_stage, rk4_swim_sim, FIELDS)

pytestmark = pytest.mark.gpu

N = 4
FMJ_WARN_BADQVEL, FMJ_WARN_BADQACC = 2, 4
PLAIN = ('salamander33', 'eel48', 'centipede_20_25', 'shape1', 'shape6', 'tree0', 'tree1', 'tree2', 'tree3')
LIMITED = ('salamander33', 'eel48', 'centipede_20_25', 'shape6')


def _case(name, limits):
    """The model, its inputs (tree_inputs / engaged_inputs with the seeds of test_gpu_f64_step.py / test_gpu_f64_limits.py)."""
    import support_f64_step as S
    from support_limits import ENGAGED_SEEDS
    from support_models import tree_inputs
    if limits:
        m = rk4_limited(name)
        return m, _engaged_inputs(m, N, ENGAGED_SEEDS[name])
    m = rk4_model(name)
    return m, tree_inputs(m, N, S.MODELS.index(name))


@pytest.mark.parametrize('name,limits', [(n, False) for n in PLAIN] + [(n, True) for n in LIMITED])
def test_one_step_and_forward_to_the_ulp(oracle, name, limits):
    import torch
    import support_f64_step as S
    from support_limits import rows_engaged
    m, inputs = _case(name, limits)
    groups = S._field_groups(m)
    for forward in (False, True):
        phys, ins = _phys(m, N, *inputs, limits=limits)
        if limits and not forward:      # the first pass is the Euler twin's forward pass
            pos, idle = rows_engaged(oracle, as_euler(m), ins)
            print(name, 'first pass: rows with a force per env', pos, 'candidate rows without', idle)
            assert pos.min() >= 5 and idle.min() >= 1, (name, pos, idle)
        q0, v0 = phys.data.qpos.clone(), phys.data.qvel.clone()
        if forward:
            phys.forward()
        else:
            phys.step(1)
        torch.cuda.synchronize()
        assert int(phys.data.status.abs().sum()) == 0
        fp = first_pass(oracle, m, ins)
        if forward:      # the first pass alone, the state left alone
            assert torch.equal(phys.data.qpos, q0) and torch.equal(phys.data.qvel, v0)
            ref = fp
        else:
            ref = oracle.step(m, ins['qpos'], ins['qvel'], **oracle_kw(ins))
            assert not ref['status'].any()
        got = {k: getattr(phys.data, k).cpu().numpy() for k in FIELDS}
        ex = {k: S.ulp_excess(got[k], ref[k], groups[k]) for k in FIELDS}
        print(name, 'limits' if limits else 'plain', 'forward' if forward else 'step', 'error / bound per field:', {k: round(v, 3) for k, v in ex.items()})
        bad = {k: v for k, v in ex.items() if v > 1.0}
        assert not bad, (name, limits, forward, bad)
        if limits:
            njs, nl = m.n_sensor_joints, 6*(m.nbody - 1)
            assert np.abs(ref['sensordata'][:, nl + 2:nl + 3*njs:3]).max() > 0      # the reference has limit forces
        if not forward:
            # the test tells the integrators apart, and the poses are the last pass's
            eu = oracle.step(as_euler(m), ins['qpos'], ins['qvel'], **oracle_kw(ins))
            apart, err = np.abs(eu['qvel'] - ref['qvel']).max(), np.abs(got['qvel'] - ref['qvel']).max()
            moved = np.abs(ref['xpos'] - fp['xpos']).max()
            print(name, 'Euler - RK4 in qvel %.3g, device error %.3g; xpos of the last pass - first %.3g' % (apart, err, moved))
            assert apart > 10*err, (name, apart, err)
            assert moved > 1e-6, (name, moved)


def test_forward_debug_rows_are_m(oracle):
    """fmj_forward_debug on an RK4 context: H_rows is M (no h B on the diagonal), qfrc_smooth as ever."""
    import torch
    import support_f64_step as S
    from wide_trees import dof_depth
    m, inputs = _case('salamander33', False)
    assert np.abs(m.dof_damping).max() > 0
    phys, ins = _phys(m, N, *inputs)
    H, qf = phys.forward_debug()
    torch.cuda.synchronize()
    depth = dof_depth(m)
    Href = np.zeros(H.shape); qref = np.zeros((N, m.nv))
    for e in range(N):
        o = oracle.forward_debug(m, ins['qpos'][e], ins['qvel'][e], ctrl=ins['ctrl'][e], qpos_spring=ins['qpos_spring'][e], xfrc_applied=ins['xfrc_applied'][e])
        for i in range(m.nv):
            j = i
            while j >= 0:
                Href[e, i, depth[j]] = o['M'][i, j]; j = m.dof_parentid[j]
        qref[e] = o['qfrc_smooth']
    eh, eq = S.ulp_excess(H.cpu().numpy(), Href), S.ulp_excess(qf.cpu().numpy(), qref)
    print('RK4 context: H error / bound', eh, 'qfrc_smooth error / bound', eq)
    assert eh <= 1.0 and eq <= 1.0, (eh, eq)


def _order_inputs(h):
    """The set-up of test_oracle_rk4._run: salamander33 at timestep h, synthetic_batch(seed=1), a constant ctrl on the first 27 actuators."""
    from farms_mujoco_amd.model import salamander33, synthetic_batch
    m = salamander33(timestep=h)
    m.integrator = 1
    q, v, _ = synthetic_batch(m, 2, seed=1)
    ctrl = np.zeros((2, m.nu)); ctrl[:, :27] = 0.2*np.sin(np.arange(27))
    return m, q, v, ctrl


def test_fourth_order_on_the_device(oracle):
    """e(h) = max |qpos(device, h) - qpos(oracle RK4, h = 1e-3 / 16)| after T seconds, each device run ONE fmj_step launch."""
    import torch
    f32 = lambda a: np.asarray(a, np.float32).astype(np.float64)
    hs = (1e-3, 5e-4)
    used = None
    for T in (0.032, 0.064, 0.128, 0.256):      # lengthened until the oracle's own error at 5e-4 stands clear of the fp32 store
        m, q, v, ctrl = _order_inputs(1e-3/16)
        q, v, ctrl = f32(q), f32(v), f32(ctrl)
        ref = oracle.step(m, q, v, ctrl=ctrl, n_steps=int(round(T/m.timestep)), n_threads=2)
        m2 = _order_inputs(5e-4)[0]
        e_half = np.abs(oracle.step(m2, q, v, ctrl=ctrl, n_steps=int(round(T/5e-4)), n_threads=2)['qpos'] - ref['qpos']).max()
        half_ulp = 0.5*float(np.spacing(np.float32(np.abs(ref['qpos']).max())))
        print('T', T, 'oracle e(5e-4) %.3g, half an ulp32 of the largest |qpos| %.3g' % (e_half, half_ulp))
        if e_half >= 5*half_ulp:
            used = T
            break
    assert used is not None
    print('T used:', used)
    err = {}
    for integrator in (1, 0):
        for h in hs:
            m = _order_inputs(h)[0]
            m.integrator = integrator
            phys, ins = _phys(m, 2, q, v, ctrl, rk4=bool(integrator))
            assert np.array_equal(ins['qpos'], q) and np.array_equal(ins['ctrl'], ctrl)
            phys.step(int(round(used/h)))
            torch.cuda.synchronize()
            assert int(phys.data.status.abs().sum()) == 0
            err[integrator, h] = np.abs(phys.data.qpos.cpu().numpy().astype(np.float64) - ref['qpos']).max()
    r4, r1 = err[1, hs[0]]/err[1, hs[1]], err[0, hs[0]]/err[0, hs[1]]
    print('device RK4 errors %.3g %.3g ratio %.3g; device Euler errors %.3g %.3g ratio %.3g' % (err[1, hs[0]], err[1, hs[1]], r4, err[0, hs[0]], err[0, hs[1]], r1))
    assert 0.75*16 < r4 < 1.3*16, (err, r4)
    assert err[1, hs[0]] < 2e-5, err
    assert 0.75*2 < r1 < 1.3*2, (err, r1)


_TRAJ = {}


TRAJ_T = 300      # recipe A's own length: over its first 100 steps from rest only 81 % of env 0's steps carry a force (200: 90.5 %, 300: 93.7 %)


def _trajectory(oracle, T=TRAJ_T):
    """Recipe A of test_gpu_f64_limits.py with RK4: eel(48), every joint limited to +-0.1, margin 0.01 on the even joints, from rest
    under a ctrl tape.  The oracle's run, its run with the state rounded to fp32 after every step (the floor), and the share of steps
    with a limit force - computed once."""
    if T not in _TRAJ:
        m = rk4_limited('eel48', 0.1, 0.01)
        tape32 = _tape(m, N, T, 2.0)
        tape = tape32.astype(np.float64)
        q0 = np.tile(m.qpos0, (N, 1)); v0 = np.zeros((N, m.nv))
        q, v, ws = q0, v0, None
        with_force = np.zeros(N)
        for t in range(T):
            o = oracle.step_tf(m, q, v, ctrl=tape[t], warmstart=ws, want_AR=False)
            with_force += np.array([(o['efc'][e, :o['nefc'][e], 0] > 0).any() for e in range(N)])
            q, v, ws = o['qpos'], o['qvel'], o['warmstart']
        ref = oracle.step(m, q0, v0, ctrl=tape, n_steps=T, ctrl_step_stride=N*m.nu, n_threads=4)
        fq, fv = q0, v0
        for t in range(T):
            o = oracle.step(m, fq, fv, ctrl=tape[t], n_steps=1, n_threads=4)
            fq = o['qpos'].astype(np.float32).astype(np.float64); fv = o['qvel'].astype(np.float32).astype(np.float64)
        floor = dict(qpos=relerr(fq, ref['qpos']), qvel=relerr(fv, ref['qvel']))
        _TRAJ[T] = (m, tape32, q0, v0, ref, floor, with_force/T)
    return _TRAJ[T]


def test_trajectory_against_the_state_rounding_floor(oracle):
    import torch
    T = TRAJ_T
    m, tape32, q0, v0, ref, floor, share = _trajectory(oracle, T)
    print('share of steps with a limit force', share)
    assert share.min() >= 0.9, share
    phys, _ = _phys(m, N, q0, v0, limits=True)
    phys.step(T, torch.as_tensor(tape32, device=phys.device).contiguous())
    torch.cuda.synchronize()
    assert int(phys.data.status.abs().sum()) == 0
    assert float(phys.data.time.min()) == pytest.approx(T*m.timestep, rel=1e-5)
    for k in ('qpos', 'qvel'):
        err = relerr(getattr(phys.data, k).cpu().numpy(), ref[k])
        print(k, 'after', T, 'RK4 steps: fp64 kernel %.3g  floor_state %.3g  ratio %.3g' % (err, floor[k], err/floor[k]))
        assert err <= floor[k], (k, err, floor[k])


def _limited_swim(T, fused):
    import support_f64_fused as F
    m = rk4_limited('eel48', 0.1, 0.01)
    assert m.timestep == 1e-3
    kw = dict(fp64_fused=True) if fused else {}
    sim = rk4_swim_sim(N, T, m, controller_of=wave_at(1.5), water_kwargs=dict(height=F.SURFACE['eel48'], velocity=F.CURRENT), fp64_limits=True, **kw)
    rng = np.random.default_rng(77)
    qpos = np.tile(m.key_qpos, (N, 1)); qpos[:, _scalar_q(m)] = rng.uniform(-0.12, 0.12, (N, len(_scalar_q(m))))
    load_batch(sim, qpos, np.zeros((N, m.nv)))
    return sim, m


@pytest.mark.parametrize('fused', [False, True])
def test_through_the_simulation(oracle, fused):
    """eel(48) with recipe A's limits, wave controller, drag and a current, 40 RK4 iterations: per-iteration (fmj_before_step +
    fmj_step(1)) and in one fused launch, against oracle.run_fused with the measures and bounds of test_gpu_f64_limits.py."""
    import support_f64_fused as F
    T = 40
    sim, m = _limited_swim(T, fused)
    assert sim.physics.rk4 and sim.physics.fp64_rk4 and sim.physics.has_constraints
    assert sim.task.fusable() == fused and sim.task.host_step_only == (not fused)
    ref, floor, fst = F._references(oracle, sim, m, T)
    assert np.abs(ref['joints'][..., 9]).max() > 0      # FMJ_JOINT_LIMIT_FORCE
    sim.run()
    got = F._got(sim)
    assert not got['status'].any() and sim.task.sim_iteration == T
    assert np.abs(got['joints'][..., 9]).max() > 0
    if fused:
        F._check_one_pass_rows(got, ref, (0, 1), 'limited RK4 eel48, fused')
        F._check_run(got, ref, floor, fst, 'limited RK4 eel48, fused')
    else:
        err = {k: relerr(got[k], ref[k]) for k in ('qpos', 'links', 'joints', 'xfrc')}; fl = {k: relerr(fst[k], ref[k]) for k in err}
        print('limited RK4 eel48, per-iteration: whole-tensor error', err, 'fp32-storage run', fl)
        assert err['qpos'] <= fl['qpos']/10, (err, fl)
        assert err['links'] <= fl['links'] and err['xfrc'] <= fl['xfrc'] and err['joints'] <= fl['joints'], (err, fl)


def test_a_tree_past_64_dofs_fused(oracle):
    """centipede(20, 25), unlimited, RK4, fused: the two-wave sizes."""
    import support_f64_fused as F
    T = 40
    m = rk4_model('centipede_20_25')
    assert m.timestep == 1e-3 and m.nv > 64
    sim = rk4_swim_sim(N, T, m, controller_of=wave_at(1.5), water_kwargs=dict(height=F.SURFACE['centipede_20_25'], velocity=F.CURRENT), fp64_fused=True)
    assert sim.task.fusable() and not sim.task.host_step_only
    ref, floor, fst = F._references(oracle, sim, m, T)
    sim.run()
    got = F._got(sim)
    assert not got['status'].any() and sim.task.sim_iteration == T
    F._check_one_pass_rows(got, ref, (0, 1), 'RK4 centipede_20_25, fused')
    F._check_run(got, ref, floor, fst, 'RK4 centipede_20_25, fused')


def test_fused_chunks_resume_bitwise(tmp_path):
    """Two fused launches of 20 iterations, and the same with save_state / load_state into a fresh simulation between them."""
    import support_f64_fused as F
    T = 40
    a, _ = _limited_swim(T, True)
    assert a.step_fused(20) == 20 and a.step_fused(20) == 20
    ga = F._got(a)
    assert not ga['status'].any() and a.task.sim_iteration == T
    b, _ = _limited_swim(T, True)
    assert b.step_fused(20) == 20
    b.save_state(str(tmp_path/'mid.npz'))
    c, _ = _limited_swim(T, True)
    c.load_state(str(tmp_path/'mid.npz'))
    assert c.step_fused(20) == 20
    gc = F._got(c)
    for k in F.STATE:
        assert np.array_equal(ga[k].view(np.int32), gc[k].view(np.int32)), k
    for r in F.RING:      # the rows of iterations 20 .. 39 (those before were written by the simulation that saved)
        assert np.array_equal(ga[r][20:].view(np.int32), gc[r][20:].view(np.int32)), r


def test_step_3_against_three_steps_of_1(oracle):
    """fmj_step(3) keeps the state in double between its steps, three fmj_step(1) round it to fp32 twice: the two differ by no more
    than the oracle's state-rounded run differs from its plain run over the trajectory above."""
    import torch
    m, tape32, q0, v0, ref, floor, _ = _trajectory(oracle, TRAJ_T)
    a, _ = _phys(m, N, q0, v0, limits=True)
    b, _ = _phys(m, N, q0, v0, limits=True)
    warm = 20      # leave rest first, so that the state has digits to round
    wt = torch.as_tensor(tape32[:warm], device='cuda:0').contiguous()
    a.step(warm, wt); b.step(warm, wt)
    tape = torch.as_tensor(tape32[warm:warm + 3], device='cuda:0').contiguous()
    a.step(3, tape)
    for t in range(3):
        b.step(1, tape[t:t + 1].contiguous())
    torch.cuda.synchronize()
    assert int(a.data.status.abs().sum()) == 0 and int(b.data.status.abs().sum()) == 0
    assert torch.equal(a.data.time, b.data.time)
    for k in ('qpos', 'qvel'):
        d = relerr(getattr(b.data, k).cpu().numpy(), getattr(a.data, k).cpu().numpy().astype(np.float64))
        print(k, 'fmj_step(3) against 3 x fmj_step(1): %.3g, floor_state of the trajectory %.3g' % (d, floor[k]))
        assert d <= floor[k], (k, d, floor[k])


def test_a_nan_freezes_one_env_and_leaves_the_rest_alone():
    import torch
    from support_limits import ENGAGED_SEEDS
    m = rk4_limited('eel48')
    qpos, qvel, ctrl, xf, qs = _engaged_inputs(m, N, ENGAGED_SEEDS['eel48'])
    clean, _ = _phys(m, N, qpos, qvel, ctrl, xf, qs, limits=True)
    clean.step(3)
    bad_v = qvel.copy(); bad_v[2, m.nv - 1] = np.nan
    phys, _ = _phys(m, N, qpos, bad_v, ctrl, xf, qs, limits=True)
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


def test_a_failure_in_a_later_pass_undoes_the_step(oracle):
    """Env 1 gets a finite torque on one link, so large that the first pass's |qacc| stays below 1e10 while the pass at X[1] (the
    velocities advanced by h/2 of that acceleration: centripetal terms grow with its square) exceeds it - both asserted from the oracle
    first.  The env ends with FMJ_WARN_BADQACC and every field it had; the others step as in a clean run."""
    import torch
    from support_models import tree_inputs
    m = rk4_model('salamander33')
    qpos, qvel, ctrl, xf, qs = tree_inputs(m, N, 0)
    bad, body = 1, m.nbody//2
    unit = np.zeros((m.nbody, 6)); unit[body, 3:] = [0.3, 0.5, 1.0]
    base = as_fp32_inputs(m, qpos, qvel, ctrl, xf, qs)      # the inputs as the device holds them
    kw = lambda X, e: dict(ctrl=base['ctrl'][e], qpos_spring=base['qpos_spring'][e], xfrc_applied=X)
    a1 = np.abs(oracle.forward_debug(m, base['qpos'][bad], base['qvel'][bad], **kw(unit, bad))['qacc']).max()
    scale = np.float32(3e9/a1)
    big = (unit*scale).astype(np.float32).astype(np.float64)
    assert np.isfinite(big).all()
    ins = dict(base, xfrc_applied=base['xfrc_applied'].copy()); ins['xfrc_applied'][bad] = big
    fd, q1, v1 = second_stage(oracle, m, ins, bad)
    a0 = np.abs(fd['qacc']).max()
    a_x1 = np.abs(oracle.forward_debug(m, q1, v1, **kw(big, bad))['qacc'])
    print('torque scale %.3g: first pass max |qacc| %.3g, at X[1] %s, stage |qvel| %.3g' % (scale, a0, np.nanmax(a_x1), np.abs(v1).max()))
    assert a0 < 1e10 and np.abs(v1).max() < 1e10 and np.abs(q1).max() < 1e10
    assert not np.all(a_x1 <= 1e10)
    xf_bad = np.array(base['xfrc_applied']); xf_bad[bad] = big
    clean, _ = _phys(m, N, qpos, qvel, ctrl, xf, qs)
    phys, _ = _phys(m, N, qpos, qvel, ctrl, xf_bad, qs)
    for p in (clean, phys):
        p.forward()      # poses and sensors of the inputs: the frozen env must keep exactly these
    torch.cuda.synchronize()
    assert int(phys.data.status.abs().sum()) == 0
    fields = ('qpos', 'qvel', 'qacc', 'time', 'xpos', 'xquat', 'xipos', 'sensordata')
    before = {k: getattr(phys.data, k)[bad].clone() for k in fields}
    clean.step(2); phys.step(2)
    torch.cuda.synchronize()
    st = phys.data.status.cpu().numpy()
    keep = [e for e in range(N) if e != bad]
    assert st[bad] & FMJ_WARN_BADQACC and not st[keep].any() and not clean.data.status.any(), st
    for k, v in before.items():
        assert torch.equal(getattr(phys.data, k)[bad].view(torch.int32), v.view(torch.int32)), k
    for k in fields:
        assert torch.equal(getattr(phys.data, k)[keep], getattr(clean.data, k)[keep]), k
    assert float(clean.data.time[bad]) > 0
