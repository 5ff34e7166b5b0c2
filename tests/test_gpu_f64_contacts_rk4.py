"""RK4 on the fp64 contact solve (BatchedPhysics(precision='fp64', fp64_contacts=True, fp64_contacts_rk4=True): fmj_create_ex2 with
FMJ_CREATE_F64_CONTACTS | FMJ_CREATE_F64_CONTACTS_RK4, fmj_step_f64_terrain_rk4_kernel / fmj_step_f64_elliptic_rk4_kernel of
csrc/fmj_f64_step.inc) against the fp64 oracle, whose rk4() restates mj_RungeKutta with contacts.

One step and fmj_forward are held to the rounding of the fp32 store, the bound of test_gpu_f64_step.py, contact records included:
    |got - ref| <= ulp32(ref_i) + ulp32(max |ref| over the component's column group in that env)
What a step leaves: the first pass's sensors, the fourth pass's poses, qacc (the next warm start) and contact list.  Every case first
asserts its conditions from the oracle alone (support_f64_contacts_rk4.conditions; test_f64_contacts_rk4_recipes.py holds them without a
GPU).  Trajectories are held to the oracle's own RK4 run with the state rounded to fp32 every step."""
import numpy as np
import pytest

from parity_metrics import relerr
import support_f64_contacts as C
import support_f64_contacts_rk4 as R
from support_f64_contacts_rk4 import N, as_euler

pytestmark = pytest.mark.gpu

FMJ_WARN_BADQACC, FMJ_WARN_CONTACTFULL = 4, 8
FIELDS = C.STATE + ('contact', 'ncon')
_CASES = {}


def _case(oracle, case):
    """The model, its inputs, and the oracle's step and stage states at them - computed once per case."""
    if case not in _CASES:
        m = R.make(case)
        ins = R.inputs(case, m)
        ok, ref, st, what = R.conditions(oracle, case, m, ins)
        assert ok, (case, what)
        _CASES[case] = (m, ins, ref, st)
    return _CASES[case]


def _kernel_of(case):
    return 'fmj_step_f64_elliptic_rk4_kernel' if case.startswith('elliptic') else 'fmj_step_f64_terrain_rk4_kernel'


def _lists(p):
    """Per env (ncon, geom pairs) of the records the device holds."""
    ncon = p.data.ncon.cpu().numpy(); c16 = p.data.contact.cpu().numpy()
    out = []
    for e in range(len(ncon)):
        gg = np.ascontiguousarray(c16[e, :ncon[e], 15]).view(np.int32)
        out.append((int(ncon[e]), np.stack([gg >> 16, gg & 0xffff], axis=1)))
    return out


@pytest.mark.parametrize('case', list(R.CASES))
def test_one_step_and_forward_to_the_ulp(oracle, case):
    import torch
    m, ins, ref, st = _case(oracle, case)
    first = R.first_pass_reference(oracle, m, ins)
    for forward in (False, True):
        p = R.phys(case, m, N, ins)
        info = p.kernel_info()
        assert info['fp64_step_kernel'] == _kernel_of(case) and info['threads_per_env'] == 128 and 0 < info['lds_bytes_per_env'] <= 160*1024
        assert p.solver_effective == 'Newton' and p.rk4
        q0, v0 = p.data.qpos.clone(), p.data.qvel.clone()
        p.forward() if forward else p.step(1)
        ex = C._excess(m, p, first if forward else ref, forward, ins)      # (asserts status 0, ncon and the geom ids)
        print(case, 'forward' if forward else 'step', 'error / bound per field:', {k: round(v, 3) for k, v in ex.items()})
        bad = {k: v for k, v in ex.items() if v > 1.0}
        assert not bad, (case, forward, bad)
        got = _lists(p)
        if forward:      # the first pass alone, with its own contact list, the state left alone
            assert torch.equal(p.data.qpos, q0) and torch.equal(p.data.qvel, v0)
            assert all(g[0] == R.pass_list(s[0][2])[0] and np.array_equal(g[1], R.pass_list(s[0][2])[1]) for g, s in zip(got, st))
            continue
        # the records are the fourth pass's, not the first's
        assert all(g[0] == R.pass_list(s[3][2])[0] and np.array_equal(g[1], R.pass_list(s[3][2])[1]) for g, s in zip(got, st))
        assert any(g[0] != R.pass_list(s[0][2])[0] or not np.array_equal(g[1], R.pass_list(s[0][2])[1]) for g, s in zip(got, st))
        # the sensors are the first pass's: the oracle's step agrees with its forward pass there, and the poses moved since
        assert np.array_equal(ref['sensordata'], first['sensordata'])
        moved = np.abs(ref['xpos'] - first['xpos']).max()
        # the test tells the integrators apart
        eu = oracle.step(as_euler(m), ins['qpos'], ins['qvel'], ctrl=ins['ctrl'])
        apart = np.abs(eu['qvel'] - ref['qvel']).max()
        err = np.abs(p.data.qvel.cpu().numpy().astype(np.float64) - ref['qvel']).max()
        print(case, 'Euler - RK4 in qvel %.3g, device error %.3g; xpos of the last pass - first %.3g' % (apart, err, moved))
        assert apart > 10*err and moved > 1e-6, (case, apart, err, moved)
        ws = p.data.qacc_warmstart.cpu().numpy().astype(np.float64)      # the stored warm start is the fourth pass's qacc, not the first's
        d4 = np.abs(ws - ref['qacc_warmstart']).max(); d1 = np.abs(ws - first['qacc']).max()
        print(case, 'warm start: distance to the fourth pass %.3g, to the first %.3g' % (d4, d1))
        assert d1 > 10*d4, (d4, d1)


def test_an_euler_walker_steps_as_without_the_flag():
    import torch
    m = C.make('centipede_20_25')
    ins = C.inputs(m, N, C.SEEDS['centipede_20_25'])
    a = C.phys(m, N, ins, fp64_contacts_rk4=True)
    b = C.phys(m, N, ins)
    assert a.kernel_info()['fp64_step_kernel'] == b.kernel_info()['fp64_step_kernel'] == 'fmj_step_f64_contacts_kernel'
    assert a.kernel_info()['lds_bytes_per_env'] == b.kernel_info()['lds_bytes_per_env']
    a.step(20); b.step(20)
    torch.cuda.synchronize()
    assert int(a.data.status.abs().sum()) == 0 and int(a.data.ncon.max()) > 0      # (some env is on the ground at the end)
    for k in FIELDS + ('time',):
        assert torch.equal(getattr(a.data, k).view(torch.int32), getattr(b.data, k).view(torch.int32)), k


def test_no_contact_no_bit_changed():
    """The RK4 centipede 1 m above the plane, 20 steps: every pass is the unconstrained RK4 kernel's, against an fp64_rk4 context of the
    same model with its geoms removed."""
    import torch
    a, b = R.make('centipede_20_25'), R.make('centipede_20_25')
    C.set_geoms(b, [], 0)
    ins = C.inputs(a, N, 5, depth=-1.0)
    assert min(C.lowest_point(a, q) for q in ins['qpos']) > 0.99
    pa = R.phys('centipede_20_25', a, N, ins)
    pb = C.phys(b, N, ins, fp64_contacts=False, fp64_rk4=True)
    assert pb.kernel_info()['fp64_step_kernel'] == 'fmj_step_f64_rk4_kernel'
    pa.step(20); pb.step(20)
    torch.cuda.synchronize()
    assert int(pa.data.status.abs().sum()) == 0 and int(pa.data.ncon.abs().sum()) == 0
    for k in ('qpos', 'qvel', 'qacc', 'sensordata', 'xpos', 'xquat', 'xipos', 'time'):
        assert torch.equal(getattr(pa.data, k), getattr(pb.data, k)), k


def test_a_full_contact_list_is_truncated_and_reported(oracle):
    import copy
    import support_f64_step as S
    import torch
    m0, ins, full, _ = _case(oracle, 'centipede_20_25')
    m = copy.copy(m0)
    m.max_contacts = int(full['ncon'].min()) - 2      # below every env's fourth-pass count
    assert m.max_contacts >= 4
    a = oracle.step(m, ins['qpos'], ins['qvel'], ctrl=ins['ctrl'])
    b = oracle.step_tf(m, ins['qpos'], ins['qvel'], ctrl=ins['ctrl'], want_AR=False)
    assert np.all(b['ncon'] == m.max_contacts) and np.all(a['status'] == FMJ_WARN_CONTACTFULL)
    p = R.phys('centipede_20_25', m, N, ins)
    p.step(1)
    torch.cuda.synchronize()
    st = p.data.status.cpu().numpy()
    assert np.all(st == FMJ_WARN_CONTACTFULL), st      # reported, and nothing else
    assert np.array_equal(p.data.ncon.cpu().numpy(), b['ncon'])
    c16 = p.data.contact.cpu().numpy()
    for e in range(N):      # the kept records are the oracle's: the first max_contacts of its order, both geom ids
        gg = np.ascontiguousarray(c16[e, :, 15]).view(np.int32)
        assert np.array_equal(gg >> 16, b['contact'][e, :, 15].astype(int)) and np.array_equal(gg & 0xffff, b['contact'][e, :, 16].astype(int))
        assert np.all(np.diff(gg & 0xffff) >= 0)
    exc = C._contact_excess(c16, b['ncon'], dict(ncon=b['ncon'], contact=b['contact'][..., :15]))      # pos, frame and force of the truncated solve
    print('truncated list, records error / bound:', exc)
    assert exc <= 1.0, exc
    groups = C._groups(m)
    ex = {k: S.ulp_excess(getattr(p.data, k).cpu().numpy(), a[k], groups[k]) for k in ('qpos', 'qvel', 'qacc')}
    print('truncated list, error / bound:', ex)
    assert max(ex.values()) <= 1.0, ex
    p.step(1)      # not frozen: the next step moves the state
    torch.cuda.synchronize()
    assert not np.array_equal(p.data.qpos.cpu().numpy(), a['qpos'].astype(np.float32)) and float(p.data.time[0]) > 1.5*m.timestep


def test_a_nan_ctrl_freezes_one_env_and_leaves_the_rest_alone(oracle):
    import torch
    m, ins, _, _ = _case(oracle, 'salamander33')
    clean = R.phys('salamander33', m, N, ins)
    phys = R.phys('salamander33', m, N, ins)
    clean.step(1); phys.step(1)      # a completed step: records and ncon to keep
    torch.cuda.synchronize()
    bad, keep = 2, [0, 1, 3]
    phys.data.ctrl[bad, 3] = float('nan')
    fields = FIELDS + ('xpos', 'xquat', 'xipos', 'time')
    before = {k: getattr(phys.data, k)[bad].clone() for k in fields}
    assert int(before['ncon']) > 0
    clean.step(2); phys.step(2)
    torch.cuda.synchronize()
    st = phys.data.status.cpu().numpy()
    assert st[bad] & FMJ_WARN_BADQACC and not st[keep].any() and not clean.data.status.any(), st
    for k, v in before.items():
        assert torch.equal(getattr(phys.data, k)[bad].view(torch.int32), v.view(torch.int32)), k
    for k in fields:
        assert torch.equal(getattr(phys.data, k)[keep], getattr(clean.data, k)[keep]), k
    assert not torch.equal(clean.data.contact[bad], before['contact'])      # (the clean env's list moved on)


def test_a_failure_in_a_later_pass_undoes_the_step(oracle):
    """Env 1 gets a finite torque on one link, so large that the first pass's |qacc| stays below 1e10 while the pass at X[1] exceeds it
    - both asserted from the oracle's stage states first.  The env ends with FMJ_WARN_BADQACC and every field it had, contact records
    and ncon included; the others step as in a clean run."""
    import torch
    m, ins, _, _ = _case(oracle, 'salamander33')
    bad, body = 1, m.nbody//2
    unit = np.zeros((m.nbody, 6)); unit[body, 3:] = [0.3, 0.5, 1.0]
    a1 = np.abs(R.stages(oracle, m, ins, bad, xfrc_applied=unit)[0][2]['qacc'] - R.stages_first(oracle, m, ins, bad)['qacc']).max()
    scale = np.float32(3e9/a1)
    big = (unit*scale).astype(np.float32).astype(np.float64)
    assert np.isfinite(big).all()
    st = R.stages(oracle, m, ins, bad, xfrc_applied=big)
    a0, a_x1 = np.abs(st[0][2]['qacc']).max(), np.abs(st[1][2]['qacc'])
    print('torque scale %.3g: first pass max |qacc| %.3g, at X[1] %s, stage |qvel| %.3g' % (scale, a0, np.nanmax(a_x1), np.abs(st[1][1]).max()))
    assert a0 < 1e10 and np.abs(st[1][1]).max() < 1e10 and np.abs(st[1][0]).max() < 1e10
    assert not np.all(a_x1 <= 1e10)
    clean = R.phys('salamander33', m, N, ins)
    phys = R.phys('salamander33', m, N, ins)
    clean.step(1); phys.step(1)      # a completed step: records and ncon to keep
    torch.cuda.synchronize()
    assert int(phys.data.status.abs().sum()) == 0
    phys.data.xfrc_applied[bad] = torch.as_tensor(big, dtype=torch.float32)
    fields = FIELDS + ('xpos', 'xquat', 'xipos', 'time')
    before = {k: getattr(phys.data, k)[bad].clone() for k in fields}
    assert int(before['ncon']) > 0
    clean.step(2); phys.step(2)
    torch.cuda.synchronize()
    s = phys.data.status.cpu().numpy()
    keep = [e for e in range(N) if e != bad]
    assert s[bad] & FMJ_WARN_BADQACC and not s[keep].any() and not clean.data.status.any(), s
    for k, v in before.items():
        assert torch.equal(getattr(phys.data, k)[bad].view(torch.int32), v.view(torch.int32)), k
    for k in fields:
        assert torch.equal(getattr(phys.data, k)[keep], getattr(clean.data, k)[keep]), k


_TRAJ = {}


def _trajectory(oracle):
    """salamander33 from just above touch height under a ctrl tape, 60 RK4 steps: the oracle's plain run, its run with the state
    rounded to fp32 after every step (the floor), both step by step with the warm start carried - computed once."""
    if not _TRAJ:
        m = R.make('salamander33')
        q0, v0, tape32 = R.trajectory_inputs(m)
        (pq, pv, pn, share), (fq, fv, fn, _) = R.trajectory_runs(oracle, m, q0, v0, tape32)
        assert np.array_equal(pn, fn) and pn.max() >= 2 and share.min() > 0, (share, pn.max())
        ref = dict(qpos=pq, qvel=pv)
        _TRAJ.update(m=m, q0=q0, v0=v0, tape32=tape32, ref=ref, floor=dict(qpos=relerr(fq, pq), qvel=relerr(fv, pv)), ncon=pn[-1])
    return _TRAJ


def test_trajectory_against_the_state_rounding_floor(oracle):
    import torch
    t = _trajectory(oracle)
    m, T = t['m'], R.TRAJ_T
    p = R.phys('salamander33', m, N, dict(qpos=t['q0'], qvel=t['v0'], ctrl=None))
    p.step(T, torch.as_tensor(t['tape32'], device=p.device).contiguous())
    torch.cuda.synchronize()
    assert int(p.data.status.abs().sum()) == 0
    assert float(p.data.time.min()) == pytest.approx(T*m.timestep, rel=1e-5)
    assert np.array_equal(p.data.ncon.cpu().numpy(), t['ncon'])
    for k in ('qpos', 'qvel'):
        err = relerr(getattr(p.data, k).cpu().numpy(), t['ref'][k])
        print(k, 'after', T, 'RK4 steps with contacts: fp64 kernel %.3g  floor_state %.3g  ratio %.3g' % (err, t['floor'][k], err/t['floor'][k]))
        assert err <= t['floor'][k], (k, err, t['floor'][k])


def test_step_3_against_three_steps_of_1(oracle):
    """fmj_step(3) keeps the state in double between its steps, three fmj_step(1) round it to fp32 twice: the two differ by no more
    than the oracle's state-rounded run differs from its plain run over the trajectory above."""
    import torch
    t = _trajectory(oracle)
    m = t['m']
    ins = dict(qpos=t['q0'], qvel=t['v0'], ctrl=None)
    a, b = R.phys('salamander33', m, N, ins), R.phys('salamander33', m, N, ins)
    warm = 40      # into the contacts first, so that the state has digits to round
    wt = torch.as_tensor(t['tape32'][:warm], device='cuda:0').contiguous()
    a.step(warm, wt); b.step(warm, wt)
    tape = torch.as_tensor(t['tape32'][warm:warm + 3], device='cuda:0').contiguous()
    a.step(3, tape)
    for s in range(3):
        b.step(1, tape[s:s + 1].contiguous())
    torch.cuda.synchronize()
    assert int(a.data.status.abs().sum()) == 0 and int(b.data.status.abs().sum()) == 0
    assert float((a.data.time - b.data.time).abs().max()) <= float(np.spacing(np.float32(a.data.time.max().item())))      # (time is rounded per launch too)
    assert torch.equal(a.data.ncon, b.data.ncon)
    for k in ('qpos', 'qvel'):
        d = relerr(getattr(b.data, k).cpu().numpy(), getattr(a.data, k).cpu().numpy().astype(np.float64))
        print(k, 'fmj_step(3) against 3 x fmj_step(1): %.3g, floor_state of the trajectory %.3g' % (d, t['floor'][k]))
        assert d <= t['floor'][k], (k, d, t['floor'][k])


def test_through_the_simulation(oracle):
    """10 RK4 iterations of the walking centipede through Simulation(fp64_contacts=True, fp64_contacts_rk4=True): run() takes the
    per-iteration path (fmj_before_step + fmj_step(1)); links, joints and contacts rows against oracle.run_fused at the thresholds of
    test_gpu_f64_contacts.test_through_the_simulation; a fused launch is refused."""
    import ctypes
    import torch
    from farms_mujoco_amd import _lib as L
    from farms_mujoco_amd._lib import FmjError
    from farms_mujoco_amd.data import AnimatData
    from farms_mujoco_amd.options import SimulationOptions
    from farms_mujoco_amd.simulation.simulation import Simulation
    from support_sims import oracle_initial_state
    m, ins, _, _ = _case(oracle, 'centipede_20_25')
    T = 10
    pairs = [(b, '') for b in m.body_names[1:] if b.endswith('_1')] + [('world', '')]
    data = AnimatData(m.timestep, T, N, m.body_names[1:], m.hinge_joint_names(), contacts=pairs)
    sim = Simulation(m, m.body_names[1], SimulationOptions(timestep=m.timestep, n_iterations=T, integrator='RK4'), n_envs=N, data=data, buffer_size=T,
                     precision='fp64', fp64_contacts=True, fp64_contacts_rk4=True)
    assert sim.physics.precision == 'fp64' and sim.physics.rk4 and sim.physics.fp64_contacts_rk4 and not sim.task.fusable() and sim.task.host_step_only
    assert sim.physics.kernel_info()['fp64_step_kernel'] == 'fmj_step_f64_terrain_rk4_kernel'
    sim.reset()
    d = sim.physics.data
    d.qpos[:] = torch.as_tensor(ins['qpos'], dtype=torch.float32)
    sim.physics.forward(disable_actuation=True)
    st = oracle_initial_state(oracle, sim, m)
    g2d = sim.task.maps['sensors']['geompair2data']
    kw = dict(swim=None, buffer_size=T, controller=0, ctrl=np.zeros((N, m.nu)), geompair2data=g2d, n_contact_rows=len(pairs), n_threads=4)
    ref = oracle.run_fused(m, st, T, **kw)
    with oracle.fp32_storage():
        flo = oracle.run_fused(m, st, T, **kw)
    with pytest.raises(FmjError, match='fp64'):
        sim.step_fused(1)
    p = sim.physics
    rc = p._lib.fmj_step_fused_f64(p._ctx, ctypes.byref(p._cdata()), ctypes.byref(L.CFusedArgs()), None, L.stream_ptr(p.device))
    msg = p._lib.fmj_last_error().decode()      # F64_NO_FUSED of csrc/fmj_hip.hip, verbatim
    assert rc != 0 and msg == ('fmj_step_fused_f64: an fp64 context with contacts (FMJ_CREATE_F64_CONTACTS) steps through fmj_step: '
                               'fused contact rows are not built'), (rc, msg)
    sim.run()
    torch.cuda.synchronize()
    assert int(d.status.abs().sum()) == 0 and sim.task.sim_iteration == T
    sens = sim.task.data.sensors
    got = dict(qpos=d.qpos.cpu().numpy(), links=sens.links.array.cpu().numpy(), joints=sens.joints.array.cpu().numpy(),
               contacts=sens.contacts.array.cpu().numpy())
    assert np.abs(ref['contacts'][..., :3]).max() > 0
    err = {k: relerr(got[k], ref[k]) for k in got}; fl = {k: relerr(flo[k], ref[k]) for k in got}
    print('walking RK4 centipede, fp64 simulation: whole-tensor error', err, 'fp32-storage run', fl)
    assert err['qpos'] <= fl['qpos']/10, (err, fl)
    assert err['links'] <= fl['links'] and err['joints'] <= fl['joints'] and err['contacts'] <= fl['contacts'], (err, fl)
