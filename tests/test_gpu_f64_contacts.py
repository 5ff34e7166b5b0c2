"""Ground contacts on the fp64 step kernel (BatchedPhysics(precision='fp64', fp64_contacts=True): fmj_create_ex2 with
FMJ_CREATE_F64_CONTACTS, fmj_step_f64_contacts_kernel of csrc/fmj_f64_step.inc) against the fp64 oracle, whose model names Newton with
100 iterations and the model's tolerance - the device runs its primal Newton solve whatever the model names.

One step and fmj_forward are held to the rounding of the fp32 store, the bound of test_gpu_f64_step.py, contact records included:
    |got - ref| <= ulp32(ref_i) + ulp32(max |ref| over the component's column group in that env)
Every case first asserts, from the oracle alone, that the contacts are engaged as it says, that no narrow-phase decision grazes and
that the reference is converged (a 100 x tighter tolerance moves nothing by a tenth of the bound).  Trajectories are held to the
oracle's own run with the state rounded to fp32 every step (floor_state of test_gpu_f64_step.py): a launch keeps its state in double."""
import warnings

import numpy as np
import pytest

from parity_metrics import relerr
from support_f64_contacts import (N, MODELS, SEEDS, FMJ_WARN_CONTACTFULL, make, inputs, conditions, reference, phys as _phys, walk_tape,
                                  lowest_point, STATE, _groups, _contact_excess, _excess)

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize('integrator', ['euler', 'implicitfast'])
@pytest.mark.parametrize('name', MODELS)
def test_one_step_and_forward_to_the_ulp(oracle, name, integrator):
    import support_f64_step as S
    m = make(name, integrator)
    limited = bool(np.any(m.jnt_limited))
    ins = inputs(m, N, SEEDS[name])
    ok, ref, what = conditions(oracle, m, ins, limited)
    print(name, integrator, what)
    assert ok, (name, what)
    tight = reference(oracle, m, ins, tighter=True)      # the reference is converged
    groups = _groups(m)
    moved = {k: S.ulp_excess(tight[k], ref[k], groups[k]) for k in STATE}
    moved['contact'] = _contact_excess(tight['contact'], ref['ncon'], ref)
    print(name, integrator, 'a 100 x tighter tolerance moves the reference by (in bounds):', {k: round(v, 4) for k, v in moved.items()})
    assert max(moved.values()) <= 0.1 and np.array_equal(tight['ncon'], ref['ncon']), moved
    ex_step = None
    for forward in (False, True):
        p = _phys(m, N, ins)
        assert p.kernel_info()['threads_per_env'] == 128 and p.solver_effective == 'Newton'
        p.forward() if forward else p.step(1)
        ex = _excess(m, p, ref, forward, ins)
        print(name, integrator, 'forward' if forward else 'step', 'error / bound per field:', {k: round(v, 3) for k, v in ex.items()})
        bad = {k: v for k, v in ex.items() if v > 1.0}
        assert not bad, (name, integrator, forward, bad)
        ex_step = ex_step or ex
    if name == 'salamander33':      # also runs on the fp32 constraint kernel, which is further from the oracle
        p32 = _phys(m, N, ins, precision='fp32')
        p32.step(1)
        import torch
        torch.cuda.synchronize()
        ex32 = {k: S.ulp_excess(getattr(p32.data, k).cpu().numpy(), ref[k], groups[k]) for k in ('qvel', 'qacc')}
        print(name, integrator, 'fp32 context, error / bound:', ex32)
        assert ex32['qvel'] > ex_step['qvel'] and ex32['qacc'] > ex_step['qacc'], (ex32, ex_step)


def test_no_contact_no_bit_changed():
    """The walking centipede 1 m above the plane, 50 steps of fmj_step: every step is the unconstrained kernel's, against a plain fp64
    context of the same model with its geoms removed."""
    import torch
    from support_f64_contacts import set_geoms
    a, b = make('centipede_20_25'), make('centipede_20_25')
    set_geoms(b, [], 0)
    ins = inputs(a, N, 5, depth=-1.0)
    assert min(lowest_point(a, q) for q in ins['qpos']) > 0.99
    pa = _phys(a, N, ins)
    pb = _phys(b, N, ins, fp64_contacts=False)
    pa.step(50); pb.step(50)
    torch.cuda.synchronize()
    assert int(pa.data.status.abs().sum()) == 0 and int(pa.data.ncon.abs().sum()) == 0
    for k in ('qpos', 'qvel', 'qacc', 'sensordata', 'xpos', 'xquat', 'xipos', 'time'):
        assert torch.equal(getattr(pa.data, k), getattr(pb.data, k)), k


def test_the_solver_the_model_names_does_not_matter():
    import torch
    from farms_mujoco_amd.model import SOLVERS
    outs = []
    for solver in ('pgs', 'newton'):
        m = make('centipede_20_25')
        m.solver = SOLVERS[solver]
        ins = inputs(m, N, SEEDS['centipede_20_25'])
        with warnings.catch_warnings(record=True) as w:
            warnings.simplefilter('always')
            p = _phys(m, N, ins)
        said = [str(x.message) for x in w if 'primal Newton solve' in str(x.message)]
        assert len(said) == (solver == 'pgs'), (solver, [str(x.message) for x in w])      # only when the model asked for another solver
        assert (p.solver_requested, p.solver_effective, p.solver_budget) == ({'pgs': 'PGS', 'newton': 'Newton'}[solver], 'Newton', 100)
        p.step(3)
        torch.cuda.synchronize()
        assert int(p.data.status.abs().sum()) == 0
        outs.append({k: getattr(p.data, k).clone() for k in STATE + ('contact', 'ncon')})
    for k in outs[0]:
        assert torch.equal(outs[0][k], outs[1][k]), k
    assert int(outs[0]['ncon'].min()) > 0


def test_trajectory_against_the_state_rounding_floor(oracle):
    """The walking centipede dropped from 2 mm above the touch height under a ctrl tape, 150 steps in one launch: qpos / qvel no
    further from the plain oracle than the oracle's own run with the state rounded to fp32 every step."""
    import torch
    from farms_mujoco_amd.model import centipede_touch_height
    m = make('centipede_20_25')
    T = 150
    tape32 = walk_tape(m, N, T)
    tape = tape32.astype(np.float64)
    r32 = lambda a: np.asarray(a, np.float64).astype(np.float32).astype(np.float64)
    q0 = np.tile(m.key_qpos, (N, 1)); q0[:, 2] = centipede_touch_height() + 2e-3; q0 = r32(q0)
    v0 = np.zeros((N, m.nv))
    q, v, ws = q0, v0, None
    with_force = np.zeros(N)
    for t in range(T):      # the condition, from a step-by-step oracle run (the warm start carried as mj_step carries it)
        o = oracle.step_tf(m, q, v, ctrl=tape[t], warmstart=ws, want_AR=False)
        with_force += np.array([(o['contact'][e, :o['ncon'][e], 12] > 0).any() for e in range(N)])
        q, v, ws = o['qpos'], o['qvel'], o['warmstart']
    print('share of steps with a contact force', with_force/T)
    assert (with_force/T).min() >= 0.9, with_force/T
    ref = oracle.step(m, q0, v0, ctrl=tape, n_steps=T, ctrl_step_stride=N*m.nu, n_threads=4)
    fq, fv = q0, v0
    for t in range(T):      # floor_state: the oracle's own run with the state rounded to fp32 every step
        o = oracle.step(m, fq, fv, ctrl=tape[t], n_steps=1, n_threads=4)
        fq = r32(o['qpos']); fv = r32(o['qvel'])
    p = _phys(m, N, dict(qpos=q0, qvel=v0, ctrl=None))
    p.step(T, torch.as_tensor(tape32, device=p.device).contiguous())
    torch.cuda.synchronize()
    assert int(p.data.status.abs().sum()) == 0
    for k, fl in (('qpos', fq), ('qvel', fv)):
        err, floor = relerr(getattr(p.data, k).cpu().numpy(), ref[k]), relerr(fl, ref[k])
        print(k, 'after', T, 'steps: fp64 kernel %.3g  floor_state %.3g  ratio %.3g' % (err, floor, err/floor))
        assert err <= floor, (k, err, floor)


def test_a_full_contact_list_is_truncated_and_reported(oracle):
    import support_f64_step as S
    import torch
    m = make('centipede_20_25')
    ins = inputs(m, N, SEEDS['centipede_20_25'])
    full = reference(oracle, m, ins)
    m.max_contacts = int(full['ncon'].min()) - 2
    assert m.max_contacts >= 4
    a = oracle.step(m, ins['qpos'], ins['qvel'], ctrl=ins['ctrl'])
    b = oracle.step_tf(m, ins['qpos'], ins['qvel'], ctrl=ins['ctrl'], want_AR=False)
    assert np.all(b['ncon'] == m.max_contacts) and np.all(a['status'] & FMJ_WARN_CONTACTFULL)
    p = _phys(m, N, ins)
    p.step(1)
    torch.cuda.synchronize()
    st = p.data.status.cpu().numpy()
    assert np.all(st == FMJ_WARN_CONTACTFULL), st      # reported, and nothing else
    assert np.array_equal(p.data.ncon.cpu().numpy(), b['ncon'])
    c16 = p.data.contact.cpu().numpy()
    for e in range(N):      # the kept records are the oracle's first max_contacts
        assert np.array_equal(b['contact'][e, :, :3], full['contact'][e, :m.max_contacts, :3])
        assert S.ulp_excess(c16[e:e + 1, :, :3], b['contact'][e:e + 1, :, :3]) <= 1.0
        gg = np.ascontiguousarray(c16[e, :, 15]).view(np.int32)
        assert np.array_equal(gg & 0xffff, b['contact'][e, :, 16].astype(int))
    groups = _groups(m)
    ex = {k: S.ulp_excess(getattr(p.data, k).cpu().numpy(), a[k], groups[k]) for k in ('qpos', 'qvel', 'qacc')}
    print('truncated list, error / bound:', ex)
    assert max(ex.values()) <= 1.0, ex
    p.step(1)      # not frozen: the next step moves the state
    torch.cuda.synchronize()
    assert not np.array_equal(p.data.qpos.cpu().numpy(), a['qpos'].astype(np.float32)) and float(p.data.time[0]) > 1.5*m.timestep


def test_through_the_simulation(oracle):
    """10 iterations of the walking centipede through Simulation(fp64_contacts=True): run() takes the per-iteration path; links, joints
    and contacts rows against oracle.run_fused with the measures of test_gpu_f64_step.py's Simulation run (the oracle's fused loop
    with fp32 storage is the yardstick: rows and drag are fp32 operators on this path)."""
    import torch
    from farms_mujoco_amd._lib import FmjError
    from farms_mujoco_amd.data import AnimatData
    from farms_mujoco_amd.options import SimulationOptions
    from farms_mujoco_amd.simulation.simulation import Simulation
    from support_sims import oracle_initial_state
    m = make('centipede_20_25')
    T = 10
    pairs = [(b, '') for b in m.body_names[1:] if b.endswith('_1')] + [('world', '')]
    data = AnimatData(m.timestep, T, N, m.body_names[1:], m.hinge_joint_names(), contacts=pairs)
    sim = Simulation(m, m.body_names[1], SimulationOptions(timestep=m.timestep, n_iterations=T), n_envs=N, data=data, buffer_size=T,
                     precision='fp64', fp64_contacts=True)
    assert sim.physics.precision == 'fp64' and sim.physics.fp64_contacts and not sim.task.fusable()
    sim.reset()
    ins = inputs(m, N, SEEDS['centipede_20_25'])
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
    sim.run()
    torch.cuda.synchronize()
    assert int(d.status.abs().sum()) == 0 and sim.task.sim_iteration == T
    sens = sim.task.data.sensors
    got = dict(qpos=d.qpos.cpu().numpy(), links=sens.links.array.cpu().numpy(), joints=sens.joints.array.cpu().numpy(),
               contacts=sens.contacts.array.cpu().numpy())
    assert np.abs(ref['contacts'][..., :3]).max() > 0
    err = {k: relerr(got[k], ref[k]) for k in got}; fl = {k: relerr(flo[k], ref[k]) for k in got}
    print('walking centipede, fp64 simulation: whole-tensor error', err, 'fp32-storage run', fl)
    assert err['qpos'] <= fl['qpos']/10, (err, fl)
    assert err['links'] <= fl['links'] and err['joints'] <= fl['joints'] and err['contacts'] <= fl['contacts'], (err, fl)


def test_a_fused_launch_is_refused_and_the_context_reports_its_rows():
    import ctypes
    from farms_mujoco_amd import _lib as L
    m = make('centipede_20_25')
    p = _phys(m, N, inputs(m, N, SEEDS['centipede_20_25']))
    args = L.CFusedArgs()
    rc = p._lib.fmj_step_fused_f64(p._ctx, ctypes.byref(p._cdata()), ctypes.byref(args), None, L.stream_ptr(p.device))
    msg = p._lib.fmj_last_error().decode()
    assert rc != 0 and 'fp64' in msg and 'contact' in msg, (rc, msg)
    maxefc, max_contacts, iterations = L.ints(p._lib.fmj_constraint_info, p._ctx)
    assert (maxefc, max_contacts, iterations) == (2*m.njnt + 4*m.max_contacts, m.max_contacts, 100)
    assert p.kernel_info()['lds_bytes_per_env'] <= 160*1024
