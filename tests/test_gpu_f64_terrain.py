"""Heightfield ground and cylinder geoms on the fp64 contact solve (BatchedPhysics(precision='fp64', fp64_contacts=True,
fp64_terrain=True): fmj_create_ex2 with FMJ_CREATE_F64_CONTACTS | FMJ_CREATE_F64_TERRAIN, fmj_step_f64_terrain_kernel of
csrc/fmj_f64_step.inc) against the fp64 oracle (Newton, 100 iterations, the model's tolerance).

One step and fmj_forward are held to the bound of test_gpu_f64_contacts.py, contact records included:
    |got - ref| <= ulp32(ref_i) + ulp32(max |ref| over the component's column group in that env)
Every case first asserts, from the oracle alone, what support_f64_terrain.conditions states (engaged contacts, idle contacts, limit rows,
cylinder contacts, normals that differ, no grazing decision of the narrow phase or of the grid lookup) and that the reference is
converged.  The trajectory is held to the oracle's own run with the state rounded to fp32 every step, as the plane walker's is."""
import numpy as np
import pytest

from parity_metrics import relerr
import support_f64_contacts as C
import support_f64_terrain as T
from support_f64_terrain import N
from support_f64_contacts import STATE, _groups, _contact_excess, _excess

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize('integrator', ['euler', 'implicitfast'])
@pytest.mark.parametrize('name', T.MODELS)
def test_one_step_and_forward_to_the_ulp(oracle, name, integrator):
    import support_f64_step as S
    m = T.make(name, integrator)
    ins = T.inputs(m, N, T.SEEDS[name])
    ok, ref, what = T.conditions_of(oracle, name, m, ins)
    print(name, integrator, what)
    assert ok, (name, what)
    tight = C.reference(oracle, m, ins, tighter=True)      # the reference is converged
    groups = _groups(m)
    moved = {k: S.ulp_excess(tight[k], ref[k], groups[k]) for k in STATE}
    moved['contact'] = _contact_excess(tight['contact'], ref['ncon'], ref)
    print(name, integrator, 'a 100 x tighter tolerance moves the reference by (in bounds):', {k: round(v, 4) for k, v in moved.items()})
    assert max(moved.values()) <= 0.1 and np.array_equal(tight['ncon'], ref['ncon']), moved
    for forward in (False, True):
        p = T.phys(m, N, ins)
        info = p.kernel_info()
        assert info['threads_per_env'] == 128 and info['fp64_step_kernel'] == 'fmj_step_f64_terrain_kernel' and p.solver_effective == 'Newton'
        p.forward() if forward else p.step(1)
        ex = _excess(m, p, ref, forward, ins)
        print(name, integrator, 'forward' if forward else 'step', 'error / bound per field:', {k: round(v, 3) for k, v in ex.items()})
        bad = {k: v for k, v in ex.items() if v > 1.0}
        assert not bad, (name, integrator, forward, bad)


def test_the_flag_changes_nothing_on_flat_ground(oracle):
    """centipede(20, 25, contacts=True) on its plane, the one-step inputs of test_gpu_f64_contacts.py: the contacts context and the
    terrain context are both within the one-step bound of the oracle; whether they agree bit for bit is printed."""
    import torch
    m = C.make('centipede_20_25')
    ins = C.inputs(m, N, C.SEEDS['centipede_20_25'])
    ok, ref, what = C.conditions(oracle, m, ins, False)
    assert ok, what
    got = {}
    for terrain in (False, True):
        p = C.phys(m, N, ins, fp64_terrain=terrain)
        assert p.kernel_info()['fp64_step_kernel'] == ('fmj_step_f64_terrain_kernel' if terrain else 'fmj_step_f64_contacts_kernel')
        p.step(1)
        ex = _excess(m, p, ref, False, ins)
        print('flat ground, terrain flag', terrain, 'error / bound per field:', {k: round(v, 3) for k, v in ex.items()})
        assert max(ex.values()) <= 1.0, (terrain, ex)
        got[terrain] = {k: getattr(p.data, k).clone() for k in STATE + ('contact', 'ncon')}
    same = {k: bool(torch.equal(got[False][k], got[True][k])) for k in got[False]}
    print('flat ground: the terrain kernel agrees bit for bit with the contacts kernel:', same)


def test_no_contact_no_bit_changed():
    """The heightfield centipede 1 m above the terrain, 50 steps of fmj_step: every step is the unconstrained kernel's, against a plain
    fp64 context of the same model with its geoms removed."""
    import torch
    a, b = T.make('centipede_hfield'), T.make('centipede_hfield')
    C.set_geoms(b, [], 0)
    b.hfield_nrow = b.hfield_ncol = 0; b.hfield_data = None; b.hfield_size = np.zeros(4)
    ins = T.inputs(a, N, 5, depth=-1.0)
    assert min(T.lowest(a, q) for q in ins['qpos']) > 0.99
    pa = T.phys(a, N, ins)
    pb = C.phys(b, N, ins, fp64_contacts=False)
    pa.step(50); pb.step(50)
    torch.cuda.synchronize()
    assert int(pa.data.status.abs().sum()) == 0 and int(pa.data.ncon.abs().sum()) == 0
    for k in ('qpos', 'qvel', 'qacc', 'sensordata', 'xpos', 'xquat', 'xipos', 'time'):
        assert torch.equal(getattr(pa.data, k), getattr(pb.data, k)), k


def test_trajectory_against_the_state_rounding_floor(oracle):
    """The heightfield centipede dropped from 2 mm above its touch height under walk_tape, 150 steps in one launch: qpos / qvel no
    further from the plain oracle than the oracle's own run with the state rounded to fp32 every step (the form and margin of the
    plane walker's test).  'Most steps' with a contact force: more than half in every env - free fall over the 2 mm takes 20 of the
    150 steps, and only the foot over the highest ground touches that early."""
    import torch
    m = T.make('centipede_hfield')
    Tn = 150
    tape32 = C.walk_tape(m, N, Tn)
    tape = tape32.astype(np.float64)
    r32 = lambda a: np.asarray(a, np.float64).astype(np.float32).astype(np.float64)
    q0 = np.tile(m.key_qpos, (N, 1)); q0[:, 2] += 2e-4 + 2e-3; q0 = r32(q0)      # (key_qpos: the touch height less 0.2 mm)
    v0 = np.zeros((N, m.nv))
    q, v, ws = q0, v0, None
    with_force = np.zeros(N)
    for t in range(Tn):
        o = oracle.step_tf(m, q, v, ctrl=tape[t], warmstart=ws, want_AR=False)
        with_force += np.array([(o['contact'][e, :o['ncon'][e], 12] > 0).any() for e in range(N)])
        q, v, ws = o['qpos'], o['qvel'], o['warmstart']
    print('share of steps with a contact force', with_force/Tn)
    assert (with_force/Tn).min() > 0.5, with_force/Tn
    ref = oracle.step(m, q0, v0, ctrl=tape, n_steps=Tn, ctrl_step_stride=N*m.nu, n_threads=4)
    fq, fv = q0, v0
    for t in range(Tn):      # floor_state: the oracle's own run with the state rounded to fp32 every step
        o = oracle.step(m, fq, fv, ctrl=tape[t], n_steps=1, n_threads=4)
        fq = r32(o['qpos']); fv = r32(o['qvel'])
    p = T.phys(m, N, dict(qpos=q0, qvel=v0, ctrl=None))
    p.step(Tn, torch.as_tensor(tape32, device=p.device).contiguous())
    torch.cuda.synchronize()
    assert int(p.data.status.abs().sum()) == 0
    for k, fl in (('qpos', fq), ('qvel', fv)):
        err, floor = relerr(getattr(p.data, k).cpu().numpy(), ref[k]), relerr(fl, ref[k])
        print(k, 'after', Tn, 'steps: fp64 terrain kernel %.3g  floor_state %.3g  ratio %.3g' % (err, floor, err/floor))
        assert err <= floor, (k, err, floor)


def test_a_full_contact_list_is_truncated_and_reported(oracle):
    import support_f64_step as S
    import torch
    name = 'centipede_hfield_cyl'
    m = T.make(name)
    ins = T.inputs(m, N, T.SEEDS[name])
    full = C.reference(oracle, m, ins)
    m.max_contacts = int(full['ncon'].min()) - 2
    assert m.max_contacts >= 4
    a = oracle.step(m, ins['qpos'], ins['qvel'], ctrl=ins['ctrl'])
    b = oracle.step_tf(m, ins['qpos'], ins['qvel'], ctrl=ins['ctrl'], want_AR=False)
    assert np.all(b['ncon'] == m.max_contacts) and np.all(a['status'] & C.FMJ_WARN_CONTACTFULL)
    p = T.phys(m, N, ins)
    p.step(1)
    torch.cuda.synchronize()
    st = p.data.status.cpu().numpy()
    assert np.all(st == C.FMJ_WARN_CONTACTFULL), st      # reported, and nothing else
    assert np.array_equal(p.data.ncon.cpu().numpy(), b['ncon'])
    c16 = p.data.contact.cpu().numpy()
    for e in range(N):      # the kept records are the oracle's first max_contacts
        assert np.array_equal(b['contact'][e, :, :3], full['contact'][e, :m.max_contacts, :3])
        assert S.ulp_excess(c16[e:e + 1, :, :3], b['contact'][e:e + 1, :, :3]) <= 1.0
        assert S.ulp_excess(c16[e:e + 1, :, 3:12], b['contact'][e:e + 1, :, 3:12]) <= 1.0
        gg = np.ascontiguousarray(c16[e, :, 15]).view(np.int32)
        assert np.array_equal(gg & 0xffff, b['contact'][e, :, 16].astype(int))
    groups = _groups(m)
    ex = {k: S.ulp_excess(getattr(p.data, k).cpu().numpy(), a[k], groups[k]) for k in ('qpos', 'qvel', 'qacc')}
    print('truncated list on terrain, error / bound:', ex)
    assert max(ex.values()) <= 1.0, ex
    p.step(1)      # not frozen: the next step moves the state
    torch.cuda.synchronize()
    assert not np.array_equal(p.data.qpos.cpu().numpy(), a['qpos'].astype(np.float32)) and float(p.data.time[0]) > 1.5*m.timestep


def test_through_the_simulation(oracle):
    """10 iterations of the heightfield centipede through Simulation(fp64_contacts=True, fp64_terrain=True) on the per-iteration path
    with contact rows logged: links, joints and contacts rows against oracle.run_fused, below the oracle's fp32-storage run (the
    measures of test_gpu_f64_contacts.py's Simulation run)."""
    import torch
    from farms_mujoco_amd._lib import FmjError
    from farms_mujoco_amd.data import AnimatData
    from farms_mujoco_amd.options import SimulationOptions
    from farms_mujoco_amd.simulation.simulation import Simulation
    from support_sims import oracle_initial_state
    m = T.make('centipede_hfield')
    Tn = 10
    pairs = [(b, '') for b in m.body_names[1:] if b.endswith('_1')] + [('world', '')]
    data = AnimatData(m.timestep, Tn, N, m.body_names[1:], m.hinge_joint_names(), contacts=pairs)
    sim = Simulation(m, m.body_names[1], SimulationOptions(timestep=m.timestep, n_iterations=Tn), n_envs=N, data=data, buffer_size=Tn,
                     precision='fp64', fp64_contacts=True, fp64_terrain=True)
    assert sim.physics.precision == 'fp64' and sim.physics.fp64_terrain and not sim.task.fusable()
    assert sim.physics.kernel_info()['fp64_step_kernel'] == 'fmj_step_f64_terrain_kernel'
    sim.reset()
    ins = T.inputs(m, N, T.SEEDS['centipede_hfield_cyl'])
    d = sim.physics.data
    d.qpos[:] = torch.as_tensor(ins['qpos'], dtype=torch.float32)
    sim.physics.forward(disable_actuation=True)
    st = oracle_initial_state(oracle, sim, m)
    g2d = sim.task.maps['sensors']['geompair2data']
    kw = dict(swim=None, buffer_size=Tn, controller=0, ctrl=np.zeros((N, m.nu)), geompair2data=g2d, n_contact_rows=len(pairs), n_threads=4)
    ref = oracle.run_fused(m, st, Tn, **kw)
    with oracle.fp32_storage():
        flo = oracle.run_fused(m, st, Tn, **kw)
    with pytest.raises(FmjError, match='fp64'):
        sim.step_fused(1)
    sim.run()
    torch.cuda.synchronize()
    assert int(d.status.abs().sum()) == 0 and sim.task.sim_iteration == Tn
    sens = sim.task.data.sensors
    got = dict(qpos=d.qpos.cpu().numpy(), links=sens.links.array.cpu().numpy(), joints=sens.joints.array.cpu().numpy(),
               contacts=sens.contacts.array.cpu().numpy())
    assert np.abs(ref['contacts'][..., :3]).max() > 0
    err = {k: relerr(got[k], ref[k]) for k in got}; fl = {k: relerr(flo[k], ref[k]) for k in got}
    print('heightfield centipede, fp64 simulation: whole-tensor error', err, 'fp32-storage run', fl)
    assert err['qpos'] <= fl['qpos']/10, (err, fl)
    assert err['links'] <= fl['links'] and err['joints'] <= fl['joints'] and err['contacts'] <= fl['contacts'], (err, fl)


def test_a_fused_launch_is_refused_and_the_context_reports_its_kernel():
    import ctypes
    from farms_mujoco_amd import _lib as L
    name = 'centipede_hfield_cyl'
    m = T.make(name)
    p = T.phys(m, N, T.inputs(m, N, T.SEEDS[name]))
    args = L.CFusedArgs()
    rc = p._lib.fmj_step_fused_f64(p._ctx, ctypes.byref(p._cdata()), ctypes.byref(args), None, L.stream_ptr(p.device))
    msg = p._lib.fmj_last_error().decode()
    assert rc != 0 and 'fp64' in msg and 'contact' in msg, (rc, msg)
    maxefc, max_contacts, iterations = L.ints(p._lib.fmj_constraint_info, p._ctx)
    assert (maxefc, max_contacts, iterations) == (2*m.njnt + 4*m.max_contacts, m.max_contacts, 100)
    info = p.kernel_info()
    assert info['fp64_step_kernel'] == 'fmj_step_f64_terrain_kernel' and info['lds_bytes_per_env'] <= 160*1024
    flat = C.make('centipede_20_25')      # ldsd_terrain_bytes: 3 more doubles per contact than the contacts kernels' map
    pf = C.phys(flat, N, C.inputs(flat, N, C.SEEDS['centipede_20_25']))
    assert info['lds_bytes_per_env'] - pf.kernel_info()['lds_bytes_per_env'] == 8*3*m.max_contacts and flat.max_contacts == m.max_contacts
