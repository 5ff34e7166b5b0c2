"""Convex mesh geoms on the fp64 contact solve (BatchedPhysics(precision='fp64', fp64_contacts=True, fp64_mesh=True): fmj_create_ex2 with
FMJ_CREATE_F64_CONTACTS | FMJ_CREATE_F64_MESH, fmj_step_f64_mesh_kernel / fmj_step_f64_mesh_elliptic_kernel of csrc/fmj_f64_step.inc)
against the fp64 oracle (Newton, 100 iterations, the model's tolerance).

One step and fmj_forward are held to the bound of test_gpu_f64_contacts.py, contact records included:
    |got - ref| <= ulp32(ref_i) + ulp32(max |ref| over the component's column group in that env)
Every case first asserts, from the oracle alone, what support_f64_mesh.conditions states (engaged and idle contacts, limit rows, mesh
geoms whose selection evicts, geoms with one to three and with no penetrating vertex, no grazing decision and no tie of two depths).
The trajectory is held to the oracle's own run with the state rounded to fp32 every step, as the terrain walker's is."""
import numpy as np
import pytest

from parity_metrics import relerr
import support_f64_contacts as C
import support_f64_terrain as T
import support_f64_mesh as M
from support_f64_mesh import N
from support_f64_contacts import STATE, _groups, _contact_excess, _excess

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize('integrator', ['euler', 'implicitfast'])
@pytest.mark.parametrize('name', M.MODELS)
def test_one_step_and_forward_to_the_ulp(oracle, name, integrator):
    import support_f64_step as S
    m = M.make(name, integrator)
    ins = M.inputs_of(name, m)
    ok, ref, what = M.conditions(oracle, name, m, ins)
    print(name, integrator, what)
    assert ok, (name, what)
    if name == 'centipede_mesh':      # over the envs together: a mesh geom on the second wave of the prefix sum, a contact past slot 63
        assert max(ref['geoms'][e, :ref['ncon'][e], 1].max() for e in range(N)) >= 64 and ref['ncon'].max() > 64
    for forward in (False, True):
        p = M.phys(m, N, ins)
        info = p.kernel_info()
        assert info['threads_per_env'] == 128 and info['fp64_step_kernel'] == M.kernel_of(m) and p.solver_effective == 'Newton'
        p.forward() if forward else p.step(1)
        ex = _excess(m, p, ref, forward, ins)
        print(name, integrator, 'forward' if forward else 'step', 'error / bound per field:', {k: round(v, 3) for k, v in ex.items()})
        bad = {k: v for k, v in ex.items() if v > 1.0}
        assert not bad, (name, integrator, forward, bad)


@pytest.mark.parametrize('name', ['centipede_20_25', 'centipede_hfield_cyl'])
def test_the_flag_changes_nothing_for_a_model_without_meshes(name):
    """The same kernel runs with and without fp64_mesh=True: an identity, not a tolerance."""
    import torch
    flat = name in C.MODELS
    m = (C if flat else T).make(name)
    ins = (C if flat else T).inputs(m, N, (C if flat else T).SEEDS[name])
    got, kernel = {}, {}
    for mesh in (False, True):
        p = C.phys(m, N, ins, fp64_terrain=not flat, fp64_mesh=mesh)
        kernel[mesh] = p.kernel_info()['fp64_step_kernel']
        p.step(1)
        torch.cuda.synchronize()
        got[mesh] = {k: getattr(p.data, k).clone() for k in STATE + ('contact', 'ncon')}
    assert kernel[False] == kernel[True] == ('fmj_step_f64_contacts_kernel' if flat else 'fmj_step_f64_terrain_kernel')
    assert int(got[True]['ncon'].min()) > 0
    for k in got[False]:
        assert torch.equal(got[False][k], got[True][k]), k


def test_no_contact_no_bit_changed():
    """centipede_mesh 1 m above the ground, 50 steps of fmj_step: every step is the unconstrained kernel's, against a plain fp64 context
    of the same model with its geoms removed."""
    import torch
    a, b = M.make('centipede_mesh'), M.make('centipede_mesh')
    C.set_geoms(b, [], 0)
    b.mesh_vert = np.zeros((0, 3)); b.nmeshvert = 0; b.geom_vertadr = np.zeros(0, np.int32); b.geom_vertnum = np.zeros(0, np.int32)
    ins = M.inputs(a, N, 5, depth=-1.0)
    assert min(M.lowest(a, q) for q in ins['qpos']) > 0.99
    pa = M.phys(a, N, ins)
    pb = C.phys(b, N, ins, fp64_contacts=False)
    assert pa.kernel_info()['fp64_step_kernel'] == 'fmj_step_f64_mesh_kernel'
    pa.step(50); pb.step(50)
    torch.cuda.synchronize()
    assert int(pa.data.status.abs().sum()) == 0 and int(pa.data.ncon.abs().sum()) == 0
    for k in ('qpos', 'qvel', 'qacc', 'sensordata', 'xpos', 'xquat', 'xipos', 'time'):
        assert torch.equal(getattr(pa.data, k), getattr(pb.data, k)), k


def test_truncation_inside_one_geoms_contacts(oracle):
    """max_contacts cuts the oracle's full list between two contacts of one mesh geom: FMJ_WARN_CONTACTFULL alone, the kept records
    are the oracle's first max_contacts, the state is within the bound of the oracle's truncated step, and the next step moves it."""
    import torch
    name = 'centipede_mesh'
    m = M.make(name)
    ins = M.inputs_of(name, m)
    full = C.reference(oracle, m, ins)
    e0 = int(np.argmax(full['ncon']))
    g = full['geoms'][e0, :full['ncon'][e0], 1]
    cut = next(k for k in range(2, len(g)) if g[k - 1] == g[k] and m.geom_type[g[k]] == M.GEOM_MESH)
    m.max_contacts = cut
    assert g[cut - 1] == g[cut]
    b = oracle.step_tf(m, ins['qpos'], ins['qvel'], ctrl=ins['ctrl'], want_AR=False)
    a = oracle.step(m, ins['qpos'], ins['qvel'], ctrl=ins['ctrl'])
    assert b['ncon'][e0] == cut and np.array_equal(b['contact'][e0, :cut, :3], full['contact'][e0, :cut, :3])
    import support_f64_step as S
    p = M.phys(m, N, ins)
    p.step(1)
    torch.cuda.synchronize()
    st = p.data.status.cpu().numpy()
    assert st[e0] == C.FMJ_WARN_CONTACTFULL and np.array_equal(st, a['status']), (st, a['status'])      # reported, and nothing else
    assert np.array_equal(p.data.ncon.cpu().numpy(), b['ncon'])
    c16 = p.data.contact.cpu().numpy()
    for e in range(N):      # the kept records are the oracle's
        k = int(b['ncon'][e])
        assert S.ulp_excess(c16[e:e + 1, :k, :3], b['contact'][e:e + 1, :k, :3]) <= 1.0
        assert S.ulp_excess(c16[e:e + 1, :k, 3:12], b['contact'][e:e + 1, :k, 3:12]) <= 1.0
        gg = np.ascontiguousarray(c16[e, :k, 15]).view(np.int32)
        assert np.array_equal(gg & 0xffff, b['contact'][e, :k, 16].astype(int))
    groups = _groups(m)      # the state: every STATE field, the warm start from the oracle's truncated solve
    a['qacc_warmstart'] = b['warmstart']
    ex = {k: S.ulp_excess(getattr(p.data, k).cpu().numpy(), a[k], groups[k]) for k in STATE}
    ex['force'] = max(S.ulp_excess(c16[e:e + 1, :int(b['ncon'][e]), 12:15], b['contact'][e:e + 1, :int(b['ncon'][e]), 12:15]) for e in range(N))
    print('truncated at', cut, 'error / bound per field:', {k: round(v, 3) for k, v in ex.items()})
    assert max(ex.values()) <= 1.0, ex
    q1 = p.data.qpos.clone()
    p.step(1)
    torch.cuda.synchronize()
    assert not torch.equal(q1, p.data.qpos)


@pytest.mark.parametrize('which', M.NARROW)
def test_hand_placed_narrow_phase_cases(oracle, which):
    """One free body over a small heightfield: a mesh across the grid's border (the vertices outside see no ground), a mesh whose
    origin is outside the grid (nothing), the single-vertex mesh, and the 42-vertex hull pressed in past its centre (the four kept are
    the oracle's four deepest).  Records, ncon and the state are held as in the one-step test."""
    m, ins = M.narrow_case(which)
    ref = C.reference(oracle, m, ins)
    M.narrow_branch(which, m, ins, ref)
    for forward in (False, True):
        p = M.phys(m, N, ins)
        assert p.kernel_info()['fp64_step_kernel'] == 'fmj_step_f64_mesh_kernel'
        p.forward() if forward else p.step(1)
        ex = _excess(m, p, ref, forward, ins)
        print(which, 'forward' if forward else 'step', 'error / bound per field:', {k: round(v, 3) for k, v in ex.items()})
        assert max(ex.values()) <= 1.0, (which, forward, ex)


def test_trajectory_against_the_state_rounding_floor(oracle):
    """centipede_mesh on the heightfield dropped from 2 mm above its touch height under walk_tape (the default stance), 150 steps in
    one launch: qpos / qvel no further from the plain oracle than the oracle's own run with the state rounded to fp32 every step (the
    form of test_gpu_f64_terrain.py's trajectory test).  More than half of the steps have a contact force in every env."""
    import torch
    m = M.make('centipede_mesh_hfield')
    Tn = 150
    tape32 = C.walk_tape(m, N, Tn)
    tape = tape32.astype(np.float64)
    r32 = lambda a: np.asarray(a, np.float64).astype(np.float32).astype(np.float64)
    q0 = np.tile(m.key_qpos, (N, 1))
    q0[:, 2] += 2e-3 - min(M.lowest(m, q) for q in q0)      # (the touch height of the mesh feet, not of the spheres they replace)
    q0 = r32(q0)
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
    p = M.phys(m, N, dict(qpos=q0, qvel=v0, ctrl=None))
    assert p.kernel_info()['fp64_step_kernel'] == 'fmj_step_f64_mesh_kernel'
    p.step(Tn, torch.as_tensor(tape32, device=p.device).contiguous())
    torch.cuda.synchronize()
    assert int(p.data.status.abs().sum()) == 0
    for k, fl in (('qpos', fq), ('qvel', fv)):
        err, floor = relerr(getattr(p.data, k).cpu().numpy(), ref[k]), relerr(fl, ref[k])
        print(k, 'after', Tn, 'steps: fp64 mesh kernel %.3g  floor_state %.3g  ratio %.3g' % (err, floor, err/floor))
        assert err <= floor, (k, err, floor)


def test_through_the_simulation(oracle):
    """10 iterations of centipede_mesh on the heightfield through Simulation(fp64_contacts=True, fp64_terrain=True, fp64_mesh=True)
    on the per-iteration path with contact rows logged: links, joints and contacts rows against oracle.run_fused, below the oracle's
    fp32-storage run (the measures of test_gpu_f64_terrain.py's Simulation run).  step_fused refuses."""
    import torch
    from farms_mujoco_amd._lib import FmjError
    from farms_mujoco_amd.data import AnimatData
    from farms_mujoco_amd.options import SimulationOptions
    from farms_mujoco_amd.simulation.simulation import Simulation
    from support_sims import oracle_initial_state
    m = M.make('centipede_mesh_hfield')
    Tn = 10
    pairs = [(b, '') for b in m.body_names[1:] if b.endswith('_1')] + [('world', '')]
    data = AnimatData(m.timestep, Tn, N, m.body_names[1:], m.hinge_joint_names(), contacts=pairs)
    sim = Simulation(m, m.body_names[1], SimulationOptions(timestep=m.timestep, n_iterations=Tn), n_envs=N, data=data, buffer_size=Tn,
                     precision='fp64', fp64_contacts=True, fp64_terrain=True, fp64_mesh=True)
    assert sim.physics.precision == 'fp64' and sim.physics.fp64_mesh and not sim.task.fusable()
    assert sim.physics.kernel_info()['fp64_step_kernel'] == 'fmj_step_f64_mesh_kernel'
    sim.reset()
    ins = M.inputs(m, N, M.SEEDS['centipede_hfield_mixed'], depth=4e-3)
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
    print('centipede_mesh on the heightfield, fp64 simulation: whole-tensor error', err, 'fp32-storage run', fl)
    assert err['qpos'] <= fl['qpos']/10, (err, fl)
    assert err['links'] <= fl['links'] and err['joints'] <= fl['joints'] and err['contacts'] <= fl['contacts'], (err, fl)


def test_a_fused_launch_is_refused_and_the_lds_is_the_terrain_contexts():
    """fmj_step_fused_f64 at the C-ABI refuses with the contacts text; the reported LDS bytes equal the terrain context's for the same
    model sizes and max_contacts."""
    import ctypes
    from farms_mujoco_amd import _lib as L
    m = M.make('centipede_mesh_hfield')
    ins = M.inputs(m, N, M.SEEDS['centipede_hfield_mixed'], depth=4e-3)
    p = M.phys(m, N, ins)
    args = L.CFusedArgs()
    rc = p._lib.fmj_step_fused_f64(p._ctx, ctypes.byref(p._cdata()), ctypes.byref(args), None, L.stream_ptr(p.device))
    msg = p._lib.fmj_last_error().decode()
    assert rc != 0 and msg.startswith('fmj_step_fused_f64: an fp64 context with contacts (FMJ_CREATE_F64_CONTACTS) steps through fmj_step'), (rc, msg)
    maxefc, max_contacts, iterations = L.ints(p._lib.fmj_constraint_info, p._ctx)
    assert (maxefc, max_contacts, iterations) == (2*m.njnt + 4*m.max_contacts, m.max_contacts, 100)
    info = p.kernel_info()
    assert info['fp64_step_kernel'] == 'fmj_step_f64_mesh_kernel' and info['lds_bytes_per_env'] <= 160*1024
    t = T.make('centipede_hfield'); t.max_contacts = m.max_contacts
    pt = T.phys(t, N, T.inputs(t, N, T.SEEDS['centipede_hfield_cyl']))
    assert pt.kernel_info()['fp64_step_kernel'] == 'fmj_step_f64_terrain_kernel'
    assert (t.nbody, t.nv, t.nq) == (m.nbody, m.nv, m.nq) and info['lds_bytes_per_env'] == pt.kernel_info()['lds_bytes_per_env']
