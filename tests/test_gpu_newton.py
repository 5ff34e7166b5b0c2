"""The Newton solver of the HIP constraint path (solver = 'Newton', reference mjcf.py:1348-1359: the reference's own fallback)
against the oracle's Newton (oracle/fmj_oracle.c solve_primal), itself cross-checked against a converged PGS on CPU
(tests/test_oracle_solvers.py)."""
import copy
import functools

import numpy as np
import pytest

from parity_metrics import group_relerr, qvel_groups
from support_models import (walker, trot_tape as _trot_tape, scissors as _scissors, salamander_self_collisions as _salamander_self_collisions,
                            random_tree, FMJ_WARN_CONTACTFULL)
from support_sims import set_state as _set

pytestmark = pytest.mark.gpu

_walker = functools.partial(walker, solver='newton')


@pytest.mark.parametrize('solver', ['newton', 'cg'])
def test_newton_single_step_forces_and_kkt(oracle, solver):
    """Feet on the floor, bellies pressed in (more than 64 rows), a joint past its limit: contact list, forces and velocity of one
    step against the oracle's Newton; the forces satisfy the KKT conditions of the fp64 problem."""
    import torch
    from farms_mujoco_amd.physics import BatchedPhysics
    m = _walker(solver=solver)
    n = 12
    rng = np.random.default_rng(0)
    qpos = np.tile(m.qpos0, (n, 1)); qpos[:, 7:] += rng.uniform(-0.1, 0.1, (n, m.nq - 7))
    qpos[:4, 2] = 0.012                       # belly contacts
    qpos[:, 7 + 3] = 1.25                     # a spine joint past its +1.2 rad limit
    qvel = rng.normal(size=(n, m.nv))*0.05
    phys = BatchedPhysics(m, n)
    q32, v32, w32 = _set(phys, qpos, qvel, rng.normal(size=(n, m.nv))*5.0)
    rows, _ = phys.step_debug(want_pgs=False)
    torch.cuda.synchronize()
    d = phys.data
    assert int(d.status.abs().sum()) == 0
    o = oracle.step_tf(m, q32, v32, ctrl=np.zeros((n, m.nu)), warmstart=w32)
    with oracle.fp32_storage():
        fl = oracle.step_tf(m, q32, v32, ctrl=np.zeros((n, m.nu)), warmstart=w32, want_AR=False)
    assert np.array_equal(d.ncon.cpu().numpy(), o['ncon']) and o['nefc'].max() > 64 and o['nefc'].min() <= 40
    rows = rows.cpu().numpy().astype(np.float64)
    worst = 0.0
    for e in range(n):
        ne = int(o['nefc'][e])
        f_h = rows[e, :ne, 4]; f_o = o['efc'][e, :ne, 0]; b = o['efc'][e, :ne, 1]; AR = o['AR'][e, :ne, :ne]
        fs = max(np.abs(f_o).max(), 1e-2); bs = max(np.abs(b).max(), 1.0)
        worst = max(worst, np.abs(f_h - f_o).max()/fs)
        r = AR @ f_h + b
        assert f_h.min() >= 0.0 and r.min() > -2e-3*bs and np.abs(f_h*r).max() < 2e-3*fs*bs, (e, r.min()/bs, np.abs(f_h*r).max()/(fs*bs))
    err = group_relerr(d.qvel.cpu().numpy(), o['qvel'], qvel_groups(m)); floor = group_relerr(fl['qvel'], o['qvel'], qvel_groups(m))
    print(solver, 'single step: forces', worst, 'qvel per component', err, 'fp32-storage floor', floor)
    assert worst < 2e-3
    assert err < 6*floor + 1e-6
    assert np.abs(d.qacc_warmstart.cpu().numpy() - o['warmstart']).max() < 2e-3*np.abs(o['warmstart']).max()


@pytest.mark.parametrize('solver', ['newton', 'cg'])
def test_newton_walk_follows_the_oracle(oracle, solver):
    """300 steps of the trot with the Newton solver, fused loop with contact rows: no warning bits, the floor carries the animal,
    and since Newton converges at every step (unlike PGS cut at 50 sweeps) the walk stays on the oracle's."""
    import torch
    from farms_mujoco_amd.physics import BatchedPhysics
    m = _walker(solver=solver)
    n, T = 8, 300
    tape = _trot_tape(m, n, T)
    phys = BatchedPhysics(m, n)
    q32, v32, _ = _set(phys, np.tile(m.qpos0, (n, 1)), np.zeros((n, m.nv)))
    tape_t = torch.as_tensor(tape, dtype=torch.float32, device='cuda').contiguous()
    phys.step(T, ctrl_tape=tape_t)
    torch.cuda.synchronize()
    ref = oracle.step(m, q32, v32, ctrl=tape_t.cpu().numpy().astype(np.float64), n_steps=T, ctrl_step_stride=n*m.nu, n_threads=8)
    with oracle.fp32_storage():
        fl = oracle.step(m, q32, v32, ctrl=tape_t.cpu().numpy().astype(np.float64), n_steps=T, ctrl_step_stride=n*m.nu, n_threads=8)
    d = phys.data
    assert int(d.status.abs().sum()) == 0 and int(ref['status'].sum()) == 0
    e = np.abs(d.qpos.cpu().numpy() - ref['qpos']).max(1); f = np.abs(fl['qpos'] - ref['qpos']).max(1)
    print(solver, 'walk, qpos abs err per env after', T, 'steps:', e, 'fp32-storage floor run:', f)
    assert float(d.qpos[:, 2].min()) > 0.0 and float(d.qpos[:, 2].max()) < 0.1
    # 10 - 20x the fp32-storage floor of the same 300 steps (the order in which the Hessian rows are summed moves it between builds),
    # an order of magnitude inside the bounds of the PGS walk (5e-4 median, 5e-3 worst)
    assert np.median(e) < 1e-4 and e.max() < 1e-3 and np.median(e) < 40*np.median(f)


def test_newton_with_mesh_feet_on_a_heightfield(oracle):
    """The reference's usual configuration - SDF mesh collisions (mjcf.py:270-413) under its fallback solver Newton (:1348-1359) - here
    on a heightfield: 60 steps of standing / settling against the oracle's Newton."""
    import torch
    from farms_mujoco_amd.model import salamander33, SOLVERS
    from farms_mujoco_amd.physics import BatchedPhysics
    m = salamander33(contacts=True, limits=True, spawn_z=0.05, mesh_feet=True, terrain='hfield')
    m.solver = SOLVERS['newton']; m.solver_iterations = 100
    n, T = 6, 60
    rng = np.random.default_rng(3)
    qpos = np.tile(m.qpos0, (n, 1)); qpos[:, 7:] += rng.uniform(-0.1, 0.1, (n, m.nq - 7)); qpos[:, :2] += rng.uniform(-0.3, 0.3, (n, 2))
    phys = BatchedPhysics(m, n)
    q32, v32, _ = _set(phys, qpos, np.zeros((n, m.nv)))
    phys.step(T)
    torch.cuda.synchronize()
    ref = oracle.step(m, q32, v32, ctrl=np.zeros((n, m.nu)), n_steps=T)
    d = phys.data
    assert int(d.status.abs().sum()) == 0 and int(ref['status'].sum()) == 0
    fds = [oracle.forward_debug(m, ref['qpos'][e], ref['qvel'][e], ctrl=np.zeros(m.nu)) for e in range(n)]
    assert max(fd['ncon'] for fd in fds) >= 4
    e = np.abs(d.qpos.cpu().numpy() - ref['qpos']).max(1)
    print('Newton, mesh feet on a heightfield, qpos abs err per env after', T, 'steps:', e)
    assert e.max() < 1e-3


@pytest.mark.parametrize('solver', ['newton', 'cg'])
def test_newton_and_cg_with_self_collision_pairs(oracle, solver):
    """Explicit pairs (reference mjcf.py:1012-1033, declared with friction 0) under the primal solvers.  Their rows carry R ~ 1e-10 R0: a
    1 N force is a residual of 1e-11, which no fp32 primal iteration resolves, so an env whose step has an ACTIVE pair contact is
    solved on the dual problem (PGS to the solver's tolerance): same convex problem, same minimiser; the oracle runs the solver
    that was asked for, in fp64 - except that the reference solution is always the Newton minimiser: the oracle's own CG, capped at
    100 iterations, does not get through rows with D = 4e10 (it ends 0.6 of the largest force away from the minimiser).  Scissors (one pair row set, nothing else) and the
    salamander lying on the plane with feet meeting under the trunk / head meeting tail: forces and velocity of one step, then 40 steps."""
    import torch
    from farms_mujoco_amd.model import SOLVERS
    from farms_mujoco_amd.physics import BatchedPhysics
    for capsule in (False, True):
        m, q = _scissors(0.1, capsule=capsule)
        m.solver = SOLVERS[solver]; m.solver_iterations = 100
        mo = copy.copy(m); mo.solver = SOLVERS['newton']
        n = 6
        rng = np.random.default_rng(3)
        qpos = np.tile(q, (n, 1)) + rng.uniform(-0.03, 0.03, (n, 2)); qpos[n - 1] = [0.6, -0.6]
        phys = BatchedPhysics(m, n)
        q32, v32, _ = _set(phys, qpos, rng.normal(size=(n, 2))*0.2)
        phys.step(1)
        torch.cuda.synchronize()
        d = phys.data
        o = oracle.step_tf(mo, q32, v32, ctrl=np.zeros((n, m.nu)), want_AR=False)
        assert int(d.status.abs().sum()) == 0 and np.array_equal(d.ncon.cpu().numpy(), o['ncon']) and o['ncon'][:-1].min() == 1
        con = oracle.contacts_from_hip(d.contact.cpu().numpy())
        assert np.abs(con[:n-1, 0, 12] - o['contact'][:n-1, 0, 12]).max() < 1e-3*np.abs(o['contact'][:n-1, 0, 12]).max()
        assert np.abs(d.qvel.cpu().numpy() - o['qvel']).max() < 1e-4*np.abs(o['qvel']).max()
        phys.step(199)
        torch.cuda.synchronize()
        ref = oracle.step(mo, q32, v32, ctrl=np.zeros((n, m.nu)), n_steps=200)
        assert int(d.status.abs().sum()) == 0 and np.abs(d.qpos.cpu().numpy() - ref['qpos']).max() < 2e-4
    m = _salamander_self_collisions()
    m.solver = SOLVERS[solver]; m.solver_iterations = 100
    mo = copy.copy(m); mo.solver = SOLVERS['newton']
    plane = int(np.nonzero(m.geom_type == 0)[0][0])
    spine = [m.jnt_qposadr[m.joint_names.index(f'joint_body_{i}')] for i in range(1, 12)]
    legj = [m.jnt_qposadr[m.joint_names.index(f'joint_leg_{t}_{s_}_{k}')] for t in ('front', 'hind') for s_ in ('L', 'R') for k in range(4)]
    poses = []
    for legs in ([-1.19, 0.07, -0.84, -0.74, 0.24, -0.09, 1.01, -0.27, 0.42, -0.19, 0.52, -0.12, -0.63, 0.83, 0.69, -0.46],
                 [-0.25, -0.11, 0.59, -0.16, 1.02, 0.67, 0.77, -0.62, -0.01, -0.32, -0.9, 0.36, 0.78, 0.27, 1.14, -0.7]):
        q = m.qpos0.copy(); q[2] = 0.05; q[legj] = legs; poses.append(q)
    for curl in (0.645, 0.65):
        q = m.qpos0.copy(); q[2] = 0.03; q[spine] = curl; poses.append(q)
    q = m.qpos0.copy(); q[2] = 0.045; poses.append(q)                     # a fifth env without self-contact: takes the solver that was asked for
    qpos = np.array(poses); n = len(poses)
    rng = np.random.default_rng(21)
    phys = BatchedPhysics(m, n)
    q32, v32, w32 = _set(phys, qpos, 0.02*rng.normal(size=(n, m.nv)))
    phys.step_debug(want_pgs=False)
    torch.cuda.synchronize()
    d = phys.data
    o = oracle.step_tf(mo, q32, v32, ctrl=np.zeros((n, m.nu)), warmstart=w32, want_AR=False)
    assert int(d.status.abs().sum()) == 0 and np.array_equal(d.ncon.cpu().numpy(), o['ncon'])
    npair = [(o['contact'][e, :o['ncon'][e], 15] != plane).sum() for e in range(n)]
    assert min(npair[:4]) >= 1 and npair[4] == 0
    # contact-frame forces, not rows: the four pyramid edges of a friction-0 pair (mu = 1e-5) are the same row to 1e-5, their sum is
    # determined, its split among them is not
    con = oracle.contacts_from_hip(d.contact.cpu().numpy())
    worst = 0.0
    for e in range(n):
        nc = int(o['ncon'][e])
        if nc:
            fs = max(np.abs(o['contact'][e, :nc, 12]).max(), 1e-2)
            worst = max(worst, np.abs(con[e, :nc, 12:15] - o['contact'][e, :nc, 12:15]).max()/fs)
    err = group_relerr(d.qvel.cpu().numpy(), o['qvel'], qvel_groups(m))
    with oracle.fp32_storage(2):      # the floor of the velocity bound: the same step with fp32 state, poses and mass matrices
        fl = oracle.step_tf(mo, q32, v32, ctrl=np.zeros((n, m.nu)), warmstart=w32, want_AR=False)
    floor = group_relerr(fl['qvel'], o['qvel'], qvel_groups(m))
    print(solver, 'with self-collision pairs: contact-frame forces', worst, 'qvel per component', err, 'fp32-storage floor', floor)
    assert worst < 3e-3 and err < 6*floor + 1e-5 and err < 3e-2
    phys.step(39)
    torch.cuda.synchronize()
    ref = oracle.step(mo, q32, v32, ctrl=np.zeros((n, m.nu)), n_steps=40, n_threads=8)
    assert int(d.status.abs().sum()) == 0
    e40 = np.abs(d.qpos.cpu().numpy() - ref['qpos']).max(1)
    print('  qpos abs err after 40 steps', e40)
    assert e40.max() < 2e-3 and np.median(e40) < 3e-4


def test_elliptic_cone_with_newton_and_pairs_runs_on_the_dual_problem():
    """Round 4 refused the elliptic cone with PGS and on models with explicit pairs.  Round 5: PGS has MuJoCo's block update
    (tests/test_gpu_pgs_options.py); Newton / CG with pairs is solved on the dual problem, and says so."""
    from farms_mujoco_amd.model import salamander33, SOLVERS, CONES
    from farms_mujoco_amd.physics import BatchedPhysics
    m = salamander33(contacts=True, limits=True, spawn_z=0.045, self_collisions=True)
    m.solver = SOLVERS['newton']; m.cone = CONES['elliptic']
    with pytest.warns(UserWarning, match='dual problem'):
        phys = BatchedPhysics(m, 2)
    assert phys.solver_requested == 'Newton' and phys.solver_effective == 'PGS'
    m = salamander33(contacts=True, limits=True, spawn_z=0.045)
    m.cone = CONES['elliptic']
    assert BatchedPhysics(m, 2).solver_effective == 'PGS'


@pytest.mark.parametrize('solver,impratio', [('newton', 1.0), ('cg', 1.0), ('newton', 4.0)])
def test_elliptic_cone_single_step(oracle, solver, impratio):
    """cone = elliptic (reference mjcf.py:1342-1347): three rows per contact, MuJoCo's cone zones in the primal cost.  Sliding feet
    (forces on the cone), pressed-in bellies (more than 64 rows), a joint past its limit: the rows' forces, the contact-frame forces
    and the velocity of one step against the oracle; friction stays inside the cone."""
    import torch
    from farms_mujoco_amd.physics import BatchedPhysics
    m = _walker(solver=solver, cone='elliptic', impratio=impratio)
    n = 12
    rng = np.random.default_rng(1)
    qpos = np.tile(m.qpos0, (n, 1)); qpos[:, 7:] += rng.uniform(-0.1, 0.1, (n, m.nq - 7))
    qpos[:4, 2] = 0.012
    qpos[:, 7 + 3] = 1.25
    qvel = rng.normal(size=(n, m.nv))*0.05; qvel[:, :2] += 0.3
    phys = BatchedPhysics(m, n)
    q32, v32, w32 = _set(phys, qpos, qvel, rng.normal(size=(n, m.nv))*5.0)
    rows, _ = phys.step_debug(want_pgs=False)
    torch.cuda.synchronize()
    d = phys.data
    assert int(d.status.abs().sum()) == 0
    o = oracle.step_tf(m, q32, v32, ctrl=np.zeros((n, m.nu)), warmstart=w32)
    with oracle.fp32_storage():
        fl = oracle.step_tf(m, q32, v32, ctrl=np.zeros((n, m.nu)), warmstart=w32, want_AR=False)
    assert np.array_equal(d.ncon.cpu().numpy(), o['ncon']) and o['nefc'].max() > 50
    rows = rows.cpu().numpy().astype(np.float64)
    con = oracle.contacts_from_hip(d.contact.cpu().numpy())
    worst = worst_c = 0.0
    for e in range(n):
        ne = int(o['nefc'][e]); nc = int(o['ncon'][e])
        assert ne == int(o['nefc'][e]) and (ne - 3*nc) >= 1
        f_h = rows[e, :ne, 4]; f_o = o['efc'][e, :ne, 0]
        fs = max(np.abs(f_o).max(), 1e-2)
        worst = max(worst, np.abs(f_h - f_o).max()/fs)
        worst_c = max(worst_c, np.abs(con[e, :nc, 12:15] - o['contact'][e, :nc, 12:15]).max()/fs)
        mu = 0.8 if nc == 0 else None
        fn, ft = con[e, :nc, 12], np.hypot(con[e, :nc, 13], con[e, :nc, 14])
        g = con[e, :nc, 16].astype(int)
        mus = np.maximum(np.asarray(m.geom_friction)[g, 0], np.asarray(m.geom_friction)[con[e, :nc, 15].astype(int), 0])
        assert (fn >= 0).all() and (ft <= mus*fn*(1 + 1e-4) + 1e-6).all()
    err = group_relerr(d.qvel.cpu().numpy(), o['qvel'], qvel_groups(m)); floor = group_relerr(fl['qvel'], o['qvel'], qvel_groups(m))
    print(solver, 'elliptic single step: row forces', worst, 'contact-frame forces', worst_c, 'qvel per component', err, 'fp32-storage floor', floor)
    assert worst < 3e-3 and worst_c < 3e-3
    assert err < 6*floor + 1e-6


@pytest.mark.parametrize('solver', ['newton', 'cg'])
def test_elliptic_cone_walk_follows_the_oracle(oracle, solver):
    """300 steps of the trot with elliptic cones, fused loop with contact rows, against the oracle's walk with the same solver."""
    import torch
    from farms_mujoco_amd.physics import BatchedPhysics
    m = _walker(solver=solver, cone='elliptic')
    n, T = 8, 300
    tape = _trot_tape(m, n, T)
    phys = BatchedPhysics(m, n)
    q32, v32, _ = _set(phys, np.tile(m.qpos0, (n, 1)), np.zeros((n, m.nv)))
    tape_t = torch.as_tensor(tape, dtype=torch.float32, device='cuda').contiguous()
    phys.step(T, ctrl_tape=tape_t)
    torch.cuda.synchronize()
    ref = oracle.step(m, q32, v32, ctrl=tape_t.cpu().numpy().astype(np.float64), n_steps=T, ctrl_step_stride=n*m.nu, n_threads=8)
    d = phys.data
    assert int(d.status.abs().sum()) == 0 and int(ref['status'].sum()) == 0
    e = np.abs(d.qpos.cpu().numpy() - ref['qpos']).max(1)
    print(solver, 'elliptic walk, qpos abs err per env after', T, 'steps:', e)
    assert float(d.qpos[:, 2].min()) > 0.0 and float(d.qpos[:, 2].max()) < 0.1
    # typically 1e-5; the exact cone makes stick / slip transitions sharp, and an env that takes one a step early leaves the oracle's
    # walk by ~3e-3 (seen in one env of eight) - the per-step error is bounded in test_elliptic_cone_teacher_forced_per_step
    # CG against the cone's kinks often ends at its 100-iteration cap on both sides (two unconverged iterates, as with PGS x 50): 1e-4 .. 3e-4
    med = 1e-4 if solver == 'newton' else 5e-4
    assert np.median(e) < med and np.sum(e > 10*med) <= 1 and e.max() < 2e-2


def test_elliptic_cone_teacher_forced_per_step(oracle):
    """The oracle's elliptic Newton walk is followed for 200 steps; at every step the HIP path steps once from the teacher's state
    (rounded to fp32, as is the oracle's probe step): same contacts, row forces within 1e-3 of the largest force, velocity within 2e-3."""
    import torch
    from farms_mujoco_amd.physics import BatchedPhysics
    m = _walker(cone='elliptic')
    n, T = 8, 200
    tape = _trot_tape(m, n, T)
    phys = BatchedPhysics(m, n); d = phys.data
    f32 = lambda a: torch.as_tensor(np.asarray(a), dtype=torch.float32, device=d.qpos.device)
    r64 = lambda t: t.cpu().numpy().astype(np.float64)
    q = np.tile(m.qpos0, (n, 1)); v = np.zeros((n, m.nv)); w = np.zeros((n, m.nv))
    ef, ev, flips, cone_rows = [], [], 0, 0
    for t in range(T):
        d.qpos[:] = f32(q); d.qvel[:] = f32(v); d.qacc_warmstart[:] = f32(w); d.ctrl[:] = f32(tape[t])
        q32, v32, w32, c32 = r64(d.qpos), r64(d.qvel), r64(d.qacc_warmstart), r64(d.ctrl)
        rows, _ = phys.step_debug(want_pgs=False)
        o = oracle.step_tf(m, q32, v32, ctrl=c32, warmstart=w32, want_AR=False)
        rows = r64(rows); qv = r64(d.qvel); nc_h = d.ncon.cpu().numpy()
        for e in range(n):
            ne = int(o['nefc'][e])
            if nc_h[e] != o['ncon'][e]:
                flips += 1; continue
            if ne:
                fs = max(np.abs(o['efc'][e, :ne, 0]).max(), 1e-2)
                ef.append(np.abs(rows[e, :ne, 4] - o['efc'][e, :ne, 0]).max()/fs)
                cone_rows += int((o['efc'][e, :ne, 4] == 2).sum())
            ev.append(np.abs(qv[e] - o['qvel'][e]).max()/max(np.abs(o['qvel'][e]).max(), 1e-3))
        tch = oracle.step_tf(m, q, v, ctrl=tape[t], warmstart=w, want_AR=False)
        q, v, w = tch['qpos'], tch['qvel'], tch['warmstart']
    ef, ev = np.array(ef), np.array(ev)
    print(f'elliptic teacher-forced: {len(ev)} env-steps, {cone_rows} cone rows, contact-count flips {flips}; force err median {np.median(ef):.2e} max {ef.max():.2e}; '
          f'qvel err median {np.median(ev):.2e} max {ev.max():.2e}')
    assert flips <= 0.002*n*T and cone_rows > 3*n*T
    assert np.median(ef) < 5e-5 and ef.max() < 1e-3
    assert np.median(ev) < 1e-4 and ev.max() < 2e-3


@pytest.mark.parametrize('seed', range(100, 108))
@pytest.mark.parametrize('solver,cone', [('newton', 'pyramidal'), ('cg', 'pyramidal'), ('newton', 'elliptic')])
def test_primal_solvers_on_random_contact_trees(oracle, seed, solver, cone):
    """Random trees (limited hinges, sphere / capsule / box / cylinder geoms over a plane that cuts through the tree) under Newton, CG
    and the elliptic cone: contact lists, contact-frame forces and velocity of one step against the oracle's Newton minimiser (the
    oracle's CG, capped at 100 iterations, is itself only within ~1e-4 of it on some of these trees)."""
    import torch
    from farms_mujoco_amd.model import SOLVERS, CONES
    from farms_mujoco_amd.physics import BatchedPhysics
    m = random_tree(seed, contacts=True)
    if m is None or m.nv == 0:
        pytest.skip('degenerate draw')
    m.solver = SOLVERS[solver]; m.cone = CONES[cone]; m.solver_iterations = 100
    mo = copy.copy(m); mo.solver = SOLVERS['newton']
    rng = np.random.default_rng(2000 + seed)
    n = 6
    qpos = np.tile(m.qpos0, (n, 1)) + rng.uniform(-0.4, 0.4, (n, m.nq))
    for j in range(m.njnt):
        if m.jnt_type[j] == 0:
            a = m.jnt_qposadr[j]; q = rng.normal(size=(n, 4)); qpos[:, a+3:a+7] = q/np.linalg.norm(q, axis=1, keepdims=True)
            qpos[:, a+2] = rng.uniform(-0.05, 0.1, n)
    qvel = rng.normal(size=(n, m.nv))*0.2
    ctrl = rng.uniform(-0.4, 0.4, (n, max(m.nu, 1)))[:, :m.nu]
    phys = BatchedPhysics(m, n)
    d = phys.data
    q32, v32, w32 = _set(phys, qpos, qvel)
    if m.nu:
        d.ctrl[:] = torch.as_tensor(ctrl, dtype=torch.float32)
    c32 = d.ctrl.cpu().numpy().astype(np.float64) if m.nu else None
    phys.step(1)
    torch.cuda.synchronize()
    assert int((d.status & ~FMJ_WARN_CONTACTFULL).abs().sum()) == 0
    o = oracle.step_tf(mo, q32, v32, ctrl=c32, warmstart=w32, want_AR=False)
    with oracle.fp32_storage(3):
        fl = oracle.step_tf(mo, q32, v32, ctrl=c32, warmstart=w32, want_AR=False)
    assert np.array_equal(d.ncon.cpu().numpy(), o['ncon'])
    if o['nefc'].max() == 0:
        pytest.skip('no active constraint in this draw')
    con = oracle.contacts_from_hip(d.contact.cpu().numpy())
    for e in range(n):
        nc = int(o['ncon'][e])
        if nc:
            fs = max(np.abs(o['contact'][e, :nc, 12:15]).max(), 1e-2)
            # contact-frame forces of random contact trees: 6 x the floor (the same step of the fp64 oracle with fp32 storage of every array)
            # + 3e-3 of the largest force (what the fp32 primal iteration resolves: tests above), instead of round 4's fitted 2e-2 fs + 2e-3
            ef = np.abs(con[e, :nc, 12:15] - o['contact'][e, :nc, 12:15]).max()
            ff = np.abs(fl['contact'][e, :nc, 12:15] - o['contact'][e, :nc, 12:15]).max() if int(fl['ncon'][e]) == nc else 0.0
            assert ef <= 6*ff + 3e-3*fs + 1e-4, (seed, e, ef, ff, fs)
    ev = np.abs(d.qvel.cpu().numpy() - o['qvel']).max()/max(np.abs(o['qvel']).max(), 1e-9)
    assert ev < 3e-3, (seed, m.nbody, m.nv, ev)


@pytest.mark.parametrize('solver', ['newton', 'cg'])
def test_elliptic_cone_more_rows_than_the_chip_holds(oracle, solver):
    """Bellies pressed in (20 contacts = 60 cone rows) and six spine joints past their limits: more than 64 rows, so the rows, their
    parameters and the values the rows of a contact exchange live in the HBM scratch of the env (the 'big' copy of the constraint
    code) - same bounds as on chip."""
    import torch
    from farms_mujoco_amd.physics import BatchedPhysics
    m = _walker(solver=solver, cone='elliptic')
    n = 6
    rng = np.random.default_rng(5)
    qpos = np.tile(m.qpos0, (n, 1)); qpos[:, 7:] += rng.uniform(-0.05, 0.05, (n, m.nq - 7))
    qpos[:, 2] = 0.012
    qpos[:4, 7 + 2:7 + 8] = 1.25
    qvel = rng.normal(size=(n, m.nv))*0.05; qvel[:, :2] += 0.2
    phys = BatchedPhysics(m, n)
    q32, v32, w32 = _set(phys, qpos, qvel, rng.normal(size=(n, m.nv))*2.0)
    rows, _ = phys.step_debug(want_pgs=False)
    torch.cuda.synchronize()
    d = phys.data
    assert int((d.status & ~8).abs().sum()) == 0                      # FMJ_WARN_CONTACTFULL allowed: both sides truncate alike
    o = oracle.step_tf(m, q32, v32, ctrl=np.zeros((n, m.nu)), warmstart=w32, want_AR=False)
    assert np.array_equal(d.ncon.cpu().numpy(), o['ncon']) and (o['nefc'][:4] > 64).all() and (o['nefc'][4:] <= 64).all()
    rows = rows.cpu().numpy().astype(np.float64)
    worst = 0.0
    for e in range(n):
        ne = int(o['nefc'][e]); fs = max(np.abs(o['efc'][e, :ne, 0]).max(), 1e-2)
        worst = max(worst, np.abs(rows[e, :ne, 4] - o['efc'][e, :ne, 0]).max()/fs)
    ev = np.abs(d.qvel.cpu().numpy() - o['qvel']).max()/np.abs(o['qvel']).max()
    print(solver, 'elliptic, rows', o['nefc'], 'row forces', worst, 'qvel', ev)
    assert worst < 3e-3 and ev < 3e-3


@pytest.mark.parametrize('seed', (301, 302, 303, 304, 305, 306))      # = test_gpu_random_trees.MESH_SEEDS[:6]: every draw has mesh geoms
@pytest.mark.parametrize('solver,cone', [('newton', 'pyramidal'), ('newton', 'elliptic')])
def test_primal_solvers_on_random_mesh_trees(oracle, seed, solver, cone):
    """Random trees whose collision shapes include convex meshes (hulls of 4 to ~30 vertices), with limits, over a plane, under Newton
    with either cone (the NEWTON + MESH and ELL instantiations): contact lists, contact-frame forces, velocity of one step."""
    import torch
    from farms_mujoco_amd.model import SOLVERS, CONES
    from farms_mujoco_amd.physics import BatchedPhysics
    m = random_tree(seed, contacts=True, meshes=True)
    assert m is not None and m.nv > 0 and m.nmeshvert > 0, f'seed {seed} no longer draws a tree with mesh geoms'
    m.solver = SOLVERS[solver]; m.cone = CONES[cone]; m.solver_iterations = 100
    rng = np.random.default_rng(5000 + seed)
    n = 6
    qpos = np.tile(m.qpos0, (n, 1)) + rng.uniform(-0.4, 0.4, (n, m.nq))
    for j in range(m.njnt):
        if m.jnt_type[j] == 0:
            a = m.jnt_qposadr[j]; q = rng.normal(size=(n, 4)); qpos[:, a+3:a+7] = q/np.linalg.norm(q, axis=1, keepdims=True)
            qpos[:, a+2] = rng.uniform(-0.05, 0.1, n)
    phys = BatchedPhysics(m, n)
    d = phys.data
    q32, v32, w32 = _set(phys, qpos, rng.normal(size=(n, m.nv))*0.2)
    phys.step(1)
    torch.cuda.synchronize()
    assert int((d.status & ~FMJ_WARN_CONTACTFULL).abs().sum()) == 0
    o = oracle.step_tf(m, q32, v32, ctrl=np.zeros((n, m.nu)) if m.nu else None, warmstart=w32, want_AR=False)
    assert np.array_equal(d.ncon.cpu().numpy(), o['ncon'])
    if o['nefc'].max() == 0:
        pytest.skip('no active constraint in this draw')
    con = oracle.contacts_from_hip(d.contact.cpu().numpy())
    for e in range(n):
        nc = int(o['ncon'][e])
        if nc:
            fs = max(np.abs(o['contact'][e, :nc, 12:15]).max(), 1e-2)
            assert np.abs(con[e, :nc, 12:15] - o['contact'][e, :nc, 12:15]).max() < 2e-2*fs + 2e-3, (seed, e)
    # per env: 3e-3 of the largest velocity; an env thrown into the plane so that it has more rows than the chip holds (here up to 126
    # rows from 31 mesh contacts, most of them redundant) is held to 1e-2: the dual costs of the two solutions agree to 3e-6 there,
    # the forces to 3e-3 of the largest, the velocity to 5e-3 - the conditioning of that contact set, not the stored matrices
    # (oracle.fp32_storage moves this step by 8e-6)
    vs = max(np.abs(o['qvel']).max(), 1e-9)
    for e in range(n):
        ev = np.abs(d.qvel.cpu().numpy()[e] - o['qvel'][e]).max()/vs
        assert ev < (3e-3 if o['nefc'][e] <= 64 else 1e-2), (seed, e, int(o['nefc'][e]), ev)


@pytest.mark.parametrize('solver', ['newton', 'cg'])
def test_frictionless_contacts_under_the_primal_solvers(oracle, solver):
    """The reference's arena has friction 0 (mjcf.py:1202) and a link without a friction option brings none either: the contact's
    friction is MuJoCo's floor 1e-5 and its pyramid rows carry R = 2 mu^2 R0 ~ 1e-10 R0, out of reach of an fp32 primal iteration.
    fmj_create then solves the whole model on the dual problem (PGS to the solver's tolerance, up to 10 x solver_iterations sweeps).
    A salamander settling on a frictionless floor, bellies pressed in and a joint past its limit.  The reference solution is the
    oracle's PGS with the same sweep budget: on the stiffest of these states (14 belly contacts, D = 1e10) the oracle's own fp64
    Newton does not get through in 100 iterations (it ends at a dual cost of +2e12), where it does the dual solve is within
    1e-3 of it."""
    import torch
    from farms_mujoco_amd.model import salamander33, SOLVERS
    from farms_mujoco_amd.physics import BatchedPhysics
    m = salamander33(contacts=True, limits=True, spawn_z=0.045)
    m.geom_friction = np.zeros_like(m.geom_friction)
    m.solver = SOLVERS[solver]; m.solver_iterations = 100
    mo = copy.copy(m); mo.solver = SOLVERS['pgs']; mo.solver_iterations = 1000
    n = 8
    rng = np.random.default_rng(2)
    qpos = np.tile(m.qpos0, (n, 1)); qpos[:, 7:] += rng.uniform(-0.1, 0.1, (n, m.nq - 7))
    qpos[:3, 2] = 0.015; qpos[:, 7 + 3] = 1.25
    qvel = rng.normal(size=(n, m.nv))*0.05; qvel[:, :2] += 0.2
    with pytest.warns(UserWarning, match='solved on the dual problem'):      # the swap is visible to the caller (fmj_solver_info, round 4)
        phys = BatchedPhysics(m, n)
    assert phys.solver_requested == {'newton': 'Newton', 'cg': 'CG'}[solver] and phys.solver_effective == 'PGS' and phys.solver_budget == 1000
    q32, v32, w32 = _set(phys, qpos, qvel)
    phys.step(1)
    torch.cuda.synchronize()
    d = phys.data
    o = oracle.step_tf(mo, q32, v32, ctrl=np.zeros((n, m.nu)), warmstart=w32, want_AR=False)
    assert int(d.status.abs().sum()) == 0 and np.array_equal(d.ncon.cpu().numpy(), o['ncon']) and o['ncon'].min() >= 1
    con = oracle.contacts_from_hip(d.contact.cpu().numpy())
    worst = 0.0
    for e in range(n):
        nc = int(o['ncon'][e]); fs = max(np.abs(o['contact'][e, :nc, 12]).max(), 1e-2)
        worst = max(worst, np.abs(con[e, :nc, 12:15] - o['contact'][e, :nc, 12:15]).max()/fs)
    ev = np.abs(d.qvel.cpu().numpy() - o['qvel']).max()/np.abs(o['qvel']).max()
    print(solver, 'frictionless: contact-frame forces', worst, 'qvel', ev)
    assert worst < 3e-3 and ev < 3e-3
    phys.step(59)
    torch.cuda.synchronize()
    ref = oracle.step(mo, q32, v32, ctrl=np.zeros((n, m.nu)), n_steps=60, n_threads=8)
    assert int(d.status.abs().sum()) == 0 and int(ref['status'].sum()) == 0
    e60 = np.abs(d.qpos.cpu().numpy() - ref['qpos']).max(1)
    print('  qpos abs err after 60 steps', e60)
    assert np.median(e60) < 2e-4 and e60.max() < 2e-3
