"""The opt-in fp64 step kernel (BatchedPhysics(precision='fp64'), csrc/fmj_f64.inc) against the plain fp64 oracle on inputs that are
fp32-representable.

One step, fmj_forward and the stage outputs of fmj_forward_debug are held to the rounding of the fp32 store:
    |got - ref| <= ulp32(ref_i) + ulp32(max |ref| over the component's column group in that env)
The output is rounded to fp32 once (half an ulp of its own size); fp64 arithmetic noise times the documented condition numbers (2e5 to
above 1e6) is about 1e-9 of the group's size, a small fraction of one ulp32 of it, which the second term allows with about 50x room.
Rollouts are held to the oracle stepped with its state rounded to fp32 between steps (the only rounding the fp32 C-ABI forces)."""
import ctypes

import numpy as np
import pytest

from parity_metrics import relerr, link_row_groups
from wide_trees import WIDE_SHAPES, shape_tree, dof_depth
from support_models import random_tree, tree_inputs as _inputs
from support_sims import f64 as _f64, swim_sim, wave_at, swim_oracle as _swim_oracle
from support_f64_step import MODELS, _make, _phys, ulp_excess, _field_groups

pytestmark = pytest.mark.gpu


def _step_excess(oracle, m, n, seed, precision, forward):
    import torch
    qpos, qvel, ctrl, xf, qs = _inputs(m, n, seed)
    phys, ins = _phys(m, n, qpos, qvel, ctrl, xf, qs, precision)
    q0, v0 = phys.data.qpos.clone(), phys.data.qvel.clone()
    if forward:
        phys.forward()
    else:
        phys.step(1)
    torch.cuda.synchronize()
    assert int(phys.data.status.abs().sum()) == 0
    ref = oracle.step(m, ins['qpos'], ins['qvel'], ctrl=ins['ctrl'], qpos_spring=ins['qpos_spring'], xfrc_applied=ins['xfrc_applied'])
    if forward:      # mj_forward leaves the state alone; the derived fields are those of the step's forward pass
        assert torch.equal(phys.data.qpos, q0) and torch.equal(phys.data.qvel, v0)
        ref = dict(ref, qpos=ins['qpos'], qvel=ins['qvel'])
    return {k: ulp_excess(getattr(phys.data, k).cpu().numpy(), ref[k], g) for k, g in _field_groups(m).items()}


@pytest.mark.parametrize('integrator', ['Euler', 'implicitfast'])
@pytest.mark.parametrize('name', MODELS)
def test_one_step_and_forward_to_the_ulp(oracle, name, integrator):
    m = _make(name, integrator)
    seed = MODELS.index(name)
    for forward in (False, True):
        ex = _step_excess(oracle, m, 4, seed, 'fp64', forward)
        print(name, integrator, 'forward' if forward else 'step', 'error / bound per field:', {k: round(v, 3) for k, v in ex.items()})
        bad = {k: v for k, v in ex.items() if v > 1.0}
        assert not bad, (name, integrator, forward, bad)


def test_the_fp32_context_fails_the_ulp_bound_on_eel48(oracle):
    """The bound tells the two paths apart: the fp32 step kernel on the same inputs is far outside it."""
    m = _make('eel48')
    ex = _step_excess(oracle, m, 4, MODELS.index('eel48'), 'fp32', False)
    print('eel48 fp32 context, error / bound per field:', ex)
    assert ex['qvel'] > 1.0 and ex['qacc'] > 1.0, ex


@pytest.mark.parametrize('name', MODELS)
def test_stage_outputs_to_the_ulp(oracle, name):
    """fmj_forward_debug: the rows of H = M + diag(armature + h damping) and qfrc_smooth against oracle.forward_debug (the fp32
    kernels' yardstick for this stage is 1e-5 absolute).  Groups: the entries of H of one env; qfrc_smooth of one env."""
    import torch
    m = _make(name)
    n = 4
    qpos, qvel, ctrl, xf, qs = _inputs(m, n, MODELS.index(name))
    phys, ins = _phys(m, n, qpos, qvel, ctrl, xf, qs)
    H, qf = phys.forward_debug()
    torch.cuda.synchronize()
    rs = H.shape[2]
    depth = dof_depth(m)
    assert rs == (int(depth.max()) + 4)//4*4
    Hrows = H.cpu().numpy()
    assert H.shape == (n, m.nv, rs) and np.all(H._base.cpu().numpy()[n*m.nv*rs:] == 0.0)
    Href = np.zeros_like(Hrows, dtype=np.float64); qref = np.zeros((n, m.nv))
    for e in range(n):
        o = oracle.forward_debug(m, ins['qpos'][e], ins['qvel'][e], ctrl=ins['ctrl'][e] if m.nu else None, qpos_spring=ins['qpos_spring'][e],
                                 xfrc_applied=ins['xfrc_applied'][e])
        Hd = o['M'] + np.diag(m.timestep*m.dof_damping)
        for i in range(m.nv):
            j = i
            while j >= 0:
                Href[e, i, depth[j]] = Hd[i, j]; j = m.dof_parentid[j]
        qref[e] = o['qfrc_smooth']
    eh, eq = ulp_excess(Hrows, Href), ulp_excess(qf.cpu().numpy(), qref)
    print(name, 'H error / bound', eh, 'qfrc_smooth error / bound', eq)
    assert eh <= 1.0 and eq <= 1.0, (name, eh, eq)


def _rollout_setup(m, n=4):
    """synthetic_batch(seed=9) and a constant ctrl."""
    import farms_mujoco_amd.model as mm
    # a constant ctrl, random per env: the travelling-wave command frozen at the env's random phase (what the project's controller sends
    # at one instant; zero on velocity / torque actuators).  A uniform random ctrl on all 81 actuators of the salamander is not a usable
    # input: held for 1000 steps it drives the ORACLE itself to NaN in two of four envs.
    qpos, qvel, psi = mm.synthetic_batch(m, n, seed=9)
    amp, lag = mm.wave_controller_params(m, amplitude=0.25)
    return qpos, qvel, amp[None, :]*np.sin(psi[:, None] - lag[None, :])


@pytest.mark.parametrize('name,T', [('eel48', 300), ('eel58', 300), ('centipede_20_25', 300), ('salamander33', 1000)])
def test_rollout_against_the_state_rounding_floor(oracle, name, T):
    """fmj_step(n_steps=T) against the plain oracle.  floor_state: the oracle stepped one step at a time with qpos / qvel rounded to fp32
    between steps; floor_store: oracle.fp32_storage() (M / H stored in fp32: the floor of the fp32 kernels).  The device rounds the state
    at other points than floor_state does - two realisations of the same random walk - hence the factor 3."""
    import torch
    m = _make(name)
    n = 4
    qpos, qvel, ctrl = _rollout_setup(m, n)
    phys, ins = _phys(m, n, qpos, qvel, ctrl)
    phys.step(T)
    torch.cuda.synchronize()
    assert int(phys.data.status.abs().sum()) == 0
    kw = dict(ctrl=ins['ctrl'], qpos_spring=ins['qpos_spring'])
    ref = oracle.step(m, ins['qpos'], ins['qvel'], n_steps=T, n_threads=4, **kw)
    with oracle.fp32_storage():
        fst = oracle.step(m, ins['qpos'], ins['qvel'], n_steps=T, n_threads=4, **kw)
    q, v = ins['qpos'], ins['qvel']
    for _ in range(T):
        o = oracle.step(m, q, v, n_steps=1, n_threads=4, **kw)
        q = o['qpos'].astype(np.float32).astype(np.float64); v = o['qvel'].astype(np.float32).astype(np.float64)
    got = phys.data.qpos.cpu().numpy()
    err, floor_state, floor_store = relerr(got, ref['qpos']), relerr(q, ref['qpos']), relerr(fst['qpos'], ref['qpos'])
    print(name, 'qpos after', T, 'steps: fp64 kernel', err, 'floor_state', floor_state, 'floor_store', floor_store)
    assert err <= 3*floor_state, (name, err, floor_state)
    if name in ('eel48', 'eel58'):
        assert err <= floor_store/10, (name, err, floor_store)
    per_env = [relerr(got[e], ref['qpos'][e]) for e in range(n)]
    assert max(per_env) <= 1e-4, (name, per_env)


def test_swim_of_a_long_eel_through_the_api(oracle):
    """Simulation(precision='fp64') on eel(48), 40 iterations with drag and the wave controller: run() takes the per-iteration path
    by itself.  Rows and drag are fp32 operators on this path, so it is measured against the oracle's fused loop with fp32 storage:
    qpos at least 10x below that run's error, link and xfrc rows at or below it."""
    import torch
    from farms_mujoco_amd._lib import FmjError
    m = _make('eel48')
    T, n = 40, 12
    sim = swim_sim(n, T, m=m, seed=9, controller_of=wave_at(1.5), precision='fp64')[0]
    assert sim.physics.precision == 'fp64' and not sim.task.fusable()
    ref = _swim_oracle(oracle, sim, m, T)
    with oracle.fp32_storage():
        flo = _swim_oracle(oracle, sim, m, T)
    with pytest.raises(FmjError, match='fp64'):
        sim.step_fused(1)
    sim.run()
    torch.cuda.synchronize()
    assert int(sim.physics.data.status.abs().sum()) == 0 and sim.task.sim_iteration == T
    sens = sim.task.data.sensors
    got = dict(qpos=sim.physics.data.qpos.cpu().numpy(), links=sens.links.array.cpu().numpy(), xfrc=sens.xfrc.array.cpu().numpy())
    err = {k: relerr(got[k], ref[k]) for k in got}; fl = {k: relerr(flo[k], ref[k]) for k in got}
    print('eel48 fp64 simulation, whole-tensor error', err, 'fp32-storage run', fl)
    assert err['qpos'] <= fl['qpos']/10, (err, fl)
    assert err['links'] <= fl['links'] and err['xfrc'] <= fl['xfrc'], (err, fl)


def test_checkpoint_continues_bit_for_bit(tmp_path):
    import torch
    m = _make('eel20')
    T, n = 24, 4
    a = swim_sim(n, T, m=m, seed=9, controller_of=wave_at(1.5), precision='fp64')[0]
    a.run()
    b = swim_sim(n, T, m=m, seed=9, controller_of=wave_at(1.5), precision='fp64')[0]
    for _ in range(10):
        b._env_step()
    b.save_state(str(tmp_path/'mid.npz'))
    c = swim_sim(n, T, m=m, seed=9, controller_of=wave_at(1.5), precision='fp64')[0]
    c.load_state(str(tmp_path/'mid.npz'))
    c.run()
    torch.cuda.synchronize()
    for k in ('qpos', 'qvel', 'sensordata', 'xpos'):
        assert torch.equal(getattr(a.physics.data, k), getattr(c.physics.data, k)), k
    assert torch.equal(a.task.data.sensors.links.array, c.task.data.sensors.links.array)


def test_results_do_not_depend_on_the_batch_slot(oracle):
    import torch
    m = _make('centipede_20_25')
    qpos, qvel, ctrl = _rollout_setup(m, 3)
    outs = []
    for n, slots in ((3, [0, 1, 2]), (7, [5, 0, 3]), (130, [129, 64, 1])):
        Q = np.tile(qpos[:1], (n, 1)); V = np.tile(qvel[:1], (n, 1))*0.5; C = np.zeros((n, m.nu))
        for s, e in zip(slots, range(3)):
            Q[s], V[s], C[s] = qpos[e], qvel[e], ctrl[e]
        phys, _ = _phys(m, n, Q, V, C)
        phys.step(5)
        torch.cuda.synchronize()
        outs.append({k: getattr(phys.data, k)[slots].cpu().numpy() for k in ('qpos', 'qvel', 'qacc', 'sensordata', 'xpos')})
    for o in outs[1:]:
        for k in o:
            assert np.array_equal(o[k], outs[0][k]), k


def test_a_nan_freezes_one_env_and_leaves_the_rest_alone():
    import torch
    m = _make('centipede_20_25')
    n = 6
    qpos, qvel, ctrl = _rollout_setup(m, n)
    clean, _ = _phys(m, n, qpos, qvel, ctrl)
    clean.step(3); clean.step(2)
    bad_q = qpos.copy(); bad_q[2, m.nq - 1] = np.nan
    phys, _ = _phys(m, n, bad_q, qvel, ctrl)
    before = {k: getattr(phys.data, k)[2].clone() for k in ('qpos', 'qvel', 'qacc', 'xpos', 'xquat', 'xipos', 'sensordata', 'time')}
    phys.step(3)
    torch.cuda.synchronize()
    st = phys.data.status.cpu().numpy()
    assert st[2] & 1 and not st[[0, 1, 3, 4, 5]].any(), st        # FMJ_WARN_BADQPOS
    phys.step(2)                                                   # a later launch still skips the frozen env
    torch.cuda.synchronize()
    for k, v in before.items():
        assert torch.equal(getattr(phys.data, k)[2].view(torch.int32), v.view(torch.int32)), k
    keep = [0, 1, 3, 4, 5]
    for k in ('qpos', 'qvel', 'qacc', 'xpos', 'sensordata', 'time'):
        assert torch.equal(getattr(phys.data, k)[keep], getattr(clean.data, k)[keep]), k


@pytest.mark.parametrize('name', ['salamander33', 'centipede_20_25'])
def test_create_ex_with_null_options_is_fmj_create(name):
    """fmj_create_ex(opts = NULL) and fmj_create choose the same path and step to identical bits."""
    import torch
    from farms_mujoco_amd import _lib
    from farms_mujoco_amd.physics import BatchedPhysics
    m = _make(name)
    n = 8
    qpos, qvel, ctrl = _rollout_setup(m, n)
    a, _ = _phys(m, n, qpos, qvel, ctrl, precision='fp32')
    b, _ = _phys(m, n, qpos, qvel, ctrl, precision='fp32')
    ctx = ctypes.c_void_p()
    _lib.check(b._lib.fmj_create_ex(ctypes.byref(b._cmodel), n, 0, None, ctypes.byref(ctx)))
    b._lib.fmj_destroy(b._ctx); b._ctx = ctx
    assert b._lib.fmj_precision(ctx) == 0 and a.kernel_info() == b.kernel_info()
    a.step(20); b.step(20)
    torch.cuda.synchronize()
    for k in ('qpos', 'qvel', 'qacc', 'sensordata', 'xpos', 'xquat', 'xipos', 'time'):
        assert torch.equal(getattr(a.data, k), getattr(b.data, k)), k


def test_kernel_info_reports_the_fp64_kernel():
    m = _make('centipede_20_25')
    phys, _ = _phys(m, 2, *_rollout_setup(m, 2))
    info = phys.kernel_info()
    assert info['threads_per_env'] == 128 and 0 < info['lds_bytes_per_env'] <= 160*1024, info
