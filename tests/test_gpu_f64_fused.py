"""The opt-in fused launch of an fp64 context (fmj_step_fused_f64; Simulation(precision='fp64', fp64_fused=True)) against the fp64
oracle's fused loop (oracle.run_fused) on inputs that are fp32-representable; the oracle gets the controller's parameters, the units
and the water as the device holds them (fp32, widened).

Two bounds.  What a single forward pass produces - the rows of iteration0 and iteration0 + 1 and ctrl_out - is held to the rounding of
the fp32 store, the one-step bound of test_gpu_f64_step.py:
    |got - ref| <= ulp32(ref_i) + ulp32(max |ref| over the component's column group in that env)
A whole run (qpos, qvel, every ring row) is held to ``floor_state``: the same run as T oracle launches of one iteration each with qpos,
qvel, the poses and sensordata rounded to fp32 between them - what the per-iteration path realises at best.  The kernel keeps its state
in double inside a launch, so relerr(kernel) <= relerr(floor_state), per tensor, and the links / xfrc rows are at least 10x below the
oracle.fp32_storage() run's error (the floor of the fp32 kernels), which the per-iteration path can promise of qpos only."""
import ctypes

import numpy as np
import pytest

from parity_metrics import relerr
from support_sims import f64 as _f64, swim_sim, wave_at, rows as _rows
from support_f64_step import ulp_excess
from support_f64_fused import (FMJ_WARN_BADQPOS, CURRENT, STATE, RING, _model, _scaled_units, _sim, _f32, _oracle_args, _units, _device_state, _floor_state,
                                _references, _got, _check_one_pass_rows, _check_run)

pytestmark = pytest.mark.gpu

FMJ_ERR_ARG, FMJ_ERR_UNSUPPORTED = 1, 2      # include/fmj.h


def _wave_ctrl(wave, it, h):
    amp, lag = np.atleast_2d(wave['amplitude']), np.atleast_2d(wave['phase_lag'])
    f = np.atleast_1d(wave['frequency'])[:, None]
    return amp*np.sin(2*np.pi*f*(it*h) - lag + wave['env_phase'][:, None])


def _check_row0_positions_are_correctly_rounded(got, ref):
    """The positions of the iteration0 links row are fp32 inputs times 1 / meters: one double product, rounded once.  The oracle divides;
    the two differ by an ulp of the double, so the fp32 values are equal except where the quotient lies within 2^-52 of a rounding tie
    (a chance of 2^-29 per entry: none among these few hundred); a reciprocal taken in fp32 would move about a third of them."""
    pos = [0, 1, 2, 7, 8, 9]
    miss = float(np.mean(got['links'][0][..., pos] != ref['links'][0][..., pos].astype(np.float32)))
    print('row 0 positions not the correctly rounded quotient:', miss)
    assert miss <= 1e-3, miss


@pytest.mark.parametrize('name', ['salamander33', 'eel48', 'centipede_20_25', 'salamander33-units'])
def test_one_fused_launch_against_the_oracle(oracle, name):
    n, T = 4, 40
    units = _scaled_units() if name.endswith('-units') else None
    sim = _sim(name.split('-')[0], n, T, units=units)
    m = sim.physics.model
    assert (units is None) or min(abs(u - 1.0) for u in _units(sim)) > 0.2
    assert sim.physics.precision == 'fp64' and sim.physics.fp64_fused and sim.task.fusable()
    ref, floor, fst = _references(oracle, sim, m, T)
    # the water branches the run takes, from the reference's rows: a link above the surface leaves its xfrc row unwritten (zero), a
    # partly submerged one has 0 < surface - z < height
    swim, water, wave = _oracle_args(sim)
    z = ref['links'][:, :, swim['links_index'], 2]
    written = np.abs(ref['xfrc'][:, :, swim['xfrc_index']]).sum(-1) != 0
    depth = water['surface'] - z
    assert np.array_equal(written, z <= water['surface'])
    assert (~written).any() and (written & (depth < swim['heights'])).any(), (name, (~written).sum())
    assert sim.step_fused(T) == T
    got = _got(sim)
    assert not got['status'].any() and sim.task.sim_iteration == T
    _check_one_pass_rows(got, ref, (0, 1), name)
    _check_row0_positions_are_correctly_rounded(got, ref)
    ex = ulp_excess(got['ctrl'], _wave_ctrl(wave, T - 1, m.timestep))
    print(name, 'ctrl_out error / one-step bound', round(ex, 3))
    assert ex <= 1.0, ex
    _check_run(got, ref, floor, fst, name)


@pytest.mark.parametrize('units', [False, True])
def test_sub_steps_with_scaled_units(oracle, units):
    """S = 2 with links-only rows and drag on the sub-steps, in units other than 1: the carried torque / torques of the joints rows and the
    newtons / torques of the wrench the drag hands to the next step (and the same case in units of 1 beside it)."""
    _sub_step_case(oracle, 2, True, _scaled_units() if units else None)


@pytest.mark.parametrize('swim_substep', [True, False])
@pytest.mark.parametrize('S', [2, 3])
def test_sub_steps_and_the_end_rule(oracle, S, swim_substep):
    _sub_step_case(oracle, S, swim_substep)


def _sub_step_case(oracle, S, swim_substep, units=None):
    n, T = 3, 6
    sim = _sim('salamander33', n, T, substeps=S, swim_substep=swim_substep, units=units)
    m = sim.physics.model
    assert sim.task.substeps == S and bool(sim.task.substeps_links) == swim_substep and sim.task.fusable()
    ref, floor, fst = _references(oracle, sim, m, T, substeps=S, substep_links=swim_substep, n_iterations=T)
    assert sim.step_fused(T) == T
    got = _got(sim)
    assert not got['status'].any() and sim.task.sim_iteration == T*S
    what = f'S={S} substep={swim_substep} units={_units(sim)[0]:.3g}'
    _check_one_pass_rows(got, ref, (0,), what)
    _check_row0_positions_are_correctly_rounded(got, ref)
    _check_run(got, ref, floor, fst, what)
    assert np.abs(ref['joints'][..., 8]).max() > 0 and np.abs(ref['xfrc']).max() > 0      # torques and drag are in the rows
    for k in ('xpos', 'xquat', 'sensordata'):
        assert relerr(got[k], ref[k]) <= relerr(floor[k], ref[k]), k


def _launch(sim, cd, a, ext=None):
    """fmj_step_fused_f64 through the C-ABI; returns the status code."""
    from farms_mujoco_amd import _lib
    return sim.physics._lib.fmj_step_fused_f64(sim.physics._ctx, ctypes.byref(cd), ctypes.byref(a), None if ext is None else ctypes.byref(ext),
                                               _lib.stream_ptr(sim.physics.device))


def _abi_args(sim, T):
    from farms_mujoco_amd.simulation.simulation import _fused_args
    cd, a, ext = _fused_args(sim.task, sim.physics, T)
    a.iteration0, a.substep_links, a.n_iterations = 0, int(sim.task.substeps_links), T
    return cd, a, ext


@pytest.mark.parametrize('S', [1, 2])
def test_ctrl_tape_one_row_per_iteration(oracle, S):
    import torch
    n, T = 4, 10
    sim = _sim('eel20', n, T, substeps=S)
    m = sim.physics.model
    rng = np.random.default_rng(5)
    tape = torch.as_tensor(rng.uniform(-0.3, 0.3, (T, n, m.nu)), dtype=torch.float32, device='cuda:0')
    swim, water, _ = _oracle_args(sim)
    st = _device_state(sim)
    kw = dict(swim=swim, water=water, controller=0, ctrl=_f64(tape), ctrl_step_stride=n*m.nu, n_threads=8, substeps=S, n_iterations=T, units=_units(sim))
    ref = oracle.run_fused(m, st, T, buffer_size=T, **kw)
    with oracle.fp32_storage():
        fst = oracle.run_fused(m, st, T, buffer_size=T, **kw)
    # floor_state: a launch per iteration reads its own row of the tape
    fl, ring = st, {r: np.zeros_like(ref[r]) for r in RING}
    for k in range(T):
        o = oracle.run_fused(m, fl, 1, iteration0=k, buffer_size=T, **dict(kw, ctrl=_f64(tape[k:k + 1])))
        for r in RING:
            ring[r][k] = o[r][k]
        fl = {s: _f32(o[s]) for s in STATE}
    cd, a, _ = _abi_args(sim, T)
    a.controller, a.ctrl_step_stride, a.ctrl_out = 0, tape.stride(0), None
    cd.ctrl = tape.data_ptr()
    assert _launch(sim, cd, a) == 0, sim.physics._lib.fmj_last_error()
    got = _got(sim)
    assert not got['status'].any()
    _check_run(got, ref, dict(fl, **ring), fst, f'tape S={S}')


@pytest.mark.parametrize('fields', [('frequency',), ('amplitude',), ('phase_lag',), ('frequency', 'amplitude', 'phase_lag')])
def test_per_env_wave_parameters(oracle, fields):
    from farms_mujoco_amd.control import WaveController
    from farms_mujoco_amd.model import wave_controller_params
    n, T = 4, 10
    rng = np.random.default_rng(11)

    def controller(m, psi):
        amp, lag = wave_controller_params(m, 0.3, 1.0)
        kw = {}
        if 'amplitude' in fields:
            kw['amplitude_env'] = amp[None, :]*rng.uniform(0.5, 1.2, (n, 1))
        if 'phase_lag' in fields:
            kw['phase_lag_env'] = lag[None, :]*rng.uniform(0.6, 1.4, (n, 1))
        return WaveController(m, psi, frequency=_f32(rng.uniform(0.8, 2.5, n)) if 'frequency' in fields else 1.5, **kw)
    sim = _sim('eel20', n, T, controller_of=controller)
    m = sim.physics.model
    cd, a, ext = _abi_args(sim, T)
    assert ext is not None and bool(ext.wave_frequency_env) == ('frequency' in fields)
    assert (ext.wave_amplitude_env_stride != 0) == ('amplitude' in fields) and (ext.wave_phase_lag_env_stride != 0) == ('phase_lag' in fields)
    # the oracle once per env, with that env's own wave dict
    refs, floors, fsts = [], [], []
    for e in range(n):
        swim, water, wave = _oracle_args(sim, envs=slice(e, e + 1))
        wave = dict(wave, amplitude=wave['amplitude'][e] if wave['amplitude'].ndim == 2 else wave['amplitude'],
                    phase_lag=wave['phase_lag'][e] if wave['phase_lag'].ndim == 2 else wave['phase_lag'],
                    frequency=float(np.atleast_1d(wave['frequency'])[0]))
        st = _device_state(sim, slice(e, e + 1))
        kw = dict(swim=swim, water=water, controller=1, wave=wave, units=_units(sim))
        refs.append(oracle.run_fused(m, st, T, buffer_size=T, **kw))
        with oracle.fp32_storage():
            fsts.append(oracle.run_fused(m, st, T, buffer_size=T, **kw))
        floors.append(_floor_state(oracle, m, st, T, **kw))
    join = lambda outs: {k: np.concatenate([o[k] for o in outs], axis=1 if k in RING else 0) for k in ('qpos', 'qvel') + RING}
    assert _launch(sim, cd, a, ext) == 0, sim.physics._lib.fmj_last_error()
    got = _got(sim)
    assert not got['status'].any()
    ref = join(refs)
    _check_one_pass_rows(got, ref, (0, 1), str(fields))
    # ctrl_out: each env's own last command (the oracle hands no ctrl back: its expression, task.py:288-346, on the device's parameters)
    ex = ulp_excess(got['ctrl'], _wave_ctrl(_oracle_args(sim)[2], T - 1, m.timestep))
    print(fields, 'ctrl_out error / one-step bound', round(ex, 3))
    assert ex <= 1.0, ex
    _check_run(got, ref, join(floors), join(fsts), str(fields))


def test_ring_wraps_and_chunked_runs_repeat_and_resume_bitwise(tmp_path):
    import torch
    n, T, ring, chunk = 4, 24, 10, 10
    a = _sim('eel20', n, T, ring); a.run(chunk=chunk)
    b = _sim('eel20', n, T, ring); b.run(chunk=chunk)
    ga, gb = _got(a), _got(b)
    assert not ga['status'].any() and a.task.sim_iteration == T
    for k in STATE + RING:
        assert np.array_equal(ga[k], gb[k]), k
    # the same launches with a ring of T rows: row it of that ring is row it % ring here, for the last `ring` iterations
    full = _sim('eel20', n, T, T); full.run(chunk=chunk)
    gf = _got(full)
    for it in range(T - ring, T):
        for r in RING:
            assert np.array_equal(ga[r][it % ring], gf[r][it]), (r, it)
    for k in STATE:
        assert np.array_equal(ga[k], gf[k]), k
    # saved at a chunk boundary, loaded into a fresh simulation, continued with the same chunking
    c = _sim('eel20', n, T, ring)
    assert c.step_fused(chunk) == chunk
    c.save_state(str(tmp_path/'mid.npz'))
    d = _sim('eel20', n, T, ring)
    d.load_state(str(tmp_path/'mid.npz'))
    d.run(chunk=chunk)
    torch.cuda.synchronize()
    gd = _got(d)
    for k in ('qpos', 'qvel', 'sensordata', 'xpos'):
        assert np.array_equal(ga[k].view(np.int32), gd[k].view(np.int32)), k
    for r in RING:      # every row of the ring is written after the resume (iterations 10 .. 23)
        assert np.array_equal(ga[r].view(np.int32), gd[r].view(np.int32)), r


def test_a_nan_freezes_one_env_and_leaves_the_rest_alone():
    import torch
    n, T, bad = 6, 10, 2
    clean = _sim('centipede_20_25', n, T)
    clean.step_fused(5); clean.step_fused(5)
    gc = _got(clean)
    sim = _sim('centipede_20_25', n, T)
    d, sens = sim.physics.data, sim.task.data.sensors
    d.qpos[bad, sim.physics.model.nq - 1] = float('nan')
    for r in RING:
        getattr(sens, r).array[:, bad] = 7.25      # the sentinel
    before = {k: getattr(d, k)[bad].clone() for k in STATE + ('qacc', 'time', 'ctrl')}
    sim.step_fused(5)
    torch.cuda.synchronize()
    st = d.status.cpu().numpy()
    keep = [e for e in range(n) if e != bad]
    assert st[bad] & FMJ_WARN_BADQPOS and not st[keep].any(), st
    sim.step_fused(5)                                              # a second fused launch still skips the frozen env
    g = _got(sim)
    for k, v in before.items():
        assert torch.equal(getattr(d, k)[bad].view(torch.int32), v.view(torch.int32)), k
    for r in RING:
        assert np.all(g[r][:, bad] == np.float32(7.25)), r
        assert np.array_equal(g[r][:, keep], gc[r][:, keep]), r
    for k in STATE + ('ctrl',):
        assert np.array_equal(g[k][keep], gc[k][keep]), k


def test_results_do_not_depend_on_the_batch_slot():
    import torch
    from farms_mujoco_amd.model import synthetic_batch
    T = 8
    m0 = _model('salamander33')
    qpos, qvel, psi = synthetic_batch(m0, 3, seed=9)
    outs = []
    for n, slots in ((3, [0, 1, 2]), (7, [5, 0, 3]), (130, [129, 64, 1])):
        sim = _sim('salamander33', n, T)
        Q = np.tile(qpos[:1], (n, 1)); P = np.full(n, psi[0])
        for s, e in zip(slots, range(3)):
            Q[s], P[s] = qpos[e], psi[e]
        sim.task._controller.env_phase[:] = torch.as_tensor(P, dtype=torch.float32)
        sim.physics.data.qpos[:] = torch.as_tensor(Q, dtype=torch.float32)
        sim.physics.forward(disable_actuation=True)
        assert sim.step_fused(T) == T
        g = _got(sim)
        assert not g['status'].any()
        outs.append({k: (g[k][:, slots] if k in RING else g[k][slots]) for k in STATE + RING + ('ctrl',)})
    for o in outs[1:]:
        for k in o:
            assert np.array_equal(o[k], outs[0][k]), k


def _count_launches(monkeypatch):
    from farms_mujoco_amd.simulation import simulation as S
    calls, real = [], S._launch_fused

    def counted(phys, cd, a, ext):
        calls.append((int(a.n_steps), int(a.do_readout), int(a.do_drag), int(a.rows_ahead)))
        return real(phys, cd, a, ext)
    monkeypatch.setattr(S, '_launch_fused', counted)
    return calls


def test_through_the_api_fused(oracle, monkeypatch):
    n, T = 12, 40
    sim = _sim('eel48', n, T)
    m = sim.physics.model
    assert sim.task.fusable() and not sim.task.host_step_only
    ref, floor, fst = _references(oracle, sim, m, T)
    calls = _count_launches(monkeypatch)
    sim.run()
    got = _got(sim)
    assert calls == [(T, 1, 1, 0)], calls      # one fused launch of the whole ring
    assert not got['status'].any() and sim.task.sim_iteration == T
    _check_one_pass_rows(got, ref, (0, 1), 'eel48 api')
    _check_run(got, ref, floor, fst, 'eel48 api')


def test_through_the_api_with_a_host_callback(oracle, monkeypatch):
    """One callback without a device implementation: run() steps per iteration, every step a one-step launch of the new entry without rows
    or drag (before_step wrote them, in fp32).  Held to what the per-iteration fp64 path promises (test_gpu_f64_step.py)."""
    from farms_mujoco_amd.simulation.task import TaskCallback
    n, T = 12, 40
    sim = _sim('eel48', n, T, callbacks=[TaskCallback()])
    m = sim.physics.model
    assert not sim.task.fusable() and sim.task.controller_in_step() and not sim.task.rows_ahead_ok(sim.physics)
    swim, water, wave = _oracle_args(sim)
    st = _device_state(sim)
    kw = dict(swim=swim, water=water, controller=1, wave=wave, n_threads=8, units=_units(sim))
    ref = oracle.run_fused(m, st, T, buffer_size=T, **kw)
    with oracle.fp32_storage():
        fst = oracle.run_fused(m, st, T, buffer_size=T, **kw)
    calls = _count_launches(monkeypatch)
    sim.run()
    got = _got(sim)
    assert calls == [(1, 0, 0, 0)]*T, calls[:3]
    assert not got['status'].any() and sim.task.sim_iteration == T
    err = {k: relerr(got[k], ref[k]) for k in ('qpos', 'links', 'xfrc')}; fl = {k: relerr(fst[k], ref[k]) for k in err}
    print('eel48 fp64_fused, per-iteration path: whole-tensor error', err, 'fp32-storage run', fl)
    assert err['qpos'] <= fl['qpos']/10, (err, fl)
    assert err['links'] <= fl['links'] and err['xfrc'] <= fl['xfrc'], (err, fl)


def test_refusals_leave_the_state_and_the_ring_alone():
    import torch
    from farms_mujoco_amd import _lib
    n, T = 3, 4
    water = dict(height=-0.11, velocity=CURRENT)
    f32sim = swim_sim(n, T, seed=9, water_kwargs=water, controller_of=wave_at(1.5))[0]
    f64sim = _sim('salamander33', n, T)
    msg = lambda s: s.physics._lib.fmj_last_error().decode()

    def refused(sim, code, word, edit=lambda cd, a: None, ext=None):
        cd, a, _ = _abi_args(sim, T)
        edit(cd, a)
        q0 = sim.physics.data.qpos.clone(); ring0 = {r: v.copy() for r, v in _rows(sim).items()}
        rc = _launch(sim, cd, a, ext)
        torch.cuda.synchronize()
        assert rc == code and word in msg(sim), (rc, msg(sim))
        assert torch.equal(sim.physics.data.qpos, q0)
        for r, v in _rows(sim).items():
            assert np.array_equal(v, ring0[r]), r

    refused(f32sim, FMJ_ERR_UNSUPPORTED, 'fp64')

    def ahead(cd, a):
        a.rows_ahead = 1

    def contacts(cd, a):
        a.rows_base.contacts = a.rows_base.links
    refused(f64sim, FMJ_ERR_UNSUPPORTED, 'rows_ahead', ahead)
    refused(f64sim, FMJ_ERR_ARG, 'contact', contacts)
    refused(f64sim, FMJ_ERR_ARG, 'size', ext=_lib.CFusedExt(8, 0))
    # and the entry points that were there before keep refusing the fp64 context
    with pytest.raises(_lib.FmjError, match='fp64'):
        cd, a, _ = _abi_args(f64sim, T)
        _lib.check(f64sim.physics._lib.fmj_step_fused(f64sim.physics._ctx, ctypes.byref(cd), ctypes.byref(a), _lib.stream_ptr(f64sim.physics.device)))
