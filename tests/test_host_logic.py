"""ExperimentTask / Simulation sequencing logic (no GPU): iteration counters, ring index, sub-step quirk,
kwargs strictness — mirrored from reference farms_mujoco/simulation/task.py."""
import ctypes
from types import SimpleNamespace

import numpy as np
import pytest

from farms_mujoco_amd.simulation.task import ExperimentTask, SwimmingCallback, TaskCallback, duration2nit


class _FakePhysics:
    pass


class _Recorder(TaskCallback):
    def __init__(self, substep=False):
        super().__init__(substep=substep)
        self.before, self.after = [], []

    def before_step(self, task, action, physics): self.before.append((task.sim_iteration, task.iteration))
    def after_step(self, task, physics): self.after.append((task.sim_iteration, task.iteration))


def _task(**kw):
    t = ExperimentTask(base_link='b', n_iterations=kw.pop('n_iterations', 6), timestep=1e-3, **kw)
    t.update_sensors = lambda physics, links_only=False, swimming=None: t._sensor_calls.append((t.iteration % t.buffer_size, links_only))
    t._sensor_calls = []
    return t


def test_kwargs_strictness():
    with pytest.raises(AssertionError):
        ExperimentTask(base_link='b', n_iterations=1, timestep=1e-3, bogus=1)      # task.py:73
    assert duration2nit(1.0, 1e-3) == 1000


def test_counters_no_substeps():
    cb = _Recorder()
    t = _task(callbacks=[cb], buffer_size=4)
    for _ in range(6):
        t.before_step(None, _FakePhysics()); t.after_step(_FakePhysics())
    assert t.iteration == 6 and t.sim_iteration == 6
    assert [c[0] for c in t._sensor_calls] == [0, 1, 2, 3, 0, 1]          # ring index = iteration % buffer_size
    assert all(not lo for _, lo in t._sensor_calls)
    assert cb.before == [(i, i) for i in range(6)]
    assert t.get_termination(_FakePhysics()) == 1


def test_substep_quirk_matches_reference():
    """With substeps > 1 the reference advances `iteration` after the first sub-step of each group
    (task.py:352-355 tests (sim_iteration + 1) % substeps after incrementing)."""
    sub = 3
    cb, cbs = _Recorder(), _Recorder(substep=True)
    t = _task(n_iterations=4, substeps=sub, callbacks=[cb, cbs])
    its = []
    for _ in range(4*sub - 1):
        t.before_step(None, _FakePhysics()); t.after_step(_FakePhysics())
        its.append(t.iteration)
    assert its[:7] == [0, 1, 1, 1, 2, 2, 2]
    # full-step callback only on sim_iteration % substeps == 0, sub-step callback every step
    assert [s for s, _ in cb.before] == [0, 3, 6, 9]
    assert len(cbs.before) == 4*sub - 1
    # sensors: full rows on full steps, links_only rows on sub-steps because a callback asked for sub-steps
    assert [lo for _, lo in t._sensor_calls[:4]] == [False, True, True, False]


def test_substeps_past_the_last_iteration_write_nothing():
    """run() executes all n_iterations * substeps steps; the reference never executes the sub-steps whose task.iteration
    has reached n_iterations (its assert at task.py:170).  They run here, but write no rows and call no sub-step callback: ring index
    n_iterations % buffer_size would be row 0 of a full log."""
    sub, n_it = 3, 4
    cb, cbs = _Recorder(), _Recorder(substep=True)
    t = _task(n_iterations=n_it, substeps=sub, callbacks=[cb, cbs], buffer_size=n_it)
    for _ in range(n_it*sub):
        t.before_step(None, _FakePhysics()); t.after_step(_FakePhysics())
    assert t.sim_iteration == n_it*sub and t.iteration == n_it
    assert len(cbs.before) == n_it*sub - 1 and all(it < n_it for _, it in cbs.before)
    assert len(t._sensor_calls) == n_it*sub - 1
    assert [i for i, lo in t._sensor_calls if i == 0] == [0, 0]            # row 0: the first full step and its first sub-step, nothing later


def test_fusable_rules():
    class DevCb(TaskCallback):
        fusable = True
    assert _task().fusable()
    assert _task(callbacks=[DevCb()]).fusable()
    assert not _task(callbacks=[_Recorder()]).fusable()        # arbitrary host callbacks need per-step launches
    assert _task(callbacks=[DevCb()], substeps=2).fusable()     # round 4: the fused kernel sequences sub-steps itself (include/fmj.h)
    assert not _task(callbacks=[_Recorder(substep=True)], substeps=2).fusable()


def test_units_and_options():
    from farms_mujoco_amd.units import SimulationUnitScaling
    from farms_mujoco_amd.options import SimulationOptions, WaterOptions
    u = SimulationUnitScaling(meters=2.0, seconds=0.5, kilograms=3.0)
    assert u.velocity == 4.0 and u.acceleration == 8.0 and u.newtons == 24.0 and u.torques == 48.0
    assert u.angular_velocity == 2.0 and u.inertia == 12.0
    with pytest.raises(AssertionError):
        SimulationOptions(nope=1)
    with pytest.raises(AssertionError):
        WaterOptions(nope=1)
    assert SimulationOptions().integrator == 'Euler'


def test_synthetic_batch_is_keyed_by_global_index():
    """Env e's inputs depend only on its global index, so any contiguous sharding reproduces them."""
    from farms_mujoco_amd.model import salamander33, synthetic_batch
    m = salamander33()
    q, v, psi = synthetic_batch(m, 12, seed=3)
    q2, v2, psi2 = synthetic_batch(m, 5, seed=3, env_offset=4)
    assert np.array_equal(q[4:9], q2) and np.array_equal(psi[4:9], psi2)


def test_animat_data_log_round_trip(tmp_path):
    """AnimatData.to_file / from_file (reference simulation.py:200-203 writes simulation.hdf5; .npz when h5py is
    absent): arrays, names and the iteration cut survive."""
    import torch
    from farms_mujoco_amd.data import AnimatData
    d = AnimatData(1e-3, 6, 3, ['a', 'b'], ['j0'], contacts=[('a', ''), ('b', 'a')], device='cpu')
    g = torch.Generator().manual_seed(0)
    for k in ('links', 'joints', 'xfrc', 'contacts'):
        arr = getattr(d.sensors, k).array
        arr.copy_(torch.rand(arr.shape, generator=g))
    path = d.to_file(str(tmp_path/'simulation.hdf5'), iteration=4)
    back = AnimatData.from_file(path)
    assert back.timestep == 1e-3 and back.buffer_size == 4 and back.n_envs == 3
    assert back.sensors.links.names == ['a', 'b'] and back.sensors.joints.names == ['j0']
    for k in ('links', 'joints', 'xfrc', 'contacts'):
        assert torch.equal(getattr(back.sensors, k).array, getattr(d.sensors, k).array[:4])
    assert len(back.sensors.contacts.names) == 2


class _StatusPhysics:
    """Stands in for BatchedPhysics in the host-logic tests: counts steps, reports a bad env from step `bad_at` on."""
    def __init__(self, bad_at=None):
        self.steps, self.bad_at = 0, bad_at

    def step(self, n=1):
        self.steps += n

    def check_invalid_state(self):
        from farms_mujoco_amd.physics import PhysicsError
        if self.bad_at is not None and self.steps >= self.bad_at:
            raise PhysicsError('bad simulation state in 1 env(s); first env 0 status bits 2')


def _host_sim(n_iterations=30, handle_exceptions=False, bad_at=None, check_every=5, substeps=1):
    """Simulation with the device side stubbed out (constructor bypassed): sequencing and error policy only."""
    from farms_mujoco_amd.simulation.simulation import Simulation
    sim = Simulation.__new__(Simulation)
    sim.physics = _StatusPhysics(bad_at)
    sim.handle_exceptions = handle_exceptions
    sim.check_every = check_every
    sim.task = _task(n_iterations=n_iterations, substeps=substeps)
    sim._needs_reset = False
    return sim


def test_run_physics_error_policy():
    """reference simulation.py:153-161: run() logs and re-raises PhysicsError, or returns when handle_exceptions."""
    from farms_mujoco_amd.physics import PhysicsError
    sim = _host_sim(bad_at=12)
    with pytest.raises(PhysicsError):
        sim.run(fused=False)
    assert sim.physics.steps == 15 and sim.task.iteration == 15        # noticed at the first status look after step 12
    sim = _host_sim(bad_at=12, handle_exceptions=True)
    assert sim.run(fused=False) is None and sim.physics.steps == 15
    ok = _host_sim()
    ok.run(fused=False)
    assert ok.physics.steps == 30 and ok.task.iteration == 30


def test_iterator_physics_error_policy():
    """reference simulation.py:164-179: iterator() yields the iteration before stepping it and always re-raises."""
    from farms_mujoco_amd.physics import PhysicsError
    sim = _host_sim(bad_at=7, handle_exceptions=True, substeps=2, n_iterations=10)
    seen = []
    with pytest.raises(PhysicsError):
        for it in sim.iterator(show_progress=False, verbose=False):
            seen.append(it)
    assert seen == list(range(5)) and sim.physics.steps == 10           # 5 iterations x 2 sub-steps, checked every 5
    ok = _host_sim(n_iterations=4)
    assert list(ok.iterator()) == [0, 1, 2, 3] and ok.physics.steps == 4


def test_unsupported_solver_options_are_refused():
    """integrator / cone / solver other than Euler / pyramidal / PGS, CG or Newton must not silently run different physics
    (the reference forwards them to MuJoCo, mjcf.py:1342-1365)."""
    from farms_mujoco_amd.options import SimulationOptions
    from farms_mujoco_amd.simulation.mjcf import check_supported_options
    check_supported_options(SimulationOptions())
    check_supported_options(SimulationOptions(solver='Newton'))        # round 3: the device has MuJoCo's Newton and CG solvers too
    check_supported_options(SimulationOptions(solver='CG'))
    check_supported_options(SimulationOptions(solver='Newton', cone='elliptic'))
    check_supported_options(SimulationOptions(integrator='implicitfast'))     # round 4
    check_supported_options(SimulationOptions(noslip_iterations=3), compile_only=True)      # the model compiler forwards it (MJCF export)
    check_supported_options(None)
    check_supported_options(SimulationOptions(cone='elliptic', solver='PGS'))     # round 5: MuJoCo's elliptic PGS on the device
    check_supported_options(SimulationOptions(noslip_iterations=3))               # round 5: the noslip post-pass
    check_supported_options(SimulationOptions(integrator='RK4'))                  # round 5: mj_RungeKutta through fmj_step
    for kw, word in ((dict(integrator='implicit'), 'Coriolis'), (dict(solver='SOR'), 'pgs')):
        with pytest.raises(NotImplementedError, match=word):      # a refusal says why
            check_supported_options(SimulationOptions(**kw))


def test_task_spec_hooks_and_restart_flag():
    """reference task.py:371-412: the spec hooks fan out to the callbacks, action_spec concatenates what they return;
    restart needs an application (task.py:91-94)."""
    class Cb(TaskCallback):
        def __init__(self): super().__init__(); self.calls = []
        def action_spec(self, task, physics): self.calls.append('a'); return ['u']
        def step_spec(self, task, physics): self.calls.append('s')
        def get_observation(self, task, physics): self.calls.append('o')
        def observation_spec(self, task, physics): self.calls.append('os')
    a, b = Cb(), Cb()
    t = _task(callbacks=[a, b])
    assert t.action_spec(_FakePhysics()) == ['u', 'u']
    t.step_spec(_FakePhysics()); t.get_observation(_FakePhysics()); t.observation_spec(_FakePhysics())
    assert a.calls == b.calls == ['a', 's', 'o', 'os']
    closed = []
    t2 = _task(n_iterations=2)
    t2.set_app(type('App', (), {'close': lambda self: closed.append(1)})())
    for _ in range(2):
        t2.before_step(None, _FakePhysics()); t2.after_step(_FakePhysics())
    assert closed == [1]                                                  # task.py:358-364: the app is closed at the end
    with pytest.raises(AssertionError):
        ExperimentTask(base_link='b', n_iterations=1, timestep=1e-3, restart=True).initialize_episode(_FakePhysics())


# ---- what a fused launch is told ----------------------------------------------------------------------------------------------

def _fields(s):
    """A ctypes struct as a dict: nested structs as dicts, arrays as lists, pointers as integers or None."""
    get = lambda v: _fields(v) if isinstance(v, ctypes.Structure) else list(v) if isinstance(v, ctypes.Array) else v
    return {name: get(getattr(s, name)) for name, _ in s._fields_}


def _launch_sim(monkeypatch, substeps, controller, callbacks):
    """A Simulation over stand-ins (constructor bypassed; AnimatData on the CPU, only data_ptr() and stride() are read) whose launches
    are recorded instead of made: ``(sim, launches)``, a launch = the fields of (CData, CFusedArgs, ext) as _launch_fused got them."""
    import torch
    from farms_mujoco_amd import _lib
    from farms_mujoco_amd.data import AnimatData
    from farms_mujoco_amd.simulation import simulation
    from farms_mujoco_amd.swimming.drag import WaterProperties
    from farms_mujoco_amd.units import SimulationUnitScaling
    n_envs, nu = 3, 4
    data = AnimatData(1e-3, 5, n_envs, ['a', 'b', 'c'], ['j0', 'j1'], contacts=[('a', '')] if substeps > 1 else (), device='cpu')
    swim = SwimmingCallback(None, None)
    swim.handler = SimpleNamespace(drag=True, buoyancy=False, water=WaterProperties(0.25, 1000.0, [0.5, -1.0, 2.0], 1.5))
    task = ExperimentTask(base_link='a', n_iterations=7, timestep=1e-3, data=data, controller=controller, callbacks=[swim] + callbacks,
                          substeps=substeps, buffer_size=5, units=SimulationUnitScaling(meters=2.0, seconds=0.5, kilograms=3.0))
    phys = SimpleNamespace(n_envs=n_envs, model=SimpleNamespace(nu=nu), device='cpu', precision='fp32', has_constraints=substeps > 1,
                           data=SimpleNamespace(ctrl=torch.zeros(n_envs, nu), ncon=torch.tensor([1, 4, 4], dtype=torch.int32)),
                           _cdata=lambda: _lib.CData(*range(101, 116)))
    sim = simulation.Simulation.__new__(simulation.Simulation)
    sim.task, sim.physics, sim.order_by_contacts = task, phys, True
    launches = []
    monkeypatch.setattr(simulation, '_launch_fused',
                        lambda phys, cd, a, ext: launches.append((_fields(cd), _fields(a), None if ext is None else _fields(ext))))
    return sim, launches


def test_fused_launch_descriptions(monkeypatch):
    """Every field of what Simulation.step_fused and Simulation._step_with_controller hand to _launch_fused (simulation._fused_args
    and what each adds to it), against values written out here from the stand-ins' tensors as the two methods filled them before
    they shared that function - the fields that stay zero included.  The one-step launches alternate on their one struct: a launch
    without rows switches off (do_readout = do_drag = rows_ahead = 0) what the launch with rows before it left there, and the water
    is read again at every launch with rows."""
    import torch
    from farms_mujoco_amd import _lib
    f32 = lambda x: float(np.float32(x))
    zero = _fields(_lib.CFusedArgs())
    assert zero['rows_base'] == dict(links=None, joints=None, xfrc=None, contacts=None) and zero['n_iterations'] == 0
    cdata = _fields(_lib.CData(*range(101, 116)))
    units = dict(meters=2.0, newtons=24.0, torques=48.0, velocity=4.0, angular_velocity=2.0, kilograms=3.0)
    water = lambda vel: dict(surface=0.25, density=1000.0, viscosity=1.5, velocity=[f32(v) for v in vel], gravity=f32(-9.81), use_buoyancy=0)

    # a chunk: sub-steps, a sub-step callback, a contact sensor, a swimming callback, a controller that hands over a ctrl tape
    class Sub(TaskCallback):
        fusable = True
    tape = torch.zeros(8, 3, 4)
    sim, launches = _launch_sim(monkeypatch, 2, SimpleNamespace(fusable=True, tape=True, ctrl_tape=lambda n: tape[:n]), [Sub(substep=True)])
    s, task = sim.task.data.sensors, sim.task
    task.sim_iteration, task.iteration = 8, 4
    assert sim.step_fused(5) == 3 and (task.sim_iteration, task.iteration, sim._rows_for) == (14, 7, -1)      # 7 iterations in all
    assert sim._env_order.tolist() == [1, 2, 0] and sim._env_order.dtype == torch.int32
    (cd, a, ext), = launches
    assert ext is None and cd == dict(cdata, ctrl=tape.data_ptr())
    assert a == dict(zero, n_steps=3, iteration0=4, buffer_size=5, do_readout=1, do_drag=1, controller=0, ctrl_step_stride=12,
                     row_stride_links=s.links.array.stride(0), row_stride_joints=s.joints.array.stride(0),
                     row_stride_xfrc=s.xfrc.array.stride(0), row_stride_contacts=s.contacts.array.stride(0),
                     rows_base=dict(links=s.links.array.data_ptr(), joints=s.joints.array.data_ptr(), xfrc=s.xfrc.array.data_ptr(),
                                    contacts=s.contacts.array.data_ptr()),
                     water=water([0.5, -1.0, 2.0]), units=units, env_order=sim._env_order.data_ptr(), substeps=2, substep_links=1,
                     n_iterations=7)
    assert (a['row_stride_links'], a['row_stride_contacts']) == (3*3*s.links.array.shape[3], 3*1*s.contacts.array.shape[3])

    # one step with the wave controller (per-env phase lags: an ext), without and with the next iteration's rows
    wave = SimpleNamespace(fusable=True, frequency=1.5, amplitude=torch.zeros(4), phase_lag=torch.zeros(3, 4), env_phase=torch.zeros(3))
    sim, launches = _launch_sim(monkeypatch, 1, wave, [_Recorder()])
    s, task, h = sim.task.data.sensors, sim.task, sim.task._callbacks[0].handler
    task.sim_iteration = task.iteration = 3
    want_ext = dict(size=ctypes.sizeof(_lib.CFusedExt), reserved=0, wave_frequency_env=None, wave_amplitude_env_stride=0,
                    wave_phase_lag_env_stride=4)
    plain = dict(zero, n_steps=1, iteration0=3, buffer_size=5, controller=1, units=units, substeps=1, ctrl_out=sim.physics.data.ctrl.data_ptr(),
                 wave=dict(amplitude=wave.amplitude.data_ptr(), phase_lag=wave.phase_lag.data_ptr(), env_phase=wave.env_phase.data_ptr(),
                           frequency=1.5))
    rows = dict(row_stride_links=s.links.array.stride(0), row_stride_joints=s.joints.array.stride(0), row_stride_xfrc=s.xfrc.array.stride(0),
                rows_base=dict(links=s.links.array.data_ptr(), joints=s.joints.array.data_ptr(), xfrc=s.xfrc.array.data_ptr(), contacts=None))
    sim._step_with_controller(rows_ahead=False)
    assert launches[-1] == (cdata, plain, want_ext)                        # a new struct: no rows, no strides, no water
    sim._step_with_controller(rows_ahead=True)
    ahead = dict(plain, do_readout=1, do_drag=1, rows_ahead=1, water=water([0.5, -1.0, 2.0]), **rows)
    assert launches[-1] == (cdata, ahead, want_ext)
    task.iteration = 4
    h.water.set_velocity(0.0, 0.25, 0.0)
    sim._step_with_controller(rows_ahead=False)                            # the rows and the water of the launch before: switched off
    assert launches[-1] == (cdata, dict(ahead, iteration0=4, do_readout=0, do_drag=0, rows_ahead=0), want_ext)
    h.drag = False
    sim._step_with_controller(rows_ahead=True)
    assert launches[-1] == (cdata, dict(ahead, iteration0=4, do_drag=0, water=water([0.0, 0.25, 0.0])), want_ext)
    assert sim._step_args is not None and len(launches) == 4
