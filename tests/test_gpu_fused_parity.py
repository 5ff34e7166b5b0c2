"""GPU parity of the drag / readout operators and of the fused loop against the fp64 oracle."""
import numpy as np
import pytest

from parity_metrics import relerr as _relerr
from support_models import SDF, sdf_options as _options
from support_sims import (swim_sim as _make_sim, oracle_initial_state as _oracle_initial_state, swim_water as _swim_water,
                          sdf_wave as _SdfWave)

pytestmark = pytest.mark.gpu


def test_reset_forward_matches_oracle(oracle):
    sim, m, psi = _make_sim(8, 10)
    st = _oracle_initial_state(oracle, sim, m)
    d = sim.physics.data
    for k in ('xpos', 'xquat', 'xipos', 'sensordata'):
        assert _relerr(getattr(d, k).cpu().numpy(), st[k]) < 2e-6, k


@pytest.mark.parametrize('water_kwargs', [dict(height=0.0), dict(height=-0.12, velocity=[0.05, -0.02, 0.01], viscosity=1.3)])
def test_fused_loop_matches_oracle(oracle, water_kwargs):
    """200 fused iterations (readout -> drag -> glue -> wave ctrl -> mj_step): ring-buffer rows and final state
    vs the fp64 oracle.  The second case puts the surface through the animal (some links dry, partial
    buoyancy) and adds a water current."""
    import torch
    n, T = 16, 200
    sim, m, psi = _make_sim(n, T, water_kwargs=water_kwargs)
    st = _oracle_initial_state(oracle, sim, m)
    swim, water = _swim_water(sim)
    sim.run(fused=True)
    torch.cuda.synchronize()
    c = sim.task._controller
    wave = dict(amplitude=c.amplitude.cpu().numpy(), phase_lag=c.phase_lag.cpu().numpy(),
                env_phase=c.env_phase.cpu().numpy(), frequency=c.frequency)
    ref = oracle.run_fused(m, st, T, swim=swim, water=water, buffer_size=T, controller=1, wave=wave, n_threads=8)
    d = sim.physics.data
    assert int(d.status.abs().sum()) == 0
    sens = sim.task.data.sensors
    errs = dict(qpos=_relerr(d.qpos.cpu().numpy(), ref['qpos']), qvel=_relerr(d.qvel.cpu().numpy(), ref['qvel']),
                links=_relerr(sens.links.array.cpu().numpy(), ref['links']),
                joints=_relerr(sens.joints.array.cpu().numpy(), ref['joints']),
                xfrc=_relerr(sens.xfrc.array.cpu().numpy(), ref['xfrc']))
    print(errs)
    assert errs['qpos'] < 1e-4 and errs['links'] < 1e-4 and errs['joints'] < 1e-3 and errs['xfrc'] < 1e-3, errs
    # rows of links above the surface are never written (drag.pyx:192-194)
    dry = ref['links'][..., 2] > water['surface']
    assert np.all(sens.xfrc.array.cpu().numpy()[dry] == 0.0)
    if water['surface'] < 0:
        assert dry.any() and (~dry).any()


def test_fused_loop_with_network_controller(oracle):
    """The fused launch consumes the ctrl tape the device oscillator network writes; rows and state
    match the oracle stepping the oracle's own tape."""
    import torch
    from farms_mujoco_amd.control import salamander_network, NetworkController
    n, T = 8, 200
    sim, m, psi = _make_sim(n, T, buffer_size=50)
    net = salamander_network(m)
    ctl = NetworkController(m, net, n, env_phase=psi)
    sim.task._controller = ctl
    assert sim.task.fusable()
    ph0, a0, d0 = (x.cpu().numpy().astype(np.float64) for x in (ctl.phase, ctl.amp, ctl.damp))
    st = _oracle_initial_state(oracle, sim, m)
    swim, water = _swim_water(sim)
    sim.run(fused=True)
    torch.cuda.synchronize()
    tape, *_ = oracle.cpg_tape(net, T, m.timestep, ph0, a0, d0)
    ref = oracle.run_fused(m, st, T, swim=swim, water=water, buffer_size=50, controller=0, ctrl=tape,
                           ctrl_step_stride=n*m.nu, n_threads=8)
    d = sim.physics.data
    assert int(d.status.abs().sum()) == 0
    sens = sim.task.data.sensors
    errs = dict(qpos=_relerr(d.qpos.cpu().numpy(), ref['qpos']), links=_relerr(sens.links.array.cpu().numpy(), ref['links']))
    print(errs)
    assert errs['qpos'] < 1e-4 and errs['links'] < 1e-4, errs
    assert np.abs(d.qpos.cpu().numpy()[:, 7:]).max() > 0.05            # the network does bend the spine


def test_fused_equals_unfused_operators(oracle):
    """The fused launch and the per-iteration host path (round 5: one launch per iteration for a swimming model - the step's launch
    writes the next iteration's rows -, the device controller evaluated by the step's launch in both) agree to fp32 rounding of the
    drag operator: the first iteration's drag (every iteration's in the two-launch variant, fmj_before_step + step) comes from the
    standalone operator, which reads the link row back and keeps the reference's general form (two quaternions, divisions), where the
    fused loop uses the row's values in registers with precomputed reciprocals - 1e-7 per step, 8e-6 of the pose after 50 steps
    (round 4, with torch's sin() in the host path: 5e-4)."""
    import torch
    n, T = 8, 50
    sim_f, m, _ = _make_sim(n, T)
    sim_u, _, _ = _make_sim(n, T)
    sim_2, _, _ = _make_sim(n, T)
    sim_f.run(fused=True)
    sim_u.run(fused=False)
    sim_2._ahead_ok = False                      # two launches per iteration
    sim_2.run(fused=False)
    torch.cuda.synchronize()
    assert sim_f.task.iteration == sim_u.task.iteration == sim_2.task.iteration == T and sim_u._ahead_ok is True
    for other in (sim_u, sim_2):
        for k in ('qpos', 'qvel', 'xpos', 'sensordata', 'time'):
            a = getattr(sim_f.physics.data, k).cpu().numpy(); b = getattr(other.physics.data, k).cpu().numpy()
            assert _relerr(a, b) < 5e-4, (k, _relerr(a, b))
        for k in ('links', 'joints', 'xfrc'):
            a = getattr(sim_f.task.data.sensors, k).array.cpu().numpy(); b = getattr(other.task.data.sensors, k).array.cpu().numpy()
            assert _relerr(a, b) < 5e-4, (k, _relerr(a, b))


def test_ring_buffer_wraps(oracle):
    """buffer_size < n_iterations: row index = iteration % buffer_size (task.py:158); chunked fused launches."""
    import torch
    n, T, B = 4, 37, 8
    sim, m, _ = _make_sim(n, T, buffer_size=B)
    sim_full, _, _ = _make_sim(n, T, buffer_size=T)
    sim.run(fused=True); sim_full.run(fused=True)
    torch.cuda.synchronize()
    a = sim.task.data.sensors.links.array.cpu().numpy(); b = sim_full.task.data.sensors.links.array.cpu().numpy()
    for it in range(T - B, T):
        assert np.array_equal(a[it % B], b[it])
    assert torch.equal(sim.physics.data.qpos, sim_full.physics.data.qpos)


def test_drag_operator_random_rows(oracle):
    """fmj_drag on random link rows (arbitrary quaternions incl. com != urdf orientation, links above and
    below the surface, partial submersion, water current) vs drag.pyx restated in the oracle."""
    import torch, ctypes
    from farms_mujoco_amd.units import SimulationUnitScaling
    units = SimulationUnitScaling(meters=2.0, seconds=0.5, kilograms=3.0)
    sim, m, _ = _make_sim(32, 2, units=units, water_kwargs=dict(height=0.0, velocity=[0.1, 0.2, -0.05], viscosity=0.7))
    h = sim.task._callbacks[0].handler
    rng = np.random.default_rng(3)
    L = sim.task.data.sensors.links.array
    rows = rng.normal(size=tuple(L.shape[1:]))*0.3
    for c0 in (3, 10):
        q = rng.normal(size=rows.shape[:-1] + (4,)); rows[..., c0:c0+4] = q/np.linalg.norm(q, axis=-1, keepdims=True)
    rows[..., 2] = rng.uniform(-0.05, 0.02, rows.shape[:-1])     # some above, some partially submerged
    L[0] = torch.as_tensor(rows, dtype=torch.float32)
    rows32 = L[0].cpu().numpy().astype(np.float64)
    X = sim.task.data.sensors.xfrc.array
    X[0] = 7.0                                                   # sentinel: dry links must keep it
    sim.physics.data.xfrc_applied[:] = 5.0
    h.step(0)
    torch.cuda.synchronize()
    swim, water = _swim_water(sim)
    xref, xaref = oracle.drag(swim, water, rows32, np.full(tuple(X.shape[1:]), 7.0), m.nbody,
                              units=(units.newtons, units.torques))
    got = X[0].cpu().numpy()
    assert np.abs(got - xref).max() < 2e-6*max(1.0, np.abs(xref).max())
    dry = rows32[..., 2] > 0.0
    assert dry.any() and np.all(got[dry] == 7.0)
    xa = sim.physics.data.xfrc_applied.cpu().numpy()
    assert np.abs(xa[:, 1:] - xaref[:, 1:]).max() < 2e-6*max(1.0, np.abs(xaref).max())
    assert np.all(xa[:, 1:][dry] == 0.0)                         # glue zeroes rows of dry links


def test_physics2data_operator_units(oracle):
    """fmj_physics2data with non-unit scaling vs physics.py:449-524 restated in the oracle."""
    import torch
    from farms_mujoco_amd.units import SimulationUnitScaling
    from farms_mujoco_amd.simulation.physics import physics2data
    units = SimulationUnitScaling(meters=2.0, seconds=0.5, kilograms=3.0)
    sim, m, _ = _make_sim(8, 4, units=units)
    phys = sim.physics
    rng = np.random.default_rng(5)
    d = phys.data
    d.qvel[:] = torch.as_tensor(rng.normal(size=tuple(d.qvel.shape))*0.3, dtype=torch.float32)
    d.ctrl[:] = torch.as_tensor(rng.normal(size=tuple(d.ctrl.shape))*0.05, dtype=torch.float32)
    phys.step(3)
    physics2data(phys, 1, sim.task.data, sim.task.maps, units)
    torch.cuda.synchronize()
    f64 = lambda t: t.cpu().numpy().astype(np.float64)
    links, joints = oracle.physics2data(m, f64(d.qpos), f64(d.qvel), f64(d.xpos), f64(d.xquat), f64(d.xipos),
                                        f64(d.sensordata), phys.links_body, phys.joints_jnt, units=units.as_array())
    assert _relerr(sim.task.data.sensors.links.array[1].cpu().numpy(), links) < 1e-6
    assert _relerr(sim.task.data.sensors.joints.array[1].cpu().numpy(), joints) < 1e-6
    assert float(sim.task.data.sensors.links.array[0].abs().max()) == 0.0      # other ring rows untouched


def test_from_sdf_end_to_end(oracle, tmp_path):
    """Simulation.from_sdf on a real SDF file (reference simulation.py:96-124 -> setup_mjcf_xml): compile, swim 150
    fused iterations with the host-callback-free fast path, compare with the oracle."""
    import torch
    from farms_mujoco_amd.options import SimulationOptions, ArenaOptions, WaterOptions
    from farms_mujoco_amd.control import WaveController
    from farms_mujoco_amd.simulation.simulation import Simulation
    p = tmp_path/'swimmer.sdf'; p.write_text(SDF)
    ao = _options(str(p))
    n, T = 8, 150
    psi = np.linspace(0, 5, n)
    opts = SimulationOptions(timestep=1e-3, n_iterations=T)
    from farms_mujoco_amd.simulation.mjcf import setup_model
    m = setup_model(opts, ao, ArenaOptions())
    sim = Simulation.from_sdf(opts, ao, ArenaOptions(water=WaterOptions(height=0.5)), n_envs=n, buffer_size=T,
                              controller=_SdfWave(m, psi))
    sim.reset()
    m = sim.physics.model
    assert m.body_names[1] == 'swimmer' and sim.task.base_link == 'swimmer'
    st = _oracle_initial_state(oracle, sim, m)
    swim, water = _swim_water(sim)
    c = sim.task._controller
    sim.run(fused=True)
    torch.cuda.synchronize()
    ref = oracle.run_fused(m, st, T, swim=swim, water=water, buffer_size=T, controller=1,
                           wave=dict(amplitude=c.amplitude.cpu().numpy(), phase_lag=c.phase_lag.cpu().numpy(),
                                     env_phase=c.env_phase.cpu().numpy(), frequency=c.frequency))
    assert int(sim.physics.data.status.abs().sum()) == 0
    assert _relerr(sim.physics.data.qpos.cpu().numpy(), ref['qpos']) < 1e-4
    assert _relerr(sim.task.data.sensors.links.array.cpu().numpy(), ref['links']) < 2e-4
    assert _relerr(sim.task.data.sensors.xfrc.array.cpu().numpy(), ref['xfrc']) < 1e-3


@pytest.mark.parametrize('solver,cone', [('Newton', 'pyramidal'), ('Newton', 'elliptic'), ('CG', 'pyramidal')])
def test_from_sdf_on_the_ground_with_the_primal_solvers(oracle, tmp_path, solver, cone):
    """The host API end to end with the options the reference forwards to MuJoCo (mjcf.py:1342-1353): Simulation.from_sdf compiles the
    SDF with simulation_options.solver / cone, drops the animal on a flat arena and runs 200 fused iterations; state and link rows
    against the oracle stepping the same compiled model."""
    import torch
    from farms_mujoco_amd.options import SimulationOptions, ArenaOptions, WaterOptions
    from farms_mujoco_amd.simulation.simulation import Simulation
    from farms_mujoco_amd.simulation.mjcf import setup_model
    from farms_mujoco_amd.model import SOLVERS, CONES
    p = tmp_path/'swimmer.sdf'; p.write_text(SDF)
    ao = _options(str(p))
    ao.spawn.pose = [0.0, 0.0, 0.08, 0.0, 0.0, 0.0]
    for lo in ao.morphology.links:                       # the arena has friction 0 (mjcf.py:1202): a contact's friction is its link's (:1420-1422)
        lo.friction = [0.7, 0.0, 0.0]
    n, T = 6, 200
    psi = np.linspace(0, 5, n)
    opts = SimulationOptions(timestep=1e-3, n_iterations=T, solver=solver, cone=cone, n_solver_iters=100)
    arena = ArenaOptions(water=WaterOptions(height=None, drag=False), ground_height=0.0)
    m = setup_model(opts, ao, arena)
    assert m.solver == SOLVERS[solver.lower()] and m.cone == CONES[cone]
    sim = Simulation.from_sdf(opts, ao, arena, n_envs=n, buffer_size=T, controller=_SdfWave(m, psi))
    sim.reset()
    m = sim.physics.model
    st = _oracle_initial_state(oracle, sim, m)
    c = sim.task._controller
    sim.run(fused=True)
    torch.cuda.synchronize()
    ref = oracle.run_fused(m, st, T, buffer_size=T, controller=1,
                           wave=dict(amplitude=c.amplitude.cpu().numpy(), phase_lag=c.phase_lag.cpu().numpy(),
                                     env_phase=c.env_phase.cpu().numpy(), frequency=c.frequency))
    d = sim.physics.data
    assert int(d.status.abs().sum()) == 0 and int(d.ncon.max()) >= 1            # it lies on the floor
    e = np.abs(d.qpos.cpu().numpy() - ref['qpos']).max(1)
    print(solver, cone, 'from_sdf on the ground: qpos abs err per env', e)
    assert e.max() < 5e-5                                       # measured 2e-7 .. 1.3e-6
    assert _relerr(sim.task.data.sensors.links.array.cpu().numpy(), ref['links']) < 1e-3


@pytest.mark.parametrize('N', [4096, 8192])
def test_full_size_config2_properties(oracle, N):
    """BASELINE configs[1] at full size (4096 envs) and the per-GPU shard of configs[2] (8192 envs = 65536 / 8), 1000
    fused steps, ring of 100 rows: no warning bits; envs with
    identical inputs give bitwise identical rows wherever they sit in the batch (both halves of a wave, first and last
    workgroup); the second half of the batch run on its own reproduces the full run bitwise (sharding invariance,
    SURVEY 8e); a sample of envs matches the fp64 oracle to the north-star tolerance."""
    import torch
    from farms_mujoco_amd.model import salamander33, synthetic_batch
    from farms_mujoco_amd.options import SimulationOptions, ArenaOptions, AnimatOptions, WaterOptions
    from farms_mujoco_amd.control import WaveController
    from farms_mujoco_amd.simulation.simulation import Simulation
    m = salamander33()
    T, ring = 1000, 100
    qpos, qvel, psi = synthetic_batch(m, N)
    twins = [1, N//2 + 1, N - 1]                  # copies of env 0
    for e in twins:
        qpos[e] = qpos[0]; qvel[e] = qvel[0]; psi[e] = psi[0]

    def run(sl):
        n = sl.stop - sl.start
        sim = Simulation.from_sdf(SimulationOptions(timestep=m.timestep, n_iterations=T), AnimatOptions.from_model(m),
                                  ArenaOptions(water=WaterOptions(height=0.0, drag=True, buoyancy=True, viscosity=1.0)),
                                  model=m, n_envs=n, controller=WaveController(m, psi[sl]), buffer_size=ring)
        sim.reset()
        d = sim.physics.data
        d.qpos[:] = torch.as_tensor(qpos[sl], dtype=torch.float32); d.qvel[:] = torch.as_tensor(qvel[sl], dtype=torch.float32)
        sim.physics.forward(disable_actuation=True)
        st = _oracle_initial_state(oracle, sim, m) if n <= 64 else None
        sim.run(fused=True)
        torch.cuda.synchronize()
        return sim, st

    sim, _ = run(slice(0, N))
    d = sim.physics.data
    assert int(d.status.abs().sum()) == 0
    q = d.qpos.cpu().numpy(); links = sim.task.data.sensors.links.array.cpu().numpy()
    assert np.isfinite(q).all() and np.isfinite(links).all()
    for e in twins:
        assert np.array_equal(q[e], q[0]) and np.array_equal(links[:, e], links[:, 0])
    half, _ = run(slice(N//2, N))
    assert np.array_equal(half.physics.data.qpos.cpu().numpy(), q[N//2:])
    assert np.array_equal(half.task.data.sensors.links.array.cpu().numpy(), links[:, N//2:])
    # sample vs oracle: the first 8 envs stepped by the fp64 restatement from the same fp32 inputs
    small, st = run(slice(0, 8))
    assert np.array_equal(small.physics.data.qpos.cpu().numpy(), q[:8])
    swim, water = _swim_water(small)
    c = small.task._controller
    wave = dict(amplitude=c.amplitude.cpu().numpy(), phase_lag=c.phase_lag.cpu().numpy(),
                env_phase=c.env_phase.cpu().numpy(), frequency=c.frequency)
    ref = oracle.run_fused(m, st, T, swim=swim, water=water, buffer_size=ring, controller=1, wave=wave, n_threads=8)
    err = _relerr(q[:8], ref['qpos'])
    print('full-size sample qpos rel err after 1000 steps:', err)
    assert err < 1e-4, err
    assert _relerr(links[:, :8], ref['links']) < 2e-4
    # the animals did swim: forward displacement of the root along -x/+x beyond a body width
    assert np.abs(q[:, 0] - qpos[:, 0]).mean() > 0.02


@pytest.mark.parametrize('kernel', [dict(wps=3), dict(wps=4), dict(two_env=False)], ids=['wps3', 'wps4', 'one_env_per_wave'])
def test_every_step_kernel_build_matches_oracle(oracle, kernel):
    """The kernel a context uses is picked at fmj_create (batch size, model, KernelOptions): the two-env kernel in its
    168- and 128-register builds and the one-env kernel all reproduce the oracle on the same fused
    workload (odd batch: the last wave of the two-env kernels has an idle half)."""
    import torch
    from farms_mujoco_amd.options import KernelOptions
    n, T = 7, 120
    sim, m, psi = _make_sim(n, T, buffer_size=40, water_kwargs=dict(height=-0.11, velocity=[0.03, 0.0, -0.01]), kernel=KernelOptions(**kernel))
    info = sim.physics.kernel_info()
    assert info['threads_per_env'] == (32 if kernel.get('two_env', True) else 64)
    assert info.get('dual_wps') == kernel.get('wps')      # the tier asked for; the one-env kernel has none
    st = _oracle_initial_state(oracle, sim, m)
    swim, water = _swim_water(sim)
    sim.run(fused=True)
    torch.cuda.synchronize()
    c = sim.task._controller
    wave = dict(amplitude=c.amplitude.cpu().numpy(), phase_lag=c.phase_lag.cpu().numpy(),
                env_phase=c.env_phase.cpu().numpy(), frequency=c.frequency)
    ref = oracle.run_fused(m, st, T, swim=swim, water=water, buffer_size=40, controller=1, wave=wave, n_threads=8)
    d = sim.physics.data
    assert int(d.status.abs().sum()) == 0
    sens = sim.task.data.sensors
    errs = dict(qpos=_relerr(d.qpos.cpu().numpy(), ref['qpos']), links=_relerr(sens.links.array.cpu().numpy(), ref['links']),
                joints=_relerr(sens.joints.array.cpu().numpy(), ref['joints']), xfrc=_relerr(sens.xfrc.array.cpu().numpy(), ref['xfrc']),
                sensordata=_relerr(d.sensordata.cpu().numpy(), ref['sensordata']))
    print(kernel, errs)
    # link rows carry velocities: 0.8e-4 (two-env builds) to 1.1e-4 (one-env build) after 120 steps, fp32 rounding of
    # differently scheduled but identical arithmetic; the state itself is at 6e-6
    assert errs['qpos'] < 1e-4 and errs['links'] < 2e-4 and errs['joints'] < 1e-3 and errs['xfrc'] < 1e-3 and errs['sensordata'] < 2e-3, errs


@pytest.mark.parametrize('substeps,sub_links', [(2, False), (2, True), (3, True), (5, False), (5, True)])
def test_fused_substeps_match_oracle(oracle, substeps, sub_links):
    """num_sub_steps > 1 inside the fused launch (round 4; reference task.py:168-186,348-369, mjcf.py:1187-1192): full steps write
    full rows, run the drag and the controller; sub-steps keep the ctrl and - unless the swimming callback asked for sub-steps -
    the drag force; with sub-step callbacks they write links-only rows at the ring index of the reference's own (early)
    iteration counter.  Checked against the oracle's run_fused, whose loop restates ExperimentTask's counters literally."""
    import torch
    n, T = 4, 24
    sim, m, psi = _make_sim(n, T, substeps=substeps, swim_substep=sub_links)
    assert sim.task.fusable() and sim.task.substeps == substeps and sim.task.substeps_links == sub_links
    st = _oracle_initial_state(oracle, sim, m)
    swim, water = _swim_water(sim)
    c = sim.task._controller
    ref = oracle.run_fused(m, st, T, swim=swim, water=water, buffer_size=T, controller=1, substeps=substeps, substep_links=sub_links, n_iterations=T,
                           wave=dict(amplitude=c.amplitude.cpu().numpy(), phase_lag=c.phase_lag.cpu().numpy(),
                                     env_phase=c.env_phase.cpu().numpy(), frequency=c.frequency))
    sim.run(fused=True)
    torch.cuda.synchronize()
    assert sim.task.sim_iteration == T*substeps and sim.task.iteration == T
    d = sim.physics.data
    assert int(d.status.abs().sum()) == 0
    assert abs(float(d.time[0]) - T*1e-3) < 1e-6
    errs = {k: _relerr(getattr(d, k).cpu().numpy(), ref[k]) for k in ('qpos', 'qvel', 'xpos')}
    for k in ('links', 'joints', 'xfrc'):
        errs[k] = _relerr(getattr(sim.task.data.sensors, k).array.cpu().numpy(), ref[k])
    print(substeps, sub_links, errs)
    assert errs['qpos'] < 1e-5 and errs['xpos'] < 1e-5 and errs['links'] < 1e-4 and errs['joints'] < 1e-3 and errs['xfrc'] < 1e-3 and errs['qvel'] < 2e-3, errs
    # the quirk is really there: with sub-step rows and S >= 3 the links of row m are those sub-step 1 saw, not the full step's
    if sub_links and substeps >= 3:
        ref_nolinks = oracle.run_fused(m, st, T, swim=swim, water=water, buffer_size=T, controller=1, substeps=substeps, substep_links=False,
                                       wave=dict(amplitude=c.amplitude.cpu().numpy(), phase_lag=c.phase_lag.cpu().numpy(),
                                                 env_phase=c.env_phase.cpu().numpy(), frequency=c.frequency))
        assert _relerr(ref['links'][5], ref_nolinks['links'][5]) > 1e-6


@pytest.mark.parametrize('substeps', [1, 2, 5])
def test_fused_equals_unfused_with_substeps(oracle, substeps):
    """The fused launch against ExperimentTask.before_step / after_step driven from the host, one launch per operator and physics
    step (the path of callers with host callbacks): same rows, same state (the only arithmetic difference is sin() by torch
    against the in-kernel sine of the wave controller)."""
    import torch
    n, T = 4, 12
    for sub_links in ((False,) if substeps == 1 else (False, True)):
        sim_f, m, _ = _make_sim(n, T, substeps=substeps, swim_substep=sub_links)
        sim_u, _, _ = _make_sim(n, T, substeps=substeps, swim_substep=sub_links)
        sim_f.run(fused=True)
        sim_u.run(fused=False)
        torch.cuda.synchronize()
        assert sim_f.task.sim_iteration == sim_u.task.sim_iteration == T*substeps
        assert sim_f.task.iteration == T and sim_u.task.iteration in (T, T - 1 + (substeps == 1) + (substeps > 1))
        for k in ('qpos', 'qvel', 'xpos', 'sensordata'):
            a = getattr(sim_f.physics.data, k).cpu().numpy(); b = getattr(sim_u.physics.data, k).cpu().numpy()
            assert _relerr(a, b) < 5e-4, (substeps, sub_links, k, _relerr(a, b))
        # every row, row 0 included: the sub-steps of the last iteration whose task.iteration has reached n_iterations (the reference never
        # executes them: its assert at task.py:170) write nothing, so the ring index n_iterations % buffer_size = 0 keeps the first
        # full step's row (include/fmj.h: fmj_fused_args::n_iterations)
        for k in ('links', 'joints', 'xfrc'):
            a = getattr(sim_f.task.data.sensors, k).array.cpu().numpy(); b = getattr(sim_u.task.data.sensors, k).array.cpu().numpy()
            assert _relerr(a, b) < 5e-4, (substeps, sub_links, k, _relerr(a, b))
            assert _relerr(a[0], b[0]) < 5e-4 and np.abs(a[0]).max() > 0
        if sub_links and substeps > 1:      # ... and that row 0 is the FIRST iteration's: its joints row was written once, by the first full step
            q0 = sim_f.task.data.sensors.joints.array[0].cpu().numpy()[..., 0]
            qT = sim_f.physics.data.qpos.cpu().numpy()[:, 7:]
            assert np.abs(q0 - qT).max() > 1e-3


def test_fused_substeps_chunked_equals_one_launch(oracle):
    """Sub-steps across launch boundaries: a run chunked by a short ring buffer is bitwise the run of one launch (state) and holds
    the same rows in its ring."""
    import torch
    n, T, B, S = 4, 23, 6, 3
    sim, m, _ = _make_sim(n, T, buffer_size=B, substeps=S, swim_substep=True)
    sim_full, _, _ = _make_sim(n, T, buffer_size=T, substeps=S, swim_substep=True)
    sim.run(fused=True); sim_full.run(fused=True)
    torch.cuda.synchronize()
    assert torch.equal(sim.physics.data.qpos, sim_full.physics.data.qpos) and torch.equal(sim.physics.data.qvel, sim_full.physics.data.qvel)
    a = sim.task.data.sensors.links.array.cpu().numpy(); b = sim_full.task.data.sensors.links.array.cpu().numpy()
    aj = sim.task.data.sensors.joints.array.cpu().numpy(); bj = sim_full.task.data.sensors.joints.array.cpu().numpy()
    for it in range(T - B + 1, T):
        assert np.array_equal(a[it % B], b[it]), it
        # the motor-torque column of the first row of a launch is summed from the stored actuator forces (library sine on the last step)
        # instead of the in-loop carry (kp (ctrl - q) with the two sines a few 1e-8 apart): equal to ~1e-7 of the command, not bitwise
        assert np.allclose(aj[it % B], bj[it], rtol=1e-5, atol=2e-7), (it, np.abs(aj[it % B] - bj[it]).max())
