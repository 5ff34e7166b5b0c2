"""Simulation builders, state transfer and output gathering that more than one GPU test file uses.  torch is imported inside the
functions, so importing this module needs no GPU."""
import numpy as np
import pytest

from support_models import random_tree


def f64(t):
    return t.cpu().numpy().astype(np.float64)


def set_state(phys, qpos, qvel, warm=None):
    """Write qpos / qvel (and the solver's warm start) as fp32; returns what the device holds, in fp64: qpos, qvel, qacc_warmstart."""
    import torch
    d = phys.data
    d.qpos[:] = torch.as_tensor(qpos, dtype=torch.float32); d.qvel[:] = torch.as_tensor(qvel, dtype=torch.float32)
    if warm is not None:
        d.qacc_warmstart[:] = torch.as_tensor(warm, dtype=torch.float32)
    return f64(d.qpos), f64(d.qvel), f64(d.qacc_warmstart)


def load_batch(sim, qpos, qvel):
    """Reset ``sim``, write the batch's initial state as fp32 and run forward with actuation disabled (the state a run starts from)."""
    import torch
    sim.reset()
    d = sim.physics.data
    d.qpos[:] = torch.as_tensor(qpos, dtype=torch.float32)
    d.qvel[:] = torch.as_tensor(qvel, dtype=torch.float32)
    sim.physics.forward(disable_actuation=True)


def swim_sim(n_envs, n_iterations, buffer_size=None, m=None, seed=0, units=None, water_kwargs=None, substeps=1, swim_substep=None,
             swimming_links=None, controller_of=None, **sim_kw):
    """A swimming Simulation on synthetic_batch(m, n_envs, seed), loaded with load_batch: returns sim, m, psi.

    An iteration is 1 ms.  ``m`` defaults to salamander33 stepping at 1 ms / substeps; a model passed in must have that timestep (the
    model steps at timestep / num_sub_steps, reference mjcf.py:1187-1192).  ``controller_of(m, psi)`` makes the controller (default:
    WaveController(m, psi)); ``swim_substep`` installs the swimming callback with its substep flag (TaskCallback(substep=...), task.py:415-420);
    ``swimming_links`` keeps drag on those links only; ``sim_kw`` (data, handle_exceptions, precision, ...) goes to Simulation."""
    from farms_mujoco_amd.model import salamander33, synthetic_batch
    from farms_mujoco_amd.options import SimulationOptions, ArenaOptions, AnimatOptions, WaterOptions
    from farms_mujoco_amd.control import WaveController
    from farms_mujoco_amd.simulation.simulation import Simulation
    from farms_mujoco_amd.units import SimulationUnitScaling
    if m is None:
        m = salamander33(timestep=1e-3/substeps)
    qpos, qvel, psi = synthetic_batch(m, n_envs, seed=seed)
    opts = SimulationOptions(timestep=1e-3, n_iterations=n_iterations, units=units or SimulationUnitScaling(), num_sub_steps=substeps)
    arena = ArenaOptions(water=WaterOptions(**(water_kwargs or {})))
    animat = AnimatOptions.from_model(m)
    if swimming_links is not None:
        for link in animat.morphology.links:
            link.swimming = link.swimming and link.name in swimming_links
    if swim_substep is not None:
        from farms_mujoco_amd.simulation.task import SwimmingCallback
        sim_kw['callbacks'] = [SwimmingCallback(animat, arena, substep=swim_substep)]
    sim = Simulation.from_sdf(opts, animat, arena, model=m, n_envs=n_envs, controller=(controller_of or WaveController)(m, psi),
                              buffer_size=buffer_size or n_iterations, **sim_kw)
    load_batch(sim, qpos, qvel)
    return sim, m, psi


def wave_at(frequency):
    """A ``controller_of`` for swim_sim: the wave controller at ``frequency`` Hz."""
    from farms_mujoco_amd.control import WaveController
    return lambda m, psi: WaveController(m, psi, frequency=frequency)


def sdf_wave(m, psi):
    """Wave controller on every position actuator of an arbitrary model (joint names are not 'joint_body_*')."""
    import torch
    from farms_mujoco_amd.control import WaveController
    c = WaveController(m, psi, frequency=1.5)
    amp = np.array([0.25 if t == 'position' else 0.0 for t in m.actuator_tags])
    lag = np.array([0.8*m.actuator_jntid[a] for a in range(m.nu)])
    c.amplitude = torch.as_tensor(amp, dtype=torch.float32, device='cuda:0')
    c.phase_lag = torch.as_tensor(lag, dtype=torch.float32, device='cuda:0')
    return c


def oracle_initial_state(oracle, sim, m, envs=slice(None)):
    """The state dict oracle.run_fused starts from: the device's fp32 qpos / qvel (of ``envs``) and the oracle's own forward pass on
    them, actuator sensors zeroed (actuation is disabled at reset)."""
    d = sim.physics.data
    st = dict(qpos=f64(d.qpos[envs]), qvel=f64(d.qvel[envs]))
    fds = [oracle.forward_debug(m, q, v) for q, v in zip(st['qpos'], st['qvel'])]
    for k in ('xpos', 'xquat', 'xipos'):
        st[k] = np.array([fd[k] for fd in fds])
    sd = np.array([fd['sensordata'] for fd in fds]); sd[:, 6*(m.nbody - 1) + 3*m.n_sensor_joints:] = 0.0
    st['sensordata'] = sd
    return st


def swim_water(sim, wave=False, envs=slice(None)):
    """What oracle.run_fused needs of the simulation's swimming handler: swim, water and, with ``wave``, the wave controller's
    parameters (env_phase of ``envs``)."""
    h = sim.task._callbacks[0].handler
    water = dict(surface=h.water._surface, velocity=h.water._velocity, viscosity=h.water._viscosity, gravity=-9.81,
                 use_buoyancy=h.buoyancy)
    if not wave:
        return h.swim_dict(), water
    c = sim.task._controller
    return h.swim_dict(), water, dict(amplitude=c.amplitude.cpu().numpy(), phase_lag=c.phase_lag.cpu().numpy(),
                                      env_phase=c.env_phase[envs].cpu().numpy(), frequency=c.frequency)


def swim_oracle(oracle, sim, m, T):
    """The oracle's fused loop (wave controller, ring of T rows) from the simulation's current state."""
    swim, water, wave = swim_water(sim, wave=True)
    return oracle.run_fused(m, oracle_initial_state(oracle, sim, m), T, swim=swim, water=water, buffer_size=T, controller=1, wave=wave,
                            n_threads=8)


def rows(sim):
    """Host copies of the ring-buffer arrays of a simulation (contacts too when it logs any)."""
    s = sim.task.data.sensors
    return {k: getattr(s, k).array.cpu().numpy() for k in ('links', 'joints', 'xfrc') + (('contacts',) if s.contacts.names else ())}


def outputs(sim, fields):
    """``fields`` of physics.data, the ring-buffer arrays and (when contacts are logged) ncon after a synchronize: all finite."""
    import torch
    torch.cuda.synchronize()
    d = sim.physics.data
    out = {k: getattr(d, k).cpu().numpy() for k in fields}
    out.update(rows(sim))
    if 'contacts' in out:
        out['ncon'] = d.ncon.cpu().numpy()
    assert all(np.isfinite(v).all() for v in out.values())
    return out


def dual2_swim(n_envs, n_iterations, ring, kernel):
    """The swimming workload of the two-env kernel's A/B tests, its context created with ``kernel`` (a KernelOptions)."""
    return swim_sim(n_envs, n_iterations, ring, water_kwargs=dict(height=-0.11, velocity=[0.03, 0.0, -0.01]), kernel=kernel)[0]      # the surface cuts the animal, a current


def dual2_finish(sim, fused=True):
    """Run a dual2_swim simulation - one fused launch, or the per-iteration host path (one-step launches with rows_ahead: the generic
    build, whose every launch sets the priority at its step 0).  Returns its outputs, the context's kernel_info after the run and, for
    the host path, the build every single launch ran."""
    launches = set()
    if fused:
        sim.run(fused=True)
    else:
        for _ in range(sim.options.n_iterations):
            sim._env_step()
            launches.add(sim.physics.kernel_info()['dual_last_launch'])
        sim.physics.check_invalid_state()
    out = outputs(sim, ('qpos', 'qvel', 'sensordata', 'xpos', 'xquat'))
    assert {'links', 'joints', 'xfrc'} <= set(out)
    assert int(sim.physics.data.status.abs().sum()) == 0
    return out, sim.physics.kernel_info(), launches


def dual2_run(n_envs, n_iterations, ring, kernel, fused=True):
    return dual2_finish(dual2_swim(n_envs, n_iterations, ring, kernel), fused)


def env_of(out, e):
    """Env ``e`` of an outputs() dict (the ring-buffer arrays carry the env in their second axis)."""
    return {k: (v[:, e] if k in ('links', 'joints', 'xfrc', 'contacts') else v[e]) for k, v in out.items()}


def assert_bitwise(a, b, what):
    for k in a:
        print(what, k, 'max abs diff', float(np.abs(a[k].astype(np.float64) - b[k].astype(np.float64)).max()))
    for k in a:
        assert np.array_equal(a[k], b[k]), (what, k)


def check_random_tree_vs_oracle(oracle, seed, threads_per_env, kernel):
    """The assertions of test_random_tree_vs_oracle on random_tree(seed), run in the kernel of ``threads_per_env`` lanes per env, which
    ``kernel`` (a KernelOptions) chooses."""
    import torch
    from farms_mujoco_amd.physics import BatchedPhysics
    m = random_tree(seed)
    if m is None or m.nv == 0:
        pytest.skip('degenerate draw')
    rng = np.random.default_rng(1000 + seed)
    n = 6
    qpos = np.tile(m.qpos0, (n, 1)) + rng.uniform(-0.4, 0.4, (n, m.nq))
    for j in range(m.njnt):
        if m.jnt_type[j] == 0:
            a = m.jnt_qposadr[j]; q = rng.normal(size=(n, 4)); qpos[:, a+3:a+7] = q/np.linalg.norm(q, axis=1, keepdims=True)
    qvel = rng.normal(size=(n, m.nv))*0.5
    ctrl = rng.uniform(-0.6, 0.6, (n, max(m.nu, 1)))[:, :m.nu]
    xf = rng.normal(size=(n, m.nbody, 6))*0.05; xf[:, 0] = 0
    qs = np.tile(m.qpos_spring, (n, 1)) + rng.uniform(-0.1, 0.1, (n, m.nq))
    phys = BatchedPhysics(m, n, kernel=kernel)
    assert phys.kernel_info()['threads_per_env'] == threads_per_env
    d = phys.data
    f32 = lambda a: torch.as_tensor(a, dtype=torch.float32)
    d.qpos[:] = f32(qpos); d.qvel[:] = f32(qvel); d.xfrc_applied[:] = f32(xf); d.qpos_spring[:] = f32(qs)
    if m.nu:
        d.ctrl[:] = f32(ctrl)
    r64 = lambda t: t.cpu().numpy().astype(np.float64)
    q32, v32, c32, x32, s32 = r64(d.qpos), r64(d.qvel), r64(d.ctrl), r64(d.xfrc_applied), r64(d.qpos_spring)
    phys.step(1)
    torch.cuda.synchronize()
    ref = oracle.step(m, q32, v32, ctrl=c32 if m.nu else None, qpos_spring=s32, xfrc_applied=x32)
    assert int(d.status.abs().sum()) == 0

    def err(k):
        a = r64(getattr(d, k)); bb = ref[k]
        return np.abs(a - bb).max()/max(np.abs(bb).max(), 1e-9)
    for k, tol in (('xpos', 5e-6), ('xquat', 5e-6), ('xipos', 5e-6), ('sensordata', 1e-4), ('qpos', 5e-6)):
        assert err(k) < tol, (seed, m.nbody, m.nv, k, err(k))
    # the velocity comes out of the (M + hB) solve: bounded by a small multiple of what fp32 storage of that matrix alone costs
    # on this tree (oracle.fp32_storage), plus the fp32 rounding of a well-conditioned solve
    with oracle.fp32_storage():
        floor = oracle.step(m, q32, v32, ctrl=c32 if m.nu else None, qpos_spring=s32, xfrc_applied=x32)
    fl = np.abs(floor['qvel'] - ref['qvel']).max()/max(np.abs(ref['qvel']).max(), 1e-9)
    assert err('qvel') < 6*fl + 2e-6, (seed, m.nbody, m.nv, 'qvel', err('qvel'), fl)
    phys.step(49)
    torch.cuda.synchronize()
    ref = oracle.step(m, q32, v32, ctrl=c32 if m.nu else None, qpos_spring=s32, xfrc_applied=x32, n_steps=50)
    assert err('qpos') < 2e-3, (seed, 'qpos50', err('qpos'))
