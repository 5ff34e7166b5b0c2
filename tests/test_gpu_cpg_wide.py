"""The device oscillator network past one wave (include/fmj.h: FMJ_CPG_MAX_OSC; one workgroup of 64 ceil(n_osc / 64) threads per
env): tapes against the numpy restatement of the oracle (tests/support_cpg.py: the oracle itself stops at 64 oscillators) at sizes on
both sides of every wave boundary, the bitwise promises (disconnected copies, chunking, per-env parameters) across waves, and the
long swimmers driven through the API on the two-wave and the fp64 fused step kernels."""
import numpy as np
import pytest

from parity_metrics import group_relerr, qpos_groups, link_row_groups
from support_cpg import cpg_reference, replicate, ring_network, position_model, wrapped, tape_and_state
from support_sims import swim_sim, swim_water, oracle_initial_state, f64

pytestmark = pytest.mark.gpu

T = 500
TAPE_TOL, AMP_TOL, PHASE_TOL = 2e-4, 1e-5, 2e-4      # tests/test_cpg_network.py::test_hip_tape_matches_oracle


def _model(name):
    import farms_mujoco_amd.model as mm
    return {'centipede': mm.centipede, 'eel48': lambda: mm.eel(48), 'centipede_20_25': lambda: mm.centipede(20, 25)}[name]()


def _check_against_reference(what, c, net, h, drive):
    """T steps of controller ``c`` against cpg_reference from the device's initial state; the fp32 emulation's error printed beside.

    The bounds are the project's for this kernel.  They carry over where fp32 itself can meet them: the error is per oscillator and the
    in-degree is at most 4 in every network here (the emulation shows tape 3e-6 .. 9e-5 and phase 9e-6 .. 7e-5 up to 193 oscillators;
    the salamander case the bounds were set on: 5e-6 / 2.4e-5).  Where the emulation on the same inputs misses a bound, no fp32
    evaluation of these equations can be held to it, and the bound is 4 x the emulation's error instead.  That is the ring of 256 from
    random phases alone: after 500 steps it still holds neighbours 2.9 rad apart, where the coupling drives them further apart and a
    rounding error grows exponentially (the emulation's phase error is 1.4e-5 after 250 steps and 2.68e-4 after 500; from a start near
    the lock 2e-6).  The device: phase 2.52e-4, tape 8.6e-5 (emulation 8.5e-5; within the project's 2e-4)."""
    start = [f64(x) for x in (c.phase, c.amp, c.damp)]
    got = tape_and_state(c, T)
    ref = cpg_reference(net, T, h, *start, drive=drive.astype(np.float32))
    emu = cpg_reference(net, T, h, *start, drive=drive.astype(np.float32), dtype=np.float32)
    errs = {}
    for k, r, e in zip(('tape', 'phase', 'amp', 'damp'), ref, emu):
        d = (lambda x: wrapped(x)) if k == 'phase' else (lambda x: x)
        errs[k] = (np.abs(d(got[k] - r)).max(), np.abs(d(e - r)).max())
        print(what, k, 'device error %.3g   fp32 emulation error %.3g' % errs[k])
    assert np.abs(ref[0]).max() > 0.1
    for k, tol in (('tape', TAPE_TOL), ('amp', AMP_TOL), ('phase', PHASE_TOL)):
        device, emulation = errs[k]
        if emulation >= tol:
            print(what, k, f'the fp32 emulation misses {tol:g}: bound {4*emulation:.3g}')
            tol = 4*emulation
        assert device < tol, (what, k, device, emulation, tol)


@pytest.mark.parametrize('name,n_osc', [('centipede', 70), ('eel48', 96), ('centipede_20_25', 130)])
def test_tape_of_a_long_swimmer_matches_the_reference(name, n_osc):
    from farms_mujoco_amd.control import NetworkController, axial_limb_network
    from farms_mujoco_amd.model import synthetic_batch
    m = _model(name)
    net = axial_limb_network(m)
    assert net.n_osc == n_osc
    n = 8
    _, _, psi = synthetic_batch(m, n)
    drive = 1.0 + 0.1*np.arange(n)/n
    _check_against_reference(name, NetworkController(m, net, n, env_phase=psi, drive=drive), net, m.timestep, drive)


@pytest.mark.parametrize('n_osc', [64, 65, 128, 129, 192, 193, 256])
def test_tape_of_a_ring_matches_the_reference(n_osc):
    """Sizes on both sides of every block size; nu = 2 n_osc + 7 outputs: more than the block has threads."""
    import torch
    from farms_mujoco_amd.control import NetworkController
    nu, n = 2*n_osc + 7, 4
    net = ring_network(n_osc, nu)
    m = position_model(nu)
    drive = 1.0 + 0.1*np.arange(n)/n
    c = NetworkController(m, net, n, drive=drive)
    rng = np.random.default_rng(n_osc)
    c.phase[:] = torch.as_tensor(rng.uniform(-np.pi, np.pi, (n, n_osc)), dtype=torch.float32)
    c.amp[:] = 0.15
    _check_against_reference(f'ring {n_osc}', c, net, m.timestep, drive)


@pytest.mark.parametrize('k', [3, 8])
def test_disconnected_copies_are_bitwise_the_single_network(k):
    """k copies of the 30-oscillator salamander network in one network of 90 (a copy straddles the first wave boundary) and 240
    oscillators: every copy's tape and state equal the single network's, which runs on one wave."""
    import torch
    from farms_mujoco_amd.control import NetworkController, salamander_network
    from farms_mujoco_amd.model import salamander33, synthetic_batch
    m = salamander33()
    net = salamander_network(m)
    big = replicate(net, k)
    assert big.n_osc == 30*k and big.nu == k*m.nu and big.n_conn == k*net.n_conn
    n = 5
    _, _, psi = synthetic_batch(m, n)
    drive = 1.0 + 0.1*np.arange(n)/n
    one = NetworkController(m, net, n, env_phase=psi, drive=drive)
    rng = np.random.default_rng(1)
    one.amp[:] = torch.as_tensor(rng.uniform(0.0, 0.2, (n, 30)), dtype=torch.float32)
    one.damp[:] = torch.as_tensor(rng.uniform(-0.1, 0.1, (n, 30)), dtype=torch.float32)
    many = NetworkController(position_model(big.nu, m.timestep), big, n, drive=drive)
    for key in ('phase', 'amp', 'damp'):
        getattr(many, key)[:] = getattr(one, key).repeat(1, k)
    want, got = tape_and_state(one, T), tape_and_state(many, T)
    assert np.abs(want['tape']).max() > 0.1
    for c in range(k):
        assert np.array_equal(got['tape'][:, :, c*m.nu:(c + 1)*m.nu], want['tape']), c
        for key in ('phase', 'amp', 'damp'):
            assert np.array_equal(got[key][:, 30*c:30*(c + 1)], want[key]), (c, key)


def test_chunking_is_bitwise_at_130_oscillators():
    import torch
    from farms_mujoco_amd.control import NetworkController, axial_limb_network
    from farms_mujoco_amd.model import synthetic_batch
    m = _model('centipede_20_25')
    net = axial_limb_network(m)
    n = 4
    _, _, psi = synthetic_batch(m, n)
    whole = tape_and_state(NetworkController(m, net, n, env_phase=psi), T)
    c = NetworkController(m, net, n, env_phase=psi)
    first = c.ctrl_tape(T//2).clone()
    halves = tape_and_state(c, T - T//2)
    halves['tape'] = np.concatenate([first.cpu().numpy(), halves['tape']])
    assert np.abs(whole['tape'][-1]).max() > 0.1
    for key in whole:
        assert np.array_equal(whole[key], halves[key]), key


def test_per_env_parameters_at_130_oscillators():
    """include/fmj.h, fmj_cpg_tape_ex: env e of a per-env launch equals, bit for bit, a one-env network created from e's values -
    with the connections shuffled, so that the descriptor's order is not the library's."""
    from farms_mujoco_amd.control import NetworkController, OscillatorNetwork, axial_limb_network
    from farms_mujoco_amd.model import synthetic_batch
    m = _model('centipede_20_25')
    base = axial_limb_network(m)
    order = np.random.default_rng(5).permutation(base.n_conn)
    con = np.c_[base.conn_to, base.conn_from, base.conn_weight, base.conn_bias][order]
    out = np.c_[base.out_a, base.out_b, base.out_gain, base.out_offset]
    net = OscillatorNetwork(base.frequency, base.rate, base.amplitude, con, out, initial_phase=base.initial_phase)
    assert net.n_osc == 130
    n, steps = 2, 100
    _, _, psi = synthetic_batch(m, n)
    rng = np.random.default_rng(6)
    f32 = lambda x: x.astype(np.float32).astype(np.float64)      # exact in fp32, so that a network created from a row rounds to the same
    P = dict(frequency=rng.uniform(0.5, 2.0, (n, net.n_osc)), conn_weight=f32(rng.uniform(10.0, 40.0, (n, net.n_conn))),
             conn_bias=f32(net.conn_bias[None] + rng.uniform(-0.3, 0.3, (n, net.n_conn))),
             out_gain=f32(net.out_gain[None]*rng.uniform(0.5, 1.5, (n, net.nu))))
    got = tape_and_state(NetworkController(m, net, n, env_phase=psi, env_params=P), steps)
    assert np.abs(got['tape'][:, 0] - got['tape'][:, 1]).max() > 1e-3
    for e in range(n):
        con_e = np.c_[net.conn_to, net.conn_from, P['conn_weight'][e], P['conn_bias'][e]]
        out_e = np.c_[net.out_a, net.out_b, P['out_gain'][e], net.out_offset]
        net_e = OscillatorNetwork(P['frequency'][e], net.rate, net.amplitude, con_e, out_e, initial_phase=net.initial_phase)
        one = tape_and_state(NetworkController(m, net_e, 1, env_phase=psi[e:e + 1]), steps)
        assert np.array_equal(got['tape'][:, e:e + 1], one['tape']), e
        for key in ('phase', 'amp', 'damp'):
            assert np.array_equal(got[key][e:e + 1], one[key]), (e, key)


class _Twins:
    """``controller_of`` for swim_sim: NetworkController(axial_limb_network(m)) with the amplitudes at their targets, so that the body
    bends within a short run.  ``twin()`` makes the same controller again: its tape is what the simulation's controller hands the step."""

    def __init__(self, n):
        self.n = n

    def __call__(self, m, psi):
        import torch
        from farms_mujoco_amd.control import NetworkController, axial_limb_network
        self.args = (m, psi)
        net = axial_limb_network(m)
        c = NetworkController(m, net, self.n, env_phase=psi)
        c.amp[:] = torch.as_tensor(net.amplitude, dtype=torch.float32)
        return c

    def twin(self):
        return self(*self.args)


def test_network_drives_the_two_wave_kernel_through_the_api(oracle):
    """Simulation.run(fused=True) on centipede(20, 25) under its 130-oscillator network: the step alone against the oracle's fused loop
    fed the device tape of a twin controller, at the bound of tests/test_gpu_wide_models.py::test_fused_swim_of_a_wide_centipede."""
    import torch
    m = _model('centipede_20_25')
    n, steps = 4, 40
    twins = _Twins(n)
    sim = swim_sim(n, steps, m=m, seed=9, controller_of=twins)[0]
    assert sim.task.fusable() and sim.physics.kernel_info()['threads_per_env'] == 128
    twin = twins.twin()
    tape = f64(twin.ctrl_tape(steps))
    swim, water = swim_water(sim)
    kw = dict(swim=swim, water=water, buffer_size=steps, controller=0, ctrl=tape, ctrl_step_stride=n*m.nu, n_threads=8)
    st = oracle_initial_state(oracle, sim, m)
    ref = oracle.run_fused(m, st, steps, **kw)
    with oracle.fp32_storage():
        flo = oracle.run_fused(m, st, steps, **kw)
    sim.run(fused=True)
    torch.cuda.synchronize()
    assert int(sim.physics.data.status.abs().sum()) == 0
    assert torch.equal(sim.task._controller.phase, twin.phase)      # the simulation's controller advanced as its twin did
    sens = sim.task.data.sensors
    got = dict(qpos=sim.physics.data.qpos.cpu().numpy(), links=sens.links.array.cpu().numpy(), xfrc=sens.xfrc.array.cpu().numpy())
    assert np.abs(got['qpos'][:, 7:]).max() > 0.02
    groups = dict(qpos=qpos_groups(m), links=link_row_groups(), xfrc=[slice(0, 3), slice(3, 6)])
    for k in got:
        err = group_relerr(got[k], ref[k], groups[k]); fl = group_relerr(flo[k], ref[k], groups[k])
        print('centipede(20, 25) under its network', k, 'per-component err', err, 'fp32-storage floor', fl)
        assert err < 6*fl + 1e-6, (k, err, fl)


def test_network_drives_the_fp64_fused_step_through_the_api(oracle):
    """The same on eel(48) with precision='fp64', fp64_fused=True, with the helpers and bounds of the ctrl-tape case of
    tests/test_gpu_f64_fused.py (test_ctrl_tape_one_row_per_iteration)."""
    import support_f64_fused as F
    n, steps = 4, 40
    twins = _Twins(n)
    sim = F._sim('eel48', n, steps, controller_of=twins)
    m = sim.physics.model
    assert sim.physics.precision == 'fp64' and sim.physics.fp64_fused and sim.task.fusable()
    tape = twins.twin().ctrl_tape(steps)
    swim, water = swim_water(sim)
    water = dict(water, surface=float(np.float32(water['surface'])), velocity=F._f32(water['velocity']), viscosity=float(np.float32(water['viscosity'])),
                 gravity=float(np.float32(water['gravity'])))      # as the device holds them (_oracle_args of that file)
    st = F._device_state(sim)
    kw = dict(swim=swim, water=water, controller=0, ctrl=f64(tape), ctrl_step_stride=n*m.nu, n_threads=8, n_iterations=steps, units=F._units(sim))
    ref = oracle.run_fused(m, st, steps, buffer_size=steps, **kw)
    with oracle.fp32_storage():
        fst = oracle.run_fused(m, st, steps, buffer_size=steps, **kw)
    fl, ring = st, {r: np.zeros_like(ref[r]) for r in F.RING}      # floor_state: a launch per iteration reads its own row of the tape
    for k in range(steps):
        o = oracle.run_fused(m, fl, 1, iteration0=k, buffer_size=steps, **dict(kw, ctrl=f64(tape[k:k + 1])))
        for r in F.RING:
            ring[r][k] = o[r][k]
        fl = {s: F._f32(o[s]) for s in F.STATE}
    sim.run()
    got = F._got(sim)
    assert not got['status'].any() and sim.task.sim_iteration == steps
    assert np.abs(got['qpos'][:, 7:]).max() > 0.02
    F._check_run(got, ref, dict(fl, **ring), fst, 'eel48 under its network')
