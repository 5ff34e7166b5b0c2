"""Oscillator networks past one wave (include/fmj.h: FMJ_CPG_MAX_OSC): a numpy checker for any size, and network shapes that put
oscillators on every wave boundary.  The oracle's fmjo_cpg_tape stops at 64 oscillators; ``cpg_reference`` restates it without the
limit and tests/test_cpg_wide_interface.py pins the two together where the oracle works.  No GPU is needed to import this."""
import types

import numpy as np


def cpg_reference(net, T, h, phase, amp, damp, drive=None, dtype=np.float64):
    """fmjo_cpg_tape (oracle/fmj_oracle.c) over all envs at once: returns (tape[T, n_envs, nu], phase, amp, damp) after T steps.
    The tape holds the output of the state before each step; an oscillator's incoming connections are added in the order of the
    connection list; the phase wraps only where it exceeds pi.  ``dtype=np.float32`` computes everything in fp32 with the device's
    roundings of the parameters (2 pi f rounded once, then scaled by the drive): an emulation of the kernel's precision up to its
    fused multiply-adds and the device's sin / cos, for reporting what fp32 can give - never a reference."""
    f = np.dtype(dtype).type
    th, r, rd = (np.array(x, dtype=f).reshape(len(phase), net.n_osc) for x in (phase, amp, damp))
    n = th.shape[0]
    dr = np.ones(n, f) if drive is None else np.asarray(drive).astype(f)
    omega = (2*np.pi*net.frequency).astype(f)[None, :]*dr[:, None]
    a, R = net.rate.astype(f), net.amplitude.astype(f)
    w, phi = net.conn_weight.astype(f), net.conn_bias.astype(f)
    to, fr = net.conn_to, net.conn_from
    # round k holds every oscillator's k-th incoming connection: targets within a round are distinct, so `+=` on them is well defined
    seen = np.zeros(net.n_osc, int)
    rank = np.zeros(net.n_conn, int)
    for k in range(net.n_conn):
        rank[k] = seen[to[k]]; seen[to[k]] += 1
    rounds = [np.nonzero(rank == k)[0] for k in range(int(rank.max()) + 1 if net.n_conn else 0)]
    gain, offset = net.out_gain.astype(f), net.out_offset.astype(f)
    ia, ib = np.maximum(net.out_a, 0), np.maximum(net.out_b, 0)
    ga, gb = gain*(net.out_a >= 0), gain*(net.out_b >= 0)
    tape = np.zeros((T, n, net.nu), f)
    h, pi, quarter = f(h), f(np.pi), f(0.25)
    for s in range(T):
        c = f(1) + np.cos(th)
        tape[s] = offset + ga*r[:, ia]*c[:, ia] - gb*r[:, ib]*c[:, ib]
        dth = omega.copy()
        for idx in rounds:
            dth[:, to[idx]] += r[:, fr[idx]]*w[idx]*np.sin(th[:, fr[idx]] - th[:, to[idx]] - phi[idx])
        rdd = a*(quarter*a*(R - r) - rd)
        nth = th + h*dth
        r = r + h*rd
        rd = rd + h*rdd
        th = np.where(nth > pi, nth - f(2)*pi, nth)
    assert tape.dtype == th.dtype == r.dtype == rd.dtype == np.dtype(dtype)
    return tape, th, r, rd


def _rows(net):
    return (np.c_[net.conn_to, net.conn_from, net.conn_weight, net.conn_bias],
            np.c_[net.out_a, net.out_b, net.out_gain, net.out_offset])


def replicate(net, k):
    """``k`` disconnected copies of ``net``: copy c owns oscillators [c n_osc, (c + 1) n_osc) and outputs [c nu, (c + 1) nu); its
    connections keep their order."""
    from farms_mujoco_amd.control import OscillatorNetwork
    con, out = _rows(net)
    cons, outs = [], []
    for c in range(k):
        cc = con.copy(); cc[:, :2] += c*net.n_osc
        oo = out.copy()
        for col, idx in ((0, net.out_a), (1, net.out_b)):
            oo[:, col] = np.where(idx >= 0, idx + c*net.n_osc, -1)
        cons.append(cc); outs.append(oo)
    ph = None if net.initial_phase is None else np.tile(net.initial_phase, k)
    return OscillatorNetwork(np.tile(net.frequency, k), np.tile(net.rate, k), np.tile(net.amplitude, k), np.concatenate(cons), np.concatenate(outs),
                             initial_phase=ph)


def ring_network(n_osc, nu):
    """A ring of any size: oscillator i is coupled from i - 1 (bias 2 pi / n_osc: it lags its predecessor) and from i + 1 (the opposite
    bias), weight 30; output u is single-sided from oscillator u % n_osc with gain 1 + 0.01 u."""
    from farms_mujoco_amd.control import OscillatorNetwork
    bias = 2*np.pi/n_osc
    con = [x for i in range(n_osc) for x in ((i, (i - 1) % n_osc, 30.0, bias), (i, (i + 1) % n_osc, 30.0, -bias))]
    out = [(u % n_osc, -1, 1.0 + 0.01*u, 0.0) for u in range(nu)]
    return OscillatorNetwork(np.full(n_osc, 1.0), np.full(n_osc, 20.0), np.full(n_osc, 0.15), con, out)


def position_model(nu, timestep=1e-3):
    """What NetworkController reads of a model, for a network that belongs to none: ``nu`` position actuators."""
    return types.SimpleNamespace(nu=nu, timestep=timestep, joint_names=['joint'], actuator_jntid=np.zeros(nu, np.int32),
                                 actuator_tags=['position']*nu)


def wrapped(dphi):
    return (np.asarray(dphi) + np.pi) % (2*np.pi) - np.pi


def tape_and_state(controller, n_steps):
    """The tape of the next ``n_steps`` and the oscillator state after them, on the host."""
    import torch
    tape = controller.ctrl_tape(n_steps).clone()
    torch.cuda.synchronize()
    return dict(tape=tape.cpu().numpy(), **{k: getattr(controller, k).cpu().numpy() for k in ('phase', 'amp', 'damp')})
