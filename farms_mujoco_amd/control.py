"""Controller interface stand-ins (farms_core.model.control is not in the reference tree).

The reference's ExperimentTask calls ``controller.step/positions/torques/springrefs`` and reads
``controller.joints_names[ControlType.*]`` every control step (reference task.py:229-252,292-346).
Here the same interface returns batched device tensors instead of per-joint dicts.
"""
import ctypes
import enum
import math

import numpy as np
import torch

from . import _lib
from .model import wave_controller_params


class ControlType(enum.IntEnum):
    POSITION = 0
    VELOCITY = 1
    TORQUE = 2


class AnimatController:
    """Base: subclasses return ``[n_envs, n_joints_of_that_type]`` tensors ordered like ``joints_names``."""

    def __init__(self, joints_names=None, muscles_names=None):
        self.joints_names = joints_names or {ControlType.POSITION: [], ControlType.VELOCITY: [], ControlType.TORQUE: []}
        self.muscles_names = muscles_names or []

    def step(self, iteration, time, timestep):
        """Advance the controller state (called once per control step, task.py:292-296)."""

    def positions(self, iteration, time, timestep):
        raise NotImplementedError

    def torques(self, iteration, time, timestep):
        raise NotImplementedError

    def springrefs(self, iteration, time, timestep):
        return None


class WaveController(AnimatController):
    """Travelling-wave position controller of the benchmark configs:
    ``ctrl_j(t, e) = A_j sin(2 pi f t - phi_j + psi_e)``.  ``fusable``: the fused HIP loop evaluates the
    same expression on the device (include/fmj.h: fmj_wave_controller), so no per-step host work remains.

    Every env may swim its own gait (a parameter sweep; include/fmj.h: fmj_fused_ext): ``frequency`` is a scalar or ``[n_envs]``,
    and the keyword-only ``amplitude_env`` / ``phase_lag_env`` = ``[n_envs, nu]`` in actuator order replace the rows that
    ``amplitude`` / ``n_wave`` describe (entries of non-position actuators must be 0, as ``wave_controller_params`` leaves them).
    The attributes carry the shapes: ``frequency`` a float or a tensor ``[n_envs]``, ``amplitude`` / ``phase_lag`` ``[nu]`` or
    ``[n_envs, nu]``."""
    fusable = True

    def __init__(self, model, env_phase, frequency=1.0, amplitude=0.3, n_wave=1.0, device='cuda:0', *, amplitude_env=None,
                 phase_lag_env=None):
        names = [model.joint_names[model.actuator_jntid[a]] for a in range(model.nu)
                 if model.actuator_tags[a] == 'position']
        super().__init__({ControlType.POSITION: names, ControlType.VELOCITY: [], ControlType.TORQUE: []})
        amp, lag = wave_controller_params(model, amplitude, n_wave)
        env_phase = np.asarray(env_phase)
        if env_phase.ndim != 1:
            raise ValueError(f'env_phase: expected shape [n_envs], not {env_phase.shape}')
        n_envs, nu = len(env_phase), model.nu
        if np.ndim(frequency) == 0:
            self.frequency = float(frequency)
        else:
            if np.shape(frequency) != (n_envs,):
                raise ValueError(f'frequency: expected a scalar or shape [n_envs] = ({n_envs},), not {np.shape(frequency)}')
            self.frequency = torch.as_tensor(np.asarray(frequency), dtype=torch.float32, device=device).contiguous()      # [n_envs]
        other = np.array([t != 'position' for t in model.actuator_tags[:nu]], bool)
        for name, rows in (('amplitude_env', amplitude_env), ('phase_lag_env', phase_lag_env)):
            if rows is None:
                continue
            rows = np.asarray(rows, np.float64)
            if rows.shape != (n_envs, nu):
                raise ValueError(f'{name}: expected shape [n_envs, nu] = ({n_envs}, {nu}), not {rows.shape}')
            if np.any(rows[:, other] != 0):
                raise ValueError(f'{name}: entries of non-position actuators must be 0')
            if name == 'amplitude_env':
                amp = rows
            else:
                lag = rows
        self.amplitude = torch.as_tensor(amp, dtype=torch.float32, device=device).contiguous()      # [nu] or [n_envs, nu]
        self.phase_lag = torch.as_tensor(lag, dtype=torch.float32, device=device).contiguous()      # [nu] or [n_envs, nu]
        self.env_phase = torch.as_tensor(env_phase, dtype=torch.float32, device=device)  # [n_envs]
        self._pos_idx = torch.as_tensor([a for a in range(model.nu) if model.actuator_tags[a] == 'position'],
                                        device=device)

    def positions(self, iteration, time, timestep):
        if torch.is_tensor(self.frequency):      # the env's own clock, in fp64 like the device's (fmj_stage_q.inc)
            cyc = torch.remainder(self.frequency.to(torch.float64)*time, 1.0)
            turn = (2*math.pi*cyc).to(torch.float32)[:, None]
        else:
            cyc = (self.frequency*time) % 1.0
            turn = (2*math.pi*cyc)
        rows = lambda t: t[:, self._pos_idx] if t.dim() == 2 else t[None, self._pos_idx]
        arg = turn + self.env_phase[:, None] - rows(self.phase_lag)
        return rows(self.amplitude)*torch.sin(arg)


class OscillatorNetwork:
    """Host description of a network of amplitude-controlled phase oscillators (include/fmj.h: fmj_cpg_desc).
    ``connections`` = rows (to, from, weight, phase_bias); ``outputs`` = per actuator (osc_a, osc_b, gain, offset),
    ``ctrl_u = gain (r_a (1 + cos theta_a) - r_b (1 + cos theta_b)) + offset``."""

    def __init__(self, frequency, rate, amplitude, connections, outputs, initial_phase=None):
        self.initial_phase = None if initial_phase is None else np.ascontiguousarray(initial_phase, np.float64)
        self.frequency = np.ascontiguousarray(frequency, np.float64)
        self.rate = np.ascontiguousarray(rate, np.float64)
        self.amplitude = np.ascontiguousarray(amplitude, np.float64)
        con = np.asarray(connections, np.float64).reshape(-1, 4)
        self.conn_to = np.ascontiguousarray(con[:, 0], np.int32)
        self.conn_from = np.ascontiguousarray(con[:, 1], np.int32)
        self.conn_weight = np.ascontiguousarray(con[:, 2])
        self.conn_bias = np.ascontiguousarray(con[:, 3])
        out = np.asarray(outputs, np.float64).reshape(-1, 4)
        self.out_a = np.ascontiguousarray(out[:, 0], np.int32)
        self.out_b = np.ascontiguousarray(out[:, 1], np.int32)
        self.out_gain = np.ascontiguousarray(out[:, 2])
        self.out_offset = np.ascontiguousarray(out[:, 3])
        self.n_osc, self.n_conn, self.nu = len(self.frequency), len(self.conn_to), len(self.out_a)

    def as_c(self, struct):
        """Fill a ctypes mirror of fmj_cpg_desc (``struct`` = its class); arrays stay owned by self."""
        I, D = ctypes.POINTER(ctypes.c_int32), ctypes.POINTER(ctypes.c_double)
        d = struct()
        d.n_osc, d.n_conn, d.nu = self.n_osc, self.n_conn, self.nu
        for k in ('frequency', 'rate', 'amplitude', 'conn_weight', 'conn_bias', 'out_gain', 'out_offset'):
            setattr(d, k, getattr(self, k).ctypes.data_as(D))
        for k in ('conn_to', 'conn_from', 'out_a', 'out_b'):
            setattr(d, k, getattr(self, k).ctypes.data_as(I))
        return d


def _chain_and_limbs_network(model, girdle_of, frequency, amplitude, n_wave, limb_amplitude, rate, weight):
    """The double chain on the ``joint_body_*`` joints plus one oscillator pair per limb (the joints ``joint_leg_*`` that share a name
    up to the last ``_k``), the pair's first oscillator coupled with bias pi to the axial oscillator, on the limb's side (``_L`` = 0,
    ``_R`` = 1), of axial joint ``girdle_of(limb, n_axial)``."""
    axial = [j for j, n in enumerate(model.joint_names) if n.startswith('joint_body_')]
    na = len(axial)
    limbs = sorted({n.rsplit('_', 1)[0] for n in model.joint_names if n.startswith('joint_leg_')})
    n_osc = 2*na + 2*len(limbs)
    freq = np.full(n_osc, float(frequency)); rt = np.full(n_osc, float(rate))
    amp = np.concatenate([np.full(2*na, float(amplitude)), np.full(2*len(limbs), float(limb_amplitude))])
    con = []
    bias = 2*np.pi*n_wave/na
    for k in range(na):
        for side in (0, 1):
            i = 2*k + side
            con.append((i, 2*k + (1 - side), weight, np.pi))                    # contralateral, antiphase
            if k + 1 < na:
                con.append((2*(k + 1) + side, i, weight, bias))                 # descending: the next segment lags
                con.append((i, 2*(k + 1) + side, weight, -bias))                # ascending
    for li, name in enumerate(limbs):
        a, b = 2*na + 2*li, 2*na + 2*li + 1
        con.append((a, b, weight, np.pi)); con.append((b, a, weight, np.pi))
        girdle = girdle_of(name, na)
        side = 0 if name.endswith('_L') else 1
        con.append((a, 2*girdle + side, weight, np.pi))                         # limb swings against its body side
    out = []
    for u in range(model.nu):
        jn = model.joint_names[model.actuator_jntid[u]]
        if model.actuator_tags[u] != 'position':
            out.append((-1, -1, 0.0, 0.0))
        elif jn.startswith('joint_body_'):
            k = axial.index(int(model.actuator_jntid[u]))
            out.append((2*k, 2*k + 1, 1.0, 0.0))
        elif jn.endswith('_0') and jn.rsplit('_', 1)[0] in limbs:
            li = limbs.index(jn.rsplit('_', 1)[0])
            out.append((2*na + 2*li, 2*na + 2*li + 1, 1.0, 0.0))
        else:
            out.append((-1, -1, 0.0, 0.0))
    ph0 = np.zeros(n_osc)                     # the limit cycle: head-to-tail lag, sides and limb pairs in antiphase
    for k in range(na):
        ph0[2*k] = -k*bias; ph0[2*k + 1] = -k*bias + np.pi
    for li, name in enumerate(limbs):
        girdle = girdle_of(name, na)
        side = 0 if name.endswith('_L') else 1
        ph0[2*na + 2*li] = ph0[2*girdle + side] + np.pi; ph0[2*na + 2*li + 1] = ph0[2*girdle + side]
    return OscillatorNetwork(freq, rt, amp, con, out, initial_phase=(ph0 + np.pi) % (2*np.pi) - np.pi)


def salamander_network(model, frequency=1.0, amplitude=0.15, n_wave=1.0, limb_amplitude=0.15, rate=20.0,
                       weight=30.0):
    """Double-chain salamander CPG on the axial joints (left/right oscillator per ``joint_body_*``: ascending and
    descending nearest-neighbour couplings with the travelling-wave phase bias, antiphase contralateral couplings)
    plus one oscillator pair per limb coupled to the axial oscillator at its girdle and to the diagonal limb.
    Axial outputs drive the position actuators with r_L (1 + cos th_L) - r_R (1 + cos th_R); each limb drives the
    position actuator of its ``_0`` joint.  Amplitude 0.15 gives a 0.3 rad joint swing."""
    return _chain_and_limbs_network(model, lambda name, na: 0 if 'front' in name else min(na - 1, na//2), frequency, amplitude, n_wave,
                                    limb_amplitude, rate, weight)


def axial_limb_network(model, frequency=1.0, amplitude=0.15, n_wave=1.0, limb_amplitude=0.15, rate=20.0, weight=30.0):
    """``salamander_network``'s double chain for a body with any number of limbs (a centipede: forty legs; an eel: none): each limb's
    pair couples to the axial oscillator of the joint that moves the segment the limb is mounted on - the parent body of the limb's
    ``_0`` joint - where ``salamander_network`` knows two girdles only.  Limbs on the root segment, which no axial joint moves, follow
    the first axial joint.  Two oscillators per axial joint and per limb: centipede() 70, eel(48) 96, centipede(20, 25) 130 (at most
    ``_lib.CPG_MAX_OSC``).  Outputs and ``initial_phase`` as in ``salamander_network``."""
    names = list(model.joint_names)
    axial_of_body = {int(model.jnt_bodyid[j]): k for k, j in enumerate(j for j, n in enumerate(names) if n.startswith('joint_body_'))}

    def girdle_of(limb, na):
        segment = int(model.body_parentid[model.jnt_bodyid[names.index(limb + '_0')]])
        return axial_of_body.get(segment, 0)
    return _chain_and_limbs_network(model, girdle_of, frequency, amplitude, n_wave, limb_amplitude, rate, weight)


class NetworkController(AnimatController):
    """AnimatController (reference task.py:292-346) whose joint position commands come from an OscillatorNetwork
    of at most ``_lib.CPG_MAX_OSC`` oscillators, integrated on the device by ``fmj_cpg_tape``.  ``fusable``: a chunk of the fused loop asks for its
    ctrl tape up front (``ctrl_tape``), so no host work or host->device copy remains per step.  ``drive`` ([n_envs],
    optional) scales the intrinsic frequencies per env.  ``env_params`` gives every env its own numbers on the network's topology
    (``fmj_cpg_tape_ex``): a dict with any of ``frequency``, ``rate``, ``amplitude`` ([n_envs, n_osc]), ``conn_weight``,
    ``conn_bias`` ([n_envs, n_conn], in the order of ``network``'s connection list), ``out_gain``, ``out_offset`` ([n_envs, nu]);
    an entry left out keeps the network's shared values."""
    fusable = True
    tape = True
    ENV_PARAMS = dict(frequency='n_osc', rate='n_osc', amplitude='n_osc', conn_weight='n_conn', conn_bias='n_conn', out_gain='nu',
                      out_offset='nu')

    def __init__(self, model, network, n_envs, env_phase=None, drive=None, device='cuda:0', timestep=None, env_params=None):
        names = [model.joint_names[model.actuator_jntid[a]] for a in range(model.nu)
                 if model.actuator_tags[a] == 'position']
        super().__init__({ControlType.POSITION: names, ControlType.VELOCITY: [], ControlType.TORQUE: []})
        assert network.nu == model.nu
        self.network, self.n_envs, self.nu, self.device = network, n_envs, model.nu, torch.device(device)
        # the network advances once per ITERATION (task.py:288-346 calls the controller on full steps only): with sub-steps pass
        # simulation_options.timestep, the model's own timestep being timestep / num_sub_steps (mjcf.py:1187-1192)
        self.timestep = float(model.timestep if timestep is None else timestep)
        self._timestep_given = timestep is not None      # ExperimentTask.initialize_control sets / validates it against task.timestep
        self._lib = _lib.load()
        self._ctx = ctypes.c_void_p()
        self._desc = network.as_c(_lib.CCpgDesc)
        _lib.check(self._lib.fmj_cpg_create(ctypes.byref(self._desc), self.device.index or 0, ctypes.byref(self._ctx)))
        ph = np.zeros((n_envs, network.n_osc))
        if network.initial_phase is not None:
            ph += network.initial_phase[None, :]
        if env_phase is not None:
            ph += np.asarray(env_phase, np.float64).reshape(n_envs, 1)
        ph = (ph + np.pi) % (2*np.pi) - np.pi
        self.phase = torch.as_tensor(ph, dtype=torch.float32, device=self.device).contiguous()
        self.amp = torch.zeros(n_envs, network.n_osc, dtype=torch.float32, device=self.device)
        self.damp = torch.zeros_like(self.amp)
        self.drive = None if drive is None else torch.as_tensor(np.asarray(drive), dtype=torch.float32,
                                                                device=self.device).contiguous()
        self._pos_idx = torch.as_tensor([a for a in range(model.nu) if model.actuator_tags[a] == 'position'],
                                        device=self.device)
        self._tape = None
        self.env_params = {}      # name of fmj_cpg_env_params -> [n_envs, n] fp32 device tensor
        for k, v in (env_params or {}).items():
            if k not in self.ENV_PARAMS:
                raise ValueError(f'env_params: unknown entry {k!r} (one of {sorted(self.ENV_PARAMS)})')
            v = np.asarray(v, np.float64)
            width = getattr(network, self.ENV_PARAMS[k])
            if v.shape != (n_envs, width):
                raise ValueError(f'env_params[{k!r}]: expected shape [n_envs, {self.ENV_PARAMS[k]}] = ({n_envs}, {width}), not {v.shape}')
            if k == 'frequency':      # rad/s, rounded once as fmj_cpg_create rounds the shared value
                k, v = 'omega', np.float32(2*np.pi*v)
            self.env_params[k] = torch.as_tensor(v, dtype=torch.float32, device=self.device).contiguous()

    def __del__(self):
        try:
            if getattr(self, '_ctx', None):
                self._lib.fmj_cpg_destroy(self._ctx)
                self._ctx = None
        except Exception:
            pass

    def state_dict(self):
        """Oscillator state for Simulation.save_state (phases, amplitudes and their rates, per env)."""
        return {k: getattr(self, k).detach().cpu().numpy().copy() for k in ('phase', 'amp', 'damp')}

    def load_state_dict(self, state):
        for k in ('phase', 'amp', 'damp'):
            t = getattr(self, k)
            t.copy_(torch.as_tensor(np.asarray(state[k]), dtype=t.dtype))

    def ctrl_tape(self, n_steps):
        """Advance the network ``n_steps`` and return ctrl[n_steps, n_envs, nu] (device)."""
        if self._tape is None or self._tape.shape[0] < n_steps:
            self._tape = torch.empty(n_steps, self.n_envs, self.nu, dtype=torch.float32, device=self.device)
        tape = self._tape[:n_steps]
        stream = _lib.stream_ptr(self.device)
        drive = None if self.drive is None else self.drive.data_ptr()
        if not self.env_params:
            _lib.check(self._lib.fmj_cpg_tape(self._ctx, self.n_envs, n_steps, self.timestep, self.phase.data_ptr(),
                                              self.amp.data_ptr(), self.damp.data_ptr(), drive, tape.data_ptr(), stream))
            return tape
        p = _lib.CCpgEnvParams(ctypes.sizeof(_lib.CCpgEnvParams), 0)
        p.drive = drive
        for k, t in self.env_params.items():
            setattr(p, k, t.data_ptr())
        _lib.check(self._lib.fmj_cpg_tape_ex(self._ctx, self.n_envs, n_steps, self.timestep, self.phase.data_ptr(),
                                             self.amp.data_ptr(), self.damp.data_ptr(), ctypes.byref(p), tape.data_ptr(), stream))
        return tape

    def positions(self, iteration, time, timestep):
        return self.ctrl_tape(1)[0][:, self._pos_idx]
