"""Per-environment parameters of the device controllers as far as they can be checked without a GPU: the two new entry points
(fmj_step_fused_ex, fmj_cpg_tape_ex), their argument checks that come before any device call, and the host evaluation of a
WaveController whose frequency, amplitudes and phase lags differ per env (the device evaluates the same expression,
include/fmj.h: fmj_fused_ext)."""
import ctypes
import math
import os

import numpy as np
import pytest

from support_capi import lib as _lib, FMJ_ERR_ARG

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
N = 5


def _model_and_rows(seed=0):
    """salamander33 with a seeded per-env parameter set: frequency in [0.5, 2] Hz, amplitudes in [0, 0.4], lags in [-2 pi, 2 pi],
    zero on every non-position actuator."""
    from farms_mujoco_amd.model import salamander33
    m = salamander33()
    rng = np.random.default_rng(seed)
    pos = np.array([t == 'position' for t in m.actuator_tags[:m.nu]])
    freq = rng.uniform(0.5, 2.0, N)
    amp = rng.uniform(0.0, 0.4, (N, m.nu))*pos
    lag = rng.uniform(-2*np.pi, 2*np.pi, (N, m.nu))*pos
    psi = rng.uniform(0.0, 2*np.pi, N)
    return m, pos, freq, amp, lag, psi


def test_header_declares_both_entries_and_the_abi_version_stays():
    hdr = open(os.path.join(ROOT, 'include', 'fmj.h')).read()
    assert '#define FMJ_ABI_VERSION 6' in hdr
    assert 'int fmj_step_fused_ex(fmj_ctx*' in hdr and 'typedef struct fmj_fused_ext {' in hdr
    assert 'int fmj_cpg_tape_ex(fmj_cpg*' in hdr and 'typedef struct fmj_cpg_env_params {' in hdr


def test_library_exports_both_symbols_and_the_mirrors_have_the_c_sizes():
    L, lib = _lib()
    assert hasattr(lib, 'fmj_step_fused_ex') and hasattr(lib, 'fmj_cpg_tape_ex')
    assert lib.fmj_abi_version() == 6 and L.ABI_VERSION == 6
    # LP64: int32 size, int32 reserved, a pointer, two int64 / two int32 and eight pointers
    assert ctypes.sizeof(L.CFusedExt) == 32 and ctypes.sizeof(L.CCpgEnvParams) == 72


def test_null_handles_are_argument_errors():
    L, lib = _lib()
    ext = L.CFusedExt(ctypes.sizeof(L.CFusedExt), 0)
    assert lib.fmj_step_fused_ex(None, None, None, ctypes.byref(ext), None) == FMJ_ERR_ARG
    assert lib.fmj_step_fused_ex(None, None, None, None, None) == FMJ_ERR_ARG
    p = L.CCpgEnvParams(ctypes.sizeof(L.CCpgEnvParams), 0)
    assert lib.fmj_cpg_tape_ex(None, 1, 1, 1e-3, None, None, None, ctypes.byref(p), None, None) == FMJ_ERR_ARG
    assert lib.fmj_cpg_tape_ex(None, 1, 1, 1e-3, None, None, None, None, None, None) == FMJ_ERR_ARG


def test_per_env_positions_match_the_closed_form():
    """positions() = A[e,j] sin(2 pi frac(f_e t) + psi_e - phi[e,j]) against numpy fp64 from the controller's own fp32 parameters.
    Bound: the host (like the device) forms the argument in fp32 from an fp64 clock, a = fl(fl(fl(2 pi c) + psi) - phi) with
    u = 2^-24: the three roundings are at most u 2 pi, u (2 pi + |psi|) and u (2 pi + |psi| + |phi|), together <= 3 u S with
    S = 2 pi + |psi| + |phi|, and u S <= ulp(S).  |sin'| <= 1 carries that to the sine; the fp32 sine (<= 2 ulp of a value <= 1) and the
    product's rounding add <= 3 u <= 0.4 ulp(S) because S >= 2 pi gives ulp(S) >= 8 u.  Hence |error| <= A 4 ulp(S)."""
    import torch
    from farms_mujoco_amd.control import WaveController
    m, pos, freq, amp, lag, psi = _model_and_rows()
    c = WaveController(m, psi, frequency=freq, amplitude_env=amp, phase_lag_env=lag, device='cpu')
    assert tuple(c.frequency.shape) == (N,) and tuple(c.amplitude.shape) == (N, m.nu) and tuple(c.phase_lag.shape) == (N, m.nu)
    f = c.frequency.numpy().astype(np.float64); A = c.amplitude.numpy().astype(np.float64)[:, pos]
    phi = c.phase_lag.numpy().astype(np.float64)[:, pos]; ps = c.env_phase.numpy().astype(np.float64)
    assert np.ptp(f) > 0.1 and np.abs(A - A[0]).max() > 0.05      # the envs do differ
    for it in (0, 1, 777, 123456):
        t = it*1e-3
        got = c.positions(it, t, 1e-3)
        assert got.dtype == torch.float32 and tuple(got.shape) == (N, int(pos.sum()))
        cyc = f*t - np.floor(f*t)
        want = A*np.sin(2*np.pi*cyc[:, None] + ps[:, None] - phi)
        S = 2*np.pi + np.abs(ps)[:, None] + np.abs(phi)
        bound = A*4*np.spacing(S.astype(np.float32)).astype(np.float64)
        err = np.abs(got.numpy().astype(np.float64) - want)
        print('iteration', it, 'max error', err.max(), 'max of error / bound', (err/np.maximum(bound, 1e-300))[A > 0].max())
        assert np.all(err <= bound)


def test_each_field_alone_may_be_per_env():
    from farms_mujoco_amd.control import WaveController
    m, pos, freq, amp, lag, psi = _model_and_rows(1)
    shared = WaveController(m, psi, frequency=1.25, device='cpu')
    t = 0.321
    base = shared.positions(321, t, 1e-3).numpy()
    # uniform rows of the shared values: the same numbers
    rows = WaveController(m, psi, frequency=np.full(N, 1.25), amplitude_env=np.tile(shared.amplitude.numpy(), (N, 1)),
                          phase_lag_env=np.tile(shared.phase_lag.numpy(), (N, 1)), device='cpu')
    assert np.array_equal(rows.positions(321, t, 1e-3).numpy(), base)
    only_f = WaveController(m, psi, frequency=freq, device='cpu')
    assert tuple(only_f.amplitude.shape) == (m.nu,) and not np.array_equal(only_f.positions(321, t, 1e-3).numpy(), base)
    only_a = WaveController(m, psi, frequency=1.25, amplitude_env=amp, device='cpu')
    assert isinstance(only_a.frequency, float) and tuple(only_a.phase_lag.shape) == (m.nu,)
    assert not np.array_equal(only_a.positions(321, t, 1e-3).numpy(), base)


def test_bad_shapes_raise_value_error_naming_the_shape():
    from farms_mujoco_amd.control import NetworkController, WaveController
    m, pos, freq, amp, lag, psi = _model_and_rows()
    with pytest.raises(ValueError, match=r'frequency.*\(5,\)'):
        WaveController(m, psi, frequency=freq[:4], device='cpu')
    with pytest.raises(ValueError, match=rf'amplitude_env.*\(5, {m.nu}\)'):
        WaveController(m, psi, amplitude_env=amp[:, :-1], device='cpu')
    with pytest.raises(ValueError, match=rf'amplitude_env.*\(5, {m.nu}\)'):
        WaveController(m, psi, amplitude_env=amp[0], device='cpu')
    with pytest.raises(ValueError, match=rf'phase_lag_env.*\(5, {m.nu}\)'):
        WaveController(m, psi, phase_lag_env=lag[:3], device='cpu')
    assert not pos.all()
    bad = amp.copy(); bad[2, np.nonzero(~pos)[0][0]] = 0.1
    with pytest.raises(ValueError, match='non-position'):
        WaveController(m, psi, amplitude_env=bad, device='cpu')
    assert 'env_params' in NetworkController.__init__.__code__.co_varnames


def test_todays_arguments_give_todays_values():
    """The default path is unchanged: positions() equals the expression the controller has always evaluated, bit for bit, and the
    literal below was computed with it (float32; amplitude 0.3, n_wave 1, 1.5 Hz, t = 0.4321)."""
    import torch
    from farms_mujoco_amd.control import WaveController
    from farms_mujoco_amd.model import salamander33, wave_controller_params
    m = salamander33()
    psi = np.array([0.0, 1.0, 2.5])
    c = WaveController(m, psi, frequency=1.5, device='cpu')
    assert isinstance(c.frequency, float) and tuple(c.amplitude.shape) == (m.nu,) and tuple(c.phase_lag.shape) == (m.nu,)
    t = 0.4321
    got = c.positions(432, t, 1e-3)
    amp, lag = wave_controller_params(m, 0.3, 1.0)
    idx = torch.as_tensor([a for a in range(m.nu) if m.actuator_tags[a] == 'position'])
    A = torch.as_tensor(amp, dtype=torch.float32); L = torch.as_tensor(lag, dtype=torch.float32)
    P = torch.as_tensor(psi, dtype=torch.float32)
    cyc = (1.5*t) % 1.0
    arg = (2*math.pi*cyc) + P[:, None] - L[None, idx]
    want = A[None, idx]*torch.sin(arg)
    assert torch.equal(got, want)
    # the first axial actuator has lag 0: 0.3 sin(2 pi frac(1.5 * 0.4321) + psi)
    first = int(np.nonzero(amp[idx.numpy()])[0][0])
    assert np.allclose(got[:, first].numpy(), LITERAL, rtol=0, atol=6e-8), got[:, first].numpy().tolist()


LITERAL = [-0.24063900113105774, -0.28076300024986267, 0.0855732187628746]
