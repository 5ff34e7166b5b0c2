"""GPU parity: HIP fp32 step (through the C-ABI) vs the fp64 CPU oracle on identical inputs.

The oracle is the checker only.  Tolerances are stated per test; north-star: qpos within 1e-4
relative error after 1000 steps (fp64 -> fp32).
"""
import numpy as np
import pytest

from parity_metrics import relerr as _relerr, group_relerr, qpos_groups, qvel_groups
from support_models import rand_state as _rand_state

pytestmark = pytest.mark.gpu


@pytest.fixture(scope='module')
def sal():
    from farms_mujoco_amd.model import salamander33
    return salamander33()


def _gpu_physics(m, n):
    import torch
    from farms_mujoco_amd.physics import BatchedPhysics
    return BatchedPhysics(m, n, 'cuda:0'), torch


def test_single_step_all_fields(sal, oracle):
    """One mj_step from random states.  Kinematic fields and sensors agree to fp32 rounding (2e-6 .. 2e-5 of the field
    maximum).  qvel / qacc come out of the (M + hB) solve, and that matrix is ill-conditioned (light, stiffly actuated limb
    chains on a heavy trunk: scaled condition number 3e4): merely STORING it in fp32 moves the solution by ~1e-5 of its
    maximum, whatever computes it.  The bound is therefore stated against that floor - the fp64 oracle with its stored M / H
    rounded to fp32 and nothing else (oracle.fp32_storage) - per component (parity_metrics.group_relerr), not as a fitted
    number: the HIP step stays within 6x of it (measured 2 - 3x)."""
    m, n = sal, 64
    phys, torch = _gpu_physics(m, n)
    qpos, qvel, ctrl = _rand_state(m, n, 1)
    xf = np.random.default_rng(2).normal(size=(n, m.nbody, 6))*0.01
    xf[:, 0] = 0
    d = phys.data
    d.qpos[:] = torch.as_tensor(qpos, dtype=torch.float32); d.qvel[:] = torch.as_tensor(qvel, dtype=torch.float32)
    d.ctrl[:] = torch.as_tensor(ctrl, dtype=torch.float32); d.xfrc_applied[:] = torch.as_tensor(xf, dtype=torch.float32)
    r64 = lambda t: t.cpu().numpy().astype(np.float64)
    q32, v32, c32, x32 = r64(d.qpos), r64(d.qvel), r64(d.ctrl), r64(d.xfrc_applied)     # the fp32-rounded inputs are THE inputs
    phys.step(1)
    torch.cuda.synchronize()
    ref = oracle.step(m, q32, v32, ctrl=c32, xfrc_applied=x32)
    with oracle.fp32_storage():
        floor = oracle.step(m, q32, v32, ctrl=c32, xfrc_applied=x32)
    assert int(d.status.abs().sum()) == 0
    for name, tol in (('xpos', 2e-6), ('xquat', 2e-6), ('xipos', 2e-6), ('sensordata', 2e-5)):
        err = _relerr(getattr(d, name).cpu().numpy(), ref[name])
        assert err < tol, (name, err)
    for name in ('qpos', 'qvel', 'qacc'):
        groups = qpos_groups(m) if name == 'qpos' else qvel_groups(m)
        err = group_relerr(r64(getattr(d, name)), ref[name], groups)
        fl = group_relerr(floor[name], ref[name], groups) + (1e-6 if name == 'qpos' else 0.0)     # + the fp32 rounding of q itself
        print(name, 'per-component err', err, 'fp32-storage floor', fl)
        assert err < 6*fl, (name, err, fl)
        assert _relerr(r64(getattr(d, name)), ref[name]) < 1e-4        # and the old whole-tensor statement still holds (qpos: 2e-6)


def test_forward_only_matches_oracle_derived(sal, oracle):
    """fmj_forward (no integration): derived fields equal the oracle's, state untouched."""
    m, n = sal, 8
    phys, torch = _gpu_physics(m, n)
    qpos, qvel, ctrl = _rand_state(m, n, 3)
    d = phys.data
    d.qpos[:] = torch.as_tensor(qpos, dtype=torch.float32); d.qvel[:] = torch.as_tensor(qvel, dtype=torch.float32)
    q0 = d.qpos.clone(); v0 = d.qvel.clone()
    phys.forward(disable_actuation=True)
    torch.cuda.synchronize()
    assert torch.equal(d.qpos, q0) and torch.equal(d.qvel, v0)
    ref = oracle.step(m, qpos, qvel, ctrl=None)     # ctrl None -> zero ctrl; kp*q bias still acts in the oracle
    for name in ('xpos', 'xquat', 'xipos'):
        assert _relerr(getattr(d, name).cpu().numpy(), ref[name]) < 2e-6
    # actuator forces are zero with actuation disabled
    adr = phys.sensor_layout.actuatorfrc_adr
    assert float(d.sensordata[:, adr:].abs().max()) == 0.0


def test_thousand_steps_qpos(sal, oracle):
    """North-star tolerance: qpos within 1e-4 relative error of the fp64 oracle after 1000 steps."""
    m, n = sal, 32
    phys, torch = _gpu_physics(m, n)
    qpos, qvel, ctrl = _rand_state(m, n, 5, qscale=0.05, vscale=0.0)
    qpos[:, :3] = m.qpos0[:3]; qpos[:, 3:7] = [1, 0, 0, 0]
    from farms_mujoco_amd.model import wave_controller_params
    rng = np.random.default_rng(6)
    T = 1000
    t = np.arange(T)[:, None, None]*m.timestep
    amp, lag = wave_controller_params(m)
    psi = rng.uniform(0, 2*np.pi, (1, n, 1))
    tape = amp[None, None, :]*np.sin(2*np.pi*1.0*t - lag[None, None, :] + psi)
    d = phys.data
    d.qpos[:] = torch.as_tensor(qpos, dtype=torch.float32); d.qvel[:] = torch.as_tensor(qvel, dtype=torch.float32)
    # fp32-rounded inputs are THE inputs for both sides
    qpos32 = d.qpos.cpu().numpy().astype(np.float64); qvel32 = d.qvel.cpu().numpy().astype(np.float64)
    tape_t = torch.as_tensor(tape, dtype=torch.float32, device='cuda').contiguous()
    tape32 = tape_t.cpu().numpy().astype(np.float64)
    phys.step(T, ctrl_tape=tape_t)
    torch.cuda.synchronize()
    ref = oracle.step(m, qpos32, qvel32, ctrl=tape32, n_steps=T, ctrl_step_stride=n*m.nu, n_threads=8)
    assert int(d.status.abs().sum()) == 0
    err = _relerr(d.qpos.cpu().numpy(), ref['qpos'])
    # per component (root position, quaternion, joint angles each against their own scale): small joint angles are the hardest
    # (6.5e-6 rad on angles of 0.02 .. 0.3 rad); stated against the same 1000 steps with M / H merely stored in fp32
    with oracle.fp32_storage():
        floor = oracle.step(m, qpos32, qvel32, ctrl=tape32, n_steps=T, ctrl_step_stride=n*m.nu, n_threads=8)
    gerr = group_relerr(d.qpos.cpu().numpy(), ref['qpos'], qpos_groups(m))
    gfl = group_relerr(floor['qpos'], ref['qpos'], qpos_groups(m))
    print('qpos rel err after 1000 steps:', err, 'per component:', gerr, 'fp32-storage floor per component:', gfl)
    assert err < 1e-4, err                               # the north-star statement (whole-vector relative error)
    assert gerr < 6*gfl and gerr < 5e-4, (gerr, gfl)


def test_batch_invariance_bitwise(sal):
    """Env e's result is independent of batch size and position in the batch (bitwise)."""
    m = sal
    qpos, qvel, ctrl = _rand_state(m, 96, 9)
    outs = []
    for n, sl in ((96, slice(0, 96)), (17, slice(40, 57))):
        phys, torch = _gpu_physics(m, n)
        d = phys.data
        d.qpos[:] = torch.as_tensor(qpos[sl], dtype=torch.float32); d.qvel[:] = torch.as_tensor(qvel[sl], dtype=torch.float32)
        d.ctrl[:] = torch.as_tensor(ctrl[sl], dtype=torch.float32)
        phys.step(20)
        torch.cuda.synchronize()
        outs.append((d.qpos.cpu().numpy().copy(), d.qvel.cpu().numpy().copy(), d.sensordata.cpu().numpy().copy()))
    for a, b in zip(outs[0], outs[1]):
        assert np.isfinite(b).all() and np.array_equal(a[40:57], b)
