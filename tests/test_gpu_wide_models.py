"""Models past one wavefront: the two-wave step kernel (csrc/fmj_wide.inc, one workgroup of 128 threads per env) on unconstrained
models of up to 128 bodies / dofs, against the fp64 oracle with the fp32-storage-floor yardsticks of test_gpu_morphologies.py, against
the one-wave kernels on the same model (KernelOptions(two_wave=True)), and through the product path (fused swim, freeze, checkpoint)."""
import numpy as np
import pytest

from parity_metrics import relerr as _relerr, group_relerr, qpos_groups, qvel_groups, link_row_groups
from support_models import finned_eel as _finned_eel
from support_sims import swim_sim, wave_at, swim_oracle as _swim_oracle

pytestmark = pytest.mark.gpu


def _make(name):
    import farms_mujoco_amd.model as mm
    return {'centipede_20_25': lambda: mm.centipede(20, 25), 'centipede_12_50': lambda: mm.centipede(12, 50),
            'finned_eel': _finned_eel}[name]()


def _tape(m, n, T, psi):
    import farms_mujoco_amd.model as mm
    amp, lag = mm.wave_controller_params(m, amplitude=0.25)
    t = np.arange(T)[:, None, None]*m.timestep
    return amp[None, None, :]*np.sin(2*np.pi*1.5*t - lag[None, None, :] + psi[None, :, None])


def _phys(m, qpos, qvel, kernel=None):
    import torch
    from farms_mujoco_amd.physics import BatchedPhysics
    phys = BatchedPhysics(m, qpos.shape[0], kernel=kernel)
    phys.data.qpos[:] = torch.as_tensor(qpos, dtype=torch.float32)
    phys.data.qvel[:] = torch.as_tensor(qvel, dtype=torch.float32)
    return phys


@pytest.mark.parametrize('name,T', [('centipede_20_25', 300), ('centipede_12_50', 300), ('finned_eel', 100)])
def test_step_parity_wide_models(oracle, name, T):
    """One step and a rollout of T steps against the oracle (wave-controller ctrl tape, 16 envs); the bounds of
    test_step_parity_other_morphologies, the rollout's against the fp32-storage floor's own rollout."""
    import torch
    import farms_mujoco_amd.model as mm
    m = _make(name)
    assert m.nbody > 64
    n = 16
    qpos, qvel, psi = mm.synthetic_batch(m, n, seed=4)
    tape_t = torch.as_tensor(_tape(m, n, T, psi), dtype=torch.float32, device='cuda').contiguous()
    phys = _phys(m, qpos, qvel)
    assert phys.kernel_info()['threads_per_env'] == 128
    d = phys.data
    phys.step(1, ctrl_tape=tape_t[:1].contiguous())
    torch.cuda.synchronize()
    q32 = torch.as_tensor(qpos, dtype=torch.float32).numpy().astype(np.float64)
    ctrl = tape_t.cpu().numpy().astype(np.float64)
    ref1 = oracle.step(m, q32, qvel, ctrl=ctrl[:1], n_steps=1, ctrl_step_stride=n*m.nu)
    with oracle.fp32_storage():
        floor1 = oracle.step(m, q32, qvel, ctrl=ctrl[:1], n_steps=1, ctrl_step_stride=n*m.nu)
    for k, tol in (('xpos', 2e-6), ('xquat', 2e-6), ('sensordata', 5e-5)):
        assert _relerr(getattr(d, k).cpu().numpy(), ref1[k]) < tol, (name, k, _relerr(getattr(d, k).cpu().numpy(), ref1[k]))
    for k, groups in (('qvel', qvel_groups(m)), ('qpos', qpos_groups(m))):
        got = getattr(d, k).cpu().numpy()
        err = group_relerr(got, ref1[k], groups); fl = group_relerr(floor1[k], ref1[k], groups)
        whole, whole_fl = _relerr(got, ref1[k]), _relerr(floor1[k], ref1[k])
        print(name, k, 'first step: per-component err', err, 'fp32-storage floor', fl, ' whole-tensor err', whole, 'floor', whole_fl)
        if fl < 0.1:
            assert err < 6*fl + 1e-6, (name, k, err, fl)
        else:
            # centipede(12, 50): a spine of 50 light links, where fp32 storage of M alone moves some component by 40 %: the per-component
            # metric is set by entries near zero (test_gpu_morphologies.py, CAP48); the whole tensor is held to 6 x its own floor instead
            assert whole < 6*whole_fl + 1e-6, (name, k, whole, whole_fl)
    phys.step(T - 1, ctrl_tape=tape_t[1:].contiguous())
    torch.cuda.synchronize()
    assert int(d.status.abs().sum()) == 0
    ref = oracle.step(m, q32, qvel, ctrl=ctrl, n_steps=T, ctrl_step_stride=n*m.nu, n_threads=8)
    with oracle.fp32_storage():
        fl = oracle.step(m, q32, qvel, ctrl=ctrl, n_steps=T, ctrl_step_stride=n*m.nu, n_threads=8)
    err, flo = _relerr(d.qpos.cpu().numpy(), ref['qpos']), _relerr(fl['qpos'], ref['qpos'])
    print(name, 'nbody', m.nbody, 'nv', m.nv, 'qpos rel err after', T, 'steps:', err, 'fp32-storage floor', flo)
    assert err < max(1e-4, 6*flo)


def test_fused_swim_of_a_wide_centipede(oracle):
    """Simulation.run(fused=True) on centipede(20, 25): rows, drag + buoyancy, wave controller in the kernel, against the oracle's
    fused loop at 6x the fp32-storage floor."""
    import torch
    import farms_mujoco_amd.model as mm
    m = mm.centipede(20, 25)
    T = 40
    sim = swim_sim(12, T, m=m, seed=9, controller_of=wave_at(1.5))[0]
    assert sim.physics.kernel_info()['threads_per_env'] == 128
    ref = _swim_oracle(oracle, sim, m, T)
    with oracle.fp32_storage():
        flo = _swim_oracle(oracle, sim, m, T)
    sim.run(fused=True)
    torch.cuda.synchronize()
    assert int(sim.physics.data.status.abs().sum()) == 0
    sens = sim.task.data.sensors
    got = dict(qpos=sim.physics.data.qpos.cpu().numpy(), links=sens.links.array.cpu().numpy(), xfrc=sens.xfrc.array.cpu().numpy())
    groups = dict(qpos=qpos_groups(m), links=link_row_groups(), xfrc=[slice(0, 3), slice(3, 6)])
    for k in got:
        err = group_relerr(got[k], ref[k], groups[k]); fl = group_relerr(flo[k], ref[k], groups[k])
        print('centipede(20, 25)', k, 'per-component err', err, 'fp32-storage floor', fl)
        assert err < 6*fl + 1e-6, (k, err, fl)
    assert np.abs(sens.links.array.cpu().numpy()[-1, :, :, 14:17]).max() > 1e-3      # it swims


@pytest.mark.parametrize('maker', ['centipede', 'salamander33', 'eel58'])
def test_forced_wide_kernel_matches_the_one_wave_kernel(oracle, maker):
    """KernelOptions(two_wave=True) runs the two-wave kernel on a model that fits one wave: after 1 and 100 steps it agrees with the model's own kernel
    per component within 6x the fp32-storage floor (two fp32 kernels with different reduction orders: not bitwise).  eel58: a dof
    chain of 64, the register row of the MAXD 64 instantiation."""
    import torch
    import farms_mujoco_amd.model as mm
    from farms_mujoco_amd.options import KernelOptions
    m = mm.eel(n_joints=58) if maker == 'eel58' else getattr(mm, maker)()
    n = 8
    qpos, qvel, psi = mm.synthetic_batch(m, n, seed=4)
    T = 100
    tape_t = torch.as_tensor(_tape(m, n, T, psi), dtype=torch.float32, device='cuda').contiguous()
    base = _phys(m, qpos, qvel, KernelOptions())
    assert base.kernel_info()['threads_per_env'] in (32, 64)
    wide = _phys(m, qpos, qvel, KernelOptions(two_wave=True))
    assert wide.kernel_info()['threads_per_env'] == 128
    q32 = torch.as_tensor(qpos, dtype=torch.float32).numpy().astype(np.float64)
    ctrl = tape_t.cpu().numpy().astype(np.float64)
    done = 0
    for steps in (1, T - 1):
        base.step(steps, ctrl_tape=tape_t[done:done + steps].contiguous())
        wide.step(steps, ctrl_tape=tape_t[done:done + steps].contiguous())
        done += steps
        torch.cuda.synchronize()
        ref = oracle.step(m, q32, qvel, ctrl=ctrl[:done], n_steps=done, ctrl_step_stride=n*m.nu, n_threads=8)
        with oracle.fp32_storage():
            flo = oracle.step(m, q32, qvel, ctrl=ctrl[:done], n_steps=done, ctrl_step_stride=n*m.nu, n_threads=8)
        for k, groups in (('qvel', qvel_groups(m)), ('qpos', qpos_groups(m))):
            err = group_relerr(getattr(wide.data, k).cpu().numpy(), getattr(base.data, k).cpu().numpy(), groups)
            fl = group_relerr(flo[k], ref[k], groups)
            print(maker, done, k, 'two-wave vs one-wave per component', err, 'fp32-storage floor', fl)
            assert err < 6*fl + 1e-6, (maker, done, k, err, fl)
    assert int(wide.data.status.abs().sum()) == 0 and int(base.data.status.abs().sum()) == 0


def test_wide_results_do_not_depend_on_the_batch():
    """The same env's inputs at different batch indices (a permuted batch, a batch of one) give bitwise the same state after 100 steps."""
    import torch
    import farms_mujoco_amd.model as mm
    m = mm.centipede(20, 25)
    n, T = 8, 100
    qpos, qvel, psi = mm.synthetic_batch(m, n, seed=2)
    tape = _tape(m, n, T, psi)
    perm = np.array([5, 2, 7, 0, 3, 6, 1, 4])
    out = []
    for idx in (np.arange(n), perm, np.array([3])):
        phys = _phys(m, qpos[idx], qvel[idx])
        phys.step(T, ctrl_tape=torch.as_tensor(tape[:, idx], dtype=torch.float32, device='cuda').contiguous())
        torch.cuda.synchronize()
        assert int(phys.data.status.abs().sum()) == 0
        out.append((idx, phys.data.qpos.cpu().numpy(), phys.data.qvel.cpu().numpy()))
    (_, q0, v0) = out[0]
    for idx, q, v in out[1:]:
        assert np.array_equal(q, q0[idx]) and np.array_equal(v, v0[idx]), idx


def test_nan_state_freezes_a_wide_env():
    """A NaN in one env's qvel, on a dof of the second wave (index >= 64), freezes that env for the whole workgroup: its status word
    says FMJ_WARN_BADQVEL, its qpos is the pre-launch qpos, it writes no links rows, and every other env matches an unpoisoned run."""
    import torch
    import farms_mujoco_amd.model as mm
    from farms_mujoco_amd.physics import PhysicsError
    m = mm.centipede(20, 25)
    n, T, bad, dof = 5, 30, 2, 100
    assert dof >= 64 and dof < m.nv
    clean = swim_sim(n, T, m=m, seed=9, controller_of=wave_at(1.5))[0]
    clean.run(fused=True)
    sim = swim_sim(n, T, m=m, seed=9, controller_of=wave_at(1.5))[0]
    sim.physics.data.qvel[bad, dof] = float('nan')
    q_before = sim.physics.data.qpos[bad].clone()
    with pytest.raises(PhysicsError):
        sim.run(fused=True)
    torch.cuda.synchronize()
    d = sim.physics.data
    st = d.status.cpu().numpy()
    assert st[bad] & 2 and not st[np.arange(n) != bad].any()
    assert torch.equal(d.qpos[bad], q_before)
    links = sim.task.data.sensors.links.array.cpu().numpy()
    assert np.all(links[:, bad] == 0.0)
    others = np.arange(n) != bad
    assert torch.equal(d.qpos[others], clean.physics.data.qpos[others])
    assert np.array_equal(links[:, others], clean.task.data.sensors.links.array.cpu().numpy()[:, others])


def test_checkpoint_of_a_wide_model_is_bitwise(tmp_path):
    """save_state -> 50 steps -> load_state -> the same 50 steps: bitwise the same state and rows."""
    import torch
    import farms_mujoco_amd.model as mm
    m = mm.centipede(20, 25)
    sim = swim_sim(4, 100, m=m, seed=9, controller_of=wave_at(1.5))[0]
    ck = sim.save_state(str(tmp_path/'state.npz'))
    sim.step_fused(50)
    torch.cuda.synchronize()
    first = (sim.physics.data.qpos.clone(), sim.physics.data.qvel.clone(), sim.task.data.sensors.links.array.clone(),
             sim.task.data.sensors.xfrc.array.clone())
    sim.load_state(ck)
    assert sim.task.sim_iteration == 0
    sim.step_fused(50)
    torch.cuda.synchronize()
    again = (sim.physics.data.qpos, sim.physics.data.qvel, sim.task.data.sensors.links.array, sim.task.data.sensors.xfrc.array)
    for a, b in zip(first, again):
        assert torch.equal(a, b)
    assert int(sim.physics.data.status.abs().sum()) == 0 and float(first[2].abs().max()) > 0
