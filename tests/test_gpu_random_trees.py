"""Generality of the HIP path: seeded random kinematic trees (branching, welded bodies, hinge + slide joints with
off-centre anchors, rotated inertial frames, free or fixed base, spring-dampers, armature, all three actuator kinds
with control / force limits, external forces) against the fp64 oracle."""
import numpy as np
import pytest

from farms_mujoco_amd.options import KernelOptions
from support_models import random_tree, FMJ_WARN_CONTACTFULL
from support_sims import check_random_tree_vs_oracle

pytestmark = pytest.mark.gpu

@pytest.mark.parametrize('seed,two_per_wave', [(s, True) for s in range(20)] + [(s, False) for s in range(0, 20, 2)])
def test_random_tree_vs_oracle(oracle, seed, two_per_wave):
    """Every tree here has <= 32 bodies, so it runs in the two-envs-per-wave kernel by default; KernelOptions(two_env=False)
    sends the same tree through the one-env-per-wave kernel."""
    check_random_tree_vs_oracle(oracle, seed, 32 if two_per_wave else 64, KernelOptions(two_env=two_per_wave))


@pytest.mark.parametrize('seed,two_per_wave', [(s, True) for s in range(100, 112)] + [(s, False) for s in range(100, 112, 2)])
def test_random_tree_with_limits_and_contacts(oracle, seed, two_per_wave):
    """The constraint path on random trees: limited hinges, sphere / capsule / box / cylinder geoms over a plane that cuts
    through the tree; contact lists, constraint forces and the state after one and after 30 steps vs the oracle.  Every tree here has
    <= 32 bodies: it runs in the two-env constraint kernel (fmj_cons2.inc) by default, KernelOptions(two_env=False) sends it through the one-env kernel."""
    import torch
    from farms_mujoco_amd.physics import BatchedPhysics
    m = random_tree(seed, contacts=True)
    if m is None or m.nv == 0:
        pytest.skip('degenerate draw')
    rng = np.random.default_rng(2000 + seed)
    n = 6
    qpos = np.tile(m.qpos0, (n, 1)) + rng.uniform(-0.4, 0.4, (n, m.nq))
    for j in range(m.njnt):
        if m.jnt_type[j] == 0:
            a = m.jnt_qposadr[j]; q = rng.normal(size=(n, 4)); qpos[:, a+3:a+7] = q/np.linalg.norm(q, axis=1, keepdims=True)
            qpos[:, a+2] = rng.uniform(-0.05, 0.1, n)
    qvel = rng.normal(size=(n, m.nv))*0.2
    ctrl = rng.uniform(-0.4, 0.4, (n, max(m.nu, 1)))[:, :m.nu]
    phys = BatchedPhysics(m, n, kernel=KernelOptions(two_env=two_per_wave))
    assert phys.kernel_info()['threads_per_env'] == (32 if two_per_wave else 64)
    d = phys.data
    f32 = lambda a: torch.as_tensor(a, dtype=torch.float32)
    d.qpos[:] = f32(qpos); d.qvel[:] = f32(qvel)
    if m.nu:
        d.ctrl[:] = f32(ctrl)
    r64 = lambda t: t.cpu().numpy().astype(np.float64)
    q32, v32, c32 = r64(d.qpos), r64(d.qvel), r64(d.ctrl)
    phys.step(1)
    torch.cuda.synchronize()
    assert int((d.status & ~FMJ_WARN_CONTACTFULL).abs().sum()) == 0     # a truncated contact list (both sides truncate alike) is the only bit allowed
    fds = [oracle.forward_debug(m, q32[e], v32[e], ctrl=c32[e] if m.nu else None) for e in range(n)]
    ncon_ref = np.array([fd['ncon'] for fd in fds])
    assert np.array_equal(d.ncon.cpu().numpy(), ncon_ref), (d.ncon.cpu().numpy(), ncon_ref)
    ref = oracle.step(m, q32, v32, ctrl=c32 if m.nu else None)

    def err(k):
        a = r64(getattr(d, k)); bb = ref[k]
        return np.abs(a - bb).max()/max(np.abs(bb).max(), 1e-9)
    for k, tol in (('xpos', 5e-6), ('qvel', 3e-3), ('qpos', 2e-5)):
        assert err(k) < tol, (seed, m.nbody, m.nv, ncon_ref, k, err(k))
    for e in range(n):
        fd = fds[e]
        if fd['ncon']:
            f = fd['efc_force'][fd['nefc'] - 4*fd['ncon']:fd['nefc']].reshape(-1, 4).sum(1)
            got = d.contact.cpu().numpy()[e, :fd['ncon'], 12]
            assert np.allclose(got, f, rtol=3e-2, atol=2e-3*max(1.0, np.abs(f).max())), (seed, e, got, f)


MESH_SEEDS = (301, 302, 303, 304, 305, 306, 307, 308, 310, 311)      # draws with a movable tree and at least one mesh geom (300 and 309 have none)


@pytest.mark.parametrize('seed', MESH_SEEDS)
def test_random_tree_with_mesh_geoms(oracle, seed):
    """Random trees whose collision shapes include convex meshes (random point clouds, hulls of 4 to ~30 vertices, rotated
    and off-centre), with limits, over a plane: contact counts, the state after one step and the contact forces vs the
    oracle (models with meshes run the PAIRS instantiation of the constraint kernel)."""
    import torch
    from farms_mujoco_amd.physics import BatchedPhysics
    m = random_tree(seed, contacts=True, meshes=True)
    assert m is not None and m.nv > 0 and m.nmeshvert > 0, f'seed {seed} no longer draws a tree with mesh geoms: pick another for MESH_SEEDS'
    rng = np.random.default_rng(5000 + seed)
    n = 6
    qpos = np.tile(m.qpos0, (n, 1)) + rng.uniform(-0.4, 0.4, (n, m.nq))
    for j in range(m.njnt):
        if m.jnt_type[j] == 0:
            a = m.jnt_qposadr[j]; q = rng.normal(size=(n, 4)); qpos[:, a+3:a+7] = q/np.linalg.norm(q, axis=1, keepdims=True)
            qpos[:, a+2] = rng.uniform(-0.05, 0.1, n)
    qvel = rng.normal(size=(n, m.nv))*0.2
    phys = BatchedPhysics(m, n)
    d = phys.data
    f32 = lambda a: torch.as_tensor(a, dtype=torch.float32)
    d.qpos[:] = f32(qpos); d.qvel[:] = f32(qvel)
    r64 = lambda t: t.cpu().numpy().astype(np.float64)
    q32, v32 = r64(d.qpos), r64(d.qvel)
    phys.step(1)
    torch.cuda.synchronize()
    assert int((d.status & ~FMJ_WARN_CONTACTFULL).abs().sum()) == 0
    fds = [oracle.forward_debug(m, q32[e], v32[e], ctrl=np.zeros(m.nu) if m.nu else None) for e in range(n)]
    ncon_ref = np.array([fd['ncon'] for fd in fds])
    assert np.array_equal(d.ncon.cpu().numpy(), ncon_ref), (d.ncon.cpu().numpy(), ncon_ref)
    ref = oracle.step(m, q32, v32, ctrl=np.zeros((n, m.nu)) if m.nu else None)
    for k, tol in (('xpos', 5e-6), ('qvel', 3e-3), ('qpos', 2e-5)):
        a = r64(getattr(d, k)); bb = ref[k]
        e_ = np.abs(a - bb).max()/max(np.abs(bb).max(), 1e-9)
        assert e_ < tol, (seed, m.nbody, m.nv, ncon_ref, k, e_)
    for e in range(n):
        fd = fds[e]
        if fd['ncon']:
            got = d.contact.cpu().numpy()[e, :fd['ncon']]
            assert np.allclose(got[:, :3], fd['contact'][:fd['ncon'], :3], atol=2e-6), (seed, e)
            f = fd['efc_force'][fd['nefc'] - 4*fd['ncon']:fd['nefc']].reshape(-1, 4).sum(1)
            assert np.allclose(got[:, 12], f, rtol=3e-2, atol=2e-3*max(1.0, np.abs(f).max())), (seed, e, got[:, 12], f)
