"""The device narrow phase (fmj_narrow.inc: ground_dist, CONTACT_RECORD; fmj_narrow_ground.inc: sphere, capsule, box, cylinder against one
ground entry; the mesh block and the slot bookkeeping of the including kernels) against the independent numpy reference of
support_narrow.py, which shares no text with the kernels or the oracle and is itself pinned on the CPU by test_narrow_reference.py.

Procedure (the pattern of test_plane_box_contacts): create BatchedPhysics(model, n), set_state and take back the fp32 state, step once,
convert the records with oracle.contacts_from_hip, compare env by env with ref_ground_contacts(model, q32[e]).  The envs of one batch are
the poses of one model, batch sizes are odd and neighbouring envs hold different cases, so the two halves of a wave of the two-env kernel
disagree about their contact counts.  Models the two-env constraint kernel accepts (one ground, at most 32 geoms, no mesh, PGS, pyramidal)
run twice - default path and KernelOptions(two_env=False) - and every run asserts kernel_info()['threads_per_env'], so it is known which kernel ran.

Per env: ncon equal; geom ids of every record equal, in the reference's order; positions within 2e-6 m and the nine frame entries within
2e-5 (the bounds of test_heightfield_contacts_match_oracle, for every case); status 0, or exactly FMJ_WARN_CONTACTFULL where the case is a
truncation; each frame orthonormal to 1e-5 and right-handed on its own.  Cases whose deepest penetration is under 1 cm also compare qvel
after the step (parity_metrics.relerr < 2e-3) and every contact's normal force with the oracle's pyramid rows (rtol 2e-2, atol 2e-4: the
bounds of test_plane_box_contacts).  In the exactly symmetric cases (flat box, upright cylinder, parallel capsule) the contacts of one geom
share a load; the oracle.fp32_storage() runs (levels 1 to 3) move no single contact's force there by more than 1e-3 of that bound - the
one free body's inertia is diagonal and well conditioned - so the forces are compared contact by contact in those cases too."""
import zlib

import numpy as np
import pytest

from parity_metrics import relerr
from support_sims import set_state
from support_narrow import (ref_ground_contacts, admissible, contact_frame, directed_batches, directed_model, seeded_scenes, build_model,
                            FMJ_WARN_CONTACTFULL)

pytestmark = pytest.mark.gpu

POS_TOL, FRAME_TOL = 2e-6, 2e-5
ONE_ENV_ONLY = ('two_grounds', 'chunk')          # two ground entries; more than 32 geoms


def _run(oracle, m, qpos, threads, label, exact=(), truncated=(), forces=True):
    """One batch through the device and the reference; returns (worst position error, worst frame error, contacts compared)."""
    import torch
    from farms_mujoco_amd.options import KernelOptions
    from farms_mujoco_amd.physics import BatchedPhysics
    qpos = np.asarray(qpos, float)
    n = len(qpos)
    assert n % 2 == 1
    rng = np.random.default_rng(zlib.crc32(label.encode()))
    phys = BatchedPhysics(m, n, kernel=KernelOptions(two_env=threads == 32))
    assert phys.kernel_info()['threads_per_env'] == threads, (label, phys.kernel_info())
    q32, v32, _ = set_state(phys, qpos, 0.05*rng.normal(size=(n, m.nv)))
    phys.data.status.zero_()          # OR-accumulated: the constructor's reset ran a forward pass at qpos0, where the body lies in the ground
    phys.step(1)
    torch.cuda.synchronize()
    d = phys.data
    ncon, status = d.ncon.cpu().numpy(), d.status.cpu().numpy()
    con = oracle.contacts_from_hip(d.contact.cpu().numpy())
    worst_p = worst_f = 0.0
    compared = 0
    shallow = []
    for e in range(n):
        ok, why = admissible(m, q32[e], exact=e in exact)
        assert ok, (label, e, why)
        ref = ref_ground_contacts(m, q32[e])
        k = len(ref['contacts'])
        assert ncon[e] == k, (label, e, int(ncon[e]), k)
        assert status[e] == (FMJ_WARN_CONTACTFULL if ref['full'] else 0) and ref['full'] == (e in truncated), (label, e, int(status[e]), ref['full'])
        got = con[e, :k]
        assert np.array_equal(got[:, 15], [c[0] for c in ref['contacts']]) and np.array_equal(got[:, 16], [c[1] for c in ref['contacts']]), \
            (label, e, got[:, 15:17], [c[:2] for c in ref['contacts']])
        if k:
            pos = np.array([c[2] for c in ref['contacts']]); frames = np.array([contact_frame(c[3]) for c in ref['contacts']])
            ep, ef = np.abs(got[:, :3] - pos).max(), np.abs(got[:, 3:12] - frames).max()
            worst_p, worst_f, compared = max(worst_p, ep), max(worst_f, ef), compared + k
            F = got[:, 3:12].reshape(k, 3, 3)
            eo = np.abs(F @ F.transpose(0, 2, 1) - np.eye(3)).max()
            eh = np.abs(np.cross(F[:, 0], F[:, 1]) - F[:, 2]).max()
            print(f'  {label} env {e}: {k} contacts, pos err {ep:.2e}, frame err {ef:.2e}, orthonormality {eo:.1e}, t2 - n x t1 {eh:.1e}')
            assert ep < POS_TOL and ef < FRAME_TOL, (label, e, ep, ef)
            assert eo < 1e-5 and eh < 1e-5, (label, e, eo, eh)
        if forces and (k == 0 or min(c[4] for c in ref['contacts']) > -0.01):
            shallow.append(e)
            if k:
                fd = oracle.forward_debug(m, q32[e], v32[e])
                assert fd['ncon'] == k
                f = fd['efc_force'][fd['nefc'] - 4*k:fd['nefc']].reshape(-1, 4).sum(1)
                print(f'  {label} env {e}: normal forces {np.round(got[:, 12], 4)} oracle {np.round(f, 4)}')
                assert np.allclose(got[:, 12], f, rtol=2e-2, atol=2e-4), (label, e, got[:, 12], f)
    if shallow:
        ref = oracle.step(m, q32[shallow], v32[shallow])
        ev = relerr(d.qvel.cpu().numpy()[shallow], ref['qvel'])
        print(f'  {label}: qvel relerr {ev:.2e} over envs {shallow}')
        assert ev < 2e-3, (label, ev)
    print(f'NARROW {label} threads_per_env={threads} contacts={compared} worst pos {worst_p:.2e} (bound {POS_TOL}) worst frame {worst_f:.2e} (bound {FRAME_TOL})')
    return worst_p, worst_f, compared


DIRECTED = [(key, t) for key in directed_batches() for t in ((64,) if key in ONE_ENV_ONLY else (32, 64))]


@pytest.mark.parametrize('key,threads', DIRECTED)
def test_directed_cases(oracle, key, threads):
    """The table of directed cases of support_narrow.py, one batch per model, on each kernel that accepts the model."""
    cases = directed_batches()[key]
    m = directed_model(key)
    _, _, compared = _run(oracle, m, [c.qpos for c in cases], threads, f'directed/{key}',
                          exact={e for e, c in enumerate(cases) if c.exact}, truncated={e for e, c in enumerate(cases) if c.truncated})
    assert compared == sum(c.ncon for c in cases)


@pytest.mark.parametrize('i', range(8))
def test_seeded_scenes_two_grounds(oracle, i):
    """A four-shape body over a tilted plane plus a rotated heightfield: the loop over ground entries of the one-env kernel."""
    grounds, geoms, qs = seeded_scenes().two_grounds[i]
    _run(oracle, build_model(grounds, geoms, max_contacts=32), qs, 64, f'seeded/two_grounds/{i}')


@pytest.mark.parametrize('i,threads', [(i, t) for i in range(8) for t in (32, 64)])
def test_seeded_scenes_single_ground(oracle, i, threads):
    """The same bodies and poses over one of the two grounds (plane and heightfield alternating): these reach the two-env kernel."""
    grounds, geoms, qs = seeded_scenes().single[i]
    _run(oracle, build_model(grounds, geoms, max_contacts=32), qs, threads, f'seeded/single/{i}')


@pytest.mark.parametrize('i', range(4))
def test_seeded_scenes_with_a_convex_mesh(oracle, i):
    """A cube given as 8 vertices / a hull of 20, over the tilted plane or the heightfield: the MESH build keeps the deepest four in order."""
    grounds, geoms, qs = seeded_scenes().mesh[i]
    _, _, compared = _run(oracle, build_model(grounds, geoms, max_contacts=32), qs, 64, f'seeded/mesh/{i}')
    assert compared >= 1


@pytest.mark.parametrize('solver,cone', [('newton', 'pyramidal'), ('cg', 'pyramidal'), ('newton', 'elliptic'), ('cg', 'elliptic')])
@pytest.mark.parametrize('i', range(8))
def test_seeded_scenes_other_solvers(oracle, i, solver, cone):
    """The Newton / CG and elliptic instantiations compile the narrow phase on their own: ncon, ids, positions and frames only."""
    grounds, geoms, qs = seeded_scenes().two_grounds[i]
    m = build_model(grounds, geoms, max_contacts=32, solver=solver, cone=cone)
    _run(oracle, m, qs, 64, f'seeded/{solver}-{cone}/{i}', forces=False)
