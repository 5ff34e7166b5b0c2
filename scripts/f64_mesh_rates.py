"""Rate (env-steps/s) of the fp64 contact solve with convex mesh feet (fp64_contacts=True, fp64_mesh=True: fmj_step_f64_mesh_kernel /
fmj_step_f64_mesh_elliptic_kernel of csrc/fmj_f64_step.inc) on 4096 envs, fmj_step in launches of 100 steps under a ctrl tape.  The
walking centipede(20, 25) on its plane (the tape of scripts/f64_contacts_rates.py), per cone:
  with its sphere feet through the terrain kernel (the elliptic kernel) - the same narrow phase without a vertex loop;
  with all 40 feet the irregular 12-vertex hull through the mesh kernel (the mesh-elliptic kernel);
  with all 40 feet the irregular 42-vertex hull;
  with all 40 feet the 12-vertex hull plus 30 vertices of the 42-vertex hull at a tenth of their radius, which never touch the
  ground: the contacts of the 12-vertex run with the vertex loop of the 42-vertex run, so the difference to the 12-vertex run is the
  cost of 30 more vertices in the loop and nothing else.
The hulls are the irregular ones of tests/support_f64_mesh.py, built here the same way: an icosahedron, or the 42 vertices of its
first subdivision, each vertex's radius scaled by a seeded factor in [0.8, 1], times the foot sphere's radius.
usage: python scripts/f64_mesh_rates.py [n_envs] [samples] [repeats] [pyramidal|elliptic]

The four runs are sampled in turn, ``samples`` times (default 5) after two warm-up passes each; the whole measurement is repeated
``repeats`` times (default 3) on fresh contexts.  Printed per repeat: the median rate of each run, its spread (min .. max over the
samples), the mean contacts per env at the end and each run's ratio to the first; then the spread of the medians over the repeats."""
import sys

import numpy as np

from f64_rates_common import context, tape_of, centipede_stance, sample, stepping, over_repeats


def hull(nvert):
    """The irregular 12- or 42-vertex hull at unit scale."""
    f = (1 + np.sqrt(5))/2
    v = [(0, s1, s2*f) for s1 in (-1, 1) for s2 in (-1, 1)]
    v = np.array(v + [(b, c, a) for a, b, c in v] + [(c, a, b) for a, b, c in v], float)
    v /= np.linalg.norm(v, axis=1, keepdims=True)
    if nvert == 42:
        d = np.linalg.norm(v[:, None] - v[None], axis=2)
        edge = d[d > 1e-9].min()
        mids = np.array([(v[i] + v[j])/2 for i in range(12) for j in range(i + 1, 12) if abs(d[i, j] - edge) < 1e-9])
        v = np.concatenate([v, mids/np.linalg.norm(mids, axis=1, keepdims=True)])
    assert len(v) == nvert
    return v*np.random.default_rng([4711, nvert]).uniform(0.8, 1.0, (nvert, 1))


def mesh_feet(w, verts):
    """Every sphere geom of ``w`` becomes a mesh geom of ``verts`` times its radius (include/fmj.h: mesh_vert, geom_vertadr,
    geom_vertnum; geom_size[2] is the bounding radius)."""
    feet = np.nonzero(w.geom_type == 2)[0]
    w.geom_type = w.geom_type.copy(); w.geom_size = w.geom_size.copy()
    w.geom_vertadr = np.full(w.ngeom, -1, np.int32); w.geom_vertnum = np.zeros(w.ngeom, np.int32)
    all_verts = []
    for i, g in enumerate(feet):
        v = verts*w.geom_size[g, 0]
        w.geom_type[g] = 7; w.geom_size[g] = (0.0, 0.0, np.linalg.norm(v, axis=1).max())
        w.geom_vertadr[g] = i*len(verts); w.geom_vertnum[g] = len(verts)
        all_verts.append(v)
    w.mesh_vert = np.concatenate(all_verts); w.nmeshvert = len(w.mesh_vert)
    return w


def centipede_runs(n, chunk, cone):
    import farms_mujoco_amd.model as mm
    elliptic = cone == 'elliptic'

    def walker(verts=None):
        w = mm.centipede(20, 25, contacts=True)
        if verts is not None:
            mesh_feet(w, verts)
        w.max_contacts = 120
        w.solver = mm.SOLVERS['newton']; w.solver_iterations = 100
        w.cone = mm.CONES[cone]
        return w
    w = walker()
    amp, lag = mm.wave_controller_params(w, amplitude=0.1)
    stance = centipede_stance(w)
    runs = {}
    padded = np.concatenate([hull(12), 0.1*hull(42)[12:]])
    for key, verts in (('sphere feet', None), ('12-vertex hulls', hull(12)), ('42-vertex hulls', hull(42)), ('12 + 30 interior vertices', padded)):
        p, psi = context(walker(verts), n, precision='fp64', fp64_contacts=True, fp64_terrain=True, fp64_elliptic=elliptic, fp64_mesh=True)
        want = ('fmj_step_f64_mesh_elliptic_kernel' if elliptic else 'fmj_step_f64_mesh_kernel') if verts is not None else \
               ('fmj_step_f64_elliptic_kernel' if elliptic else 'fmj_step_f64_terrain_kernel')
        assert p.kernel_info()['fp64_step_kernel'] == want
        runs[key] = (p, tape_of(w, psi, amp, lag, chunk, stance))
    return w, runs


def rates(name, n, samples, cone, chunk=100):
    m, runs = centipede_runs(n, chunk, cone)
    out = sample(stepping(runs, chunk), n, chunk, samples, warmup=2)      # (the animal settles on the ground)
    for phys, _ in runs.values():
        assert int((phys.data.status & 7).abs().sum()) == 0      # (a full contact list is reported, not an error)
    med = {k: float(np.median(v)) for k, v in out.items()}
    ncon = {k: float(p.data.ncon.float().mean()) for k, (p, _) in runs.items()}
    first = list(runs)[0]
    print(f'{name} nbody {m.nbody} nv {m.nv} envs {n}: ' +
          '; '.join(f'{k} {med[k]/1e6:.4f} M env-steps/s ({min(v)/1e6:.4f} .. {max(v)/1e6:.4f}), {ncon[k]:.1f} contacts per env, '
                    f'{med[k]/med[first]:.3f} of the first' for k, v in out.items()), flush=True)
    return med


if __name__ == '__main__':
    n = int(sys.argv[1]) if len(sys.argv) > 1 else 4096
    samples = int(sys.argv[2]) if len(sys.argv) > 2 else 5
    repeats = int(sys.argv[3]) if len(sys.argv) > 3 else 3
    for cone in ([sys.argv[4]] if len(sys.argv) > 4 else ['pyramidal', 'elliptic']):
        name = f'centipede(20, 25) walking, {cone} cone'
        over_repeats(name, lambda: rates(name, n, samples, cone), repeats, 4)
