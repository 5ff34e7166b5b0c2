"""Random trees with collision geoms for the fp64 contact step (test_f64_contact_tree_recipes.py, test_gpu_f64_contact_trees.py): the
twelve WIDE_SHAPES trees of wide_trees.py - free, fixed and hinged / sliding bases, dof chains up to 64, up to 128 bodies and dofs -
under the five kernel families of csrc/fmj_f64_step.inc (contacts, terrain, elliptic, mesh, mesh-elliptic), up to the LDS edge of the
largest model (max_contacts = 128 on the contacts family, 120 on the families built from the terrain text).  Builds on
support_f64_contacts.py, support_f64_terrain.py, support_f64_mesh.py and support_f64_elliptic.py; torch and the GPU modules are imported
inside the functions, so importing this module needs no GPU.

A case is a name of ``CASES``: ``case(name)`` gives its model and inputs, ``conditions`` what the case is about, asserted from the model
and the oracle alone (``CLAIMS`` names the structural facts: which dof chains, waves and welded bodies the contacts with a force sit
on).  The narrow phase is restated in numpy (``geom_candidates``, support_f64_terrain.candidates, support_f64_mesh.candidates) only to
place the ground and to state that no decision grazes.  Every reference value comes from the oracle (Newton, 100 iterations, the
model's tolerance; 1e-10 under the elliptic cone, as in support_f64_elliptic.py)."""
import copy

import numpy as np

import support_f64_contacts as C
import support_f64_terrain as T
import support_f64_elliptic as E
import support_f64_mesh as M
from support_f64_contacts import GEOM_PLANE, GEOM_SPHERE, GEOM_CAPSULE, GEOM_BOX, FMJ_WARN_CONTACTFULL
from support_f64_terrain import GEOM_HFIELD, GEOM_CYLINDER
from support_f64_mesh import GEOM_MESH
from wide_trees import WIDE_SHAPES, shape_tree, dof_depth

N = 4
FAMILIES = ('contacts', 'terrain', 'elliptic', 'mesh', 'mesh_elliptic')
KERNELS = {'contacts': 'fmj_step_f64_contacts_kernel', 'terrain': 'fmj_step_f64_terrain_kernel', 'elliptic': 'fmj_step_f64_elliptic_kernel',
           'mesh': 'fmj_step_f64_mesh_kernel', 'mesh_elliptic': 'fmj_step_f64_mesh_elliptic_kernel'}
GROUND_FRICTION = 0.8
LDS_MAX_CONTACTS = {'contacts': 128, 'terrain': 120, 'elliptic': 120, 'mesh': 120, 'mesh_elliptic': 120}
LDS_BYTES = {'contacts': 163024, 'terrain': 163792}      # shape 1 (128 / 128 / nq 129 / rs 64) at those max_contacts: 48 bytes under 160 KB on terrain
BASE = {s[0]: s[3] for s in WIDE_SHAPES}


# ---- the tree, as the solve reads it ---------------------------------------------------------------------------------------------

def jointed_ancestor(m):
    """Per body: its nearest ancestor-or-self with a dof (0: none), and how many bodies up that is."""
    anc, up = np.zeros(m.nbody, int), np.zeros(m.nbody, int)
    for b in range(1, m.nbody):
        a, k = b, 0
        while a >= 1 and m.body_dofnum[a] == 0:
            a, k = int(m.body_parentid[a]), k + 1
        anc[b], up[b] = max(a, 0), k
    return anc, up


def last_dof(m):
    """Per body: the last dof of its nearest jointed ancestor-or-self (-1: none) - gi[.][2] of the geom table."""
    anc, _ = jointed_ancestor(m)
    return np.array([m.body_dofadr[a] + m.body_dofnum[a] - 1 if a >= 1 else -1 for a in anc])


def chain(m, dof):
    """The dofs from the root to ``dof``, root-most first."""
    out = []
    while dof >= 0:
        out.append(int(dof)); dof = int(m.dof_parentid[dof])
    return out[::-1]


def first_split(m):
    """The number of dofs every dof chain of the tree that reaches past them shares: the trunk before the tree's first branching
    (0: two branches leave a root without dofs; the root body's dofs: two branches leave the root body)."""
    kids = {}
    for d in range(m.nv):
        kids.setdefault(int(m.dof_parentid[d]), []).append(d)
    n, at = 0, -1
    while len(kids.get(at, [])) == 1:
        at = kids[at][0]; n += 1
    return n


def dof_joint(m):
    j = np.zeros(m.nv, int)
    for k in range(m.njnt):
        j[m.jnt_dofadr[k]:m.jnt_dofadr[k] + (6 if m.jnt_type[k] == 0 else 1)] = k
    return j


# ---- models ----------------------------------------------------------------------------------------------------------------------

_HFIELD = {}


def centipede_hfield():
    """The heightfield centipede(terrain='hfield') builds: (data, size)."""
    if not _HFIELD:
        import farms_mujoco_amd.model as mm
        c = mm.centipede(20, 25, contacts=True, terrain='hfield')
        _HFIELD.update(data=np.array(c.hfield_data, float).reshape(c.hfield_nrow, c.hfield_ncol), size=np.array(c.hfield_size, float))
    return _HFIELD['data'], _HFIELD['size']


def _quat(rng):
    q = rng.normal(size=4)
    return tuple(q/np.linalg.norm(q))


def _geom(rng, b, kind=None):
    """One seeded animat geom on body ``b``: off-centre, turned, friction 0.5 .. 1.2."""
    kind = int(rng.integers(0, 3)) if kind is None else kind
    size = ((float(rng.uniform(0.02, 0.04)), 0.0, 0.0), (float(rng.uniform(0.015, 0.03)), float(rng.uniform(0.02, 0.04)), 0.0),
            tuple(rng.uniform(0.02, 0.04, 3)))[kind]
    return ((GEOM_SPHERE, GEOM_CAPSULE, GEOM_BOX)[kind], int(b), size, tuple(rng.normal(size=3)*0.015), _quat(rng), float(rng.uniform(0.5, 1.2)))


def geom_bodies(m, rng, n_bodies):
    """The bodies that carry geoms: the jointed root, the bodies of the deepest dof, three welded bodies whose nearest jointed ancestor
    is at least two bodies up (where the tree has them), two bodies of each of up to four branches that leave the root body beside
    the largest one, then a seeded draw among the bodies with a jointed ancestor, up to ``n_bodies``; in body order."""
    anc, up = jointed_ancestor(m)
    ok = [b for b in range(1, m.nbody) if anc[b] >= 1]
    ld, depth = last_dof(m), dof_depth(m)
    deep = [b for b in ok if depth[ld[b]] == depth.max()]
    trunk = first_split(m)
    branch = {}      # the first dof past the trunk on each body's chain: the branch it sits on
    for b in ok:
        c = chain(m, ld[b])[trunk:]
        if c:
            branch.setdefault(c[0], []).append(b)
    side = sorted(branch.values(), key=len)[:-1][-4:]
    must = ([1] if anc[1] == 1 else []) + deep[:3] + [b for b in ok if up[b] >= 2][:8] + [b for grp in side for b in grp[:2]]
    must = list(dict.fromkeys(must))
    rest = [b for b in ok if b not in must]
    rng.shuffle(rest)
    return sorted(must + rest[:max(0, n_bodies - len(must))]), deep


def lds_room(m, family):
    """The most contacts (up to 128) the family's LDS map holds for this tree within gfx950's 160 KB (support_f64_interface.lds_bytes)."""
    from support_f64_interface import lds_bytes
    rs = 32 if int(dof_depth(m).max()) + 1 <= 32 else 64
    text = 'contacts' if family == 'contacts' else 'terrain'
    return max(k for k in range(1, 129) if lds_bytes(text, m.nbody, m.nv, m.nq, rs, k) <= 160*1024)


def contact_tree(shape,family='contacts', integrator='euler', ground='plane', ground_friction=0.0, limits=False, lds=False, n_bodies=40):
    """WIDE_SHAPES tree ``shape`` with seeded collision geoms (ground first) for ``family``: a mix of spheres, capsules and boxes on
    ``geom_bodies``, a second geom on every fourth of them and on the deepest body; every third sphere a cylinder for the terrain text,
    every second sphere and every second box a mesh for the mesh families.  ``ground``: 'plane' (level, its frame turned about z) or
    'hfield' (centipede_hfield).  ``lds``: geoms on every body, 127 in all, boxes, cylinders and meshes before spheres, and
    max_contacts = LDS_MAX_CONTACTS[family].  ``limits``: ``limited``."""
    import farms_mujoco_amd.model as mm
    assert family in FAMILIES and ground in ('plane', 'hfield') and (ground == 'plane' or family != 'contacts')
    m = shape_tree(shape)
    rng = np.random.default_rng([4040, shape])
    geoms = [(GEOM_PLANE, 0, (0, 0, 0), (0, 0, 0), (np.cos(0.2), 0.0, 0.0, np.sin(0.2)), float(ground_friction))]
    if lds:
        assert m.nbody == 128
        anc, _ = jointed_ancestor(m)
        bodies = [b for b in range(1, m.nbody) if anc[b] >= 1]
        assert len(bodies) == 127
        for b in bodies:      # four-contact geoms on three bodies of four
            geoms.append(_geom(rng, b, kind=2 if b % 4 else int(rng.integers(0, 2))))
    elif m.nbody == 2:      # the smallest model: one sphere, far enough off the joint that the envs' heights differ
        geoms.append((GEOM_SPHERE, 1, (0.03, 0.0, 0.0), (0.05, -0.04, 0.03), _quat(rng), 0.7))
    else:
        bodies, deep = geom_bodies(m, rng, n_bodies)
        for i, b in enumerate(bodies):
            geoms.append(_geom(rng, b))
            if i % 4 == 1 or b in deep:
                geoms.append(_geom(rng, b))
            if b == 1 and m.body_dofnum[1] == 1:      # a hinged or sliding root: three geoms whose last dof it is
                geoms += [_geom(rng, b), _geom(rng, b)]
    C.set_geoms(m, geoms, LDS_MAX_CONTACTS[family] if lds else min(lds_room(m, family), 4*(len(geoms) - 1)))
    m.nmeshvert = 0
    if family != 'contacts':
        sph = T.spheres(m)
        if family == 'terrain' or (lds and family == 'elliptic'):
            T.cylinders(m, sph[::2] if not lds else sph)
        if family in ('mesh', 'mesh_elliptic'):
            vs = M.vertex_sets()
            order = ('hull12', 'hull42', 'tetrahedron', 'triangle', 'vertex')
            boxes = np.nonzero(m.geom_type == GEOM_BOX)[0]
            which = list(sph[::2]) + list(boxes[1::2])
            M.meshes(m, which, [vs[order[i % 5]] for i in range(len(which))])
        if ground == 'hfield':
            data, size = centipede_hfield()
            m.geom_type = m.geom_type.copy(); m.geom_type[0] = GEOM_HFIELD
            m.hfield_data = data.copy(); m.hfield_nrow, m.hfield_ncol = data.shape; m.hfield_size = size.copy()
    if family in ('elliptic', 'mesh_elliptic'):
        m.cone = mm.CONES['elliptic']; m.impratio = 4.0; m.solver_tolerance = E.TOLERANCE
    m.integrator = mm.INTEGRATORS[integrator]
    m.solver = mm.SOLVERS['newton']; m.solver_iterations = 100
    if limits:
        limited(m)
    return m


def limited(m, lim=0.1, margin_even=0.02):
    """A seeded third of the scalar joints limited to the key pose +-lim, ``margin_even`` on the even joints (support_limits.limited's
    ranges, about the key pose)."""
    rng = np.random.default_rng([4141, m.nv])
    sj = np.nonzero(m.jnt_type != 0)[0]
    on = np.zeros(m.njnt, bool); on[rng.choice(sj, size=max(3, len(sj)//3), replace=False)] = True
    m.jnt_limited = on.astype(m.jnt_limited.dtype)
    key = np.array([m.key_qpos[m.jnt_qposadr[j]] if m.jnt_type[j] != 0 else 0.0 for j in range(m.njnt)])
    m.jnt_range = np.stack([key - lim, key + lim], axis=1)
    margin = np.zeros(m.njnt); margin[::2] = margin_even
    m.jnt_margin = margin
    return m


def flags_of(m, family):
    lim = C.LIMITS if np.any(m.jnt_limited) else 0
    if family in ('mesh', 'mesh_elliptic'):
        return M.flags_of(m)
    return C.CONTACTS | lim | {'contacts': 0, 'terrain': T.TERRAIN, 'elliptic': E.ELLIPTIC | T.TERRAIN}[family]


def phys(m, n, ins, family, **kw):
    if family in ('mesh', 'mesh_elliptic'):
        return M.phys(m, n, ins, **kw)
    return C.phys(m, n, ins, **dict(dict(fp64_terrain=family != 'contacts', fp64_elliptic=family == 'elliptic'), **kw))


# ---- inputs ----------------------------------------------------------------------------------------------------------------------

def geom_candidates(m, qpos):
    """Per animat geom of one env over ground geom 0: (geom, the distances the narrow phase compares with 0, the most contacts it
    makes).  A cylinder's are its four rim points', a mesh's its vertices' (support_f64_terrain.candidates, support_f64_mesh.mesh_candidates)."""
    from farms_mujoco_amd.model import np_kinematics, quat2mat, quat_mul
    kin = np_kinematics(m, qpos)
    out = []
    for g in range(m.ngeom):
        t, b = int(m.geom_type[g]), int(m.geom_bodyid[g])
        if t in (GEOM_PLANE, GEOM_HFIELD):
            continue
        gp = kin['xpos'][b] + quat2mat(kin['xquat'][b]) @ m.geom_pos[g]
        gm = quat2mat(quat_mul(kin['xquat'][b], m.geom_quat[g])); s = m.geom_size[g]
        if t == GEOM_SPHERE:
            pts, off, cap = [gp], s[0], 1
        elif t == GEOM_CAPSULE:
            pts, off, cap = [gp + s[1]*gm[:, 2], gp - s[1]*gm[:, 2]], s[0], 2
        elif t == GEOM_BOX:
            pts, off, cap = [gp + gm @ (np.array([sx, sy, sz])*s) for sz in (-1, 1) for sy in (-1, 1) for sx in (-1, 1)], 0.0, 4
        elif t == GEOM_MESH:
            V = m.mesh_vert[m.geom_vertadr[g]:m.geom_vertadr[g] + m.geom_vertnum[g]]
            pts, off, cap = [gp + gm @ v for v in V], 0.0, 4
        else:      # a cylinder: the bounding box of its rim along the ground's normal at its centre
            assert t == GEOM_CYLINDER, t
            dist, n, _ = T.ground_dist(m, 0, gp)
            a = abs(n @ gm[:, 2]); reach = s[1]*a + s[0]*np.sqrt(max(0.0, 1 - a*a))
            out.append((g, np.array([dist - reach, dist - reach + 1e-3, dist - reach + 2e-3]), 3))
            continue
        out.append((g, np.array([T.ground_dist(m, 0, pt)[0] - off for pt in pts]), cap))
    return out


def _shift(cands, share=None, count=None):
    """How far the ground has to rise (or the root to sink) so that ``share`` of the geoms have a point below it, or so that about
    ``count`` contacts are made: halfway between two candidate distances."""
    lows = np.sort([d.min() for _, d, _ in cands if np.isfinite(d.min())])
    if count is None:
        k = min(len(lows) - 1, max(1, int(round(share*len(lows)))))
        return 0.5*(lows[k - 1] + lows[k])
    alld = np.sort(np.concatenate([d[np.isfinite(d)] for _, d, _ in cands]))
    made = lambda k: sum(min(cap, int((d < 0.5*(alld[k - 1] + alld[k])).sum())) for _, d, cap in cands)
    lo, hi = 1, len(alld) - 1      # the least k whose level makes ``count`` contacts (the number made grows with the level)
    assert made(hi) >= count, 'the geoms cannot make that many contacts'
    while lo < hi:
        mid = (lo + hi)//2
        lo, hi = (lo, mid) if made(mid) >= count else (mid + 1, hi)
    return 0.5*(alld[lo - 1] + alld[lo])


def inputs(m, n, seed, share=0.3, counts=None, spread=0.15, tilt=0.3, repeat=None):
    """Scalar joints at the key pose +-``spread`` (three joints of a limited model per env at or past their upper limit), qvel normal x
    0.3, ctrl uniform +-0.3, rounded to fp32.  A free base is turned by up to ``tilt`` and lowered per env until ``share`` of the geoms
    have a point below the ground (``counts``: until env e makes about counts[e] contacts).  Under a fixed or hinged base the ground
    geom is placed instead (m.geom_pos[0] is set): one height for the batch, the highest of the envs' ``share`` levels, so that every
    env has at least that share of its geoms below the ground (a model with one geom: the ``share`` quantile of the envs' heights, so
    that some envs touch and some do not).  ``repeat`` = (a, b): env a repeats env b's inputs."""
    from farms_mujoco_amd.model import quat_mul
    rng = np.random.default_rng([779, seed])
    qpos = np.tile(m.key_qpos, (n, 1)).astype(float)
    sq = C.scalar_q(m)
    qpos[:, sq] += rng.uniform(-spread, spread, (n, len(sq)))
    if np.any(m.jnt_limited):
        lim = np.nonzero(m.jnt_limited)[0]
        for e in range(n):
            for j in rng.choice(lim, size=3, replace=False):
                qpos[e, m.jnt_qposadr[j]] = m.jnt_range[j][1] + rng.uniform(-0.005, 0.03)
    r = lambda a: np.asarray(a, np.float64).astype(np.float32).astype(np.float64)
    free = m.jnt_type[0] == 0
    m.geom_pos = m.geom_pos.copy(); m.geom_pos[0] = 0.0
    hfield = m.geom_type[0] == GEOM_HFIELD
    if free:
        for e in range(n):
            ax = rng.normal(size=3); ax /= np.linalg.norm(ax); ang = rng.uniform(-tilt, tilt)
            q = quat_mul(np.array([np.cos(ang/2), *(np.sin(ang/2)*ax)]), qpos[e, 3:7])
            qpos[e, 3:7] = q/np.linalg.norm(q)
            qpos[e, :2] = rng.uniform(-0.05, 0.05, 2)
            qpos[e, 2] = 1.0
            for _ in range(4 if hfield else 1):
                qpos[e, 2] -= _shift(geom_candidates(m, qpos[e]), share, None if counts is None else counts[e])
        qpos = r(qpos)
    else:
        qpos = r(qpos)
        z = 0.0
        single = int(np.isin(m.geom_type, (GEOM_PLANE, GEOM_HFIELD)).sum()) == m.ngeom - 1
        for _ in range(4 if hfield else 1):
            m.geom_pos[0, 2] = z
            per_env = [geom_candidates(m, qpos[e]) for e in range(n)]
            if single:      # one geom: the ground between the envs' heights
                z += float(np.quantile([c[0][1].min() for c in per_env], share))
            else:           # the highest of the envs' levels: every env has its share below the ground
                z += max(_shift(c, share) for c in per_env)
        m.geom_pos[0, 2] = z
    qvel = rng.normal(size=(n, m.nv))*0.3
    ctrl = rng.uniform(-0.3, 0.3, (n, max(m.nu, 1)))[:, :m.nu]
    ins = dict(qpos=qpos, qvel=r(qvel), ctrl=r(ctrl) if m.nu else None)
    if repeat is not None:
        a, b = repeat
        for k in ('qpos', 'qvel', 'ctrl'):
            if ins[k] is not None:
                ins[k][a] = ins[k][b]
    return ins


# ---- the cases -------------------------------------------------------------------------------------------------------------------

# name: (shape, family, integrator, what it is about).  What: 'hfield' (the heightfield ground), 'mu' (the ground's friction 0.8),
# 'limits', 'lds' (the LDS edge), 'n5' (five envs, the fifth repeats the second)
CASES = {}
for _s in range(1, 13):
    CASES['contacts-%d' % _s] = (_s, 'contacts', 'euler' if _s % 2 else 'implicitfast', {3: 'n5', 7: 'mu'}.get(_s, ''))
for _f, _about in (('terrain', {1: 'hfield', 4: 'n5', 7: 'hfield'}), ('elliptic', {3: 'mu'}), ('mesh', {4: 'hfield'}), ('mesh_elliptic', {7: 'mu'})):
    for _i, _s in enumerate((1, 3, 4, 7)):
        CASES['%s-%d' % (_f, _s)] = (_s, _f, 'implicitfast' if _i % 2 else 'euler', _about.get(_s, ''))
for _s in (1, 4, 10):
    CASES['contacts-%d-limits' % _s] = (_s, 'contacts', 'euler', 'limits')
    CASES['terrain-%d-limits' % _s] = (_s, 'terrain', 'implicitfast', 'limits')
for _f in FAMILIES:
    CASES['lds-%s' % _f] = (1, _f, 'euler', 'lds')
TRUNCATED = 'lds-contacts'      # the truncation case: its model with inputs whose full list is longer than max_contacts
# per env of the LDS cases: about how many contacts the root is lowered to (the list past 64 everywhere, full to within 8 in one env)
LDS_COUNTS = lambda maxc: [70, maxc - 3, 90, maxc - 20, 80]
TRUNCATED_COUNTS = [150, 140, 160, 135]

# the structural facts a case must show on a contact with a normal force (somewhere in the batch unless said otherwise):
#   depthD: the geom's last dof has depth D;  dof64 / body64 / slot64: its last dof, its body, its slot in the list is >= 64;
#   lane64: an animat geom on lane >= 64 has a contact;  slide: a slide joint on its chain;  root_last: the hinged / sliding root is
#   its last dof;  welded2: on a welded body whose nearest jointed ancestor is at least two bodies up;  free_root: on the free root body;
#   shared6 / disjoint (per tree of 64 bodies or more): two contacts of one env whose chains share at least six dofs and then
#   split; two whose chains split at the tree's first branching (first_split: they share the trunk every chain shares and nothing
#   else - nothing below the root body where two branches leave it);  cyl / mesh: on a cylinder, on a mesh geom
CLAIMS = {
    'contacts-1': ('depth63', 'dof64', 'body64', 'free_root'), 'contacts-2': ('depth32', 'dof64', 'body64'), 'contacts-3': ('depth31', 'dof64', 'body64'),
    'contacts-4': ('dof64', 'body64', 'slide', 'root_last'), 'contacts-5': ('body64', 'root_last'), 'contacts-6': ('dof64',),
    'contacts-7': ('body64', 'welded2'), 'contacts-8': ('depth63', 'dof64', 'body64'), 'contacts-9': ('body64',), 'contacts-10': ('slide',),
    'lds-contacts': ('slot64', 'lane64', 'dof64', 'body64', 'depth63'),
}
for _n, (_s, _f, _i, _w) in CASES.items():
    c = list(CLAIMS.get(_n, ()))
    if _s <= 10:
        c += ['shared6', 'disjoint']
    if _f == 'terrain':
        c.append('cyl')
    if _f in ('mesh', 'mesh_elliptic'):
        c.append('mesh')
    if _w == 'lds' and _n != 'lds-contacts':
        c += ['slot64', 'lane64']
    if _s == 7 and 'welded2' not in c:
        c.append('welded2')
    CLAIMS[_n] = tuple(dict.fromkeys(c))

# the seed of each case's inputs: the first of 100, 101, ... at which `conditions` holds (first_seed finds them;
# test_f64_contact_tree_recipes.py asserts the conditions at them, and every GPU case again before it looks at the device)
SEEDS = dict({n: 100 for n in CASES}, **{'contacts-2': 107, 'contacts-4': 111, 'contacts-5': 107, 'contacts-9': 102, 'contacts-10-limits': 102})
NOT_THE_FIRST_TRIED = ('contacts-2', 'contacts-4', 'contacts-5', 'contacts-9', 'contacts-10-limits')
# the input recipe of a case where it is not the default of `inputs` (none had to change: every case finds a seed among the first 12)
RECIPES = {}


def envs_of(name):
    return 5 if CASES[name][3] == 'n5' else N


def make(name):
    shape, family, integrator, what = CASES[name]
    return contact_tree(shape, family, integrator, ground='hfield' if what == 'hfield' else 'plane',
                        ground_friction=GROUND_FRICTION if what == 'mu' else 0.0, limits=what == 'limits', lds=what == 'lds',
                        **({'n_bodies': 1} if shape == 11 else {}))


def case_inputs(name, m, seed=None):
    shape, family, _, what = CASES[name]
    n = envs_of(name)
    kw = dict(RECIPES.get(name, {}))
    if what == 'lds':
        kw['counts'] = LDS_COUNTS(m.max_contacts)[:n]
    if shape == 11:
        kw.setdefault('share', 0.5)
    return inputs(m, n, SEEDS[name] if seed is None else seed, repeat=(4, 1) if n == 5 else None, **kw)


def case(name, seed=None):
    m = make(name)
    return m, case_inputs(name, m, seed), CASES[name][1]


# ---- conditions ------------------------------------------------------------------------------------------------------------------

def forced_contacts(m, ref):
    """Per env: the oracle's contacts with a normal force as (slot, geom, body, last dof)."""
    ld = last_dof(m)
    out = []
    for e in range(len(ref['ncon'])):
        k = int(ref['ncon'][e])
        out.append([(c, int(ref['geoms'][e, c, 1]), int(m.geom_bodyid[ref['geoms'][e, c, 1]]), int(ld[m.geom_bodyid[ref['geoms'][e, c, 1]]]))
                    for c in range(k) if ref['contact'][e, c, 12] > 0])
    return out


def structure(m, ref):
    """The structural facts of CLAIMS that the model and the oracle's records show: {claim: bool}, and the depths of the last dofs of
    the contacts with a force."""
    depth = dof_depth(m)
    anc, up = jointed_ancestor(m)
    fc = forced_contacts(m, ref)
    every = [x for env in fc for x in env]
    jof = dof_joint(m)
    trunk = first_split(m)
    depths = sorted({int(depth[ld]) for _, _, _, ld in every})
    said = {'depth%d' % d: True for d in depths}
    said['dof64'] = any(ld >= 64 for _, _, _, ld in every)
    said['body64'] = any(b >= 64 for _, _, b, _ in every)
    said['slot64'] = any(c >= 64 for c, _, _, _ in every)
    said['lane64'] = any(int(ref['geoms'][e, c, 1]) >= 64 for e in range(len(ref['ncon'])) for c in range(int(ref['ncon'][e])))
    said['slide'] = any(m.jnt_type[jof[d]] == 2 for _, _, _, ld in every for d in chain(m, ld))
    said['root_last'] = bool(m.body_dofnum[1] == 1) and any(ld == m.body_dofadr[1] for _, _, _, ld in every)
    said['welded2'] = any(up[b] >= 2 for _, _, b, _ in every)
    said['free_root'] = bool(m.body_dofnum[1] == 6) and any(b == 1 for _, _, b, _ in every)
    said['cyl'] = any(m.geom_type[g] == GEOM_CYLINDER for _, g, _, _ in every)
    said['mesh'] = any(m.geom_type[g] == GEOM_MESH for _, g, _, _ in every)
    shared6 = disjoint = False
    for env in fc:
        chains = [set(chain(m, ld)) for ld in sorted({x[3] for x in env})]
        for i in range(len(chains)):
            for j in range(i + 1, len(chains)):
                a, b = chains[i], chains[j]
                if not (a - b) or not (b - a):
                    continue      # one chain is the start of the other: they do not split
                shared6 = shared6 or len(a & b) >= 6
                disjoint = disjoint or len(a & b) == trunk
    said['shared6'], said['disjoint'] = shared6, disjoint
    return said, depths


def limit_rows_on_contact_chains(m, ref):
    """Per env: the oracle's limit rows with a force whose joint lies on the dof chain of a contact with a force."""
    rows = 3 if int(getattr(m, 'cone', 0)) == 1 else 4
    jof = dof_joint(m)
    fc = forced_contacts(m, ref)
    out = np.zeros(len(ref['ncon']), int)
    for e in range(len(ref['ncon'])):
        on = {int(jof[d]) for _, _, _, ld in fc[e] for d in chain(m, ld)}
        nlim = int(ref['nefc'][e] - rows*ref['ncon'][e])
        out[e] = sum(1 for i in range(nlim) if ref['efc'][e, i, 0] > 0 and int(ref['efc'][e, i, 5]) in on)
    return out


def clear(m, ins, eps=1e-9):
    """No narrow-phase distance, grid margin, depth gap between two vertices of a mesh geom or bounding-radius margin within ``eps``."""
    for q in ins['qpos']:
        d, cells = M.candidates(m, q) if np.any(m.geom_type == GEOM_MESH) else T.candidates(m, q)
        if np.abs(d).min() <= eps or cells.min() <= eps:
            return False
        if np.any(m.geom_type == GEOM_MESH):
            for rec in M.mesh_candidates(m, q):
                pen = np.sort(rec['td'][rec['td'] < 0])
                if (len(pen) > 1 and np.diff(pen).min() <= eps) or abs(rec['origin'] - rec['radius']) <= eps:
                    return False
    return True


def moved_by_a_tighter_tolerance(oracle, m, ins, ref):
    """How far a 100 x tighter tolerance with 200 iterations moves the reference, per field, in one-step bounds; ncon must not change."""
    return E.moved_by_a_tighter_tolerance(oracle, m, ins, ref)


def try_reference(oracle, m, ins):
    a = oracle.step(m, ins['qpos'], ins['qvel'], ctrl=ins['ctrl'])
    return None if a['status'].any() else C.reference(oracle, m, ins)


def conditions(oracle, name, m, ins, converged=True):
    """What the case ``name`` is about, from the model and the oracle alone; returns (ok, the reference, a description)."""
    shape, family, _, what = CASES[name]
    ref = try_reference(oracle, m, ins)
    if ref is None:
        return False, None, dict(status='the oracle reports a status')
    n = len(ref['ncon'])
    ncon = ref['ncon']
    forced = np.array([(ref['contact'][e, :ncon[e], 12] > 0).sum() for e in range(n)]); idle = ncon - forced
    mind = np.array([np.abs(ref['dist'][e, :ncon[e]]).min() if ncon[e] else np.inf for e in range(n)])
    said = dict(ncon=ncon, forced=forced, idle=idle, min_abs_dist=mind, iterations=ref['iterations'])
    free = BASE[shape] == 'free'
    if shape == 11:      # one body, one dof, one sphere: envs with and without the contact in one batch
        ok = bool((forced == 1).sum() >= 2 and (ncon == 0).sum() >= 1 and ncon.max() == 1)
    elif shape == 12:
        ok = bool(forced.min() >= 2 and idle.min() >= 1)
    else:
        ok = bool(forced.min() >= 4 and (idle.min() >= 1 if free else idle.sum() >= 1))
    ok = ok and bool(mind.min() > 1e-9) and bool(ref['iterations'].max() < m.solver_iterations) and clear(m, ins)
    facts, depths = structure(m, ref)
    said.update(depths_of_last_dofs=depths, claims={k: bool(facts.get(k, False)) for k in CLAIMS[name]})
    ok = ok and all(facts.get(k, False) for k in CLAIMS[name])
    if family in ('elliptic', 'mesh_elliptic'):      # no contact within a relative 1e-3 of its cone's surface without being on it
        nearest = E.zones(m, ref)[3]
        said['nearest_inside'] = nearest
        ok = ok and bool(nearest.min() > 1e-3)
    if what == 'limits':
        on = limit_rows_on_contact_chains(m, ref)
        said['limit_rows_with_force_on_contact_chains'] = on
        ok = ok and bool(on.min() >= 1)
    if what == 'hfield':      # all contacts lie on the heightfield (the only ground): their normals differ
        nrm = np.concatenate([ref['contact'][e, :ncon[e], 3:6][ref['contact'][e, :ncon[e], 12] > 0] for e in range(n)])
        said['normal_spread'] = (nrm.max(axis=0) - nrm.min(axis=0)).max()
        ok = ok and bool(said['normal_spread'] > 1e-3) and m.geom_type[0] == GEOM_HFIELD and T.grounds(m) == [0]
    if what == 'mu':
        wins = sum(1 for e in range(n) for c, g, _, _ in forced_contacts(m, ref)[e] if m.geom_friction[g, 0] < GROUND_FRICTION)
        said['ground_friction_wins'] = wins
        ok = ok and wins >= 1
    if what == 'lds':
        ok = ok and bool(ncon.min() > 64 and m.max_contacts - 8 <= ncon.max() <= m.max_contacts)
    if ok and converged:
        moved = moved_by_a_tighter_tolerance(oracle, m, ins, ref)
        said['moved_by_a_tighter_tolerance'] = {k: round(v, 5) for k, v in moved.items()}
        ok = max(moved.values()) <= 0.1
    return ok, ref, said


def first_seed(oracle, name, start=100, tries=60):
    m = make(name)
    for seed in range(start, start + tries):
        if conditions(oracle, name, m, case_inputs(name, m, seed))[0]:
            return seed
    raise AssertionError('no seed satisfies the conditions')


# ---- the truncated list, the trajectories, the tree above the ground ---------------------------------------------------------------

def truncated_case(seed=100):
    """The model of ``TRUNCATED`` with every env lowered until its full list is longer than max_contacts; returns (m, ins, family)."""
    m = make(TRUNCATED)
    return m, inputs(m, N, seed, counts=TRUNCATED_COUNTS), CASES[TRUNCATED][1]


def full_list(oracle, m, ins, room=256):
    """The oracle's step of a model copy with room for the whole list."""
    full = copy.copy(m); full.max_contacts = room
    return C.reference(oracle, full, ins)


TRAJECTORIES = {'contacts-3': 100, 'contacts-4': 100}      # the fixed-base and the hinged-base case the 60-step test runs, and their seeds
TRAJECTORY_STEPS = 60


def trajectory_case(name):
    """The model, initial state (at rest, at the case's inputs' pose) and ctrl tape of one trajectory case."""
    import support_limits as L
    m = make(name)
    ins = inputs(m, N, TRAJECTORIES[name], **RECIPES.get(name, {}))
    tape32 = L.tape(m, N, TRAJECTORY_STEPS, f=3.0)
    return m, ins['qpos'], np.zeros((N, m.nv)), tape32


def share_of_steps_with_a_force(oracle, m, q0, v0, tape):
    """Per env, from a step-by-step oracle run (the warm start carried as mj_step carries it): the share of steps with a contact force."""
    q, v, ws = q0, v0, None
    n = len(q0)
    with_force = np.zeros(n)
    for t in range(len(tape)):
        o = oracle.step_tf(m, q, v, ctrl=tape[t], warmstart=ws, want_AR=False)
        assert not o['status'].any(), (t, o['status'])
        with_force += np.array([(o['contact'][e, :o['ncon'][e], 12] > 0).any() for e in range(n)])
        q, v, ws = o['qpos'], o['qvel'], o['warmstart']
    return with_force/len(tape)


def lifted(shape=3, gap=1.0):
    """The contacts-family tree of ``shape`` with the plane ``gap`` below its lowest geom point over the batch, and the same tree
    without geoms; returns (with, without, ins)."""
    a, b = contact_tree(shape), contact_tree(shape)
    C.set_geoms(b, [], 0)
    ins = inputs(a, N, 5)
    low = min(d.min() for e in range(N) for _, d, _ in geom_candidates(a, ins['qpos'][e]))      # (the ground now passes through the geoms)
    a.geom_pos[0, 2] += low - gap
    assert min(d.min() for e in range(N) for _, d, _ in geom_candidates(a, ins['qpos'][e])) > 0.99*gap
    return a, b, ins
