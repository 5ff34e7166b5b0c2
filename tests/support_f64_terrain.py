"""Models, inputs and oracle-side conditions that the fp64 terrain tests share (test_f64_terrain_interface.py, test_gpu_f64_terrain.py):
heightfield ground and cylinder geoms on the fp64 contact solve (FMJ_CREATE_F64_CONTACTS | FMJ_CREATE_F64_TERRAIN).  Builds on
support_f64_contacts.py (the oracle read-outs, the flat-ground models, the context helper); torch and the GPU modules are imported
inside the functions, so importing this module needs no GPU.

The narrow phase is restated here in numpy (``ground_dist``, ``candidates``: oracle ground_dist / collide_plane's candidate points) for
two things only: to lower the root until the deepest candidate point is a given depth below the ground, and to state that no decision
of the narrow phase grazes - no candidate within 1e-9 m of the surface, none within 1e-9 grid units of a cell edge, the cell diagonal
or the grid border.  Every reference value comes from the oracle."""
import numpy as np

from support_f64_contacts import (N, CONTACTS, LIMITS, GEOM_PLANE, GEOM_SPHERE, GEOM_CAPSULE, GEOM_BOX, MODEL_INPUTS, boxfoot, scalar_q,
                                  reference, engaged, phys as _contacts_phys)

GEOM_HFIELD, GEOM_CYLINDER = 1, 5
TERRAIN = 128      # FMJ_CREATE_F64_TERRAIN
MODELS = ('salamander_hfield_cyl', 'centipede_hfield_cyl', 'boxfoot_hfield', 'salamander_tilted_cyl')
# the seed of each model's inputs: the first of 100, 101, ... at which `conditions` holds in every env (first_seed finds them; the tests
# assert the conditions before they look at the device)
SEEDS = {'salamander_hfield_cyl': 110, 'centipede_hfield_cyl': 100, 'boxfoot_hfield': 123, 'salamander_tilted_cyl': 151}


def cylinders(m, which):
    """Turn the sphere geoms ``which`` into cylinders about their geom's z axis: the sphere's radius, half-length 0.8 x radius."""
    m.geom_type = m.geom_type.copy(); m.geom_size = m.geom_size.copy()
    for g in which:
        assert m.geom_type[g] == GEOM_SPHERE
        m.geom_type[g] = GEOM_CYLINDER
        m.geom_size[g] = (m.geom_size[g, 0], 0.8*m.geom_size[g, 0], 0.0)
    return m


def spheres(m):
    return np.nonzero(m.geom_type == GEOM_SPHERE)[0]


def boxfoot_hfield():
    """support_f64_contacts.boxfoot with its plane replaced by a rolling heightfield: +-5 cm over an 8 m x 8 m patch of 33 x 33
    samples, the frame turned about z as the plane's was."""
    m = boxfoot()
    assert m.geom_type[0] == GEOM_PLANE
    m.geom_type = m.geom_type.copy(); m.geom_type[0] = GEOM_HFIELD
    gy, gx = np.meshgrid(np.linspace(-4, 4, 33), np.linspace(-4, 4, 33), indexing='ij')
    m.hfield_data = 0.5*np.sin(1.9*gx)*np.cos(1.3*gy)
    m.hfield_nrow, m.hfield_ncol = m.hfield_data.shape
    m.hfield_size = np.array([4.0, 4.0, 0.1, 0.1])
    return m


def make(name, integrator='euler'):
    """The model of ``name`` with the reference's solver fields: Newton, 100 iterations."""
    import farms_mujoco_amd.model as mm
    if name == 'salamander_hfield_cyl':      # every second sphere a cylinder
        m = mm.salamander33(contacts=True, limits=True, terrain='hfield')
        cylinders(m, spheres(m)[::2])
    elif name == 'centipede_hfield_cyl':     # every second foot a cylinder
        m = mm.centipede(20, 25, contacts=True, terrain='hfield')
        cylinders(m, spheres(m)[::2])
    elif name == 'centipede_hfield':
        m = mm.centipede(20, 25, contacts=True, terrain='hfield')
    elif name == 'boxfoot_hfield':
        m = boxfoot_hfield()
    elif name == 'salamander_tilted_cyl':    # a plane tilted by 0.12 rad about (1, 1, 0), every sphere a cylinder: no heightfield
        m = mm.salamander33(contacts=True, limits=True)
        p = int(np.nonzero(m.geom_type == GEOM_PLANE)[0][0])
        m.geom_quat = m.geom_quat.copy(); m.geom_quat[p] = mm.axisangle2quat(np.array([1.0, 1.0, 0.0])/np.sqrt(2.0), 0.12)
        cylinders(m, spheres(m))
    else:
        raise KeyError(name)
    if name.startswith('salamander'):
        m.max_contacts = 64      # a cylinder makes up to four contacts where a sphere made one
    m.integrator = mm.INTEGRATORS[integrator]
    m.solver = mm.SOLVERS['newton']; m.solver_iterations = 100
    return m


# how far the deepest candidate point is pushed below the ground under it (m): support_f64_contacts.MODEL_INPUTS' depths, the
# centipede's with the heightfield's 2 mm amplitude added (the ground under most of its feet is lower than under the deepest)
DEPTHS = {'salamander33': 0.03, 'centipede': 4e-3, 'wide6': 0.3}


def flags_of(m):
    return CONTACTS | TERRAIN | (LIMITS if np.any(m.jnt_limited) else 0)


def phys(m, n, ins, **kw):
    return _contacts_phys(m, n, ins, **dict(dict(fp64_terrain=True), **kw))


def grounds(m):
    return [g for g in range(m.ngeom) if m.geom_type[g] in (GEOM_PLANE, GEOM_HFIELD)]


def ground_dist(m, p, pt):
    """oracle ground_dist for the world-attached ground geom p: (height of pt above it along the local normal, the normal, how far the
    lookup is from a cell edge, the cell diagonal or the grid border in grid units - inf for a plane)."""
    from farms_mujoco_amd.model import quat2mat
    pm = quat2mat(m.geom_quat[p])
    dif = np.asarray(pt, float) - m.geom_pos[p]
    if m.geom_type[p] == GEOM_PLANE:
        return float(dif @ pm[:, 2]), pm[:, 2], np.inf
    lx, ly, lz = pm.T @ dif
    nc, nr = int(m.hfield_ncol), int(m.hfield_nrow)
    rx, ry, zt = m.hfield_size[:3]
    sx, sy = (nc - 1)/(2*rx), (nr - 1)/(2*ry)
    gx, gy = (lx + rx)*sx, (ly + ry)*sy
    border = min(abs(gx), abs(gx - (nc - 1)), abs(gy), abs(gy - (nr - 1)))
    if not (0 <= gx <= nc - 1 and 0 <= gy <= nr - 1):
        return np.inf, pm[:, 2], border
    c, r = min(int(gx), nc - 2), min(int(gy), nr - 2)
    fx, fy = gx - c, gy - r
    D = np.asarray(m.hfield_data, float).reshape(nr, nc)
    z00, z10, z01, z11 = D[r, c]*zt, D[r, c + 1]*zt, D[r + 1, c]*zt, D[r + 1, c + 1]*zt
    gxs, gys = (z10 - z00, z11 - z10) if fx >= fy else (z11 - z01, z01 - z00)
    nl = np.array([-gxs*sx, -gys*sy, 1.0]); inv = 1.0/np.sqrt(nl @ nl)
    # interior cell edges: fx or fy at 0 or 1 (a clamped last cell reaches 1 only on the border, which `border` has)
    edge = min(fx, fy, abs(fx - fy), 1 - fx if c < nc - 2 else np.inf, 1 - fy if r < nr - 2 else np.inf)
    return float((lz - (z00 + gxs*fx + gys*fy))*inv), pm @ (nl*inv), min(edge, border)


def candidates(m, qpos):
    """Every distance the narrow phase compares with 0 for one env (sphere and capsule-end surfaces, box corners, a cylinder's four rim
    points), and the grid margin of every heightfield lookup behind them."""
    from farms_mujoco_amd.model import np_kinematics, quat2mat, quat_mul
    kin = np_kinematics(m, qpos)
    dists, cells = [], []
    for p in grounds(m):
        for g in range(m.ngeom):
            t, b = int(m.geom_type[g]), int(m.geom_bodyid[g])
            if t in (GEOM_PLANE, GEOM_HFIELD):
                continue
            gp = kin['xpos'][b] + quat2mat(kin['xquat'][b]) @ m.geom_pos[g]
            gm = quat2mat(quat_mul(kin['xquat'][b], m.geom_quat[g])); s = m.geom_size[g]
            if t == GEOM_CYLINDER:      # oracle collide_plane, FMJ_GEOM_CYLINDER
                dist, n, cell = ground_dist(m, p, gp)
                cells.append(cell)
                axis = gm[:, 2].copy(); prjaxis = n @ axis
                if prjaxis > 0:
                    axis, prjaxis = -axis, -prjaxis
                vec = axis*prjaxis - n
                len2 = vec @ vec
                vec = vec*(s[0]/np.sqrt(len2)) if len2 >= 1e-30 else gm[:, 0]*s[0]
                prjvec = vec @ n
                axis = axis*s[1]; prjaxis *= s[1]
                vec1 = np.cross(vec, axis); l1 = np.sqrt(vec1 @ vec1)
                if l1 > 1e-15:
                    vec1 = vec1*(s[0]*0.8660254037844386/l1)
                prjvec1 = vec1 @ n
                dists += [dist + prjaxis + prjvec, dist - prjaxis + prjvec, dist + prjaxis - 0.5*prjvec + prjvec1, dist + prjaxis - 0.5*prjvec - prjvec1]
                continue
            if t == GEOM_SPHERE:
                pts, off = [gp], s[0]
            elif t == GEOM_CAPSULE:
                pts, off = [gp + s[1]*gm[:, 2], gp - s[1]*gm[:, 2]], s[0]
            else:
                assert t == GEOM_BOX, t
                pts, off = [gp + gm @ (np.array([sx, sy, sz])*s) for sz in (-1, 1) for sy in (-1, 1) for sx in (-1, 1)], 0.0
            for pt in pts:
                dist, _, cell = ground_dist(m, p, pt)
                dists.append(dist - off); cells.append(cell)
    return np.array(dists), np.array(cells)


def lowest(m, qpos):
    """The deepest candidate distance of one env (negative: below the ground)."""
    return candidates(m, qpos)[0].min()


def inputs(m, n, seed, depth=None, tilt=None, xy=(0.0, 0.0)):
    """support_f64_contacts.inputs over terrain: random joint positions (+-0.15; three joints of a limited model at or past their upper
    limit), a tilted root, qvel normal x 0.3, ctrl uniform +-0.3, and the root lowered until the deepest candidate point is ``depth``
    below the ground under it (a few passes: the ground's normal is not vertical).  ``xy``: where on the ground the root is put.  Rounded
    to fp32."""
    if depth is None:
        depth = DEPTHS[m.name]
    if tilt is None:
        tilt = MODEL_INPUTS[m.name][1]
    rng = np.random.default_rng([778, seed])
    qpos = np.tile(m.key_qpos, (n, 1)).astype(float)
    sq = scalar_q(m)
    qpos[:, sq] = rng.uniform(-0.15, 0.15, (n, len(sq)))
    if np.any(m.jnt_limited):
        lim = np.nonzero(m.jnt_limited)[0]
        for e in range(n):
            for j in rng.choice(lim, size=3, replace=False):
                qpos[e, m.jnt_qposadr[j]] = m.jnt_range[j][1] + rng.uniform(-0.005, 0.03)
    assert m.jnt_type[0] == 0
    for e in range(n):
        ax = rng.normal(size=3); ax /= np.linalg.norm(ax); ang = rng.uniform(-tilt, tilt)
        qpos[e, 3:7] = [np.cos(ang/2), *(np.sin(ang/2)*ax)]
        qpos[e, :2] = np.asarray(xy, float) + rng.uniform(-0.05, 0.05, 2)      # off the grid lines through the origin, where the models spawn
        qpos[e, 2] = 1.0
        for _ in range(6):
            qpos[e, 2] -= lowest(m, qpos[e]) + depth
    qvel = rng.normal(size=(n, m.nv))*0.3
    ctrl = rng.uniform(-0.3, 0.3, (n, max(m.nu, 1)))[:, :m.nu]
    r = lambda a: np.asarray(a, np.float64).astype(np.float32).astype(np.float64)
    return dict(qpos=r(qpos), qvel=r(qvel), ctrl=r(ctrl) if m.nu else None)


def candidates_clear(m, ins, eps=1e-9):
    for q in ins['qpos']:
        d, cells = candidates(m, q)
        if np.abs(d).min() <= eps or cells.min() <= eps:
            return False
    return True


def conditions(oracle, m, ins, want_limits, want_hfield, cylinder_contacts=1):
    """What the issue asks of a one-step case, from the oracle alone; returns (ok, the reference, a description)."""
    ref = reference(oracle, m, ins)
    forced, idle, limf, mind = engaged(m, ref)
    n = len(ref['ncon'])
    cyl = np.zeros(n, int); most = np.zeros(n, int); spread = np.zeros(n)
    for e in range(n):
        k = int(ref['ncon'][e])
        g = ref['geoms'][e, :k, 1]
        on_cyl = g[m.geom_type[g] == GEOM_CYLINDER]
        cyl[e] = len(on_cyl)
        most[e] = np.bincount(on_cyl).max() if len(on_cyl) else 0
        nrm = ref['contact'][e, :k, 3:6]
        spread[e] = (nrm.max(axis=0) - nrm.min(axis=0)).max() if k else 0.0
    ok = (forced.min() >= 4 and idle.min() >= 1 and mind.min() > 1e-9 and candidates_clear(m, ins) and (not want_limits or limf.min() >= 1) and
          (cylinder_contacts == 0 or (cyl.min() >= 1 and most.min() >= cylinder_contacts)) and (not want_hfield or spread.min() > 1e-3))
    return ok, ref, dict(forced=forced, idle=idle, limit_rows_with_force=limf, min_abs_dist=mind, ncon=ref['ncon'], cylinder_contacts=cyl,
                         most_on_one_cylinder=most, normal_spread=spread, iterations=ref['iterations'])


# per model: limited joints, a heightfield, the least number of contacts on some cylinder of every env (0: the model has boxes and a
# capsule, no cylinder to ask for)
WANTS = {'salamander_hfield_cyl': (True, True, 1), 'centipede_hfield_cyl': (False, True, 1), 'boxfoot_hfield': (False, True, 0),
         'salamander_tilted_cyl': (True, False, 3)}


def conditions_of(oracle, name, m, ins):
    return conditions(oracle, m, ins, *WANTS[name])


def first_seed(oracle, name, n=N, start=100, tries=60):
    m = make(name)
    for seed in range(start, start + tries):
        ok, _, what = conditions_of(oracle, name, m, inputs(m, n, seed))
        if ok:
            return seed
    raise AssertionError('no seed satisfies the conditions')
