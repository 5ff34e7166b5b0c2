"""An independent narrow phase for ground contacts, and the scenes the device narrow phase is held to with it: numpy only (the model
builder is imported inside the scene builders), so importing this touches neither torch nor the GPU.

``ref_ground_contacts`` restates what include/fmj.h promises for a geom against a world-attached plane or heightfield from the geometry
alone: a plane distance is a dot product, a heightfield is the triangle under the point (distance and normal from the cross product of
two of its edges, not from slopes), a cylinder is built from its rim (deepest point of the near rim, the same point of the far disk, the
two points at +-120 degrees of the near rim), box corners come in corner order, a mesh gives its four deepest vertices.  It shares no
text with oracle/fmj_oracle.c or the kernels' fmj_narrow*.inc; tests/test_narrow_reference.py holds it to the oracle and to closed forms,
tests/test_gpu_narrow_ground.py holds the device to it.

Scenes carry ONE free body (the whole tree) with its geoms; every coordinate stays within 0.5 m, the scale the position and frame bounds
of the contact tests were set at."""
import functools
from collections import namedtuple

import numpy as np

PLANE, HFIELD, SPHERE, CAPSULE, CYLINDER, BOX, MESH = 0, 1, 2, 3, 5, 6, 7      # include/fmj.h FMJ_GEOM_*
FMJ_WARN_CONTACTFULL = 8

# admissibility margins (see admissible)
DIST_MARGIN = 1e-5          # m: 50 x the |dist| <= 2e-7 m at which DESIGN section 0 measured fp32 grazing decisions
GRID_MARGIN = 1e-4          # grid units from a cell line / the cell diagonal: an fp32 position error of 1e-7 m is ~1e-6 grid units here
GRID_NEAR = 1e-3            # m: heightfield candidates this close above the surface (or below it) fall under GRID_MARGIN
MESH_GAP = 1e-5             # m between the vertex depths that decide membership / order of a mesh's kept four
SEED_MARGIN = 1e-3          # | |n_y| - 0.5 |: the tangent seed of the contact frame must not hang on rounding
# Cylinder: the rim direction is the normalisation of a vector of length sin(tilt) (tilt = angle between axis and ground normal).  An fp32
# axis error of 1e-7 moves the rim point by r 1e-7 / tilt: at r = 2 cm that passes the 2e-6 m position bound below tilt ~ 1e-3.  Tilts
# between 0 (exact: the fallback direction) and 0.05 rad are excluded, a margin of 50 x; so is an axis within 1e-3 of parallel to the
# ground, where the choice of the near disk hangs on the sign of a rounded dot product.
CYL_MIN_TILT = 0.05
CYL_MIN_PRJ = 1e-3


# ---- small rotations --------------------------------------------------------------------------------------------------------------
def quat_to_mat(q):
    """Rotation matrix of the unit quaternion q = (w, x, y, z), in q's dtype."""
    w, x, y, z = q
    one, two = q.dtype.type(1), q.dtype.type(2)
    return np.array([[one - two*(y*y + z*z), two*(x*y - w*z), two*(x*z + w*y)],
                     [two*(x*y + w*z), one - two*(x*x + z*z), two*(y*z - w*x)],
                     [two*(x*z - w*y), two*(y*z + w*x), one - two*(x*x + y*y)]], dtype=q.dtype)


def quat_mul(a, b):
    return np.array([a[0]*b[0] - a[1]*b[1] - a[2]*b[2] - a[3]*b[3], a[0]*b[1] + a[1]*b[0] + a[2]*b[3] - a[3]*b[2],
                     a[0]*b[2] - a[1]*b[3] + a[2]*b[0] + a[3]*b[1], a[0]*b[3] + a[1]*b[2] - a[2]*b[1] + a[3]*b[0]], dtype=a.dtype)


def mat_to_quat(R):
    """Unit quaternion (w, x, y, z) of a rotation matrix, through its largest component (exact for the identity and for half turns
    about a coordinate axis)."""
    R = np.asarray(R, float)
    t = np.array([1 + R[0, 0] + R[1, 1] + R[2, 2], 1 + R[0, 0] - R[1, 1] - R[2, 2], 1 - R[0, 0] + R[1, 1] - R[2, 2],
                  1 - R[0, 0] - R[1, 1] + R[2, 2]])
    k = int(np.argmax(t))
    s = 2*np.sqrt(t[k])
    if k == 0:
        q = [s/4, (R[2, 1] - R[1, 2])/s, (R[0, 2] - R[2, 0])/s, (R[1, 0] - R[0, 1])/s]
    elif k == 1:
        q = [(R[2, 1] - R[1, 2])/s, s/4, (R[0, 1] + R[1, 0])/s, (R[0, 2] + R[2, 0])/s]
    elif k == 2:
        q = [(R[0, 2] - R[2, 0])/s, (R[0, 1] + R[1, 0])/s, s/4, (R[1, 2] + R[2, 1])/s]
    else:
        q = [(R[1, 0] - R[0, 1])/s, (R[0, 2] + R[2, 0])/s, (R[1, 2] + R[2, 1])/s, s/4]
    q = np.array(q) + 0.0
    return q if q[0] >= 0 else -q


def rot(axis, angle):
    """Rotation by ``angle`` about ``axis`` (Rodrigues)."""
    a = np.asarray(axis, float); a = a/np.linalg.norm(a)
    K = np.array([[0, -a[2], a[1]], [a[2], 0, -a[0]], [-a[1], a[0], 0]])
    return np.eye(3) + np.sin(angle)*K + (1 - np.cos(angle))*(K @ K)


def rot_z_to(n):
    """The shortest rotation that takes +z to the unit vector n."""
    n = np.asarray(n, float); n = n/np.linalg.norm(n)
    ax = np.cross([0, 0, 1.0], n)
    s = np.linalg.norm(ax)
    return np.eye(3) if s < 1e-15 else rot(ax, np.arctan2(s, n[2]))


def random_rotation(rng):
    q = rng.normal(size=4)
    return quat_to_mat(q/np.linalg.norm(q))


def contact_frame(n):
    """mju_makeFrame: x = the normal, t1 = (0, 1, 0) - or (0, 0, 1) when |n_y| > 0.5 - made orthogonal to it, t2 = n x t1; nine numbers."""
    n = np.asarray(n)
    seed = np.array([0, 0, 1] if (n[1] < -0.5 or n[1] > 0.5) else [0, 1, 0], n.dtype)
    t1 = seed - n*(seed @ n)
    t1 = t1/np.sqrt(t1 @ t1)
    return np.concatenate([n, t1, np.cross(n, t1)])


# ---- the reference narrow phase -----------------------------------------------------------------------------------------------------
class _Ground:
    """A world-attached plane or heightfield in the working dtype."""

    def __init__(self, model, g, T):
        self.g, self.kind = g, int(model.geom_type[g])
        self.pos = np.asarray(model.geom_pos[g], T)
        q = np.asarray(model.geom_quat[g], T)
        self.R = quat_to_mat(q/np.sqrt(q @ q))
        self.up = self.R[:, 2]
        if self.kind == HFIELD:
            self.nr, self.nc = int(model.hfield_nrow), int(model.hfield_ncol)
            self.rx, self.ry = T(model.hfield_size[0]), T(model.hfield_size[1])
            self.z = np.asarray(model.hfield_data, T).reshape(self.nr, self.nc)*T(model.hfield_size[2])
            self.dx, self.dy = T(2)*self.rx/T(self.nc - 1), T(2)*self.ry/T(self.nr - 1)

    def query(self, p):
        """Height of world point p above the ground along the local surface normal, that normal, and - heightfield - where p fell:
        (gx, gy, column, row, upper triangle?) with column None outside the grid (distance inf there)."""
        d = p - self.pos
        if self.kind == PLANE:
            return self.up @ d, self.up, None
        T = p.dtype.type
        loc = self.R.T @ d
        gx, gy = (loc[0] + self.rx)*(T(self.nc - 1)/(T(2)*self.rx)), (loc[1] + self.ry)*(T(self.nr - 1)/(T(2)*self.ry))
        if not (0 <= gx <= self.nc - 1 and 0 <= gy <= self.nr - 1):
            return T(np.inf), self.up, (float(gx), float(gy), None, None, None)
        c, r = min(int(np.floor(gx)), self.nc - 2), min(int(np.floor(gy)), self.nr - 2)      # the last line belongs to the last cell
        upper = not (gx - T(c) >= gy - T(r))                       # the cell's diagonal runs (c, r) - (c + 1, r + 1) and belongs to the lower triangle
        node = lambda cc, rr: np.array([-self.rx + T(cc)*self.dx, -self.ry + T(rr)*self.dy, self.z[rr, cc]], dtype=p.dtype)
        A = node(c, r)
        B, C = (node(c + 1, r + 1), node(c, r + 1)) if upper else (node(c + 1, r), node(c + 1, r + 1))
        n = np.cross(B - A, C - A)
        n = n/np.sqrt(n @ n)                                       # +z side: both triangles are listed counter-clockwise seen from above
        return n @ (loc - A), self.R @ n, (float(gx), float(gy), c, r, upper)


def ref_ground_contacts(model, qpos, dtype=np.float64):
    """Every non-world geom of the one free body against every world-attached plane / heightfield.  Returns a dict:
    ``contacts`` = [(ground geom, geom, pos, normal, dist)] ground-major, then by geom, then by point, cut at max_contacts; ``full`` = the
    list was cut; ``total`` = its length before the cut; ``candidates`` = [dict(ground, geom, k, dist, grid)] for every candidate point,
    penetrating or not (grid = (gx, gy) for a heightfield); ``decisions`` = every discrete choice made (what the float32 run must
    repeat); ``mesh_gaps``, ``cyl`` = the margins admissible() looks at."""
    T = np.dtype(dtype).type
    assert model.nbody == 2 and int(model.jnt_type[0]) == 0, 'scenes carry one free body'
    q = np.asarray(qpos, dtype)
    bpos, bq = q[:3], q[3:7]/np.sqrt(q[3:7] @ q[3:7])
    bR = quat_to_mat(bq)
    grounds = [_Ground(model, g, T) for g in range(model.ngeom) if model.geom_bodyid[g] == 0 and model.geom_type[g] in (PLANE, HFIELD)]
    contacts, cands, dec, mesh_gaps, cyl = [], [], [], [], []

    def cell(grid):
        return None if grid is None else grid[2:]

    for gr in grounds:
        for g in range(model.ngeom):
            if model.geom_bodyid[g] == 0:
                continue
            typ = int(model.geom_type[g])
            size = np.asarray(model.geom_size[g], dtype)
            gq = np.asarray(model.geom_quat[g], dtype)
            R = quat_to_mat(quat_mul(bq, gq/np.sqrt(gq @ gq)))
            cen = bpos + bR @ np.asarray(model.geom_pos[g], dtype)
            found = []                                              # (point on the geom, normal, dist) -> contact at point - n (radius + dist / 2)
            radius = T(0)

            def candidate(k, dist, grid):
                cands.append(dict(ground=gr.g, geom=g, k=k, dist=float(dist), grid=None if grid is None else grid[:2]))
                dec.append((gr.g, g, k, bool(dist < 0), cell(grid)))

            if typ in (SPHERE, CAPSULE):
                radius = size[0]
                ends = [cen] if typ == SPHERE else [cen + size[1]*R[:, 2], cen - size[1]*R[:, 2]]
                for k, e in enumerate(ends):
                    d, n, grid = gr.query(e)
                    candidate(k, d - radius, grid)
                    if d - radius < 0:
                        found.append((e, n, d - radius))
            elif typ == BOX:
                for k in range(8):
                    sgn = np.array([1 if k & 1 else -1, 1 if k & 2 else -1, 1 if k & 4 else -1], dtype)
                    e = cen + R @ (sgn*size)
                    d, n, grid = gr.query(e)
                    candidate(k, d, grid)
                    if d < 0 and len(found) < 4:
                        found.append((e, n, d))
            elif typ == CYLINDER:
                dc, n, grid = gr.query(cen)                        # a heightfield is the plane under the cylinder's centre
                if not np.isfinite(dc):
                    candidate(0, dc, grid)
                else:
                    a = R[:, 2]
                    s = n @ a
                    flip = bool(s > 0)
                    if flip:                                        # a: towards the ground, the near disk is cen + half length * a
                        a, s = -a, -s
                    radial = s*a - n                                # -n projected into the disk plane: length sin(tilt)
                    L2 = radial @ radial
                    fallback = bool(L2 < 1e-30)                     # axis along the normal: every rim point is as deep, take the geom's +x
                    u = R[:, 0] if fallback else radial/np.sqrt(L2)
                    w = np.cross(u, a)
                    lw = np.sqrt(w @ w)
                    w = w/lw if lw > 0 else w
                    h, r_ = size[1], size[0]
                    half, s32 = T(0.5), T(np.sqrt(0.75))
                    pts = [cen + h*a + r_*u, cen - h*a + r_*u, cen + h*a + r_*(s32*w - half*u), cen + h*a + r_*(-s32*w - half*u)]
                    cyl.append(dict(ground=gr.g, geom=g, sin_tilt=float(np.sqrt(L2)), prj=float(s), fallback=fallback))
                    dec.append((gr.g, g, 'cyl', flip, fallback))
                    for k, e in enumerate(pts):
                        d = dc + n @ (e - cen)
                        candidate(k, d, grid)
                        if d < 0:
                            found.append((e, n, d))
            elif typ == MESH:
                dc, n, grid = gr.query(cen)
                rbound = size[2]
                candidate(-1, dc - rbound, grid)                    # nothing when the ground under the origin is farther than the bounding radius
                if dc < rbound:
                    V = np.asarray(model.mesh_vert[model.geom_vertadr[g]:model.geom_vertadr[g] + model.geom_vertnum[g]], dtype)
                    pen = []
                    for k in range(len(V)):
                        e = cen + R @ V[k]
                        d, n, grid = gr.query(e)
                        candidate(k, d, grid)
                        if d < 0:
                            pen.append((e, n, d, k))
                    order = sorted(range(len(pen)), key=lambda i: pen[i][2])          # stable: equal depths stay in vertex order
                    ds = [float(pen[i][2]) for i in order[:5]]
                    if len(ds) > 1:
                        mesh_gaps.append(min(b_ - a_ for a_, b_ in zip(ds, ds[1:])))
                    found = [pen[i][:3] for i in order[:4]]
                    dec.append((gr.g, g, 'mesh', tuple(pen[i][3] for i in order[:4])))
            else:
                raise ValueError(f'geom type {typ}')
            for e, n, d in found:
                contacts.append((gr.g, g, e - n*(radius + d/2), n, d))
    for c in contacts:
        dec.append(('seed', bool(c[3][1] < -0.5 or c[3][1] > 0.5)))
    total = len(contacts)
    mc = int(model.max_contacts)
    return dict(contacts=contacts[:mc], full=total > mc, total=total, candidates=cands, decisions=dec, mesh_gaps=mesh_gaps, cyl=cyl)


def admissible(model, qpos, exact=False):
    """(ok, reason): may a test that differs from the reference at this pose in a DISCRETE decision blame a bug, not rounding?
    1. every finite candidate distance is at least DIST_MARGIN from zero;
    2. every heightfield candidate within GRID_NEAR above the surface, below it or outside the grid is at least GRID_MARGIN grid units
       from a cell line and the cell diagonal (the cell of a point farther above decides nothing) - waived with ``exact`` (dyadic grid, identity rotation, dyadic coordinates: gx, gy are
       the same exact numbers in fp32 and fp64), where rule 4 carries the guarantee;
    3. mesh vertex depths that decide membership or order among the kept four differ by at least MESH_GAP;
    4. the float32 run of the reference makes the same decisions as the float64 run (cells, triangles, penetration flags, order);
    and the margins on the contact frame's tangent seed and the cylinder's rim direction stated at the top of this file."""
    r = ref_ground_contacts(model, qpos)
    for c in r['candidates']:
        if np.isfinite(c['dist']) and abs(c['dist']) < DIST_MARGIN:
            return False, f'grazing candidate {c}'
        if c['grid'] is not None and not exact and not c['dist'] > GRID_NEAR:
            gx, gy = c['grid']
            fx, fy = gx - np.floor(gx), gy - np.floor(gy)
            if min(fx, 1 - fx, fy, 1 - fy, abs(fx - fy)) < GRID_MARGIN:
                return False, f'candidate on a cell line or diagonal {c}'
    if any(gap < MESH_GAP for gap in r['mesh_gaps']):
        return False, f'mesh depths too close {r["mesh_gaps"]}'
    for c in r['contacts']:
        if abs(abs(c[3][1]) - 0.5) < SEED_MARGIN:
            return False, f'normal on the tangent seed threshold {c[3]}'
    for c in r['cyl']:
        if not c['fallback'] and (c['sin_tilt'] < np.sin(CYL_MIN_TILT) or abs(c['prj']) < CYL_MIN_PRJ):
            return False, f'cylinder axis too close to the normal or to the ground {c}'
    r32 = ref_ground_contacts(model, np.asarray(qpos, np.float64).astype(np.float32), dtype=np.float32)
    is_cand = lambda d: len(d) == 5 and isinstance(d[2], int)      # (ground, geom, k, penetrating, cell): one per candidate, in their order
    c64, c32 = [d for d in r['decisions'] if is_cand(d)], [d for d in r32['decisions'] if is_cand(d)]
    if [d for d in r['decisions'] if not is_cand(d)] != [d for d in r32['decisions'] if not is_cand(d)] or len(c64) != len(c32):
        return False, 'the float32 run decides differently'
    for c, d64, d32 in zip(r['candidates'], c64, c32):             # the cell of a point far above the surface decides nothing
        if d64[:4] != d32[:4] or (c['dist'] <= GRID_NEAR and d64[4] != d32[4]):
            return False, f'the float32 run decides differently at {c}'
    return True, ''


# ---- models -------------------------------------------------------------------------------------------------------------------------
MU = 0.7        # friction of every body geom (grounds: 0): far from the 1e-3 below which Newton / CG are rerouted to the dual problem


def build_model(grounds, geoms, max_contacts=16, solver=None, cone='pyramidal', name='narrow'):
    """One free body at the origin carrying ``geoms`` = [(type, size, pos, quat)] (type MESH: size = the vertices) over ``grounds`` =
    [('plane', pos, quat)] / [('hfield', data, size4, pos, quat)]."""
    from farms_mujoco_amd.model import ModelBuilder, SOLVERS, CONES
    b = ModelBuilder(name, timestep=1e-3)
    b.options['max_contacts'] = max_contacts
    b.add_body('b', 'world', pos=(0, 0, 0), mass=0.4, inertia=(4e-4, 5e-4, 6e-4), joint='free')
    for typ, size, pos, quat in geoms:
        if typ == MESH:
            b.add_mesh_geom('b', size, pos=pos, quat=quat, friction=(MU, 0, 0), hull=False)
        else:
            b.add_geom('b', typ, size, pos=pos, quat=quat, friction=(MU, 0, 0))
    for gr in grounds:
        if gr[0] == 'plane':
            b.add_geom('world', PLANE, (0, 0, 0), pos=gr[1], quat=gr[2])
        else:
            b.add_hfield(gr[1], gr[2], pos=gr[3], quat=gr[4])
    m = b.compile()
    if solver is not None:
        m.solver = SOLVERS[solver]; m.cone = CONES[cone]
        if solver != 'pgs':
            m.solver_iterations = 100
    return m


def plane_from_normal(n, pos=(0.02, -0.03, 0.01)):
    n = np.asarray(n, float)
    if len(n) == 2:
        n = np.array([n[0], n[1], np.sqrt(1 - n[0]**2 - n[1]**2)])
    return ('plane', tuple(pos), tuple(mat_to_quat(rot_z_to(n))))


I4 = (1.0, 0.0, 0.0, 0.0)
ORIGIN = (0.0, 0.0, 0.0)
SPH = [(SPHERE, (0.02,), ORIGIN, I4)]
CAP = [(CAPSULE, (0.012, 0.03), ORIGIN, I4)]
BOXG = [(BOX, (0.03, 0.02, 0.012), ORIGIN, I4)]
CYL = [(CYLINDER, (0.02, 0.004), ORIGIN, I4)]
SKEW = mat_to_quat(rot((1.0, -2.0, 0.5), 0.3))
HF_SHIFT = (0.03, -0.02, 0.04)


def exact_grid():
    """The dyadic grid: 9 x 9 samples over [-0.25, 0.25]^2 (pitch 1 / 16, 16 grid units per metre), heights multiples of 1 / 8 of the
    scale, identity rotation, dyadic position."""
    rng = np.random.default_rng(7)
    return ('hfield', rng.integers(-8, 9, (9, 9))/8.0, (0.25, 0.25, 0.015, 0.1), (0.0625, -0.125, 0.03125), I4)


def bumpy(pos=ORIGIN, quat=I4):
    """11 x 13 smooth bumps over [-0.3, 0.3] x [-0.25, 0.25], slopes up to about 30 degrees."""
    xs, ys = np.linspace(-0.3, 0.3, 13), np.linspace(-0.25, 0.25, 11)
    z = np.sin(11.0*xs[None, :] + 0.4)*np.cos(9.0*ys[:, None] - 0.7) + 0.5*np.sin(17.0*xs[None, :]*ys[:, None]*6 + 1.0)
    return ('hfield', z/np.abs(z).max(), (0.3, 0.25, 0.03, 0.1), tuple(pos), tuple(quat))


def chunk_geoms():
    """76 small spheres and boxes on a 10 x 8 grid of pitch 2.5 cm (row-major: the geoms past index 64 are the last rows)."""
    geoms = []
    rng = np.random.default_rng(5)
    for i in range(76):
        p = (0.025*(i % 10) - 0.1125, 0.025*(i//10) - 0.0875, 0.0)
        if i % 2:
            geoms.append((BOX, (0.008, 0.006, 0.005), p, tuple(mat_to_quat(random_rotation(rng)))))
        else:
            geoms.append((SPHERE, (0.008,), p, I4))
    return geoms


TWO_BOXES = [(BOX, (0.02, 0.015, 0.01), (-0.04, 0.0, 0.0), I4), (BOX, (0.02, 0.015, 0.01), (0.04, 0.0, 0.0), I4)]
QUAD = [(SPHERE, (0.02,), (0.05, 0.04, 0.0), I4), (CAPSULE, (0.012, 0.03), (-0.05, 0.04, 0.0), tuple(mat_to_quat(rot((0, 1, 0), 1.2)))),
        (BOX, (0.03, 0.02, 0.012), (0.05, -0.04, 0.0), tuple(mat_to_quat(rot((1, 1, 0), 0.5)))),
        (CYLINDER, (0.02, 0.015), (-0.05, -0.04, 0.0), tuple(mat_to_quat(rot((1, 0, 0), 0.9))))]

P_BOX = plane_from_normal((-0.25, 0.2))
P_CAP = plane_from_normal((0.2, -0.3))
P_FLAT = ('plane', ORIGIN, I4)

MODELS = {            # key: (grounds, geoms, max_contacts)
    'sphere_ny045': ([plane_from_normal((0.3, 0.45))], SPH, 4),
    'sphere_ny055': ([plane_from_normal((-0.2, 0.55))], SPH, 4),
    'sphere_ny-08': ([plane_from_normal((0.1, -0.8))], SPH, 4),
    'sphere_tilt_y': ([plane_from_normal((np.sin(0.4), 0.0))], SPH, 4),
    'capsule': ([P_CAP], CAP, 4),
    'box': ([P_BOX], BOXG, 8),
    'cylinder': ([P_FLAT], CYL, 8),
    'grid_sphere': ([exact_grid()], SPH, 4),
    'hf_sphere': ([bumpy()], SPH, 4), 'hf_capsule': ([bumpy()], CAP, 4), 'hf_box': ([bumpy()], BOXG, 8), 'hf_cylinder': ([bumpy()], CYL, 8),
    'hfr_sphere': ([bumpy(HF_SHIFT, SKEW)], SPH, 4), 'hfr_capsule': ([bumpy(HF_SHIFT, SKEW)], CAP, 4),
    'hfr_box': ([bumpy(HF_SHIFT, SKEW)], BOXG, 8), 'hfr_cylinder': ([bumpy(HF_SHIFT, SKEW)], CYL, 8),
    'two_grounds': ([plane_from_normal((0.25, -0.3), pos=(0.0, 0.0, -0.01)), bumpy((0.03, -0.02, -0.005), SKEW)], QUAD, 32),
    'chunk': ([plane_from_normal((0.05, -0.08), pos=(0.0, 0.0, 0.0))], chunk_geoms(), 48),
    'truncate': ([P_BOX], TWO_BOXES, 6),
}


@functools.lru_cache(maxsize=None)
def directed_model(key):
    """The (shared, never modified) model of a directed case."""
    grounds, geoms, mc = MODELS[key]
    return build_model(grounds, geoms, max_contacts=mc, name=key)


# ---- poses --------------------------------------------------------------------------------------------------------------------------
def _qpos(t, R):
    return np.concatenate([np.asarray(t, float), mat_to_quat(R)])


def rest(plane, R, pts, depth=None, below=None, radius=0.0, shift=(0.0, 0.0)):
    """Pose of the body (rotation R, body-frame points ``pts`` each carrying ``radius``) over ``plane``: the lowest point ``depth`` below
    the plane, or the plane halfway between the ``below``-th and the next lowest point (all of them: 2 mm above the highest)."""
    Rp = quat_to_mat(np.asarray(plane[2], float))
    n, off = Rp[:, 2], Rp[:, 2] @ np.asarray(plane[1], float)
    h = np.sort((np.asarray(pts, float) @ R.T) @ n)
    if below is None:
        level = h[0] + depth
    else:
        level = h[-1] + 0.002 if below == len(h) else 0.5*(h[below - 1] + h[below])
    return _qpos(n*(off - level + radius) + Rp @ np.array([shift[0], shift[1], 0.0]), R)


def settle(model, R, at, depth, ground=0):
    """Pose over a heightfield: rotation R, the body above the ground-frame point ``at`` = (x, y), lowered along the ground's +z until
    its deepest candidate is ``depth`` below the surface (bisection on the reference's own candidates: construction only)."""
    gpos, gR = np.asarray(model.geom_pos[ground], float), quat_to_mat(np.asarray(model.geom_quat[ground], float))

    def pose(s):
        return _qpos(gpos + gR @ np.array([at[0], at[1], s]), R)

    def f(s):
        d = [c['dist'] for c in ref_ground_contacts(model, pose(s))['candidates'] if c['ground'] == ground and c['k'] >= 0 and np.isfinite(c['dist'])]
        return min(d) + depth
    lo, hi = -0.2, 0.3
    for _ in range(50):
        mid = 0.5*(lo + hi)
        lo, hi = (mid, hi) if f(mid) < 0 else (lo, mid)
    return pose(hi)


def _corners(size):
    return [[(1 if k & 1 else -1)*size[0], (1 if k & 2 else -1)*size[1], (1 if k & 4 else -1)*size[2]] for k in range(8)]


def _rim(r, h, n=720):
    a = np.arange(n)*2*np.pi/n
    return [[r*np.cos(x), r*np.sin(x), z] for z in (h, -h) for x in a]


Case = namedtuple('Case', 'name model qpos ncon exact truncated symmetric')


@functools.lru_cache(maxsize=None)
def directed_cases():
    """The table of directed cases: name, model, pose, contacts expected; flags: ``exact`` (rule 2 of admissible waived), ``truncated``
    (FMJ_WARN_CONTACTFULL expected), ``symmetric`` (contacts of one geom share a load exactly: forces are compared per geom)."""
    cases = []

    def add(name, key, qpos, ncon, exact=False, truncated=False, symmetric=False):
        cases.append(Case(name, key, np.asarray(qpos, float), ncon, exact, truncated, symmetric))

    rng = np.random.default_rng(11)
    # sphere on tilted planes: both tangent seeds (|n_y| below and above 0.5), both signs of n_y, a tilt about y only
    for key in ('sphere_ny045', 'sphere_ny055', 'sphere_ny-08', 'sphere_tilt_y'):
        pl = MODELS[key][0][0]
        add(key + '_in2mm', key, rest(pl, random_rotation(rng), [ORIGIN], depth=0.002, radius=0.02, shift=(0.03, -0.02)), 1)
        add(key + '_clear', key, rest(pl, random_rotation(rng), [ORIGIN], depth=-0.003, radius=0.02, shift=(-0.01, 0.04)), 0)
        add(key + '_in6mm', key, rest(pl, random_rotation(rng), [ORIGIN], depth=0.006, radius=0.02, shift=(-0.05, 0.01)), 1)
    # capsule (radius 12 mm, half length 30 mm): ends = +axis, -axis
    Rp, ends = quat_to_mat(np.asarray(P_CAP[2])), [[0, 0, 0.03], [0, 0, -0.03]]
    add('capsule_both_ends', 'capsule', rest(P_CAP, Rp @ rot((0, 1, 0), np.pi/2 - 0.05) @ rot((0, 0, 1), 0.4), ends, depth=0.005, radius=0.012), 2)
    add('capsule_plus_end_only', 'capsule', rest(P_CAP, Rp @ rot((1, 0, 0), np.pi - 0.5), ends, depth=0.003, radius=0.012, shift=(0.02, 0.02)), 1)
    add('capsule_clear', 'capsule', rest(P_CAP, Rp @ rot((1, 0, 0), 0.7), ends, depth=-0.004, radius=0.012), 0)
    add('capsule_minus_end_only', 'capsule', rest(P_CAP, Rp @ rot((1, 0, 0), 0.5), ends, depth=0.003, radius=0.012, shift=(-0.03, 0.01)), 1)
    add('capsule_parallel', 'capsule', rest(P_CAP, Rp @ rot((0, 1, 0), np.pi/2), ends, depth=0.003, radius=0.012, shift=(0.01, -0.04)), 2, symmetric=True)
    # box (30 x 20 x 12 mm half extents): corners 0..3 are its -z face
    Rp, co = quat_to_mat(np.asarray(P_BOX[2])), _corners((0.03, 0.02, 0.012))
    add('box_flat', 'box', rest(P_BOX, Rp @ rot((0, 0, 1), 0.3), co, depth=0.003), 4, symmetric=True)
    add('box_on_edge', 'box', rest(P_BOX, Rp @ rot((1, 0, 0), 0.8) @ rot((0, 0, 1), 0.02), co, depth=0.003, shift=(0.03, 0.0)), 2)
    add('box_flipped', 'box', rest(P_BOX, Rp @ rot((1, 0, 0), np.pi) @ rot((0, 0, 1), 0.2) @ rot((0, 1, 0), 0.01), co, depth=0.003), 4, symmetric=True)
    add('box_on_corner', 'box', rest(P_BOX, Rp @ rot((1, 0.7, 0), 0.7), co, depth=0.003, shift=(0.0, -0.03)), 1)
    add('box_5_below', 'box', rest(P_BOX, Rp @ rot((1, 0.7, 0), 0.7), co, below=5, shift=(-0.02, 0.02)), 4)
    add('box_clear', 'box', rest(P_BOX, Rp @ rot((1, 0.2, 0), 0.3), co, depth=-0.005), 0)
    add('box_8_below', 'box', rest(P_BOX, Rp @ rot((0.3, 1, 0), 2.0), co, below=8, shift=(0.02, 0.03)), 4)
    # cylinder (radius 20 mm, half length 4 mm) on the horizontal plane z = 0
    rim = _rim(0.02, 0.004)
    add('cylinder_upright_exact', 'cylinder', rest(P_FLAT, np.eye(3), rim, depth=0.003, shift=(0.01, -0.02)), 3, symmetric=True)       # fallback direction, near disk flipped
    add('cylinder_tilt30_one', 'cylinder', rest(P_FLAT, rot((0.6, 0.8, 0), np.pi/6), rim, depth=0.003), 1)
    add('cylinder_tilt30_two', 'cylinder', rest(P_FLAT, rot((0.6, 0.8, 0), np.pi/6), rim, depth=0.009, shift=(0.02, 0.02)), 2)
    add('cylinder_upside_down_exact', 'cylinder', rest(P_FLAT, np.diag([1.0, -1.0, -1.0]), rim, depth=0.003, shift=(-0.03, 0.0)), 3, symmetric=True)
    add('cylinder_on_side', 'cylinder', rest(P_FLAT, rot((0, 1, 0), np.pi/2 - 0.03) @ rot((0, 0, 1), 1.0), rim, depth=0.003), 2)
    add('cylinder_sunk_all_four', 'cylinder', rest(P_FLAT, rot((0.6, 0.8, 0), np.pi/6), rim, depth=0.018, shift=(0.0, -0.03)), 4)
    add('cylinder_tilt150_two', 'cylinder', rest(P_FLAT, rot((0.6, 0.8, 0), np.pi - np.pi/6), rim, depth=0.009, shift=(-0.02, 0.01)), 2)
    # heightfield, exact grid cases: sphere centres with dyadic coordinates on the dyadic grid (column c = (x + 0.1875) 16, row r = (y + 0.375) 16)
    gm, (_, gdata, gsize, gpos, _) = directed_model('grid_sphere'), exact_grid()
    zn = lambda r, c: gpos[2] + gdata[r, c]*gsize[2]                  # a node's world height

    def grid_case(name, col, row, z_surface, ncon=1):
        x, y = gpos[0] - 0.25 + col/16.0, gpos[1] - 0.25 + row/16.0
        add('grid_' + name, 'grid_sphere', _qpos((x, y, z_surface + 0.02 - 0.004), random_rotation(rng)), ncon, exact=True)
    grid_case('column_line', 3, 4.5, 0.5*(zn(4, 3) + zn(5, 3)))
    grid_case('row_line', 2.25, 6, 0.75*zn(6, 2) + 0.25*zn(6, 3))
    grid_case('diagonal', 5.5, 1.5, 0.5*(zn(1, 5) + zn(2, 6)))
    grid_case('node', 4, 2, zn(2, 4))
    grid_case('last_column', 8, 3.5, 0.5*(zn(3, 8) + zn(4, 8)))
    grid_case('last_row', 1.25, 8, 0.75*zn(8, 1) + 0.25*zn(8, 2))
    grid_case('far_corner', 8, 8, zn(8, 8))
    grid_case('first_node', 0, 0, zn(0, 0))
    grid_case('outside', 8 + 1/64.0, 3.5, 0.5*(zn(3, 8) + zn(4, 8)), ncon=0)
    # heightfield, bumpy: the same ground-frame configurations over the plain and over the shifted, rotated heightfield
    for pre in ('hf', 'hfr'):
        hp, hR = np.asarray(MODELS[pre + '_sphere'][0][0][3]), quat_to_mat(np.asarray(MODELS[pre + '_sphere'][0][0][4], float))
        m = directed_model(pre + '_sphere')
        add(pre + '_sphere_lower_triangle', pre + '_sphere', settle(m, hR @ rot((1, 2, 3), 0.8), (0.115, 0.06), 0.003), 1)      # cell (8, 6), fx 0.3 fy 0.2
        add(pre + '_sphere_clear', pre + '_sphere', _qpos(hp + hR @ np.array([0.013, 0.107, 0.09]), np.eye(3)), 0)
        add(pre + '_sphere_upper_triangle', pre + '_sphere', settle(m, hR @ rot((3, 2, 1), 0.5), (0.11, 0.07), 0.003), 1)       # cell (8, 6), fx 0.2 fy 0.4
        m = directed_model(pre + '_capsule')
        add(pre + '_capsule_two_triangles', pre + '_capsule', settle(m, hR @ rot((0, 1, 0), np.pi/2) @ rot((1, 0, 0), 0.3), (0.1, 0.1), 0.008), 2)
        add(pre + '_capsule_clear', pre + '_capsule', _qpos(hp + hR @ np.array([0.103, -0.091, 0.1]), hR @ rot((1, 0, 0), 1.0)), 0)
        add(pre + '_capsule_one_end', pre + '_capsule', settle(m, hR @ rot((1, 0, 0), 0.6), (0.17, 0.12), 0.004), 1)
        m = directed_model(pre + '_box')
        add(pre + '_box_over_the_edge', pre + '_box', settle(m, hR @ rot((0, 0, 1), 0.1), (0.3, 0.02), 0.006), 2)
        add(pre + '_box_clear', pre + '_box', _qpos(hp + hR @ np.array([-0.097, 0.052, 0.12]), hR @ rot((1, 1, 0), 0.5)), 0)
        add(pre + '_box_inside_tilted', pre + '_box', settle(m, hR @ rot((1, 0.5, 0), 0.5), (-0.12, 0.1), 0.005), 1)
        m = directed_model(pre + '_cylinder')
        add(pre + '_cylinder_on_slope', pre + '_cylinder', settle(m, hR @ rot((1, 0, 0), 0.4), (0.06, -0.11), 0.004), 1)
        add(pre + '_cylinder_clear', pre + '_cylinder', _qpos(hp + hR @ np.array([0.011, -0.007, 0.1]), hR), 0)
        add(pre + '_cylinder_on_side_slope', pre + '_cylinder', settle(m, hR @ rot((0, 1, 0), 1.3), (-0.19, 0.14), 0.004), 2)
    # two grounds under the four-geom body: records are ground-major
    m = directed_model('two_grounds')
    add('two_grounds_a', 'two_grounds', _qpos((0.0, 0.0, 0.022), rot((1, 0, 0), 0.15)), 7)
    add('two_grounds_clear', 'two_grounds', _qpos((0.0, 0.0, 0.15), rot((0, 1, 0), 0.3)), 0)
    add('two_grounds_shallow', 'two_grounds', np.array([-0.0816, -0.0976, 0.0257, 0.7994, 0.4135, 0.1434, 0.4115]), 4)      # found by search: under 1 cm deep on both
    # more than 64 geoms: the grid of 76 tilted so that its low-x columns touch in every row, the last rows (geoms past 64) included
    pl = MODELS['chunk'][0][0]
    Rp = quat_to_mat(np.asarray(pl[2]))
    add('chunk_low_x', 'chunk', _qpos(Rp @ np.array([0.0, 0.0, 0.0205]), Rp @ rot((0, 1, 0), 0.22)), 46)
    add('chunk_clear', 'chunk', _qpos((0.0, 0.0, 0.08), np.eye(3)), 0)
    add('chunk_shallow', 'chunk', _qpos(Rp @ np.array([0.0, 0.0, 0.026]), Rp @ rot((0, 1, 0), 0.22)), 27)                     # under 1 cm deep: forces are compared
    # truncation: two flat boxes, six slots: the first box's four corners and the second's first two
    Rp, co2 = quat_to_mat(np.asarray(P_BOX[2])), [[x + dx, y, z] for dx in (-0.04, 0.04) for x, y, z in _corners((0.02, 0.015, 0.01))]
    add('truncate_two_flat_boxes', 'truncate', rest(P_BOX, Rp @ rot((0, 0, 1), 0.3), co2, depth=0.003), 6, truncated=True, symmetric=True)
    add('truncate_clear', 'truncate', rest(P_BOX, Rp @ rot((1, 0, 0), 0.3), co2, depth=-0.004), 0)
    add('truncate_one_box_edge', 'truncate', rest(P_BOX, Rp @ rot((0, 1, 0), 0.25), co2, depth=0.003), 2)
    return tuple(cases)


def directed_batches():
    """{model key: [Case]} in table order: the envs of one batch are the poses of one model, neighbours hold different cases."""
    out = {}
    for c in directed_cases():
        out.setdefault(c.model, []).append(c)
    return out


# ---- seeded scenes ------------------------------------------------------------------------------------------------------------------
def _random_geoms(rng):
    geoms = []
    for typ in (SPHERE, CAPSULE, BOX, CYLINDER):
        pos = tuple(rng.normal(size=3)*0.04)
        quat = tuple(mat_to_quat(random_rotation(rng)))
        size = {SPHERE: (rng.uniform(0.015, 0.03),), CAPSULE: (rng.uniform(0.01, 0.02), rng.uniform(0.02, 0.04)),
                BOX: tuple(rng.uniform(0.01, 0.03, 3)), CYLINDER: (rng.uniform(0.015, 0.03), rng.uniform(0.01, 0.03))}[typ]
        geoms.append((typ, tuple(float(s) for s in size), pos, quat))
    order = rng.permutation(4)
    return [geoms[i] for i in order]


def _random_grounds(rng):
    ax = rng.normal(size=2)
    plane = ('plane', (0.0, 0.0, float(rng.uniform(-0.02, 0.0))), tuple(mat_to_quat(rot((ax[0], ax[1], 0.0), rng.uniform(0.05, 0.6)))))
    data = rng.uniform(-1, 1, (7, 9))
    hf = ('hfield', data, (0.3, 0.25, 0.015, 0.1), (float(rng.uniform(-0.03, 0.03)), float(rng.uniform(-0.03, 0.03)), float(rng.uniform(-0.01, 0.01))),
          tuple(mat_to_quat(rot(rng.normal(size=3), rng.uniform(0.05, 0.4)))))
    return [plane, hf]


def _random_pose(rng, z_max=0.06):
    return _qpos((rng.uniform(-0.15, 0.15), rng.uniform(-0.15, 0.15), rng.uniform(0.0, z_max)), random_rotation(rng))


def _cloud(rng, n):
    v = rng.normal(size=(n, 3)); v /= np.linalg.norm(v, axis=1, keepdims=True)      # points on an ellipsoid: every one is a hull vertex
    return v*np.array([0.035, 0.025, 0.02])


CUBE = np.array(_corners((0.02, 0.02, 0.02)))
Scenes = namedtuple('Scenes', 'two_grounds single mesh draws rejected')


@functools.lru_cache(maxsize=None)
def seeded_scenes(n_models=8, n_poses=3, seed=20240):
    """Draw-and-reject with a fixed seed: ``two_grounds`` = [(grounds, geoms, [qpos])] for 8 models x 3 admissible poses of a four-shape body
    over a tilted plane plus a rotated 7 x 9 heightfield; ``single`` = the same bodies and poses over one of the two grounds (plane,
    heightfield alternating); ``mesh`` = 4 models with a convex mesh (a cube of 8 vertices / a hull of 20; next to a sphere) over the
    plane or the heightfield.  ``draws`` / ``rejected`` count the poses drawn and those admissible() refused."""
    rng = np.random.default_rng(seed)
    draws = rejected = 0

    def poses(grounds, geoms, z_max=0.06):
        nonlocal draws, rejected
        m = build_model(grounds, geoms, max_contacts=32)
        out = []
        while len(out) < n_poses:
            q = _random_pose(rng, z_max)
            draws += 1
            if admissible(m, q)[0]:
                out.append(q)
            else:
                rejected += 1
        return out
    two, single, mesh = [], [], []
    for i in range(n_models):
        grounds, geoms = _random_grounds(rng), _random_geoms(rng)
        qs = poses(grounds, geoms)
        two.append((grounds, geoms, qs))
        single.append(([grounds[i % 2]], geoms, qs))
    for i in range(4):
        grounds = [_random_grounds(rng)[i % 2]]
        verts = CUBE if i < 2 else _cloud(rng, 20)
        geoms = [(MESH, verts, tuple(rng.normal(size=3)*0.02), tuple(mat_to_quat(random_rotation(rng)))),
                 (SPHERE, (0.015,), (0.05, 0.0, 0.0), I4)]
        mesh.append((grounds, geoms, poses(grounds, geoms, z_max=0.03)))      # the small bodies sit lower: more of their vertices touch
    return Scenes(two, single, mesh, draws, rejected)
