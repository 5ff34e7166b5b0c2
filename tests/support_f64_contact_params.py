"""Models, recipes, inputs and oracle-side conditions of the fp64 contact step away from the one point of its parameter space that
test_gpu_f64_contacts.py, test_gpu_f64_terrain.py and test_gpu_f64_elliptic.py visit (test_f64_contact_recipes.py,
test_gpu_f64_contact_params.py): more than 64 contacts (the contact lanes of the second wave), solref / solimp / friction that differ
per geom (recipe P), a ground with friction, two ground geoms, geoms on bodies without dofs and past geom 64, and the branches of the
terrain narrow phase that no walking model reaches.  Builds on support_f64_contacts.py, support_f64_terrain.py and
support_f64_elliptic.py; torch and the GPU modules are imported inside the functions, so importing this module needs no GPU.

A case is a name of ``CASES``: ``case(name)`` gives its model, its inputs and the kernel family it runs on, ``conditions`` what the
case is about, asserted from the oracle alone.  Every reference value comes from the oracle (Newton, 100 iterations, the model's
tolerance; 1e-10 under the elliptic cone, as in support_f64_elliptic.py)."""
import numpy as np

import support_f64_contacts as C
import support_f64_terrain as T
import support_f64_elliptic as E
from support_f64_contacts import N, GEOM_PLANE, GEOM_SPHERE, GEOM_CAPSULE, GEOM_BOX
from support_f64_terrain import GEOM_HFIELD, GEOM_CYLINDER

MINVAL, MINIMP, MAXIMP = 1e-15, 0.0001, 0.9999      # the oracle's get_impedance
UNIT = (1.0, 0.0, 0.0, 0.0)


# ---- recipe P: per-geom solimp, solref and friction ----------------------------------------------------------------------------

def solimp_forms(width):
    """The six solimp forms the animat geoms cycle through; ``width`` is scaled to the model's penetration depth, so that
    |dist| / width falls on both sides of mid and below 1 (the default form's 1 mm saturates)."""
    return [(0.7, 0.95, width, 0.5, 1.0),       # power 1: linear
            (0.7, 0.95, width, 0.5, 2.0),       # power 2, mid 0.5
            (0.7, 0.95, width, 0.3, 3.0),       # power 3, mid 0.3
            (0.9, 0.9, width, 0.5, 2.0),        # flat: dmin == dmax
            (0.9, 0.95, 0.001, 0.5, 2.0),       # the default
            (0.8, 0.95, 0.0, 0.5, 2.0)]         # width 0


SOLREF_FORMS = [(0.02, 1.0), (0.001, 1.0), (0.01, 0.6), (0.03, 1.7), (-3000.0, -120.0), (-800.0, -40.0)]      # (0.001, 1): below 2 h, the clamp acts
GROUND_FRICTION = 0.8
# the width of the scaled solimp forms, per model: WIDTH x the depth its inputs press the deepest point in (a contact at that depth
# saturates, one at less than half of it is below mid)
WIDTH = 0.6
P_DEPTH = {'salamander33': 0.03, 'wide6': 0.5, 'centipede': 8e-3}


def grounds(m):
    return T.grounds(m)


def animat(m):
    return [g for g in range(m.ngeom) if g not in grounds(m)]


def geom_heights(m, qpos):
    """World z of the lowest point of every animat geom of one env (a cylinder's taken as its bounding sphere's)."""
    from farms_mujoco_amd.model import np_kinematics, quat2mat, quat_mul
    kin = np_kinematics(m, qpos)
    low = {}
    for g in animat(m):
        t, b = int(m.geom_type[g]), int(m.geom_bodyid[g])
        z = (kin['xpos'][b] + quat2mat(kin['xquat'][b]) @ m.geom_pos[g])[2]
        gz = quat2mat(quat_mul(kin['xquat'][b], m.geom_quat[g]))[2]; s = m.geom_size[g]
        low[g] = (z - s[0] if t == GEOM_SPHERE else z - abs(s[1]*gz[2]) - s[0] if t == GEOM_CAPSULE else
                  z - np.abs(gz*s).sum() if t == GEOM_BOX else z - np.hypot(s[0], s[1]))
    return low


def recipe_p(m, depth=None):
    """Recipe P on a compiled model.  The animat geoms are ranked by the height of their lowest point at the key pose, lowest first
    (the geoms that meet the ground come first, whatever their index); the geom of rank i takes solimp form i % 6 and solref form
    (i + i // 6) % 6 (every pairing within 36 geoms), and a friction uniform in 0.3 .. 1.3; every ground geom takes friction 0.8."""
    depth = P_DEPTH[m.name] if depth is None else depth
    forms = solimp_forms(WIDTH*depth)
    rng = np.random.default_rng([4242, m.ngeom])
    m.geom_solimp = m.geom_solimp.copy(); m.geom_solref = m.geom_solref.copy(); m.geom_friction = m.geom_friction.copy()
    low = geom_heights(m, m.key_qpos)
    for i, g in enumerate(sorted(animat(m), key=lambda g: (low[g], g))):
        m.geom_solimp[g] = forms[i % 6]
        m.geom_solref[g] = SOLREF_FORMS[(i + i//6) % 6]
        m.geom_friction[g] = (rng.uniform(0.3, 1.3), 0.0, 0.0)
    for g in grounds(m):
        m.geom_friction[g] = (GROUND_FRICTION, 0.0, 0.0)
    return m


def impedance_branch(solimp, dist):
    """The branch of the oracle's get_impedance a contact of distance ``dist`` takes (margin 0)."""
    dmin, dmax = (min(max(solimp[k], MINIMP), MAXIMP) for k in (0, 1))
    width, mid, power = max(0.0, solimp[2]), min(max(solimp[3], MINIMP), MAXIMP), max(1.0, solimp[4])
    if dmin == dmax or width <= MINVAL:
        return 'flat'
    x = abs(dist/width)
    if x >= 1:
        return 'saturated'
    assert x > 0
    return 'linear' if power == 1 else 'below_mid' if x <= mid else 'above_mid'


def solref_form(solref, h):
    return 'direct' if solref[0] <= 0 else 'floor_2h' if solref[0] < 2*h else 'time_constant'


def contact_branches(m, ref):
    """Over the batch, from the oracle's records: how many contacts with a normal force take each impedance branch and each meaning of
    solref; per env, how many contacts with a force take the ground's friction and how many their own geom's."""
    imp = dict(flat=0, saturated=0, linear=0, below_mid=0, above_mid=0)
    form = dict(time_constant=0, floor_2h=0, direct=0)
    n = len(ref['ncon'])
    ground_wins, geom_wins = np.zeros(n, int), np.zeros(n, int)
    for e in range(n):
        for c in range(int(ref['ncon'][e])):
            if not ref['contact'][e, c, 12] > 0:
                continue
            p, g = ref['geoms'][e, c]
            imp[impedance_branch(m.geom_solimp[g], ref['dist'][e, c])] += 1
            form[solref_form(m.geom_solref[g], m.timestep)] += 1
            assert m.geom_friction[p, 0] != m.geom_friction[g, 0]
            if m.geom_friction[p, 0] > m.geom_friction[g, 0]:
                ground_wins[e] += 1
            else:
                geom_wins[e] += 1
    return imp, form, ground_wins, geom_wins


# ---- models ------------------------------------------------------------------------------------------------------------------------

def insert_geom(m, at, gtype, size, pos, quat, friction):
    """A world-attached geom put in front of geom ``at`` (default solref / solimp): every later geom moves up by one."""
    ins = lambda a, v: np.insert(np.asarray(a), at, v, axis=0)
    m.geom_type = ins(m.geom_type, gtype).astype(np.int32); m.geom_bodyid = ins(m.geom_bodyid, 0).astype(np.int32)
    m.geom_size = ins(m.geom_size, size); m.geom_pos = ins(m.geom_pos, pos); m.geom_quat = ins(m.geom_quat, quat)
    m.geom_friction = ins(m.geom_friction, (friction, 0.0, 0.0))
    m.geom_solref = ins(m.geom_solref, (0.02, 1.0)); m.geom_solimp = ins(m.geom_solimp, (0.9, 0.95, 0.001, 0.5, 2.0))
    m.geom_vertadr = ins(m.geom_vertadr, -1).astype(np.int32); m.geom_vertnum = ins(m.geom_vertnum, 0).astype(np.int32)
    m.geom_faceadr = ins(m.geom_faceadr, -1).astype(np.int32); m.geom_facenum = ins(m.geom_facenum, 0).astype(np.int32)
    m.ngeom += 1
    return m


SECOND_FRICTION = 0.2
# the second plane of the two-plane models: how far its origin lies under the first plane's (m); it is tilted by 0.05 rad about (1, 2, 0)
SECOND_PLANE_Z = {'salamander33': -0.012, 'wide6': -0.12}


def second_plane(m):
    """A second world plane behind the first ground geom: tilted by 0.05 rad, a little lower, friction 0.2; max_contacts for both."""
    import farms_mujoco_amd.model as mm
    assert grounds(m) == [0]
    insert_geom(m, 1, GEOM_PLANE, (0, 0, 0), (0.0, 0.0, SECOND_PLANE_Z[m.name]), mm.axisangle2quat(np.array([1.0, 2.0, 0.0])/np.sqrt(5.0), 0.05),
                SECOND_FRICTION)
    m.max_contacts = min(128, 2*m.max_contacts)
    return m


def plane_under_hfield(m):
    """A level plane 1 cm under the lowest sample of the model's heightfield, behind it in geom order, friction 0.2."""
    assert grounds(m) == [0] and m.geom_type[0] == GEOM_HFIELD
    low = float(np.min(m.hfield_data))*float(m.hfield_size[2])
    insert_geom(m, 1, GEOM_PLANE, (0, 0, 0), (0.0, 0.0, low - 0.01), UNIT, SECOND_FRICTION)
    m.max_contacts = min(128, 2*m.max_contacts)
    return m


WELDED_BOXES = 4


def wide9():
    """WIDE_SHAPES tree 9 (72 bodies, 64 dofs, free base, a dof chain of 12; the bodies without a joint are welded to their parents)
    over the plane z = 0: a sphere on every body and a box as well on four of the welded bodies, in body order - 75 animat geoms, the
    last ones on lanes of the second wave."""
    from wide_trees import shape_tree
    m = shape_tree(9)
    rng = np.random.default_rng([99, 9])
    welded = [b for b in range(2, m.nbody) if m.body_dofnum[b] == 0]
    assert (m.nbody, m.nv) == (72, 64) and len(welded) >= WELDED_BOXES + 4
    boxed = welded[::len(welded)//WELDED_BOXES][:WELDED_BOXES]
    geoms = [(GEOM_PLANE, 0, (0, 0, 0), (0, 0, 0), UNIT, 0.0)]
    for b in range(1, m.nbody):
        geoms.append((GEOM_SPHERE, b, (float(rng.uniform(0.02, 0.04)), 0, 0), tuple(rng.normal(size=3)*0.01), UNIT, float(rng.uniform(0.5, 1.2))))
        if b in boxed:
            q = rng.normal(size=4); q /= np.linalg.norm(q)
            geoms.append((GEOM_BOX, b, tuple(rng.uniform(0.02, 0.04, 3)), tuple(rng.normal(size=3)*0.02), tuple(q), float(rng.uniform(0.5, 1.2))))
    return C.set_geoms(m, geoms, (m.nbody - 1) + 4*WELDED_BOXES)


def welded_geoms(m):
    """Animat geoms whose body has no dof of its own."""
    return [g for g in animat(m) if m.body_dofnum[m.geom_bodyid[g]] == 0]


def _solver(m, integrator, elliptic=False, impratio=1.0):
    import farms_mujoco_amd.model as mm
    m.integrator = mm.INTEGRATORS[integrator]
    m.solver = mm.SOLVERS['newton']; m.solver_iterations = 100
    m.impratio = float(impratio)
    if elliptic:
        m.cone = mm.CONES['elliptic']; m.solver_tolerance = E.TOLERANCE
    return m


# name: (model, what is done to it, integrator, kernel family, impratio)
#   models: those of support_f64_contacts.make / support_f64_terrain.make, and 'wide9'
#   'big': max_contacts = 128 and the inputs that press more than 64 contacts in; 'P': recipe P; '2planes': recipe P and the second
#   plane; 'hfield+plane': recipe P, the plane under the heightfield and the root at the grid's edge; 'welded': as built
CASES = {
    'big-euler': ('centipede_20_25', 'big', 'euler', 'contacts', 1.0),
    'big-implicitfast': ('centipede_20_25', 'big', 'implicitfast', 'contacts', 1.0),
    'big-terrain': ('centipede_hfield_cyl', 'big', 'euler', 'terrain', 1.0),
    'big-elliptic': ('centipede_20_25', 'big', 'euler', 'elliptic', 1.0),
    'P-salamander-euler': ('salamander33', 'P', 'euler', 'contacts', 1.0),
    'P-salamander-implicitfast': ('salamander33', 'P', 'implicitfast', 'contacts', 1.0),
    'P-salamander-impratio4': ('salamander33', 'P', 'euler', 'contacts', 4.0),
    'P-salamander-terrain': ('salamander33', 'P', 'euler', 'terrain', 1.0),
    'P-salamander-elliptic': ('salamander33', 'P', 'euler', 'elliptic', 1.0),
    'P-boxfoot-euler': ('boxfoot6', 'P', 'euler', 'contacts', 1.0),
    'P-boxfoot-implicitfast': ('boxfoot6', 'P', 'implicitfast', 'contacts', 1.0),
    'P-boxfoot-impratio4': ('boxfoot6', 'P', 'implicitfast', 'contacts', 4.0),
    'P-boxfoot-terrain': ('boxfoot6', 'P', 'euler', 'terrain', 1.0),
    'P-boxfoot-elliptic': ('boxfoot6', 'P', 'euler', 'elliptic', 1.0),
    'P-centipede-euler': ('centipede_20_25', 'P', 'euler', 'contacts', 1.0),
    '2planes-salamander': ('salamander33', '2planes', 'euler', 'contacts', 1.0),
    '2planes-boxfoot': ('boxfoot6', '2planes', 'implicitfast', 'contacts', 1.0),
    'hfield+plane-salamander': ('salamander_hfield_cyl', 'hfield+plane', 'euler', 'terrain', 1.0),
    'welded-contacts': ('wide9', 'welded', 'euler', 'contacts', 1.0),
    'welded-terrain': ('wide9', 'welded', 'implicitfast', 'terrain', 1.0),
}
# the depth the deepest point is pressed in and the largest tilt of the root, where they are not the model's own
# (support_f64_contacts.MODEL_INPUTS, support_f64_terrain.DEPTHS)
CASE_INPUTS = {'big': dict(depth=8e-3, tilt=0.005), 'big-terrain': dict(depth=7e-3, tilt=0.005), 'P-centipede-euler': dict(depth=8e-3, tilt=0.005),
               'boxfoot6': dict(depth=0.5), 'hfield+plane': dict(depth=0.05), 'welded': dict(depth=0.4, tilt=0.08)}
EDGE_XY = (-2.07, 0.0)     # 'hfield+plane': the salamander's head past the grid's edge at x = -2 m, its legs over the grid
# the seed of each case's inputs: the first of 100, 101, ... at which `conditions` holds in every env (first_seed finds them;
# test_f64_contact_recipes.py asserts the conditions at them, and every GPU case again before it looks at the device)
SEEDS = {'big-euler': 100, 'big-implicitfast': 100, 'big-terrain': 102, 'big-elliptic': 100,
         'P-salamander-euler': 115, 'P-salamander-implicitfast': 115, 'P-salamander-impratio4': 115, 'P-salamander-terrain': 115, 'P-salamander-elliptic': 115,
         'P-boxfoot-euler': 100, 'P-boxfoot-implicitfast': 100, 'P-boxfoot-impratio4': 100, 'P-boxfoot-terrain': 100, 'P-boxfoot-elliptic': 100,
         'P-centipede-euler': 100, '2planes-salamander': 101, '2planes-boxfoot': 100, 'hfield+plane-salamander': 100,
         'welded-contacts': 100, 'welded-terrain': 100}


def _inputs_kw(name):
    model, what = CASES[name][:2]
    return CASE_INPUTS.get(name, CASE_INPUTS.get(model, CASE_INPUTS.get(what, {})))


def make(name):
    model, what, integrator, family, impratio = CASES[name]
    m = wide9() if model == 'wide9' else (T if model in T.MODELS else C).make(model, integrator)
    if what == 'big':
        m.max_contacts = 128
    if what in ('P', '2planes', 'hfield+plane'):
        recipe_p(m, _inputs_kw(name).get('depth'))
    if what == '2planes':
        second_plane(m)
    if what == 'hfield+plane':
        plane_under_hfield(m)
    return _solver(m, integrator, family == 'elliptic', impratio)


def inputs(name, m, seed=None):
    model, what, _, _, _ = CASES[name]
    seed = SEEDS[name] if seed is None else seed
    kw = _inputs_kw(name)
    if model in T.MODELS:
        return T.inputs(m, N, seed, xy=EDGE_XY if what == 'hfield+plane' else (0.0, 0.0), **kw)
    return C.inputs(m, N, seed, **kw)


def case(name, seed=None):
    m = make(name)
    return m, inputs(name, m, seed), CASES[name][3]


def flags_of(m, family):
    return C.CONTACTS | (C.LIMITS if np.any(m.jnt_limited) else 0) | {'contacts': 0, 'terrain': T.TERRAIN, 'elliptic': E.ELLIPTIC | T.TERRAIN}[family]


KERNELS = {'contacts': 'fmj_step_f64_contacts_kernel', 'terrain': 'fmj_step_f64_terrain_kernel', 'elliptic': 'fmj_step_f64_elliptic_kernel'}


def phys(m, ins, family, **kw):
    return C.phys(m, N, ins, **dict(dict(fp64_terrain=family != 'contacts', fp64_elliptic=family == 'elliptic'), **kw))


# ---- conditions --------------------------------------------------------------------------------------------------------------------

def try_reference(oracle, m, ins):
    """support_f64_contacts.reference, or None where the oracle reports a status (a full contact list: no reference for a one-step case)."""
    a = oracle.step(m, ins['qpos'], ins['qvel'], ctrl=ins['ctrl'])
    return None if a['status'].any() else C.reference(oracle, m, ins)


def outside_points(m, qpos):
    """Per animat geom of one env: whether a point the narrow phase looks the heightfield up at (a sphere's or cylinder's centre, a
    capsule's ends, a box's corners) lies outside the grid."""
    from farms_mujoco_amd.model import np_kinematics, quat2mat, quat_mul
    kin = np_kinematics(m, qpos)
    hf = [p for p in grounds(m) if m.geom_type[p] == GEOM_HFIELD][0]
    out = {}
    for g in animat(m):
        t, b = int(m.geom_type[g]), int(m.geom_bodyid[g])
        gp = kin['xpos'][b] + quat2mat(kin['xquat'][b]) @ m.geom_pos[g]
        gm = quat2mat(quat_mul(kin['xquat'][b], m.geom_quat[g])); s = m.geom_size[g]
        pts = ([gp + s[1]*gm[:, 2], gp - s[1]*gm[:, 2]] if t == GEOM_CAPSULE else
               [gp + gm @ (np.array([sx, sy, sz])*s) for sz in (-1, 1) for sy in (-1, 1) for sx in (-1, 1)] if t == GEOM_BOX else [gp])
        out[g] = any(np.isinf(T.ground_dist(m, hf, pt)[0]) for pt in pts)
    return out


def conditions(oracle, name, m, ins):
    """What the case ``name`` is about, from the oracle alone; returns (ok, the reference, a description)."""
    model, what, _, family, _ = CASES[name]
    ref = try_reference(oracle, m, ins)
    if ref is None:
        return False, None, dict(status='the oracle reports a status')
    n = len(ref['ncon'])
    ncon = ref['ncon']
    force = [ref['contact'][e, :ncon[e], 12] > 0 for e in range(n)]
    forced = np.array([f.sum() for f in force]); idle = ncon - forced
    mind = np.array([np.abs(ref['dist'][e, :ncon[e]]).min() if ncon[e] else np.inf for e in range(n)])
    limited = bool(np.any(m.jnt_limited))
    limf = (E.limit_rows_with_force(ref) if family == 'elliptic' else C.engaged(m, ref)[2]) if limited else np.zeros(n, int)
    said = dict(ncon=ncon, forced=forced, idle=idle, min_abs_dist=mind, limit_rows_with_force=limf, iterations=ref['iterations'])
    ok = bool(forced.min() >= 4 and idle.min() >= 1 and mind.min() > 1e-9 and T.candidates_clear(m, ins))
    if limited:      # every env of a recipe-P case; some env under the elliptic cone (support_f64_elliptic.conditions: the cone changes
        # which) and in the two-ground cases, which are about the grounds
        ok = ok and bool((limf.min() if family != 'elliptic' and what == 'P' else limf.max()) >= 1)
    if family == 'elliptic':      # no contact within a relative 1e-3 of its cone's surface without being on it
        nearest = E.zones(m, ref)[3]
        said['nearest_inside'] = nearest
        ok = ok and bool(nearest.min() > 1e-3)
    if what == 'big':
        hi_forced = np.array([force[e][64:].sum() for e in range(n)]); hi_idle = np.array([(~force[e][64:]).sum() for e in range(n)])
        said.update(forced_in_slots_from_64=hi_forced, idle_in_slots_from_64=hi_idle)
        ok = ok and bool(ncon.min() > 64 and hi_forced.min() >= 4 and hi_idle.min() >= 1)
    if what in ('P', '2planes', 'hfield+plane'):
        imp, form, ground_wins, geom_wins = contact_branches(m, ref)
        said.update(impedance=imp, solref=form, ground_friction_wins=ground_wins, geom_friction_wins=geom_wins)
        ok = ok and min(imp.values()) >= 1 and min(form.values()) >= 1 and bool(ground_wins.min() >= 1 and geom_wins.min() >= 1)
    if what in ('2planes', 'hfield+plane'):
        gr = grounds(m)
        assert gr == [0, 1]
        per = np.array([[(ref['geoms'][e, :ncon[e], 0] == p).sum() for p in gr] for e in range(n)])
        both = np.array([len(set(ref['geoms'][e, :ncon[e], 1][ref['geoms'][e, :ncon[e], 0] == 0]) &
                             set(ref['geoms'][e, :ncon[e], 1][ref['geoms'][e, :ncon[e], 0] == 1])) for e in range(n)])
        major = all(np.all(np.diff(ref['geoms'][e, :ncon[e], 0]) >= 0) for e in range(n))
        said.update(contacts_per_ground=per.tolist(), geoms_on_both=both, ground_major=major)
        ok = ok and bool(per.min() >= 2 and both.min() >= 1 and major)
    if what == 'hfield+plane':      # a geom with a point outside the grid that the plane alone catches there
        caught = np.zeros(n, int)
        for e in range(n):
            out = outside_points(m, ins['qpos'][e])
            on_plane = set(ref['geoms'][e, :ncon[e], 1][ref['geoms'][e, :ncon[e], 0] == 1])
            caught[e] = sum(1 for g in on_plane if out[g])
        said['outside_the_grid_on_the_plane'] = caught
        ok = ok and bool(caught.min() >= 1)
    if what == 'welded':
        wg = welded_geoms(m)
        on_welded = np.array([np.isin(ref['geoms'][e, :ncon[e], 1][force[e]], wg).sum() for e in range(n)])
        past64 = np.array([(ref['geoms'][e, :ncon[e], 1][force[e]] >= 64).sum() for e in range(n)])
        said.update(forced_on_welded=on_welded, forced_on_geoms_from_64=past64)
        ok = ok and bool(on_welded.min() >= 1 and past64.min() >= 1)
    return ok, ref, said


def moved_by_a_tighter_tolerance(oracle, m, ins, ref):
    """How far a 100 x tighter tolerance with 200 iterations moves the reference, per field, in one-step bounds."""
    return E.moved_by_a_tighter_tolerance(oracle, m, ins, ref)


def first_seed(oracle, name, start=100, tries=60):
    m = make(name)
    for seed in range(start, start + tries):
        if conditions(oracle, name, m, inputs(name, m, seed))[0]:
            return seed
    raise AssertionError('no seed satisfies the conditions')


# ---- the truncated list --------------------------------------------------------------------------------------------------------------

TRUNCATED = 70      # max_contacts of the truncation case: past 64, below every env's 83 .. 92


# ---- narrow-phase branches on terrain: small hand-placed models ------------------------------------------------------------------------

def _table(geoms, ground, z0):
    """One free body with identity frames at (0, 0, z0) carrying ``geoms`` = [(type, size, pos, quat)], over ``ground``: 'hfield'
    (7 columns x 5 rows of samples over 1.2 m x 0.8 m, +-4 cm) or 'plane' (level, z = 0).  Friction 0.8 on the ground, 0.5 on the geoms."""
    from farms_mujoco_amd.model import ModelBuilder
    b = ModelBuilder('table', timestep=1e-3)
    b.add_body('b0', 'world', pos=(0, 0, z0), joint='free', mass=2.0, inertia=(0.05, 0.08, 0.1))
    for t, size, pos, quat in geoms:
        b.add_geom('b0', t, size, pos=pos, quat=quat, friction=(0.5, 0, 0))
    if ground == 'hfield':
        gy, gx = np.meshgrid(np.arange(5.0), np.arange(7.0), indexing='ij')
        b.add_hfield(0.5*np.sin(1.3*gx + 0.4)*np.cos(0.9*gy + 0.2) + 0.1*gx*gy/24.0, (0.6, 0.4, 0.08, 0.1), friction=(GROUND_FRICTION, 0, 0))
    else:
        b.add_geom('world', GEOM_PLANE, (0, 0, 0), friction=(GROUND_FRICTION, 0, 0))
    b.options['max_contacts'] = 4*len(geoms)
    m = b.compile()
    return _solver(m, 'euler')


def _surface(x, y):
    """Elevation of _table's heightfield under (x, y)."""
    from farms_mujoco_amd.model import hfield_height
    gy, gx = np.meshgrid(np.arange(5.0), np.arange(7.0), indexing='ij')
    return hfield_height(0.5*np.sin(1.3*gx + 0.4)*np.cos(0.9*gy + 0.2) + 0.1*gx*gy/24.0, (0.6, 0.4, 0.08, 0.1), x, y)


def narrow_case(which):
    """The model and inputs of one narrow-phase case on the terrain kernel (the root's frame is the identity; env e stands e x 0.5 mm
    lower; at rest, but for the upright cylinder); returns (m, ins).  Cells of the heightfield are 0.2 m x 0.2 m: column c = int((x + 0.6) / 0.2), row
    r = int((y + 0.4) / 0.2)."""
    import farms_mujoco_amd.model as mm
    r, z0 = 0.02, 0.0
    if which == 'last_cell':             # a sphere in the last column (5) and the last row (3) of cells, and one in cell (0, 0)
        spots = [(0.53, 0.31), (-0.47, -0.36)]
        geoms = [(GEOM_SPHERE, (r,), (x, y, _surface(x, y) + r - 0.006), UNIT) for x, y in spots]
    elif which == 'both_triangles':      # two spheres in cell (2, 1): one with fx > fy, one with fx < fy
        spots = [(-0.06, -0.17), (-0.17, -0.05)]
        geoms = [(GEOM_SPHERE, (r,), (x, y, _surface(x, y) + r - 0.006), UNIT) for x, y in spots]
    elif which == 'flat_box':            # a box lying flat, all eight corners under the surface: the first four only
        x, y = 0.09, 0.07
        geoms = [(GEOM_BOX, (0.03, 0.02, 0.004), (x, y, _surface(x, y) - 0.03), UNIT)]
    elif which == 'capsule_both_ends':   # a capsule lying along x, both end spheres in
        x, y = 0.3, -0.1
        geoms = [(GEOM_CAPSULE, (r, 0.03), (x, y, _surface(x, y) + r - 0.012), mm.axisangle2quat(np.array([0.0, 1.0, 0.0]), np.pi/2 - 0.1))]
    elif which == 'cylinder_axis_up':    # a cylinder whose z axis points up: prjaxis > 0, the axis is flipped
        x, y = -0.33, 0.1
        geoms = [(GEOM_CYLINDER, (r, 0.015), (x, y, _surface(x, y) + 0.015 - 0.008), mm.axisangle2quat(np.array([1.0, 0.0, 0.0]), 0.2))]
    elif which == 'cylinder_upright':    # exactly upright on the level plane: vec is exactly zero, the rim direction is the geom's x axis
        geoms = [(GEOM_CYLINDER, (0.03125, 0.015625), (0.0625, -0.03125, 0.0), UNIT)]      # off the body's centre: the contact forces turn it
        z0 = 0.0078125      # the lower disk 1/128 m under the plane (every operand a binary fraction)
    else:
        raise KeyError(which)
    m = _table(geoms, 'plane' if which == 'cylinder_upright' else 'hfield', z0)
    qpos = np.tile(m.key_qpos, (N, 1)).astype(float)
    qpos[:, 2] -= np.arange(N)*(0.00048828125 if which == 'cylinder_upright' else 0.0005)
    r32 = lambda a: np.asarray(a, np.float64).astype(np.float32).astype(np.float64)
    qvel = np.zeros((N, m.nv))
    if which == 'cylinder_upright':      # moving, so that no component of the reference is zero by symmetry (the narrow phase sees positions only)
        qvel[:] = (0.125, -0.25, 0.0625, 0.375, -0.125, 0.25)
    return m, dict(qpos=r32(qpos), qvel=qvel, ctrl=None)


NARROW = ('last_cell', 'both_triangles', 'flat_box', 'capsule_both_ends', 'cylinder_axis_up', 'cylinder_upright')


def narrow_branch(which, m, ins, ref):
    """Asserts, from the numpy narrow phase of support_f64_terrain.py and the oracle's records, that every env of the case takes the
    branch it is named after, and (but for the upright cylinder, whose operands are exact) that no decision grazes."""
    from farms_mujoco_amd.model import np_kinematics, quat2mat, quat_mul
    n = len(ins['qpos'])
    g0 = animat(m)[0]
    p = grounds(m)[0]
    for e in range(n):
        kin = np_kinematics(m, ins['qpos'][e])
        assert np.array_equal(kin['xquat'][1], UNIT)
        centre = lambda g: kin['xpos'][1] + m.geom_pos[g]
        gm = quat2mat(quat_mul(kin['xquat'][1], m.geom_quat[g0]))
        k = int(ref['ncon'][e])
        d, cells = T.candidates(m, ins['qpos'][e])
        if which != 'cylinder_upright':
            assert np.abs(d).min() > 1e-9 and cells.min() > 1e-9, (which, e)
        nc, nr = int(getattr(m, 'hfield_ncol', 0)), int(getattr(m, 'hfield_nrow', 0))
        cell = lambda pt: ((pt[0] + 0.6)/0.2, (pt[1] + 0.4)/0.2)
        if which == 'last_cell':
            gx, gy = cell(centre(g0))
            assert (int(gx), int(gy)) == (nc - 2, nr - 2) == (5, 3) and k == 2, (gx, gy, k)
        elif which == 'both_triangles':
            (ax, ay), (bx, by) = cell(centre(animat(m)[0])), cell(centre(animat(m)[1]))
            assert (int(ax), int(ay)) == (int(bx), int(by)) and ax % 1 > ay % 1 and bx % 1 < by % 1 and k == 2, (ax, ay, bx, by, k)
            assert np.abs(ref['contact'][e, 0, 3:6] - ref['contact'][e, 1, 3:6]).max() > 1e-3      # two planes: two normals
        elif which == 'flat_box':
            assert (d < 0).sum() == 8 and k == 4, (d, k)
        elif which == 'capsule_both_ends':
            assert (d < 0).sum() == 2 and k == 2, (d, k)
        elif which == 'cylinder_axis_up':
            nrm = T.ground_dist(m, p, centre(g0))[1]
            assert nrm @ gm[:, 2] > 0.5 and k >= 3, (nrm @ gm[:, 2], k)
        else:
            nrm = T.ground_dist(m, p, centre(g0))[1]
            axis = -gm[:, 2]
            vec = axis*(nrm @ axis) - nrm
            assert np.array_equal(nrm, (0, 0, 1)) and np.array_equal(gm, np.eye(3)) and not vec.any() and k == 3, (nrm, gm, vec, k)
            assert np.array_equal(ref['dist'][e, :3], np.full(3, d[0])) and d[0] < 0 < d[1]      # the three points of the lower rim, equally deep
            rim = ref['contact'][e, :3, :2] - centre(g0)[:2]      # the first at +x of the geom: the fallback's direction
            assert np.array_equal(rim[0], (0.03125, 0.0)) and abs(rim[1, 0] + 0.015625) < 1e-15 and abs(rim[2, 0] + 0.015625) < 1e-15, rim
