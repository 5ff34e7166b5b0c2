"""Models, inputs and oracle-side conditions that the fp64 elliptic-cone tests share (test_f64_elliptic_interface.py,
test_f64_elliptic_recipes.py, test_gpu_f64_elliptic.py): the fp64 contact solve under the elliptic cone (FMJ_CREATE_F64_CONTACTS |
FMJ_CREATE_F64_ELLIPTIC, fmj_step_f64_elliptic_kernel).  The models, inputs and seeds are those of support_f64_contacts.py (flat ground)
and support_f64_terrain.py (heightfield, cylinders) with ``cone = elliptic`` and ``solver_tolerance = 1e-10``: at the models' 1e-8 a
100 x tighter tolerance moves the oracle by up to 0.093 of the one-step bound (boxfoot6), at 1e-10 by at most 5.1e-4.  torch and the GPU
modules are imported inside the functions, so importing this module needs no GPU.  Every reference value comes from the oracle."""
import numpy as np

import support_f64_contacts as C
import support_f64_terrain as T
from support_f64_contacts import N, CONTACTS, LIMITS, RK4
from support_f64_terrain import TERRAIN

ELLIPTIC = 512      # FMJ_CREATE_F64_ELLIPTIC
TOLERANCE = 1e-10
# the one-step cases: (model, friction 0 on every geom, impratio)
ONE_STEP = ('salamander33', 'centipede_20_25', 'boxfoot6', 'salamander_hfield_cyl', 'boxfoot_hfield')
FURTHER = (('salamander33', False, 4.0), ('centipede_20_25', True, 1.0), ('centipede_hfield_cyl', True, 1.0))
# the seed of each model's inputs: those of the two support modules; `conditions` holds at them in every env (test_f64_elliptic_recipes.py)
SEEDS = dict(C.SEEDS, **T.SEEDS)
# per model, what every env must show: all three cone zones (a contact without force, one on the cone's surface, one strictly inside),
# or this many contacts on the surface
THREE_ZONES = ('salamander33', 'boxfoot6', 'boxfoot_hfield')
SURFACE_AT_LEAST = {'centipede_20_25': 4, 'centipede_hfield_cyl': 4, 'centipede_hfield': 4}


def on_terrain(name):
    return name not in C.MODELS


def make(name, integrator='euler', friction0=False, impratio=1.0):
    """The model of ``name`` (support_f64_contacts.make or support_f64_terrain.make: Newton, 100 iterations) under the elliptic cone at
    solver_tolerance = 1e-10.  ``friction0``: every geom's friction 0 (a contact's is then MuJoCo's floor, 1e-5)."""
    import farms_mujoco_amd.model as mm
    m = (T if on_terrain(name) else C).make(name, integrator)
    m.cone = mm.CONES['elliptic']
    m.solver_tolerance = TOLERANCE
    m.impratio = float(impratio)
    if friction0:
        m.geom_friction = np.zeros_like(m.geom_friction)
    return m


def inputs(name, m, n=N, seed=None, **kw):
    return (T if on_terrain(name) else C).inputs(m, n, SEEDS[name] if seed is None else seed, **kw)


def flags_of(name, m):
    return CONTACTS | ELLIPTIC | (TERRAIN if on_terrain(name) else 0) | (LIMITS if np.any(m.jnt_limited) else 0)


def phys(name, m, n, ins, **kw):
    return C.phys(m, n, ins, **dict(dict(fp64_elliptic=True, fp64_terrain=on_terrain(name)), **kw))


def zones(m, ref):
    """Every oracle contact classified from its record (force = normal, tangent 1, tangent 2 in the contact frame; the friction is the
    larger of the two geoms', floor 1e-5): per env the number without force (top zone), on the cone's surface (middle zone:
    |f_t| = fr f_n to rounding) and strictly inside (bottom zone), and the smallest relative distance (fr f_n - |f_t|) / (fr f_n) of an
    inside contact."""
    n = len(ref['ncon'])
    none, surface, inside = np.zeros(n, int), np.zeros(n, int), np.zeros(n, int)
    nearest = np.full(n, np.inf)
    for e in range(n):
        k = int(ref['ncon'][e])
        f = ref['contact'][e, :k, 12:15]
        g = ref['geoms'][e, :k]
        fr = np.maximum(np.maximum(m.geom_friction[g[:, 0], 0], m.geom_friction[g[:, 1], 0]), 1e-5)
        ft = np.hypot(f[:, 1], f[:, 2])
        for c in range(k):
            if not f[c, 0] > 0:
                assert ft[c] == 0
                none[e] += 1
                continue
            rel = (fr[c]*f[c, 0] - ft[c])/(fr[c]*f[c, 0])
            if abs(rel) <= 1e-9:
                surface[e] += 1
            else:
                assert rel > 0, (e, c, rel)      # a force outside its cone
                inside[e] += 1
                nearest[e] = min(nearest[e], rel)
    return none, surface, inside, nearest


def limit_rows_with_force(ref):
    """Per env, the oracle's limit rows with a force (three rows per contact follow them)."""
    nlim = ref['nefc'] - 3*ref['ncon']
    return np.array([(ref['efc'][e, :nlim[e], 0] > 0).sum() for e in range(len(nlim))])


def moved_by_a_tighter_tolerance(oracle, m, ins, ref):
    """How far a 100 x tighter tolerance (1e-12, 200 iterations) moves the reference, per field, in one-step bounds."""
    import support_f64_step as S
    tight = C.reference(oracle, m, ins, tighter=True)
    groups = C._groups(m)
    moved = {k: S.ulp_excess(tight[k], ref[k], groups[k]) for k in C.STATE}
    moved['contact'] = C._contact_excess(tight['contact'], ref['ncon'], ref)
    assert np.array_equal(tight['ncon'], ref['ncon'])
    return moved


def conditions(oracle, name, m, ins, want_zones=True):
    """What the GPU cases rely on, from the oracle alone; returns (ok, the reference, a description).  ``want_zones`` False (the
    friction-0 and impratio cases): a contact with a force in every env is enough."""
    ref = C.reference(oracle, m, ins)
    none, surface, inside, nearest = zones(m, ref)
    mind = np.array([np.abs(ref['dist'][e, :ref['ncon'][e]]).min() if ref['ncon'][e] else np.inf for e in range(len(ref['ncon']))])
    ok = bool((surface + inside).min() >= 1 and nearest.min() > 1e-3 and mind.min() > 1e-9 and T.candidates_clear(m, ins))
    if want_zones and name in THREE_ZONES:
        ok = ok and bool(none.min() >= 1 and surface.min() >= 1 and inside.min() >= 1)
    if want_zones and name in SURFACE_AT_LEAST:
        ok = ok and bool(surface.min() >= SURFACE_AT_LEAST[name])
    limf = limit_rows_with_force(ref)
    if np.any(m.jnt_limited):      # limit rows share the solve: some env has one with a force (not every env: the cone changes which)
        ok = ok and bool(limf.max() >= 1)
    return ok, ref, dict(limit_rows_with_force=limf, no_force=none, surface=surface, inside=inside, nearest_inside=nearest, min_abs_dist=mind, ncon=ref['ncon'],
                         iterations=ref['iterations'])


def first_seed(oracle, name, n=N, start=100, tries=60, **kw):
    m = make(name, **kw)
    for seed in range(start, start + tries):
        if conditions(oracle, name, m, inputs(name, m, n, seed))[0]:
            return seed
    raise AssertionError('no seed satisfies the conditions')
