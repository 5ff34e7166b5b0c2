"""Walking models, inputs and oracle read-outs that the fp64 ground-contact tests share (test_f64_contacts_interface.py,
test_gpu_f64_contacts.py).  torch and the GPU test modules are imported inside the functions, so importing this module needs no GPU.

The oracle (Newton, 100 iterations, the model's tolerance) gives every reference value.  ``reference`` joins its two read-outs of one
step: fmjo_step (state, poses, sensors, the qacc the integrator used) and fmjo_step_tf (contact records, ncon, the constrained qacc
that mj_step saves as the next warm start)."""
import numpy as np

from wide_trees import shape_tree

GEOM_PLANE, GEOM_SPHERE, GEOM_CAPSULE, GEOM_BOX = 0, 2, 3, 6
FMJ_WARN_CONTACTFULL = 8
N = 4
MODELS = ('salamander33', 'centipede_20_25', 'boxfoot6')
CONTACTS, LIMITS, RK4 = 32, 1, 8      # FMJ_CREATE_F64_CONTACTS, _LIMITS, _RK4


def set_geoms(m, geoms, max_contacts):
    """Put collision geoms on a compiled model: ``geoms`` = [(type, body, size(3), pos(3), quat(4), friction)], the plane first, as
    Model._from_builder orders them (world body first).  Default solref / solimp."""
    n = len(geoms)
    m.ngeom = n
    m.geom_type = np.array([g[0] for g in geoms], np.int32)
    m.geom_bodyid = np.array([g[1] for g in geoms], np.int32)
    m.geom_size = np.array([g[2] for g in geoms], float).reshape(n, 3)
    m.geom_pos = np.array([g[3] for g in geoms], float).reshape(n, 3)
    m.geom_quat = np.array([g[4] for g in geoms], float).reshape(n, 4)
    m.geom_friction = np.array([[g[5], 0, 0] for g in geoms], float).reshape(n, 3)
    m.geom_solref = np.tile([0.02, 1.0], (n, 1)).astype(float)
    m.geom_solimp = np.tile([0.9, 0.95, 0.001, 0.5, 2.0], (n, 1)).astype(float)
    m.geom_vertadr = np.full(n, -1, np.int32); m.geom_vertnum = np.zeros(n, np.int32)
    m.geom_faceadr = np.full(n, -1, np.int32); m.geom_facenum = np.zeros(n, np.int32)
    m.max_contacts = int(max_contacts)
    return m


def boxfoot(shape=6, n_feet=14):
    """WIDE_SHAPES tree ``shape`` (6: 64 bodies, 68 dofs, free base, dof chain 40) with a box on each of its last ``n_feet`` bodies and
    a capsule on its root, over the friction-0 plane z = 0 with its frame turned about z (a frame that is not the identity)."""
    m = shape_tree(shape)
    rng = np.random.default_rng([99, shape])
    unit = (1.0, 0.0, 0.0, 0.0)
    geoms = [(GEOM_PLANE, 0, (0, 0, 0), (0, 0, 0), (np.cos(0.2), 0.0, 0.0, np.sin(0.2)), 0.0),
             (GEOM_CAPSULE, 1, (0.03, 0.05, 0), (0.01, 0, 0), unit, 0.7)]
    for b in range(m.nbody - n_feet, m.nbody):
        q = rng.normal(size=4); q /= np.linalg.norm(q)
        geoms.append((GEOM_BOX, b, tuple(rng.uniform(0.02, 0.05, 3)), tuple(rng.normal(size=3)*0.01), tuple(q), float(rng.uniform(0.5, 1.2))))
    return set_geoms(m, geoms, 2 + 4*n_feet)


def make(name, integrator='euler'):
    """The walking model of ``name`` with the reference's solver fields: Newton, 100 iterations."""
    import farms_mujoco_amd.model as mm
    m = {'salamander33': lambda: mm.salamander33(contacts=True, limits=True), 'centipede_20_25': lambda: mm.centipede(20, 25, contacts=True),
         'boxfoot6': boxfoot}[name]()
    m.integrator = mm.INTEGRATORS[integrator]
    m.solver = mm.SOLVERS['newton']; m.solver_iterations = 100
    return m


def flags_of(m):
    return CONTACTS | (LIMITS if np.any(m.jnt_limited) else 0)


def scalar_q(m):
    return m.jnt_qposadr[m.jnt_type != 0]


def lowest_point(m, qpos):
    """Height of the lowest point of any animat geom (spheres, capsule ends, box corners) of one env above z = 0."""
    from farms_mujoco_amd.model import np_kinematics, quat2mat, quat_mul
    kin = np_kinematics(m, qpos)
    low = np.inf
    for g in range(m.ngeom):
        t, b = int(m.geom_type[g]), int(m.geom_bodyid[g])
        if t == GEOM_PLANE:
            continue
        R = quat2mat(kin['xquat'][b]); gp = kin['xpos'][b] + R @ m.geom_pos[g]
        gm = quat2mat(quat_mul(kin['xquat'][b], m.geom_quat[g])); s = m.geom_size[g]
        if t == GEOM_SPHERE:
            low = min(low, gp[2] - s[0])
        elif t == GEOM_CAPSULE:
            low = min(low, gp[2] + s[1]*gm[2, 2] - s[0], gp[2] - s[1]*gm[2, 2] - s[0])
        else:
            low = min(low, min(gp[2] + gm[2] @ (np.array([sx, sy, sz])*s) for sx in (-1, 1) for sy in (-1, 1) for sz in (-1, 1)))
    return low


# per model: how far the lowest geom point is pushed below the plane (m) and the largest tilt of the root (rad)
MODEL_INPUTS = {'salamander33': (0.03, 0.01), 'centipede': (2e-3, 0.08), 'wide6': (0.3, 0.08)}
# the seed of each model's inputs: the first of 100, 101, ... at which `conditions` holds in every env (first_seed finds them; the
# tests assert the conditions before they look at the device)
SEEDS = {'salamander33': 115, 'centipede_20_25': 100, 'boxfoot6': 111}


def inputs(m, n, seed, depth=None, tilt=None):
    """Random joint positions (+-0.15; three joints of a limited model at or past their upper limit), a tilted root, qvel normal x
    0.3, ctrl uniform +-0.3, and the root lowered until the lowest geom point is ``depth`` below the plane.  Rounded to fp32."""
    if depth is None:
        depth = MODEL_INPUTS[m.name][0]
    if tilt is None:
        tilt = MODEL_INPUTS[m.name][1]
    rng = np.random.default_rng([777, seed])
    qpos = np.tile(m.key_qpos, (n, 1)).astype(float)
    sq = scalar_q(m)
    qpos[:, sq] = rng.uniform(-0.15, 0.15, (n, len(sq)))
    if np.any(m.jnt_limited):      # a few joints at or past their limit
        lim = np.nonzero(m.jnt_limited)[0]
        for e in range(n):
            for j in rng.choice(lim, size=3, replace=False):
                qpos[e, m.jnt_qposadr[j]] = m.jnt_range[j][1] + rng.uniform(-0.005, 0.03)
    if m.jnt_type[0] == 0:
        for e in range(n):
            ax = rng.normal(size=3); ax /= np.linalg.norm(ax); ang = rng.uniform(-tilt, tilt)
            qpos[e, 3:7] = [np.cos(ang/2), *(np.sin(ang/2)*ax)]
            qpos[e, 2] = 0.0
            qpos[e, 2] = -lowest_point(m, qpos[e]) - depth
    qvel = rng.normal(size=(n, m.nv))*0.3
    ctrl = rng.uniform(-0.3, 0.3, (n, max(m.nu, 1)))[:, :m.nu]
    r = lambda a: np.asarray(a, np.float64).astype(np.float32).astype(np.float64)
    return dict(qpos=r(qpos), qvel=r(qvel), ctrl=r(ctrl) if m.nu else None)


def reference(oracle, m, ins, tighter=False):
    """One oracle step of ``ins``: the fields of fmjo_step, plus contact [n, max_contacts, 15] (pos, frame, force), geoms, dist, ncon,
    nefc, efc and qacc_warmstart from fmjo_step_tf.  ``tighter``: a 100 x tighter tolerance and 200 iterations."""
    import copy
    if tighter:
        m = copy.copy(m); m.solver_tolerance = m.solver_tolerance/100; m.solver_iterations = 200
    a = oracle.step(m, ins['qpos'], ins['qvel'], ctrl=ins['ctrl'])
    b = oracle.step_tf(m, ins['qpos'], ins['qvel'], ctrl=ins['ctrl'], want_AR=False)
    assert np.array_equal(a['qpos'], b['qpos']) and not a['status'].any(), a['status']
    a.update(contact=b['contact'][..., :15], geoms=b['contact'][..., 15:17].astype(int), dist=b['contact'][..., 17], ncon=b['ncon'],
             nefc=b['nefc'], efc=b['efc'], qacc_warmstart=b['warmstart'], iterations=b['iterations'])
    return a


def engaged(m, ref):
    """Per env, from the oracle's step: contacts with a normal force, penetrating contacts without, limit rows with a force, and the
    smallest |dist| of a contact (a grazing decision would be one near 0)."""
    n = len(ref['ncon'])
    forced = np.array([(ref['contact'][e, :ref['ncon'][e], 12] > 0).sum() for e in range(n)])
    idle = ref['ncon'] - forced
    nlim = ref['nefc'] - 4*ref['ncon']
    limf = np.array([(ref['efc'][e, :nlim[e], 0] > 0).sum() for e in range(n)])
    mind = np.array([np.abs(ref['dist'][e, :ref['ncon'][e]]).min() if ref['ncon'][e] else np.inf for e in range(n)])
    return forced, idle, limf, mind


def candidates_clear(m, ins, eps=1e-9):
    """No geom point of any env is within ``eps`` of the plane: no grazing decision in the narrow phase."""
    from farms_mujoco_amd.model import np_kinematics, quat2mat, quat_mul
    for e in range(len(ins['qpos'])):
        kin = np_kinematics(m, ins['qpos'][e])
        for g in range(m.ngeom):
            t, b = int(m.geom_type[g]), int(m.geom_bodyid[g])
            if t == GEOM_PLANE:
                continue
            R = quat2mat(kin['xquat'][b]); gp = kin['xpos'][b] + R @ m.geom_pos[g]
            gm = quat2mat(quat_mul(kin['xquat'][b], m.geom_quat[g])); s = m.geom_size[g]
            if t == GEOM_SPHERE:
                d = [gp[2] - s[0]]
            elif t == GEOM_CAPSULE:
                d = [gp[2] + s[1]*gm[2, 2] - s[0], gp[2] - s[1]*gm[2, 2] - s[0]]
            else:
                d = [gp[2] + gm[2] @ (np.array([sx, sy, sz])*s) for sx in (-1, 1) for sy in (-1, 1) for sz in (-1, 1)]
            if np.abs(d).min() <= eps:
                return False
    return True


def conditions(oracle, m, ins, want_limits):
    """What the issue asks of a one-step case, from the oracle alone; returns (ok, the reference, a description)."""
    ref = reference(oracle, m, ins)
    forced, idle, limf, mind = engaged(m, ref)
    ok = forced.min() >= 4 and idle.min() >= 1 and mind.min() > 1e-9 and candidates_clear(m, ins) and (not want_limits or limf.min() >= 1)
    return ok, ref, dict(forced=forced, idle=idle, limit_rows_with_force=limf, min_abs_dist=mind, ncon=ref['ncon'], iterations=ref['iterations'])


def first_seed(oracle, m, n, want_limits, start=100, tries=40):
    for seed in range(start, start + tries):
        ok, _, _ = conditions(oracle, m, inputs(m, n, seed), want_limits)
        if ok:
            return seed
    raise AssertionError('no seed satisfies the conditions')


def phys(m, n, ins, precision='fp64', **kw):
    import torch
    from farms_mujoco_amd.physics import BatchedPhysics
    if precision == 'fp64':
        kw = dict(dict(fp64_contacts=True, fp64_limits=bool(np.any(m.jnt_limited))), **kw)
    p = BatchedPhysics(m, n, precision=precision, **kw)
    assert p.precision == precision
    f32 = lambda a: torch.as_tensor(np.asarray(a), dtype=torch.float32)
    p.data.qpos[:] = f32(ins['qpos']); p.data.qvel[:] = f32(ins['qvel'])
    if m.nu and ins.get('ctrl') is not None:
        p.data.ctrl[:] = f32(ins['ctrl'])
    return p


def walk_tape(m, n, T, f=2.0, spine=0.1, legs=0.1, stance=0.25):
    """ctrl[t, env, a]: a travelling wave on the spine joints, a swing of the upper leg joints alternating by side and segment, and
    the lower legs held ``stance`` further down than at qpos0 (the feet reach for the ground)."""
    t = np.arange(T)[:, None, None]*m.timestep
    tape = np.zeros((T, n, m.nu))
    spine_j = [j for j, nm in enumerate(m.joint_names) if nm.startswith('joint_body_')]
    for a in range(m.nu):
        j = int(m.actuator_jntid[a]); nm = m.joint_names[j]
        ph = 2*np.pi*f*t[:, :, 0] + 0.7*np.arange(n)[None, :]
        if j in spine_j:
            tape[:, :, a] = spine*np.sin(ph - 2*np.pi*spine_j.index(j)/len(spine_j))
        elif nm.endswith('_0'):
            seg = int(nm.split('_')[2]); side = 1.0 if '_L_' in nm else -1.0
            tape[:, :, a] = legs*np.sin(ph + np.pi*seg + (0 if side > 0 else np.pi))
        elif nm.endswith('_1'):
            tape[:, :, a] = -stance if '_L_' in nm else stance
    return tape.astype(np.float32)


STATE = ('qpos', 'qvel', 'qacc', 'qacc_warmstart', 'sensordata', 'xpos', 'xquat', 'xipos')


def _groups(m):
    import support_f64_step as S
    g = S._field_groups(m)
    g['qacc_warmstart'] = g['qacc']
    return g


def _contact_groups():
    """Columns of one physical kind in a contact record: position, frame, force."""
    return [np.arange(0, 3), np.arange(3, 12), np.arange(12, 15)]


def _contact_excess(got16, ncon_got, ref):
    """ulp excess of the records (pos, frame, force) of every env's contacts, the groups taken per env over its contacts."""
    import support_f64_step as S
    worst = 0.0
    for e in range(len(ncon_got)):
        k = int(ref['ncon'][e])
        if k == 0:
            continue
        g, r = got16[e, :k, :15].astype(np.float64), ref['contact'][e, :k]
        for cols in _contact_groups():
            worst = max(worst, S.ulp_excess(g[None, :, cols], r[None, :, cols]))
    return worst


def _excess(m, p, ref, forward, ins):
    import support_f64_step as S
    import torch
    torch.cuda.synchronize()
    assert int(p.data.status.abs().sum()) == 0
    if forward:
        ref = dict(ref, qpos=ins['qpos'], qvel=ins['qvel'])
    groups = _groups(m)
    fields = [k for k in STATE if not (forward and k == 'qacc_warmstart')]      # (mj_forward saves no warm start)
    ex = {k: S.ulp_excess(getattr(p.data, k).cpu().numpy(), ref[k], groups[k]) for k in fields}
    ncon = p.data.ncon.cpu().numpy()
    assert np.array_equal(ncon, ref['ncon']), (ncon, ref['ncon'])
    c16 = p.data.contact.cpu().numpy()
    for e in range(len(ncon)):
        gg = np.ascontiguousarray(c16[e, :ncon[e], 15]).view(np.int32)
        assert np.array_equal(gg >> 16, ref['geoms'][e, :ncon[e], 0]) and np.array_equal(gg & 0xffff, ref['geoms'][e, :ncon[e], 1]), e
    ex['contact'] = _contact_excess(c16, ncon, ref)
    return ex
