"""Seeded random kinematic trees for the two-wave step kernel (csrc/fmj_wide.inc): unconstrained trees of 2..128 bodies and 1..128
dofs with the ingredients of ``random_tree`` in test_gpu_random_trees.py (hinge and slide joints with off-centre anchors and arbitrary
axes, welded bodies, rotated body frames and full inertias, a free / fixed / hinged base, damping, stiffness with qpos0 offsets,
armature, position / velocity-gain / motor actuators with ctrl and force ranges, both gravities), drawn at a chosen size and shape.

``WIDE_SHAPES`` are the trees the tests run; ``tree_properties`` reads from a compiled model what the kernel will make of it (the
model-wide shortcuts and the elimination rounds of fmj_create), so that the coverage claim can be checked without a GPU."""
import numpy as np

LANES = 128          # FMJ_WIDE_LANES: one workgroup of two wavefronts per env
MAX_CHAIN = 64       # FMJ_MAXD_DEEP: the longest dof chain an unconstrained model may have

# (seed, nbody, nv, base, longest dof chain); nbody counts the world body, the chain counts dofs (a free base is six)
WIDE_SHAPES = [
    (1, 128, 128, 'free', 64),       # both counts at the limit, nq 129, a chain of exactly 64
    (2, 128, 128, 'free', 33),       # the shortest chain of the rs = 64 build
    (3, 128, 126, 'fixed', 32),      # the longest chain of the rs = 32 build, root welded to the world
    (4, 128, 127, 'hinge', 20),      # hinged (or sliding) base, wide levels
    (5, 100, 40, 'hinge', 24),       # nbody past 64 with every dof in wave 0 (welded bodies)
    (6, 64, 68, 'free', 40),         # dofs in wave 1 with no body there
    (7, 128, 70, 'fixed', 48),       # many welded bodies, deep body chains
    (8, 90, 90, 'free', 64),
    (9, 72, 64, 'free', 12),         # nv exactly 64, a shallow bushy tree
    (10, 66, 65, 'hinge', 30),
    (11, 2, 1, 'hinge', 1),          # the smallest model: one body, one dof
    (12, 30, 25, 'free', 16),        # a small tree: most lanes idle
]


def wide_random_tree(seed, nbody, nv, base='free', chain=None, actuators='random', integrator='Euler'):
    """A tree of exactly ``nbody`` bodies (world included) and ``nv`` dofs whose longest dof chain is exactly ``chain`` (default: drawn).
    ``base``: 'free' (six dofs), 'fixed' (root welded to the world) or 'hinge' (a hinge or slide root).  ``actuators``: 'random'
    (the mix of random_tree plus ctrl ranges) or 'triple' (the position / velocity / motor triple on every joint, velocity gain > 0)."""
    from farms_mujoco_amd.model import ModelBuilder, euler2quat
    rng = np.random.default_rng([7919, seed])
    bd = {'free': 6, 'fixed': 0, 'hinge': 1}[base]
    n_joint = nv - bd                         # jointed bodies below the root
    n_weld = nbody - 2 - n_joint              # welded bodies below the root
    assert 2 <= nbody <= LANES and 1 <= nv <= LANES and n_joint >= 0 and n_weld >= 0, (nbody, nv, base)
    lo, hi = max(bd, 1 if n_joint else bd), min(bd + n_joint, MAX_CHAIN)
    chain = int(rng.integers(lo, hi + 1)) if chain is None else int(chain)
    assert lo <= chain <= hi, (chain, lo, hi)
    g = (0, 0, -9.81) if rng.integers(0, 2) else (0.5, -0.3, -9.0)
    b = ModelBuilder(f'wide{seed}', timestep=1e-3, gravity=g)

    def inertia():
        A = rng.normal(size=(3, 3)); S = A @ A.T*1e-4 + np.eye(3)*2e-4
        return (S[0, 0], S[1, 1], S[2, 2], S[0, 1], S[0, 2], S[1, 2])

    def body_kw():
        return dict(mass=float(rng.uniform(0.05, 0.5)), ipos=rng.normal(size=3)*0.03, fullinertia=inertia())

    def joint_kw():
        jt = 'hinge' if rng.random() < 0.8 else 'slide'
        return dict(joint=jt, axis=rng.normal(size=3), jpos=rng.normal(size=3)*0.03 if rng.random() < 0.5 else (0, 0, 0),
                    damping=float(rng.choice([0.0, 2e-3, 1e-2])), stiffness=float(rng.choice([0.0, 0.0, 0.05])),
                    armature=float(rng.choice([0.0, 1e-4])), qpos0=float(rng.choice([0.0, 0.2])))

    names, ndof = [], []                      # per body: name, dofs on the path root..body
    if base == 'free':
        b.add_body('b0', 'world', pos=rng.normal(size=3)*0.2, quat=euler2quat(rng.normal(size=3)), joint='free', **body_kw())
    elif base == 'fixed':
        b.add_body('b0', 'world', pos=rng.normal(size=3)*0.2, quat=euler2quat(rng.normal(size=3)), **body_kw())
    else:
        jk = joint_kw(); jk['damping'] = 0.01
        b.add_body('b0', 'world', pos=rng.normal(size=3)*0.2, quat=euler2quat(rng.normal(size=3)), **jk, **body_kw())
    names.append('b0'); ndof.append(bd)

    def add(parent, jointed):
        name = f'b{len(names)}'
        jk = joint_kw() if jointed else {}
        b.add_body(name, names[parent], pos=rng.normal(size=3)*0.08, quat=euler2quat(rng.normal(size=3)*0.5), **jk, **body_kw())
        names.append(name); ndof.append(ndof[parent] + int(jointed))

    # the spine carries the longest chain; some welded bodies sit inside it (body chains deeper than the dof chain)
    spine = chain - bd
    welds_in_spine = int(rng.integers(0, n_weld + 1))//2 if spine else 0
    kinds = [True]*spine + [False]*welds_in_spine
    rng.shuffle(kinds)
    for jointed in kinds:
        add(len(names) - 1, jointed)
    # the rest: a shuffled mix, each hung under a body that keeps the chain within bounds - a few hubs (wide levels), the last
    # bodies added (deep branches) or any body
    rest = [True]*(n_joint - spine) + [False]*(n_weld - welds_in_spine)
    rng.shuffle(rest)
    hubs = list(rng.choice(len(names), size=min(3, len(names)), replace=False))
    for jointed in rest:
        ok = [i for i in range(len(names)) if ndof[i] + jointed <= chain]
        u = rng.random()
        if u < 0.3:
            cand = [i for i in hubs if ndof[i] + jointed <= chain] or ok
        elif u < 0.65:
            cand = [i for i in ok if i >= len(names) - 6] or ok
        else:
            cand = ok
        add(int(rng.choice(cand)), jointed)
    assert len(names) == nbody - 1 and max(ndof) == chain
    joints = [bdy.joint['name'] for bdy in b.bodies[1:] if bdy.joint and bdy.joint['type'] != 0]
    for jn in joints:
        r = rng.random()
        if actuators == 'triple' or r < 0.5:
            lim = lambda: dict(ctrllimited=True, ctrlrange=(-0.3, 0.4)) if rng.random() < 0.3 else None
            b.add_joint_actuators(jn, kp=float(rng.uniform(0.1, 0.5)), kv=float(rng.uniform(1e-3, 0.01)),
                                  forcerange=(-0.2, 0.3) if rng.random() < 0.5 else None, pos_limits=lim(), vel_limits=lim())
        elif r < 0.75:
            b.add_position_actuator(jn, kp=0.3)
    b.options['integrator'] = integrator
    m = b.compile()
    assert (m.nbody, m.nv) == (nbody, nv)
    return m


def shape_tree(seed, **kw):
    """The tree of a WIDE_SHAPES entry."""
    s = [x for x in WIDE_SHAPES if x[0] == seed][0]
    return wide_random_tree(s[0], s[1], s[2], s[3], s[4], **kw)


def dof_depth(m):
    depth = np.zeros(m.nv, int)
    for i in range(m.nv):
        depth[i] = 0 if m.dof_parentid[i] < 0 else depth[m.dof_parentid[i]] + 1
    return depth


def elimination_rounds(m):
    """The rounds of fmj_create's two-wave branch: dof levels deepest first, each split into chunks of six in index order."""
    depth = dof_depth(m)
    rounds = []
    for dep in range(int(depth.max()), -1, -1):
        lvl = [i for i in range(m.nv) if depth[i] == dep]
        rounds += [lvl[q:q + 6] for q in range(0, len(lvl), 6)]
    return rounds


def tree_properties(m):
    """What the two-wave kernel makes of a compiled model, from its arrays alone (fmj_create, fmj_hip.hip)."""
    nb, nv = m.nbody, m.nv
    free = m.jnt_type == 0
    anchored = [j for j in range(m.njnt) if not free[j] and np.any(m.jnt_pos[j] != 0)]
    bquat = [i for i in range(1, nb) if not (m.body_jntadr[i] >= 0 and free[m.body_jntadr[i]])
             and not (abs(m.body_quat[i, 0]) == 1.0 and np.all(m.body_quat[i, 1:] == 0))]
    iquat = [i for i in range(1, nb) if not (m.body_iquat[i, 0] == 1.0 and np.all(m.body_iquat[i, 1:] == 0))]
    bdepth = np.zeros(nb, int)
    for i in range(2, nb):
        bdepth[i] = bdepth[m.body_parentid[i]] + 1
    longest_body_chain = int(bdepth[1:].max()) + 1
    jump_rounds = int(np.ceil(np.log2(longest_body_chain))) if longest_body_chain > 1 else 0
    depth = dof_depth(m)
    chain = int(depth.max()) + 1
    rs = -(-chain//4)*4
    rounds = elimination_rounds(m)
    levels = np.bincount(depth)
    kv = [a for a in range(m.nu) if m.actuator_tags[a] == 'velocity' and m.actuator_gain[a] != 0]
    j1 = m.body_jntadr[1]
    return dict(
        nbody=nb, nv=nv, nq=m.nq,
        any_jpos=bool(anchored), any_bquat=bool(bquat), any_iquat=bool(iquat),
        base='fixed' if j1 < 0 else 'free' if free[j1] else 'hinged',
        hinge=bool(np.any(m.jnt_type == 3)), slide=bool(np.any(m.jnt_type == 2)), welded=bool(np.any(m.body_jntadr[1:] < 0)),
        damping=bool(np.any(m.dof_damping != 0)), stiffness=bool(np.any(m.jnt_stiffness[~free] != 0)),
        qpos0_offset=bool(np.any(m.qpos0[m.jnt_qposadr[~free]] != 0)), armature=bool(np.any(m.dof_armature != 0)),
        position=any(t == 'position' for t in m.actuator_tags), velocity_gain=bool(kv), motor=any(t == 'torque' for t in m.actuator_tags),
        ctrlrange=bool(np.any(m.actuator_ctrllimited)), forcerange=bool(np.any(m.actuator_forcelimited)),
        tilted_gravity=bool(m.gravity[0] != 0 or m.gravity[1] != 0),
        chain=chain, rs=32 if rs <= 32 else 64, nq_past_128=m.nq > LANES,
        dofs_in_wave1=nv > 64, bodies_in_wave1=nb > 64,
        wide_level=bool(levels.max() > 6), split_round_across_waves=any(min(r) < 64 <= max(r) for r in rounds),
        jump_rounds=jump_rounds, jump_src_from_lds=jump_rounds > 4,
        body_lane_not_dof_lane=any(m.body_dofadr[i] != i for i in range(1, nb) if m.body_jntadr[i] >= 0 and not free[m.body_jntadr[i]]),
    )
