"""Models and inputs that more than one test file (and the scripts) use: numpy and farms_mujoco_amd.model only, so importing this
touches neither torch nor the GPU.  What a function builds is pinned by the tests that use it; change nothing here that a test feeds
the kernels or the oracle."""
import numpy as np

FMJ_WARN_BADQPOS = 1          # include/fmj.h
FMJ_WARN_CONTACTFULL = 8      # (FMJ_WARN_BADQACC is 4: a frozen env must fail the tests that mask this bit)


def walker(spawn_z=0.045, solver=None, cone='pyramidal', impratio=1.0, noslip=None, **kw):
    """The walking salamander: contacts, joint limits, feet just above the plane.  With ``solver`` the solver, cone and impratio are set
    (100 iterations for anything but PGS); with ``noslip`` the noslip post-pass."""
    from farms_mujoco_amd.model import salamander33, SOLVERS, CONES
    m = salamander33(contacts=True, limits=True, spawn_z=spawn_z, **kw)
    if solver is not None:
        m.solver = SOLVERS[solver]; m.cone = CONES[cone]; m.impratio = impratio
        if solver != 'pgs':
            m.solver_iterations = 100
    if noslip is not None:
        m.noslip_iterations = noslip; m.noslip_tolerance = 1e-10
    return m


def trot_tape(m, n, T, seed=0):
    """Trot-like position control: axial wave + diagonal limb pairs swinging in antiphase."""
    rng = np.random.default_rng(seed)
    psi = rng.uniform(0, 2*np.pi, n)
    t = np.arange(T)[:, None, None]*m.timestep
    tape = np.zeros((T, n, m.nu))
    for a in range(m.nu):
        if m.actuator_tags[a] != 'position':
            continue
        name = m.joint_names[m.actuator_jntid[a]]
        if name.startswith('joint_body_'):
            k = int(name.split('_')[-1])
            tape[:, :, a] = 0.2*np.sin(2*np.pi*1.0*t[:, :, 0] - 2*np.pi*k/11 + psi[None, :])
        elif name.endswith('_1'):      # shoulder pitch
            ph = 0.0 if ('front_L' in name or 'hind_R' in name) else np.pi
            tape[:, :, a] = 0.3*np.sin(2*np.pi*1.0*t[:, :, 0] + ph + psi[None, :])
    return tape


def box_walker():
    """A free box trunk with two hinged box limbs above a plane: plane-box contacts (up to 4 corners per geom)."""
    from farms_mujoco_amd.model import ModelBuilder, GEOM_BOX, GEOM_PLANE
    b = ModelBuilder('boxbot', timestep=1e-3)
    b.options['max_contacts'] = 16
    b.add_body('trunk', pos=(0, 0, 0.06), mass=0.5, inertia=(2e-4, 6e-4, 7e-4), joint='free')
    b.add_geom('trunk', GEOM_BOX, (0.06, 0.03, 0.015), friction=(0.8, 0, 0))
    for side, y in (('L', 0.04), ('R', -0.04)):
        b.add_body(f'limb_{side}', parent='trunk', pos=(0.03, y, 0.0), mass=0.05, inertia=(2e-6, 8e-6, 8e-6),
                   joint='hinge', axis=(0, 1, 0), damping=1e-3, limited=True, range=(-0.6, 0.6))
        b.add_geom(f'limb_{side}', GEOM_BOX, (0.03, 0.008, 0.008), pos=(0.03, 0, -0.02), quat=(0.9659258, 0, 0.258819, 0),
                   friction=(1.0, 0, 0))
        b.add_position_actuator(f'joint_limb_{side}', kp=0.05)
    b.add_geom('world', GEOM_PLANE, (0, 0, 0), friction=(0, 0, 0))
    return b.compile()


def _terrain(seed=0, nr=17, nc=33, rx=0.8, ry=0.4, zt=0.03):
    """Smooth random bumps, a few centimetres high, sampled on a grid."""
    rng = np.random.default_rng(seed)
    xs = np.linspace(-rx, rx, nc); ys = np.linspace(-ry, ry, nr)
    z = np.zeros((nr, nc))
    for _ in range(6):
        kx, ky, ph = rng.uniform(3, 9), rng.uniform(3, 9), rng.uniform(0, 6.28)
        z += rng.uniform(0.2, 1.0)*np.sin(kx*xs[None, :] + ph)*np.cos(ky*ys[:, None] - ph)
    return z/np.abs(z).max(), (rx, ry, zt, 0.1)


def hfield_walker(spawn_z=0.075):
    """salamander33 with its capsules / foot spheres over a heightfield instead of the plane."""
    from farms_mujoco_amd.model import salamander33
    import farms_mujoco_amd.model as mm
    b_ref = salamander33(contacts=True, limits=True, spawn_z=spawn_z)
    # rebuild through the builder API: same animat, heightfield arena
    b = mm.ModelBuilder('salamander33_hf', timestep=1e-3)
    m = b_ref
    for i in range(1, m.nbody):
        j = int(m.body_jntadr[i])
        kw = dict(pos=m.body_pos[i], quat=m.body_quat[i], mass=m.body_mass[i], ipos=m.body_ipos[i], inertia=m.body_inertia[i], iquat=m.body_iquat[i])
        if j < 0:
            b.add_body(m.body_names[i], m.body_names[m.body_parentid[i]], **kw)
        elif m.jnt_type[j] == 0:
            b.add_body(m.body_names[i], 'world', joint='free', **kw)
        else:
            b.add_body(m.body_names[i], m.body_names[m.body_parentid[i]], joint='hinge', jname=m.joint_names[j], axis=m.jnt_axis[j],
                       damping=m.dof_damping[m.jnt_dofadr[j]], limited=bool(m.jnt_limited[j]), range=m.jnt_range[j], **kw)
    for g in range(m.ngeom):
        if m.geom_type[g] != 0:
            b.add_geom(m.body_names[m.geom_bodyid[g]], int(m.geom_type[g]), m.geom_size[g], pos=m.geom_pos[g], quat=m.geom_quat[g],
                       friction=m.geom_friction[g])
    data, size = _terrain()
    b.add_hfield(data, size, pos=(0.4, 0.0, 0.0))
    b.options['max_contacts'] = 32
    for a in range(m.nu):
        if m.actuator_tags[a] == 'position':
            b.add_position_actuator(m.joint_names[m.actuator_jntid[a]], kp=m.actuator_gain[a])
    return b.compile()


def salamander_self_collisions(spawn_z=0.045):
    """The walking salamander with explicit pairs between neighbouring limbs and between head and tail, over the plane."""
    import farms_mujoco_amd.model as mm
    ref = mm.salamander33(contacts=True, limits=True, spawn_z=spawn_z)
    b = mm.ModelBuilder('salamander33_sc', timestep=1e-3)
    m = ref
    for i in range(1, m.nbody):
        j = int(m.body_jntadr[i])
        kw = dict(pos=m.body_pos[i], quat=m.body_quat[i], mass=m.body_mass[i], ipos=m.body_ipos[i], inertia=m.body_inertia[i], iquat=m.body_iquat[i])
        if m.jnt_type[j] == 0:
            b.add_body(m.body_names[i], 'world', joint='free', **kw)
        else:
            b.add_body(m.body_names[i], m.body_names[m.body_parentid[i]], joint='hinge', jname=m.joint_names[j], axis=m.jnt_axis[j],
                       damping=m.dof_damping[m.jnt_dofadr[j]], limited=bool(m.jnt_limited[j]), range=m.jnt_range[j], **kw)
    for g in range(m.ngeom):
        b.add_geom(m.body_names[m.geom_bodyid[g]], int(m.geom_type[g]), m.geom_size[g], pos=m.geom_pos[g], quat=m.geom_quat[g],
                   friction=m.geom_friction[g])
    for a in range(m.nu):
        if m.actuator_tags[a] == 'position':
            b.add_position_actuator(m.joint_names[m.actuator_jntid[a]], kp=m.actuator_gain[a])
    b.options['max_contacts'] = 32
    for pair in (('leg_front_L_3', 'leg_front_R_3'), ('leg_hind_L_3', 'leg_hind_R_3'), ('body_0', 'body_11'), ('body_2', 'body_10'),
                 ('leg_front_L_3', 'body_2'), ('leg_hind_R_3', 'body_6'), ('leg_front_R_3', 'body_1'), ('leg_hind_L_3', 'leg_front_L_3')):
        b.add_contact_pair(*pair)
    return b.compile()


def mesh_walker(seed=5):
    """A free trunk with a convex-mesh hull (random points on an ellipsoid) and two hinged limbs ending in small convex
    meshes, above a plane: every ground contact comes from a mesh vertex."""
    from farms_mujoco_amd.model import ModelBuilder, GEOM_PLANE
    rng = np.random.default_rng(seed)

    def cloud(n, a, b, c):
        v = rng.normal(size=(n, 3)); v /= np.linalg.norm(v, axis=1, keepdims=True)
        return v*np.array([a, b, c])
    b = ModelBuilder('meshbot', timestep=1e-3)
    b.options['max_contacts'] = 16
    b.add_body('trunk', pos=(0, 0, 0.06), mass=0.5, inertia=(2e-4, 6e-4, 7e-4), joint='free')
    b.add_mesh_geom('trunk', cloud(60, 0.06, 0.03, 0.015), friction=(0.8, 0, 0))
    for side, y in (('L', 0.04), ('R', -0.04)):
        b.add_body(f'limb_{side}', parent='trunk', pos=(0.03, y, 0.0), mass=0.05, inertia=(2e-6, 8e-6, 8e-6),
                   joint='hinge', axis=(0, 1, 0), damping=1e-3, limited=True, range=(-0.6, 0.6))
        b.add_mesh_geom(f'limb_{side}', cloud(24, 0.03, 0.008, 0.008), pos=(0.03, 0, -0.02), quat=(0.9659258, 0, 0.258819, 0),
                        friction=(1.0, 0, 0))
        b.add_position_actuator(f'joint_limb_{side}', kp=0.05)
    b.add_geom('world', GEOM_PLANE, (0, 0, 0), friction=(0, 0, 0))
    return b.compile()


def random_tree(seed, contacts=False, meshes=False):
    from farms_mujoco_amd.model import ModelBuilder, euler2quat, GEOM_SPHERE, GEOM_CAPSULE, GEOM_CYLINDER, GEOM_BOX, GEOM_PLANE
    rng = np.random.default_rng(seed)
    nb = int(rng.integers(3, 22))
    free = bool(rng.integers(0, 2))
    b = ModelBuilder(f'tree{seed}', timestep=1e-3, gravity=(0, 0, -9.81) if rng.integers(0, 2) else (0.5, -0.3, -9.0))
    names = []

    def inertia():
        A = rng.normal(size=(3, 3)); S = A @ A.T*1e-4 + np.eye(3)*2e-4
        return (S[0, 0], S[1, 1], S[2, 2], S[0, 1], S[0, 2], S[1, 2])
    for i in range(nb):
        name = f'b{i}'
        mass = float(rng.uniform(0.05, 0.5))
        kw = dict(mass=mass, ipos=rng.normal(size=3)*0.03, fullinertia=inertia())
        if i == 0:
            if free:
                b.add_body(name, 'world', pos=rng.normal(size=3)*0.2, quat=euler2quat(rng.normal(size=3)), joint='free', **kw)
            else:
                jt = ['hinge', 'slide', None][int(rng.integers(0, 3))]
                jkw = dict(joint=jt, axis=rng.normal(size=3), jpos=rng.normal(size=3)*0.02, damping=0.01) if jt else {}
                b.add_body(name, 'world', pos=rng.normal(size=3)*0.2, quat=euler2quat(rng.normal(size=3)), **jkw, **kw)
        else:
            parent = names[int(rng.integers(max(0, i - 4), i))]
            u = rng.random()
            jt = 'hinge' if u < 0.7 else 'slide' if u < 0.85 else None
            jkw = {}
            if jt:
                jkw = dict(joint=jt, axis=rng.normal(size=3), jpos=rng.normal(size=3)*0.03 if rng.random() < 0.5 else (0, 0, 0),
                           damping=float(rng.choice([0.0, 2e-3, 1e-2])), stiffness=float(rng.choice([0.0, 0.0, 0.05])),
                           armature=float(rng.choice([0.0, 1e-4])), qpos0=float(rng.choice([0.0, 0.2])))
                if contacts and jt == 'hinge' and rng.random() < 0.5:
                    jkw.update(limited=True, range=(-0.3, 0.25))
            b.add_body(name, parent, pos=rng.normal(size=3)*0.08, quat=euler2quat(rng.normal(size=3)*0.5), **jkw, **kw)
        names.append(name)
        if contacts and rng.random() < 0.7:
            kind = int(rng.integers(0, 5 if meshes else 4))
            gk = dict(pos=rng.normal(size=3)*0.02, quat=euler2quat(rng.normal(size=3)), friction=(float(rng.uniform(0.3, 1.0)), 0, 0))
            if kind == 0:
                b.add_geom(name, GEOM_SPHERE, (float(rng.uniform(0.02, 0.05)),), **gk)
            elif kind == 1:
                b.add_geom(name, GEOM_CAPSULE, (float(rng.uniform(0.015, 0.03)), float(rng.uniform(0.02, 0.06))), **gk)
            elif kind == 2:
                b.add_geom(name, GEOM_BOX, tuple(rng.uniform(0.015, 0.05, 3)), **gk)
            elif kind == 3:
                b.add_geom(name, GEOM_CYLINDER, (float(rng.uniform(0.02, 0.05)), float(rng.uniform(0.01, 0.05))), **gk)
            else:                       # convex mesh: a random point cloud (its hull), off-centre in the geom frame
                cloud = rng.normal(size=(int(rng.integers(5, 40)), 3))*rng.uniform(0.01, 0.04, 3) + rng.normal(size=3)*0.01
                b.add_mesh_geom(name, cloud, **gk)
    if contacts:
        b.add_geom('world', GEOM_PLANE, (0, 0, 0), pos=(0, 0, -0.05), friction=(0.2, 0, 0))
        b.options['max_contacts'] = 32
    joints = [bd.joint['name'] for bd in b.bodies[1:] if bd.joint and bd.joint['type'] != 0]
    for jn in joints:
        r = rng.random()
        if r < 0.5:
            b.add_joint_actuators(jn, kp=float(rng.uniform(0.1, 0.5)), kv=float(rng.uniform(0, 0.01)),
                                  forcerange=(-0.2, 0.3) if rng.random() < 0.5 else None)
        elif r < 0.75:
            b.add_position_actuator(jn, kp=0.3)
    if not joints and not free:
        return None
    return b.compile()


def scissors(theta=0.35, r=0.03, L=0.2, friction=0.0, capsule=False):
    """A fixed post with two equal arms hinged about z at the origin, tip spheres (or capsules along the arms) in an
    explicit contact pair: the arms close like scissors."""
    from farms_mujoco_amd.model import ModelBuilder, GEOM_SPHERE, GEOM_CAPSULE, axisangle2quat
    b = ModelBuilder('scissors', timestep=1e-3, gravity=(0, 0, 0))
    b.add_body('post', 'world', pos=(0, 0, 0.5), mass=1.0, inertia=(1e-3, 1e-3, 1e-3))
    for name, sgn in (('arm_a', +1), ('arm_b', -1)):
        b.add_body(name, 'post', mass=0.2, ipos=(L/2, 0, 0), inertia=(1e-5, 7e-4, 7e-4), joint='hinge', axis=(0, 0, 1), damping=1e-3,
                   qpos0=0.0)
        if capsule:                    # the outer half of the arm: the two capsules only meet when the arms close
            b.add_geom(name, GEOM_CAPSULE, (r, L/4), pos=(0.75*L, 0, 0), quat=axisangle2quat([0, 1, 0], np.pi/2))
        else:
            b.add_geom(name, GEOM_SPHERE, (r,), pos=(L, 0, 0))
    b.add_contact_pair('arm_a', 'arm_b', friction=friction)
    b.options['max_contacts'] = 4
    m = b.compile()
    return m, np.array([theta, -theta])


def stack(lower, upper, z, tilt=0.0, max_contacts=8, gravity=(0, 0, 0), **pair_kw):
    """A welded base carrying geom `lower`, and a body on a vertical slide joint carrying geom `upper`, in an explicit pair.
    lower / upper = (type, size[, vertices]); the slider's qpos is its height z."""
    from farms_mujoco_amd.model import ModelBuilder, GEOM_MESH, axisangle2quat
    b = ModelBuilder('stack', timestep=1e-3, gravity=gravity)
    b.add_body('base', 'world', pos=(0, 0, 0), mass=1.0, inertia=(1e-3, 1e-3, 1e-3))
    b.add_body('top', 'base', mass=0.5, inertia=(1e-3, 1e-3, 1e-3), joint='slide', axis=(0, 0, 1), damping=0.0, qpos0=0.0)
    for body, (gt, size, *rest) in (('base', lower), ('top', upper)):
        quat = axisangle2quat([1, 0, 0], tilt) if body == 'top' else (1, 0, 0, 0)
        if gt == GEOM_MESH:
            b.add_mesh_geom(body, rest[0], quat=quat)
        else:
            b.add_geom(body, gt, size, quat=quat)
    b.add_contact_pair('base', 'top', **pair_kw)
    b.options['max_contacts'] = max_contacts
    m = b.compile()
    return m, np.array([z])


def rand_state(m, n, seed, qscale=0.3, vscale=0.5):
    """Random but physically sane state: arbitrary root pose, hinge angles +-qscale, ctrl near the pose
    on the position actuators only (velocity / motor actuators idle, as in every BASELINE config)."""
    rng = np.random.default_rng(seed)
    qpos = np.tile(m.qpos0, (n, 1))
    qpos[:, 7:] += rng.uniform(-qscale, qscale, (n, m.nq - 7))
    q = rng.normal(size=(n, 4)); qpos[:, 3:7] = q/np.linalg.norm(q, axis=1, keepdims=True)
    qpos[:, :3] += rng.uniform(-0.2, 0.2, (n, 3))
    qvel = rng.normal(size=(n, m.nv))*vscale
    ctrl = np.zeros((n, m.nu))
    for a in range(m.nu):
        if m.actuator_tags[a] == 'position':
            ctrl[:, a] = qpos[:, m.jnt_qposadr[m.actuator_jntid[a]]] + rng.uniform(-0.05, 0.05, n)
    return qpos, qvel, ctrl


def finned_eel(n_joints=40):
    """An eel whose links 1..n carry a welded fin body (no joint): nbody past 64 with every dof inside one wave."""
    import farms_mujoco_amd.model as mm
    b = mm.ModelBuilder('finned_eel', timestep=1e-3)
    L, n = 0.05, n_joints + 1
    radii = np.linspace(0.015, 0.005, n)
    for i in range(n):
        r = radii[i]
        mass = 1000.0*(np.pi*r*r*L + 4.0/3.0*np.pi*r**3)
        kw = dict(pos=(0, 0, -0.1) if i == 0 else (L, 0, 0), mass=mass, ipos=(L/2, 0, 0), inertia=mm._capsule_inertia(mass, r, L))
        if i == 0:
            b.add_body('body_0', 'world', joint='free', **kw)
        else:
            b.add_body(f'body_{i}', f'body_{i-1}', joint='hinge', jname=f'joint_body_{i}', axis=(0, 0, 1), damping=5e-4, **kw)
            fm = 0.2*mass
            b.add_body(f'fin_{i}', f'body_{i}', pos=(L/2, 0, r), mass=fm, ipos=(0, 0, 0.005),
                       inertia=(fm*2e-5, fm*3e-5, fm*1e-5))
    for i in range(1, n):
        b.add_position_actuator(f'joint_body_{i}', kp=0.5)
    return b.compile()


def tree_inputs(m, n, seed):
    """Random state per env: qpos around qpos0 (normalised free quaternions), qvel, ctrl, qpos_spring and external forces on every body
    (those of index >= 64 included)."""
    rng = np.random.default_rng(3000 + seed)
    qpos = np.tile(m.qpos0, (n, 1)) + rng.uniform(-0.4, 0.4, (n, m.nq))
    for j in range(m.njnt):
        if m.jnt_type[j] == 0:
            a = m.jnt_qposadr[j]; q = rng.normal(size=(n, 4)); qpos[:, a+3:a+7] = q/np.linalg.norm(q, axis=1, keepdims=True)
    qvel = rng.normal(size=(n, m.nv))*0.5
    ctrl = rng.uniform(-0.6, 0.6, (n, m.nu))
    xf = rng.normal(size=(n, m.nbody, 6))*0.05; xf[:, 0] = 0
    qs = np.tile(m.qpos_spring, (n, 1)) + rng.uniform(-0.1, 0.1, (n, m.nq))
    return qpos, qvel, ctrl, xf, qs


SDF = """<?xml version="1.0"?>
<sdf version="1.6">
  <model name="swimmer">
    <pose>0 0 0 0 0 0</pose>
    <link name="head">
      <pose>0 0 0 0 0 0</pose>
      <inertial><pose>0.05 0 0 0 0 0</pose><mass>0.10</mass>
        <inertia><ixx>2e-5</ixx><ixy>0</ixy><ixz>0</ixz><iyy>9e-5</iyy><iyz>0</iyz><izz>9e-5</izz></inertia></inertial>
      <collision name="head_col"><pose>0.05 0 0 0 1.5707963267948966 0</pose>
        <geometry><capsule><radius>0.02</radius><length>0.1</length></capsule></geometry></collision>
    </link>
    <link name="trunk">
      <pose>0.1 0 0 0 0 0.3</pose>
      <inertial><pose>0.05 0 0 0 0 0.2</pose><mass>0.08</mass>
        <inertia><ixx>1.5e-5</ixx><ixy>1e-6</ixy><ixz>0</ixz><iyy>7e-5</iyy><iyz>0</iyz><izz>7e-5</izz></inertia></inertial>
      <collision name="trunk_col"><pose>0.05 0 0 0 0 0</pose><geometry><sphere><radius>0.02</radius></sphere></geometry></collision>
    </link>
    <link name="tail">
      <pose>0.19553365 0.02955202 0 0 0 0.3</pose>
      <inertial><pose>0.04 0 0 0 0 0</pose><mass>0.04</mass>
        <inertia><ixx>5e-6</ixx><ixy>0</ixy><ixz>0</ixz><iyy>2e-5</iyy><iyz>0</iyz><izz>2e-5</izz></inertia></inertial>
    </link>
    <link name="fin">
      <pose>0.15 0.03 0 0 0 1.0</pose>
      <inertial><pose>0.01 0 0 0 0 0</pose><mass>0.005</mass>
        <inertia><ixx>1e-6</ixx><ixy>0</ixy><ixz>0</ixz><iyy>1e-6</iyy><iyz>0</iyz><izz>1e-6</izz></inertia></inertial>
    </link>
    <joint name="j_trunk" type="revolute"><parent>head</parent><child>trunk</child><pose>0 0 0 0 0 0</pose>
      <axis><xyz>0 0 1</xyz><limit><lower>-1.0</lower><upper>1.0</upper></limit></axis></joint>
    <joint name="j_tail" type="revolute"><parent>trunk</parent><child>tail</child><pose>0 0 0 0 0 0</pose>
      <axis><xyz>0 0 1</xyz></axis></joint>
    <joint name="j_fin" type="continuous"><parent>trunk</parent><child>fin</child><pose>0.002 0 0 0 0 0</pose>
      <axis><xyz>0 1 0</xyz></axis></joint>
  </model>
</sdf>
"""


def sdf_options(sdf_path):
    """AnimatOptions for the swimmer of ``SDF`` written to ``sdf_path``."""
    from farms_mujoco_amd.options import AnimatOptions
    links = [AnimatOptions.link(n, swimming=True, drag_coefficients=[[-0.01, -0.5, -0.5], [-1e-6, -1e-5, -1e-5]])
             for n in ('head', 'trunk', 'tail', 'fin')]
    joints = [AnimatOptions.joint('j_trunk', initial=(0.1, 0.0), damping=1e-3, stiffness=0.02),
              AnimatOptions.joint('j_tail', initial=(-0.2, 0.5), damping=2e-3), AnimatOptions.joint('j_fin', damping=1e-4)]
    motors = [AnimatOptions.motor('j_trunk', gains=(0.5, 0.01)), AnimatOptions.motor('j_tail', gains=(0.4, 0.0), limits_torque=[-0.3, 0.3]),
              AnimatOptions.motor('j_fin', gains=(0.05, 0.0))]
    return AnimatOptions(name='swimmer', links=links, joints=joints, motors=motors, sdf=sdf_path,
                         spawn_pose=(0.1, -0.2, -0.05, 0.0, 0.0, 0.4), spawn_velocity=(0.1, 0, 0, 0, 0, 0.2))
