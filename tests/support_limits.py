"""Limited models, inputs and oracle read-outs that the fp64 joint-limit tests share (test_gpu_f64_limits.py, test_gpu_f64_limit_params.py,
test_f64_limit_recipes.py).  torch and the GPU test modules are imported inside the functions, so importing this module needs no GPU.

Two recipes change the limit parameters of a model made by ``limited``:
  R (``ranges_recipe``): a range and a margin of its own per joint, asymmetric, and every fifth joint so narrow (+-0.01 under a margin of
     0.03) that both of its rows are candidates whenever |q| < 0.02 - and can carry a force together.
  S (``sol_recipe``): solimp by joint index modulo 5 and solref by joint index modulo 3, so that the five impedance branches of
     get_impedance and the three stiffness forms of mj_makeImpedance all occur among the rows of one batch.
``row_branches`` names the branch of every candidate row of a state."""
import numpy as np

from wide_trees import shape_tree
from support_models import tree_inputs
from support_sims import f64 as _f64

MINVAL, MINIMP, MAXIMP = 1e-15, 0.0001, 0.9999      # oracle/fmj_oracle.c
IMPEDANCE_BRANCHES = ('flat', 'linear', 'below_mid', 'above_mid', 'saturated')
STIFFNESS_FORMS = ('time_constant', 'floor_2h', 'direct')

S_SOLIMP = ((0.9, 0.9, 0.001, 0.5, 2),      # dmin == dmax: flat
            (0.5, 0.95, 0.05, 0.5, 1),      # power 1: linear
            (0.5, 0.95, 0.05, 0.3, 3),      # pow on either side of mid = 0.3
            (0.2, 0.99, 0.0, 0.5, 2),       # width 0: flat
            (0.8, 0.95, 0.01, 0.5, 2))      # pow on either side of mid = 0.5
S_SOLREF_DIRECT = (-500.0, -20.0)           # joints 1::3: stiffness and damping given directly
S_SOLREF_SHORT = (0.001, 0.7)               # joints 2::3: a time constant below 2 h = 0.002


def base(name):
    import farms_mujoco_amd.model as mm
    if name.startswith('shape'):
        return shape_tree(int(name[5:]))
    return {'salamander33': lambda: mm.salamander33(limits=True), 'eel48': lambda: mm.eel(n_joints=48),
            'centipede_20_25': lambda: mm.centipede(20, 25)}[name]()


def newton(m):
    from farms_mujoco_amd.model import SOLVERS
    m.solver = SOLVERS['newton']; m.solver_iterations = 100
    return m


def limited(name, lim=0.1, margin_even=0.02, which=slice(None), integrator='euler'):
    """The model with joints ``which`` (of its hinge and slide joints) limited to +-lim, ``margin_even`` on the even joints, set after
    the build as test_fp64_refuses_limits does; the solver fields are the reference's: Newton, 100 iterations."""
    import farms_mujoco_amd.model as mm
    m = base(name)
    assert m.ngeom == 0
    on = np.zeros(m.njnt, bool); on[which] = True
    on &= m.jnt_type != 0
    m.jnt_limited = on.astype(m.jnt_limited.dtype)
    m.jnt_range = np.tile([-lim, lim], (m.njnt, 1)).astype(float)
    margin = np.zeros(m.njnt); margin[::2] = margin_even
    m.jnt_margin = margin
    m.integrator = mm.INTEGRATORS[integrator]
    return newton(m)


def ranges_recipe(m, rng=None):
    """R: range0 = -U(0, 0.2), range1 = +U(0, 0.2), margin = U(0, 0.03) per joint; every fifth joint instead +-0.01 with margin 0.03."""
    rng = np.random.default_rng([77, 1]) if rng is None else rng
    lo, hi, margin = -rng.uniform(0, 0.2, m.njnt), rng.uniform(0, 0.2, m.njnt), rng.uniform(0, 0.03, m.njnt)
    lo[::5], hi[::5], margin[::5] = -0.01, 0.01, 0.03
    m.jnt_range = np.stack([lo, hi], axis=1)
    m.jnt_margin = margin
    return m


def sol_recipe(m, rng=None):
    """S: solimp of joint j is S_SOLIMP[j % 5]; joints 1::3 take S_SOLREF_DIRECT, joints 2::3 S_SOLREF_SHORT, the rest keep (0.02, 1).
    Ranges and margins stay those of ``limited``.  (Nothing is drawn: ``rng`` is there for the signature the recipes share.)"""
    assert np.all(np.asarray(m.jnt_solref) == np.array([0.02, 1.0])) and 2*m.timestep > S_SOLREF_SHORT[0]
    m.jnt_solimp = np.array([S_SOLIMP[j % 5] for j in range(m.njnt)], float)
    sr = np.tile([0.02, 1.0], (m.njnt, 1))
    sr[1::3] = S_SOLREF_DIRECT; sr[2::3] = S_SOLREF_SHORT
    m.jnt_solref = sr
    return m


RECIPES = {'R': ranges_recipe, 'S': sol_recipe}


def recipe_model(name, recipe, integrator='euler'):
    """``limited(name)`` with recipe 'R', 'S' or 'RS' (R's ranges and margins with S's solref and solimp) applied."""
    m = limited(name, integrator=integrator)
    for r in recipe:
        RECIPES[r](m)
    return m


def undamped(name, integrator='euler'):
    """``limited(name)`` with nothing that damps a dof: dof_damping zero and, because implicitfast counts an actuator's velocity bias
    as damping (shape_tree's actuators have one), that bias zero as well."""
    m = limited(name, integrator=integrator)
    m.dof_damping = np.zeros_like(m.dof_damping)
    bias = np.array(m.actuator_bias, float).reshape(m.nu, 3)
    bias[:, 2] = 0.0
    m.actuator_bias = bias.reshape(np.shape(m.actuator_bias))
    return m


def margin_edge(n=4):
    """eel(48), every joint limited to +-0.5 under a margin of 0.25, at rest.  Every joint of env 0 sits at -0.25 and of env 2 at +0.25,
    where dist == margin exactly and no row is a candidate (dist < margin is strict); envs 1 and 3 are one fp32 step further out
    (nextafter32), where every joint has one.  Returns the model, qpos, qvel."""
    assert n == 4
    m = limited('eel48', lim=0.5, margin_even=0.25)
    m.jnt_margin = np.full(m.njnt, 0.25)
    f = np.float32
    at = [f(-0.25), np.nextafter(f(-0.25), f(-1)), f(0.25), np.nextafter(f(0.25), f(1))]
    qpos = np.tile(m.qpos0, (n, 1))
    for e in range(n):
        qpos[e, scalar_q(m)] = float(at[e])
    return m, qpos, np.zeros((n, m.nv))


def row_branches(m, qpos):
    """The candidate limit rows of one env's ``qpos``, in the oracle's order: a list of (joint, side, impedance branch, stiffness form)
    with the names of IMPEDANCE_BRANCHES and STIFFNESS_FORMS.  Reads the model and qpos only; the rules are those of make_constraints
    (dist < margin), get_impedance (which expression gives the impedance) and mj_makeImpedance (what solref means)."""
    rows = []
    for j in range(m.njnt):
        if not m.jnt_limited[j] or m.jnt_type[j] == 0:
            continue
        value, margin = float(qpos[m.jnt_qposadr[j]]), float(m.jnt_margin[j])
        dmin, dmax, width, mid, power = (float(x) for x in m.jnt_solimp[j])
        dmin, dmax, mid = (min(max(x, MINIMP), MAXIMP) for x in (dmin, dmax, mid))
        width, power = max(0.0, width), max(1.0, power)
        sr0 = float(m.jnt_solref[j][0])
        form = 'direct' if sr0 <= 0 else ('floor_2h' if sr0 < 2*m.timestep else 'time_constant')
        for side in (-1, 1):
            dist = side*(float(m.jnt_range[j][(side + 1)//2]) - value)
            if not dist < margin:
                continue
            if dmin == dmax or width <= MINVAL:
                imp = 'flat'
            else:
                x = abs((dist - margin)/width)
                imp = ('saturated' if x >= 1 else 'zero' if x <= 0 else 'linear' if power == 1 else 'below_mid' if x <= mid else 'above_mid')
            rows.append((j, side, imp, form))
    return rows


def scalar_q(m):
    return m.jnt_qposadr[m.jnt_type != 0]


def engaged_inputs(m, n, seed):
    """tree_inputs with the joint positions uniform in +-0.15, qvel normal x 0.5 and ctrl uniform in +-0.3."""
    qpos, qvel, ctrl, xf, qs = tree_inputs(m, n, seed)
    rng = np.random.default_rng([4242, seed])
    qpos[:, scalar_q(m)] = rng.uniform(-0.15, 0.15, (n, len(scalar_q(m))))
    qvel = rng.normal(size=(n, m.nv))*0.5
    ctrl = rng.uniform(-0.3, 0.3, (n, max(m.nu, 1)))[:, :m.nu]
    return qpos, qvel, ctrl, xf, qs


def as_fp32_inputs(m, qpos, qvel, ctrl=None, xf=None, qs=None):
    """The inputs as a context holds them (rounded to fp32), in fp64, with the keys ``phys`` returns: what the oracle is given."""
    r = lambda a: np.asarray(a, np.float64).astype(np.float32).astype(np.float64)
    n = len(qpos)
    return dict(qpos=r(qpos), qvel=r(qvel), ctrl=(r(ctrl) if ctrl is not None else np.zeros((n, m.nu))) if m.nu else None,
                xfrc_applied=r(xf) if xf is not None else np.zeros((n, m.nbody, 6)),
                qpos_spring=r(qs) if qs is not None else r(np.tile(m.qpos_spring, (n, 1))))


N = 4
# the seed of engaged_inputs per model: the first of 100, 101, ... (0, 1, ... for the larger models) at which the oracle finds, in every
# env, at least 5 rows with a force and a candidate row without one (the tests assert both before they look at the device)
ENGAGED_SEEDS = {'salamander33': 104, 'eel48': 100, 'centipede_20_25': 2, 'shape1': 3, 'shape4': 4, 'shape6': 5, 'shape10': 6}
RECIPE_MODELS = ('eel48', 'centipede_20_25', 'shape1', 'shape6')
# the seed of engaged_inputs per model and recipe: the first of 100, 101, ... at which assert_recipe_engaged holds in every env
RECIPE_SEEDS = {('eel48', 'R'): 100, ('eel48', 'S'): 100, ('centipede_20_25', 'R'): 100, ('centipede_20_25', 'S'): 100,
                ('shape1', 'R'): 100, ('shape1', 'S'): 100, ('shape6', 'R'): 100, ('shape6', 'S'): 100}
UNDAMPED_SEEDS = {'eel48': 100, 'shape6': 5}      # those of test_gpu_f64_limits.py: at least 5 rows with a force in every env


def recipe_inputs(name, recipe, integrator='euler'):
    """The model under the recipe and its N engaged input states, as fp32 numbers in fp64."""
    m = recipe_model(name, recipe, integrator)
    return m, as_fp32_inputs(m, *engaged_inputs(m, N, RECIPE_SEEDS[name, recipe]))


def undamped_inputs(name, integrator='euler'):
    m = undamped(name, integrator)
    return m, as_fp32_inputs(m, *engaged_inputs(m, N, UNDAMPED_SEEDS[name]))


def phys(m, n, qpos, qvel, ctrl=None, xf=None, qs=None, precision='fp64', limits=True):
    import support_f64_step as S
    import torch
    from farms_mujoco_amd.physics import BatchedPhysics
    if precision == 'fp32':
        return S._phys(m, n, qpos, qvel, ctrl, xf, qs, precision)
    phys = BatchedPhysics(m, n, precision='fp64', fp64_limits=limits)
    assert phys.precision == 'fp64' and phys.kernel_info()['threads_per_env'] == 128
    d = phys.data
    f32 = lambda a: torch.as_tensor(np.asarray(a), dtype=torch.float32)
    d.qpos[:] = f32(qpos); d.qvel[:] = f32(qvel)
    if xf is not None:
        d.xfrc_applied[:] = f32(xf)
    if qs is not None:
        d.qpos_spring[:] = f32(qs)
    if ctrl is not None and m.nu:
        d.ctrl[:] = f32(ctrl)
    return phys, dict(qpos=_f64(d.qpos), qvel=_f64(d.qvel), ctrl=_f64(d.ctrl) if m.nu else None, xfrc_applied=_f64(d.xfrc_applied),
                      qpos_spring=_f64(d.qpos_spring))


def step_tf(oracle, m, ins):
    return oracle.step_tf(m, ins['qpos'], ins['qvel'], ctrl=ins['ctrl'], qpos_spring=ins['qpos_spring'], xfrc_applied=ins['xfrc_applied'], want_AR=False)


def rows_engaged(oracle, m, ins):
    """Per env, from oracle.step_tf: the rows with a positive force and the candidate rows with none."""
    o = step_tf(oracle, m, ins)
    pos = np.array([(o['efc'][e, :o['nefc'][e], 0] > 0).sum() for e in range(len(o['nefc']))])
    return pos, o['nefc'] - pos


def joints_with_two_rows(o):
    """Per env of a step_tf result: the joints with both rows candidate, and those with a force on both."""
    both, both_forced = [], []
    for e in range(len(o['nefc'])):
        rows = o['efc'][e, :o['nefc'][e]]
        ids = rows[:, 5].astype(int)
        two = [j for j in np.unique(ids) if (ids == j).sum() == 2]
        both.append(two)
        both_forced.append([j for j in two if np.all(rows[ids == j, 0] > 0)])
    return both, both_forced


TWO_FORCED_ROWS = ('shape1', 'shape6')      # models on which recipe R puts a force on both rows of some joint (not the eel, not the centipede)


def assert_recipe_engaged(name, recipe, m, ins, o):
    """The floors on what a recipe exercises, from the oracle's step ``o`` = step_tf(oracle, m, ins) - asserted before a test looks at
    the device.  R: a joint with both rows candidate and five rows with a force in every env, and on TWO_FORCED_ROWS a joint with a
    force on both rows somewhere in the batch.  S: five rows with a force in every env, and every impedance branch and stiffness form
    among the batch's candidate rows.  Both: at most 10 Newton iterations, no warning."""
    n = len(o['nefc'])
    forced = np.array([(o['efc'][e, :o['nefc'][e], 0] > 0).sum() for e in range(n)])
    both, both_forced = joints_with_two_rows(o)
    rows = [row_branches(m, ins['qpos'][e]) for e in range(n)]
    assert [len(r) for r in rows] == list(o['nefc']), (name, recipe, [len(r) for r in rows], o['nefc'])      # row_branches selects the oracle's rows
    for e in range(n):
        assert [r[0] for r in rows[e]] == list(o['efc'][e, :o['nefc'][e], 5].astype(int)), (name, recipe, e)
    imps, forms = {r[2] for rr in rows for r in rr}, {r[3] for rr in rows for r in rr}
    print(name, recipe, 'rows with a force per env', forced, 'candidate rows', o['nefc'], 'joints with two rows', [len(b) for b in both],
          'with a force on both', [len(b) for b in both_forced], 'iterations', o['iterations'], sorted(imps), sorted(forms))
    assert not o['status'].any() and o['iterations'].max() <= 10, (name, recipe, o['status'], o['iterations'])
    assert forced.min() >= 5, (name, recipe, forced)
    if 'R' in recipe:
        assert min(len(b) for b in both) >= 1, (name, recipe, both)
        if name in TWO_FORCED_ROWS:
            assert sum(len(b) for b in both_forced) >= 1, (name, recipe, both_forced)
    if 'S' in recipe:
        assert imps >= set(IMPEDANCE_BRANCHES) and forms == set(STIFFNESS_FORMS), (name, recipe, imps, forms)
    return forced


def excess(oracle, m, phys, ins, forward):
    import support_f64_step as S
    import torch
    q0, v0 = phys.data.qpos.clone(), phys.data.qvel.clone()
    if forward:
        phys.forward()
    else:
        phys.step(1)
    torch.cuda.synchronize()
    assert int(phys.data.status.abs().sum()) == 0
    ref = oracle.step(m, ins['qpos'], ins['qvel'], ctrl=ins['ctrl'], qpos_spring=ins['qpos_spring'], xfrc_applied=ins['xfrc_applied'])
    if forward:
        assert torch.equal(phys.data.qpos, q0) and torch.equal(phys.data.qvel, v0)
        ref = dict(ref, qpos=ins['qpos'], qvel=ins['qvel'])
    groups = S._field_groups(m)
    return {k: S.ulp_excess(getattr(phys.data, k).cpu().numpy(), ref[k], groups[k]) for k in ('qpos', 'qvel', 'qacc', 'sensordata')}, ref


def tape(m, n, T, f, amplitude=0.3):
    """ctrl[t, env, a] = amplitude sin(2 pi f t + 0.7 env - 2 pi a / nu), rounded to fp32 as the device holds it."""
    t = np.arange(T)[:, None, None]*m.timestep
    tape = amplitude*np.sin(2*np.pi*f*t + 0.7*np.arange(n)[None, :, None] - 2*np.pi*np.arange(m.nu)[None, None, :]/m.nu)
    return tape.astype(np.float32)
