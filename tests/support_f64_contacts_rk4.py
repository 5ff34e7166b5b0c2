"""Models, inputs and oracle-side conditions that the tests of RK4 on the fp64 contact solve share (test_f64_contacts_rk4_recipes.py,
test_f64_contacts_rk4_interface.py, test_gpu_f64_contacts_rk4.py): FMJ_CREATE_F64_CONTACTS | FMJ_CREATE_F64_CONTACTS_RK4,
fmj_step_f64_terrain_rk4_kernel / fmj_step_f64_elliptic_rk4_kernel of csrc/fmj_f64_step.inc.  The models and inputs are those of
support_f64_contacts.py (flat ground), support_f64_terrain.py (heightfield, cylinders) and support_f64_elliptic.py (the elliptic cone)
with ``integrator = RK4``; the seeds are this module's own (the contact list that counts is the fourth pass's).  torch and the GPU
modules are imported inside the functions, so importing this module needs no GPU.  Every reference value comes from the oracle, whose
rk4() restates mj_RungeKutta with contacts; ``stages`` rebuilds the four stage states of a step on the host from oracle forward passes."""
import numpy as np

import support_f64_contacts as C
import support_f64_terrain as T
import support_f64_elliptic as E
from support_f64_contacts import N, CONTACTS, LIMITS, RK4
from support_f64_terrain import TERRAIN
from support_f64_elliptic import ELLIPTIC
from support_f64_rk4 import integrate_pos, as_euler

CONTACTS_RK4 = 8192      # FMJ_CREATE_F64_CONTACTS_RK4
# the one-step cases: name -> (the support module that makes the model and its inputs, the model's name there)
CASES = {'salamander33': (C, 'salamander33'), 'boxfoot6': (C, 'boxfoot6'), 'centipede_20_25': (C, 'centipede_20_25'),
         'salamander_hfield_cyl': (T, 'salamander_hfield_cyl'), 'elliptic_salamander33': (E, 'salamander33')}
# the seed of each case's inputs: the first of 100, 101, ... at which `conditions` holds in every env (first_seed finds them;
# test_f64_contacts_rk4_recipes.py asserts the conditions at them)
SEEDS = {'salamander33': 115, 'boxfoot6': 129, 'centipede_20_25': 130, 'salamander_hfield_cyl': 110, 'elliptic_salamander33': 107}
# the centipede's feet pushed 5 mm below the plane, not the Euler recipe's 2 mm: at 2 mm no seed of 100 .. 399 leaves a penetrating
# contact without a force in the fourth pass of every env (at the Euler recipe's seed 100 all 26 / 5 / 9 / 15 contacts carry one)
INPUT_KW = {'centipede_20_25': dict(depth=5e-3)}


def make(case, integrator='rk4'):
    mod, name = CASES[case]
    return mod.make(name, integrator)


def inputs(case, m, n=N, seed=None, **kw):
    mod, name = CASES[case]
    seed = SEEDS[case] if seed is None else seed
    kw = dict(INPUT_KW.get(case, {}), **kw)
    return E.inputs(name, m, n, seed, **kw) if mod is E else mod.inputs(m, n, seed, **kw)


def flags_of(case, m):
    mod, _ = CASES[case]
    return CONTACTS | CONTACTS_RK4 | (TERRAIN if mod is T else 0) | (ELLIPTIC if mod is E else 0) | (LIMITS if np.any(m.jnt_limited) else 0)


def phys(case, m, n, ins, **kw):
    mod, _ = CASES[case]
    return C.phys(m, n, ins, **dict(dict(fp64_contacts_rk4=True, fp64_terrain=mod is T, fp64_elliptic=mod is E), **kw))


def stages(oracle, m, ins, e, xfrc_applied=None):
    """The four stage states of env e's RK4 step (oracle rk4: the classical tableau), rebuilt on the host from the oracle's forward
    passes: [(qpos, qvel, forward_debug at them)] for X[0] .. X[3], X[k + 1] = X[0] (+) h A_k F[k] with A = 1/2, 1/2, 1.  Every pass is
    solved from the oracle's cold start; the reference is converged, so the start does not show.  ``xfrc_applied``: env e's external
    wrench [nbody, 6], held over the step."""
    h = m.timestep
    q0, v0 = ins['qpos'][e], ins['qvel'][e]
    ctrl = ins['ctrl'][e] if m.nu and ins.get('ctrl') is not None else None
    out, q, v = [], q0, v0
    for a in (0.5, 0.5, 1.0, None):
        fd = oracle.forward_debug(m, q, v, ctrl=ctrl, xfrc_applied=xfrc_applied)
        out.append((q, v, fd))
        if a is not None:
            q, v = integrate_pos(m, q0, v, a*h), v0 + a*h*fd['qacc']
    return out


def pass_list(fd):
    """(ncon, the geom pairs) of a forward pass's contact list."""
    k = int(fd['ncon'])
    return k, fd['contact'][:k, 15:17].astype(int)


def first_pass_reference(oracle, m, ins):
    """What fmj_forward leaves on such a context: the first pass alone, its own contact list included, in the layout of
    support_f64_contacts.reference."""
    n = len(ins['qpos'])
    fds = [stages_first(oracle, m, ins, e) for e in range(n)]
    out = {k: np.array([fd[k] for fd in fds]) for k in ('qacc', 'xpos', 'xquat', 'xipos', 'sensordata')}
    con = np.array([fd['contact'] for fd in fds])
    return dict(out, qpos=ins['qpos'], qvel=ins['qvel'], contact=con[..., :15], geoms=con[..., 15:17].astype(int), dist=con[..., 17],
                ncon=np.array([fd['ncon'] for fd in fds], np.int32))


def stages_first(oracle, m, ins, e):
    ctrl = ins['ctrl'][e] if m.nu and ins.get('ctrl') is not None else None
    return oracle.forward_debug(m, ins['qpos'][e], ins['qvel'][e], ctrl=ctrl)


def conditions(oracle, case, m, ins):
    """What the issue asks of a one-step case, from the oracle alone; returns (ok, the reference of the step, the stage states per env,
    a description).  In every env: status 0 and a converged reference, in the fourth pass at least 4 contacts with a normal force and at
    least 1 penetrating contact without, a limit row with a force where the model has limits, and in each of the four passes no
    candidate point within 1e-9 of the ground (nor of a cell edge of the heightfield).  In some env of the case the fourth pass's contact
    list differs from the first's, in ncon or geom ids; the list the step leaves is the fourth pass's."""
    mod, _ = CASES[case]
    ref = C.reference(oracle, m, ins)      # (asserts status 0)
    n = len(ref['ncon'])
    st = [stages(oracle, m, ins, e) for e in range(n)]
    forced = np.array([(ref['contact'][e, :ref['ncon'][e], 12] > 0).sum() for e in range(n)])
    idle = ref['ncon'] - forced
    rows = 3 if mod is E else 4
    nlim = ref['nefc'] - rows*ref['ncon']
    limf = np.array([(ref['efc'][e, :nlim[e], 0] > 0).sum() for e in range(n)])
    clear = all(T.candidates_clear(m, dict(qpos=[q])) for s in st for q, _, _ in s)
    fourth_is_left = all(pass_list(st[e][3][2])[0] == ref['ncon'][e] and np.array_equal(pass_list(st[e][3][2])[1], ref['geoms'][e, :ref['ncon'][e]])
                         for e in range(n))
    differs = [pass_list(st[e][0][2])[0] != pass_list(st[e][3][2])[0] or not np.array_equal(pass_list(st[e][0][2])[1], pass_list(st[e][3][2])[1])
               for e in range(n)]
    ok = bool(ref['iterations'].max() < m.solver_iterations and forced.min() >= 4 and idle.min() >= 1 and clear and fourth_is_left and any(differs) and
              (not np.any(m.jnt_limited) or limf.min() >= 1))
    return ok, ref, st, dict(forced=forced, idle=idle, limit_rows_with_force=limf, ncon_first=[pass_list(s[0][2])[0] for s in st], ncon_fourth=ref['ncon'],
                             lists_differ=differs, fourth_is_left=fourth_is_left, clear=clear, iterations=ref['iterations'])


def first_seed(oracle, case, n=N, start=100, tries=60):
    m = make(case)
    for seed in range(start, start + tries):
        if conditions(oracle, case, m, inputs(case, m, n, seed))[0]:
            return seed
    raise AssertionError('no seed satisfies the conditions')


# ---- the trajectory: salamander33 from just above touch height under a ctrl tape, 60 RK4 steps
TRAJ_T = 60
TRAJ_LIFT = 1e-4      # how far above the touch height the lowest geom point starts (m)


def trajectory_inputs(m, n=N):
    """key_qpos lowered until the lowest geom point is TRAJ_LIFT above the plane, at rest; the ctrl tape of support_limits (0.3 sin, 2 Hz)."""
    from support_limits import tape
    r32 = lambda a: np.asarray(a, np.float64).astype(np.float32).astype(np.float64)
    q0 = np.tile(m.key_qpos, (n, 1)).astype(float)
    for e in range(n):
        q0[e, 2] = 0.0
        q0[e, 2] = -C.lowest_point(m, q0[e]) + TRAJ_LIFT
    return r32(q0), np.zeros((n, m.nv)), tape(m, n, TRAJ_T, 2.0)


def trajectory_runs(oracle, m, q0, v0, tape32):
    """The oracle's RK4 run step by step, plain and with the state rounded to fp32 after every step: (plain state, rounded state, the
    ncon sequence of each [T, n], the share of steps with a contact force per env)."""
    r32 = lambda a: np.asarray(a, np.float64).astype(np.float32).astype(np.float64)
    tape = tape32.astype(np.float64)
    n = len(q0)
    out = []
    for rounded in (False, True):
        q, v, ws, ncons, forced = q0, v0, None, [], np.zeros(n)
        for t in range(len(tape)):
            o = oracle.step_tf(m, q, v, ctrl=tape[t], warmstart=ws, want_AR=False)
            assert not o['status'].any()
            ncons.append(o['ncon'].copy())
            forced += np.array([(o['contact'][e, :o['ncon'][e], 12] > 0).any() for e in range(n)])
            q, v, ws = o['qpos'], o['qvel'], o['warmstart']
            if rounded:
                q, v = r32(q), r32(v)
        out.append((q, v, np.array(ncons), forced/len(tape)))
    return out
