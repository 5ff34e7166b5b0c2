"""The elliptic friction cone on the fp64 contact solve (BatchedPhysics(precision='fp64', fp64_contacts=True, fp64_elliptic=True):
fmj_create_ex2 with FMJ_CREATE_F64_CONTACTS | FMJ_CREATE_F64_ELLIPTIC, fmj_step_f64_elliptic_kernel of csrc/fmj_f64_step.inc) against
the fp64 oracle (Newton, 100 iterations, solver_tolerance 1e-10).

One step and fmj_forward are held to the bound of test_gpu_f64_contacts.py, contact records included:
    |got - ref| <= ulp32(ref_i) + ulp32(max |ref| over the component's column group in that env)
That is the rounding of the fp32 store; it is not fitted.  Every case first asserts, from the oracle alone, what
support_f64_elliptic.conditions states (the cone zones, no contact near the cone's surface without being on it, no grazing decision of
the narrow phase); that the reference is converged is asserted in test_f64_elliptic_recipes.py.  The trajectory is held to the oracle's
own run with the state rounded to fp32 every step, as the pyramidal walker's is."""
import warnings

import numpy as np
import pytest

from parity_metrics import relerr
import support_f64_contacts as C
import support_f64_elliptic as E
from support_f64_contacts import N, STATE, _groups, _excess

pytestmark = pytest.mark.gpu
KERNEL = 'fmj_step_f64_elliptic_kernel'


def _one_step(oracle, name, integrator, friction0=False, impratio=1.0):
    m = E.make(name, integrator, friction0=friction0, impratio=impratio)
    ins = E.inputs(name, m)
    ok, ref, what = E.conditions(oracle, name, m, ins, want_zones=not friction0)
    print(name, integrator, what)
    assert ok, (name, what)
    for forward in (False, True):
        p = E.phys(name, m, N, ins)
        info = p.kernel_info()
        assert info['threads_per_env'] == 128 and info['fp64_step_kernel'] == KERNEL and p.solver_effective == 'Newton'
        p.forward() if forward else p.step(1)
        ex = _excess(m, p, ref, forward, ins)
        print(name, integrator, 'forward' if forward else 'step', 'error / bound per field:', {k: round(v, 3) for k, v in ex.items()})
        bad = {k: v for k, v in ex.items() if v > 1.0}
        assert not bad, (name, integrator, forward, bad)


@pytest.mark.parametrize('integrator', ['euler', 'implicitfast'])
@pytest.mark.parametrize('name', E.ONE_STEP)
def test_one_step_and_forward_to_the_ulp(oracle, name, integrator):
    _one_step(oracle, name, integrator)


@pytest.mark.parametrize('name,friction0,impratio', E.FURTHER, ids=['salamander33-impratio4', 'centipede_20_25-friction0', 'centipede_hfield_cyl-friction0'])
def test_impratio_and_friction_0_to_the_ulp(oracle, name, friction0, impratio):
    """impratio = 4 (mu = fr / 2 in the cone, R_t = R_n / 4), and every geom at friction 0 (1e-5 after the clamp), which the pyramid
    refuses: the same bound."""
    _one_step(oracle, name, 'euler', friction0=friction0, impratio=impratio)


def test_a_pyramidal_model_on_a_flagged_context_runs_what_it_ran():
    """centipede(20, 25, contacts=True) under the pyramidal cone, 3 steps: the flagged context runs the contacts kernel, and every
    field equals the unflagged context's bit for bit."""
    import torch
    m = C.make('centipede_20_25')
    ins = C.inputs(m, N, C.SEEDS['centipede_20_25'])
    got = {}
    for flag in (False, True):
        p = C.phys(m, N, ins, fp64_elliptic=flag)
        assert p.kernel_info()['fp64_step_kernel'] == 'fmj_step_f64_contacts_kernel'
        p.step(3)
        torch.cuda.synchronize()
        assert int(p.data.status.abs().sum()) == 0
        got[flag] = {k: getattr(p.data, k).clone() for k in STATE + ('contact', 'ncon', 'time')}
    assert int(got[True]['ncon'].min()) > 0
    for k in got[False]:
        assert torch.equal(got[False][k], got[True][k]), k


def test_no_contact_no_bit_changed():
    """The elliptic centipede 1 m above the plane, 50 steps of fmj_step: every step is the unconstrained kernel's, against a plain fp64
    context of the same model with its geoms removed."""
    import torch
    a, b = E.make('centipede_20_25'), E.make('centipede_20_25')
    C.set_geoms(b, [], 0)
    ins = C.inputs(a, N, 5, depth=-1.0)
    assert min(C.lowest_point(a, q) for q in ins['qpos']) > 0.99
    pa = E.phys('centipede_20_25', a, N, ins)
    assert pa.kernel_info()['fp64_step_kernel'] == KERNEL
    pb = C.phys(b, N, ins, fp64_contacts=False)
    pa.step(50); pb.step(50)
    torch.cuda.synchronize()
    assert int(pa.data.status.abs().sum()) == 0 and int(pa.data.ncon.abs().sum()) == 0
    for k in ('qpos', 'qvel', 'qacc', 'sensordata', 'xpos', 'xquat', 'xipos', 'time'):
        assert torch.equal(getattr(pa.data, k), getattr(pb.data, k)), k


def test_the_solver_the_model_names_does_not_matter():
    import torch
    from farms_mujoco_amd.model import SOLVERS
    outs = []
    for solver in ('pgs', 'newton'):
        m = E.make('centipede_20_25')
        m.solver = SOLVERS[solver]
        ins = E.inputs('centipede_20_25', m)
        with warnings.catch_warnings(record=True) as w:
            warnings.simplefilter('always')
            p = E.phys('centipede_20_25', m, N, ins)
        said = [str(x.message) for x in w if 'primal Newton solve' in str(x.message)]
        assert len(said) == (solver == 'pgs'), (solver, [str(x.message) for x in w])      # only when the model asked for another solver
        assert (p.solver_requested, p.solver_effective, p.solver_budget) == ({'pgs': 'PGS', 'newton': 'Newton'}[solver], 'Newton', 100)
        p.step(3)
        torch.cuda.synchronize()
        assert int(p.data.status.abs().sum()) == 0
        outs.append({k: getattr(p.data, k).clone() for k in STATE + ('contact', 'ncon')})
    for k in outs[0]:
        assert torch.equal(outs[0][k], outs[1][k]), k
    assert int(outs[0]['ncon'].min()) > 0


def test_trajectory_against_the_state_rounding_floor(oracle):
    """The elliptic centipede dropped from 2 mm above the touch height under walk_tape, 150 steps in one launch: qpos / qvel no further
    from the plain oracle than the oracle's own run with the state rounded to fp32 every step.  The tape holds the lower legs 0.2 rad
    down (walk_tape's default is 0.25): the oracle then has a contact force in 94 % of the steps in every env; at 0.25 env 2 of the
    elliptic walker leaves the ground again for nine steps after its first touch and has one in 89.3 %."""
    import torch
    from farms_mujoco_amd.model import centipede_touch_height
    m = E.make('centipede_20_25')
    Tn = 150
    tape32 = C.walk_tape(m, N, Tn, stance=0.2)
    tape = tape32.astype(np.float64)
    r32 = lambda a: np.asarray(a, np.float64).astype(np.float32).astype(np.float64)
    q0 = np.tile(m.key_qpos, (N, 1)); q0[:, 2] = centipede_touch_height() + 2e-3; q0 = r32(q0)
    v0 = np.zeros((N, m.nv))
    q, v, ws = q0, v0, None
    with_force = np.zeros(N)
    for t in range(Tn):      # the condition, from a step-by-step oracle run (the warm start carried as mj_step carries it)
        o = oracle.step_tf(m, q, v, ctrl=tape[t], warmstart=ws, want_AR=False)
        with_force += np.array([(o['contact'][e, :o['ncon'][e], 12] > 0).any() for e in range(N)])
        q, v, ws = o['qpos'], o['qvel'], o['warmstart']
    print('share of steps with a contact force', with_force/Tn)
    assert (with_force/Tn).min() >= 0.9, with_force/Tn
    ref = oracle.step(m, q0, v0, ctrl=tape, n_steps=Tn, ctrl_step_stride=N*m.nu, n_threads=4)
    fq, fv = q0, v0
    for t in range(Tn):      # floor_state: the oracle's own run with the state rounded to fp32 every step
        o = oracle.step(m, fq, fv, ctrl=tape[t], n_steps=1, n_threads=4)
        fq = r32(o['qpos']); fv = r32(o['qvel'])
    p = E.phys('centipede_20_25', m, N, dict(qpos=q0, qvel=v0, ctrl=None))
    p.step(Tn, torch.as_tensor(tape32, device=p.device).contiguous())
    torch.cuda.synchronize()
    assert int(p.data.status.abs().sum()) == 0
    for k, fl in (('qpos', fq), ('qvel', fv)):
        err, floor = relerr(getattr(p.data, k).cpu().numpy(), ref[k]), relerr(fl, ref[k])
        print(k, 'after', Tn, 'steps: fp64 elliptic kernel %.3g  floor_state %.3g  ratio %.3g' % (err, floor, err/floor))
        assert err <= floor, (k, err, floor)


def test_a_full_contact_list_is_truncated_and_reported(oracle):
    import support_f64_step as S
    import torch
    name = 'centipede_20_25'
    m = E.make(name)
    ins = E.inputs(name, m)
    full = C.reference(oracle, m, ins)
    m.max_contacts = int(full['ncon'].min()) - 2
    assert m.max_contacts >= 4
    a = oracle.step(m, ins['qpos'], ins['qvel'], ctrl=ins['ctrl'])
    b = oracle.step_tf(m, ins['qpos'], ins['qvel'], ctrl=ins['ctrl'], want_AR=False)
    assert np.all(b['ncon'] == m.max_contacts) and np.all(a['status'] & C.FMJ_WARN_CONTACTFULL)
    p = E.phys(name, m, N, ins)
    p.step(1)
    torch.cuda.synchronize()
    st = p.data.status.cpu().numpy()
    assert np.all(st == C.FMJ_WARN_CONTACTFULL), st      # reported, and nothing else
    assert np.array_equal(p.data.ncon.cpu().numpy(), b['ncon'])
    c16 = p.data.contact.cpu().numpy()
    for e in range(N):      # the kept records are the oracle's first max_contacts
        assert np.array_equal(b['contact'][e, :, :3], full['contact'][e, :m.max_contacts, :3])
        assert S.ulp_excess(c16[e:e + 1, :, :3], b['contact'][e:e + 1, :, :3]) <= 1.0
        gg = np.ascontiguousarray(c16[e, :, 15]).view(np.int32)
        assert np.array_equal(gg & 0xffff, b['contact'][e, :, 16].astype(int))
    groups = _groups(m)
    ex = {k: S.ulp_excess(getattr(p.data, k).cpu().numpy(), a[k], groups[k]) for k in ('qpos', 'qvel', 'qacc')}
    print('truncated list, error / bound:', ex)
    assert max(ex.values()) <= 1.0, ex
    p.step(1)      # not frozen: the next step moves the state
    torch.cuda.synchronize()
    assert not np.array_equal(p.data.qpos.cpu().numpy(), a['qpos'].astype(np.float32)) and float(p.data.time[0]) > 1.5*m.timestep


def test_a_nan_qvel_freezes_its_env_alone(oracle):
    import torch
    name = 'centipede_20_25'
    m = E.make(name)
    ins = E.inputs(name, m)
    ref = C.reference(oracle, m, ins)
    p = E.phys(name, m, N, ins)
    p.data.qvel[1, 7] = float('nan')
    before = {k: getattr(p.data, k)[1].clone() for k in ('qpos', 'xpos', 'sensordata', 'time')}
    p.step(1)
    torch.cuda.synchronize()
    st = p.data.status.cpu().numpy()
    assert st[1] != 0 and not st[[0, 2, 3]].any(), st
    for k, v in before.items():      # the frozen env keeps what it had
        assert torch.equal(getattr(p.data, k)[1], v), k
    import support_f64_step as S
    groups = _groups(m)
    keep = [0, 2, 3]
    for k in ('qpos', 'qvel', 'qacc'):      # the others stepped, to the bound
        assert S.ulp_excess(getattr(p.data, k).cpu().numpy()[keep], ref[k][keep], groups[k]) <= 1.0, k


def test_a_fused_launch_is_refused_and_the_context_reports_its_kernel():
    import ctypes
    from farms_mujoco_amd import _lib as L
    name = 'centipede_20_25'
    m = E.make(name)
    p = E.phys(name, m, N, E.inputs(name, m))
    args = L.CFusedArgs()
    rc = p._lib.fmj_step_fused_f64(p._ctx, ctypes.byref(p._cdata()), ctypes.byref(args), None, L.stream_ptr(p.device))
    msg = p._lib.fmj_last_error().decode()
    assert rc != 0 and 'fp64' in msg and 'contact' in msg, (rc, msg)
    maxefc, max_contacts, iterations = L.ints(p._lib.fmj_constraint_info, p._ctx)
    assert (maxefc, max_contacts, iterations) == (2*m.njnt + 4*m.max_contacts, m.max_contacts, 100)
    info = p.kernel_info()
    assert info['fp64_step_kernel'] == KERNEL and info['lds_bytes_per_env'] <= 160*1024
    pyr = C.make(name)      # the record keeps its stride: the LDS is the terrain context's
    pt = C.phys(pyr, N, C.inputs(pyr, N, C.SEEDS[name]), fp64_terrain=True)
    assert info['lds_bytes_per_env'] == pt.kernel_info()['lds_bytes_per_env'] and pyr.max_contacts == m.max_contacts
