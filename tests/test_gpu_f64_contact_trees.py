"""The fp64 contact step (the five kernel families of csrc/fmj_f64_step.inc: contacts, terrain, elliptic, mesh, mesh-elliptic) on the
random trees of tests/wide_trees.py, up to its size limits: free, fixed and hinged / sliding bases, dof chains of 64 with a contact at
the leaf, 128 bodies and 128 dofs, contacts whose last dof, body, list slot or geom lane lies in the second wave, welded geoms whose
jointed ancestor is several bodies up, a one-dof model, joint limits on the chains of the contacts, and the LDS edge of the largest model
(max_contacts = 128 on the contacts family: 163 024 bytes; 120 on the families built from the terrain text: 163 792 bytes, 48 under the
limit), where an array running past its region of the LDS map would be silent (support_f64_contact_trees.py has the models, the inputs
and the conditions; tests/test_f64_contact_tree_recipes.py shows them on the CPU).

The bound is that of test_gpu_f64_step.py everywhere, contact records, ncon and geom ids included (support_f64_contacts._excess):
    |got - ref| <= ulp32(ref_i) + ulp32(max |ref| over the component's column group in that env)
against the oracle (Newton, 100 iterations, the model's tolerance), for one fmj_step (qacc_warmstart included) and one fmj_forward.
Every case first asserts again, from the model and the oracle alone, what it is about."""
import numpy as np
import pytest

import support_f64_contacts as C
import support_f64_contact_trees as K
from parity_metrics import relerr
from support_f64_contacts import FMJ_WARN_CONTACTFULL, STATE, _groups, _excess
from support_f64_interface import lds_bytes

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize('name', list(K.CASES))
def test_one_step_and_forward_to_the_ulp(oracle, name):
    import torch
    m, ins, family = K.case(name)
    n = K.envs_of(name)
    limits = K.CASES[name][3] == 'limits'
    ok, ref, what = K.conditions(oracle, name, m, ins)
    print(name, what)
    assert ok, (name, what)
    rowless = ref['nefc'] == 0      # a step without candidate rows: qacc_warmstart is by design the step's qacc (the fp64 limits step)
    assert not rowless.any() or K.CASES[name][0] == 11, (name, ref['nefc'])
    ref = dict(ref, qacc_warmstart=np.where(rowless[:, None], ref['qacc'], ref['qacc_warmstart']))
    out = {}
    for forward in (False, True):
        p = K.phys(m, n, ins, family)
        info = p.kernel_info()
        assert info['threads_per_env'] == 128 and info['fp64_step_kernel'] == K.KERNELS[family] and p.solver_effective == 'Newton'
        assert bool(p.fp64_limits) == limits == bool(np.any(m.jnt_limited))      # the <LIMITS> build where the case has limits
        if K.CASES[name][3] == 'lds':
            text = 'contacts' if family == 'contacts' else 'terrain'
            assert info['lds_bytes_per_env'] == K.LDS_BYTES[text] == lds_bytes(text, m.nbody, m.nv, m.nq, 64, m.max_contacts), info
        p.forward() if forward else p.step(1)
        ex = _excess(m, p, ref, forward, ins)
        print(name, 'forward' if forward else 'step', 'error / bound per field:', {k: round(v, 3) for k, v in ex.items()})
        out['forward' if forward else 'step'] = ex
        if n == 5:      # env 4 repeats env 1's inputs: the result does not depend on the batch slot
            torch.cuda.synchronize()
            for k in STATE + ('contact', 'ncon'):
                if not (forward and k == 'qacc_warmstart'):
                    a = getattr(p.data, k)
                    assert torch.equal(a[4], a[1]), (name, forward, k)
    bad = {(w, k): v for w, ex in out.items() for k, v in ex.items() if v > 1.0}
    assert not bad, (name, bad)


def test_a_list_past_128_is_truncated_and_reported(oracle):
    """The largest model with every env's full list longer than max_contacts = 128 (135 .. 160 candidates): the form of
    test_gpu_f64_contact_params.py::test_a_list_past_64_is_truncated_and_reported, every contact lane in use and the cut behind the last."""
    import support_f64_step as S
    import torch
    m, ins, family = K.truncated_case()
    full = K.full_list(oracle, m, ins)
    assert full['ncon'].min() > m.max_contacts == 128
    a = oracle.step(m, ins['qpos'], ins['qvel'], ctrl=ins['ctrl'])
    b = oracle.step_tf(m, ins['qpos'], ins['qvel'], ctrl=ins['ctrl'], want_AR=False)
    assert np.all(b['ncon'] == m.max_contacts) and np.all(a['status'] == FMJ_WARN_CONTACTFULL)
    p = K.phys(m, K.N, ins, family)
    assert p.kernel_info()['lds_bytes_per_env'] == K.LDS_BYTES['contacts']
    p.step(1)
    torch.cuda.synchronize()
    st = p.data.status.cpu().numpy()
    assert np.all(st == FMJ_WARN_CONTACTFULL), st      # reported, and nothing else
    assert np.array_equal(p.data.ncon.cpu().numpy(), b['ncon'])
    c16 = p.data.contact.cpu().numpy()
    worst = 0.0
    for e in range(K.N):      # the kept records are the oracle's first max_contacts
        assert np.array_equal(b['contact'][e, :, :3], full['contact'][e, :m.max_contacts, :3])
        worst = max(worst, S.ulp_excess(c16[e:e + 1, :, :3], b['contact'][e:e + 1, :, :3]))
        gg = np.ascontiguousarray(c16[e, :, 15]).view(np.int32)
        assert np.array_equal(gg >> 16, b['contact'][e, :, 15].astype(int)) and np.array_equal(gg & 0xffff, b['contact'][e, :, 16].astype(int))
    groups = _groups(m)
    ex = {k: S.ulp_excess(getattr(p.data, k).cpu().numpy(), a[k], groups[k]) for k in ('qpos', 'qvel', 'qacc')}
    ex['contact_pos'] = worst
    print('truncated at', m.max_contacts, 'error / bound:', {k: round(v, 3) for k, v in ex.items()})
    assert max(ex.values()) <= 1.0, ex


@pytest.mark.parametrize('name', list(K.TRAJECTORIES))
def test_trajectory_against_the_state_rounding_floor(oracle, name):
    """60 steps in one launch under a ctrl tape on a fixed and on a hinged base, from rest at the case's pose: qpos / qvel no further
    from the plain oracle than the oracle's own run with the state rounded to fp32 every step."""
    import torch
    m, q0, v0, tape32 = K.trajectory_case(name)
    n, steps = K.N, K.TRAJECTORY_STEPS
    tape = tape32.astype(np.float64)
    r32 = lambda a: np.asarray(a, np.float64).astype(np.float32).astype(np.float64)
    share = K.share_of_steps_with_a_force(oracle, m, q0, v0, tape)
    print(name, 'share of steps with a contact force', share)
    assert share.min() > 0.5, share
    ref = oracle.step(m, q0, v0, ctrl=tape, n_steps=steps, ctrl_step_stride=n*m.nu, n_threads=4)
    assert not ref['status'].any()
    fq, fv = q0, v0
    for t in range(steps):      # floor_state: the oracle's own run with the state rounded to fp32 every step
        o = oracle.step(m, fq, fv, ctrl=tape[t], n_steps=1, n_threads=4)
        fq = r32(o['qpos']); fv = r32(o['qvel'])
    p = K.phys(m, n, dict(qpos=q0, qvel=v0, ctrl=None), 'contacts')
    p.step(steps, torch.as_tensor(tape32, device=p.device).contiguous())
    torch.cuda.synchronize()
    assert int(p.data.status.abs().sum()) == 0
    for k, fl in (('qpos', fq), ('qvel', fv)):
        err, floor = relerr(getattr(p.data, k).cpu().numpy(), ref[k]), relerr(fl, ref[k])
        print(name, k, 'after', steps, 'steps: fp64 kernel %.3g  floor_state %.3g  ratio %.3g' % (err, floor, err/floor))
        assert err <= floor, (k, err, floor)


def test_no_contact_no_bit_changed():
    """WIDE_SHAPES tree 3 (fixed base) with the plane 1 m below every geom, 20 steps of fmj_step: every step is the unconstrained
    kernel's, against a plain fp64 context of the same tree with its geoms removed."""
    import torch
    a, b, ins = K.lifted()
    pa = K.phys(a, K.N, ins, 'contacts')
    pb = C.phys(b, K.N, ins, fp64_contacts=False)
    assert pa.kernel_info()['fp64_step_kernel'] == 'fmj_step_f64_contacts_kernel' and pb.kernel_info()['fp64_step_kernel'] == 'fmj_step_f64_kernel'
    pa.step(20); pb.step(20)
    torch.cuda.synchronize()
    assert int(pa.data.status.abs().sum()) == 0 and int(pa.data.ncon.abs().sum()) == 0
    for k in ('qpos', 'qvel', 'qacc', 'sensordata', 'xpos', 'xquat', 'xipos', 'time'):
        assert torch.equal(getattr(pa.data, k), getattr(pb.data, k)), k
    assert not torch.equal(pa.data.qpos, torch.as_tensor(ins['qpos'], dtype=torch.float32, device=pa.data.qpos.device))
