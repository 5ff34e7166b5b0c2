"""The fp64 contact step (fmj_step_f64_contacts_kernel, fmj_step_f64_terrain_kernel, fmj_step_f64_elliptic_kernel of
csrc/fmj_f64_step.inc) away from the one point of its parameter space that test_gpu_f64_contacts.py, test_gpu_f64_terrain.py and
test_gpu_f64_elliptic.py visit: more than 64 contacts (the contact lanes of the second wave, the prefix sum across the two waves), a
truncated list past 64, solref / solimp / friction that differ per geom with every impedance branch and every meaning of solref on a
contact that carries a force (recipe P), a ground whose friction wins, pyramidal impratio 4, two ground geoms (two planes; a plane
beside the heightfield with a geom past the grid's edge), geoms on welded bodies and past geom 64, and the branches of the terrain
narrow phase that no walking model reaches (support_f64_contact_params.py has the models, the recipes and the conditions).

The bound is that of test_gpu_f64_step.py everywhere, contact records, ncon and geom ids included (support_f64_contacts._excess):
    |got - ref| <= ulp32(ref_i) + ulp32(max |ref| over the component's column group in that env)
against the oracle (Newton, 100 iterations, the model's tolerance), for one fmj_step (qacc_warmstart included) and one fmj_forward.
Every case first asserts again, from the oracle alone, what it is about; tests/test_f64_contact_recipes.py shows on the CPU that the
reference is converged on these inputs.  N = 4 everywhere."""
import numpy as np
import pytest

import support_f64_contacts as C
import support_f64_contact_params as P
from support_f64_contacts import N, FMJ_WARN_CONTACTFULL, _groups, _excess

pytestmark = pytest.mark.gpu


def _step_and_forward(m, ins, ref, family, label, forwards=(False, True)):
    """One fmj_step and one fmj_forward of ``ins`` against ``ref``: error / bound per field, all of them at most 1."""
    out = {}
    for forward in forwards:
        p = P.phys(m, ins, family)
        info = p.kernel_info()
        assert info['threads_per_env'] == 128 and info['fp64_step_kernel'] == P.KERNELS[family] and p.solver_effective == 'Newton'
        p.forward() if forward else p.step(1)
        ex = _excess(m, p, ref, forward, ins)
        print(label, 'forward' if forward else 'step', 'error / bound per field:', {k: round(v, 3) for k, v in ex.items()})
        out['forward' if forward else 'step'] = ex
    bad = {(w, k): v for w, ex in out.items() for k, v in ex.items() if v > 1.0}
    assert not bad, (label, bad)
    return out


@pytest.mark.parametrize('name', list(P.CASES))
def test_one_step_and_forward_to_the_ulp(oracle, name):
    m, ins, family = P.case(name)
    ok, ref, what = P.conditions(oracle, name, m, ins)
    print(name, what)
    assert ok, (name, what)
    _step_and_forward(m, ins, ref, family, name)


def test_a_list_past_64_is_truncated_and_reported(oracle):
    """The 'big-euler' inputs with max_contacts = 70 (every env has 92 candidates): the form of
    test_gpu_f64_contacts.py::test_a_full_contact_list_is_truncated_and_reported, the cut inside the second wave."""
    import support_f64_step as S
    import torch
    m, ins, family = P.case('big-euler')
    full = C.reference(oracle, m, ins)
    assert full['ncon'].min() > P.TRUNCATED > 64
    m.max_contacts = P.TRUNCATED
    a = oracle.step(m, ins['qpos'], ins['qvel'], ctrl=ins['ctrl'])
    b = oracle.step_tf(m, ins['qpos'], ins['qvel'], ctrl=ins['ctrl'], want_AR=False)
    assert np.all(b['ncon'] == m.max_contacts) and np.all(a['status'] == FMJ_WARN_CONTACTFULL)
    p = P.phys(m, ins, family)
    p.step(1)
    torch.cuda.synchronize()
    st = p.data.status.cpu().numpy()
    assert np.all(st == FMJ_WARN_CONTACTFULL), st      # reported, and nothing else
    assert np.array_equal(p.data.ncon.cpu().numpy(), b['ncon'])
    c16 = p.data.contact.cpu().numpy()
    worst = 0.0
    for e in range(N):      # the kept records are the oracle's first max_contacts
        assert np.array_equal(b['contact'][e, :, :3], full['contact'][e, :m.max_contacts, :3])
        worst = max(worst, S.ulp_excess(c16[e:e + 1, :, :3], b['contact'][e:e + 1, :, :3]))
        gg = np.ascontiguousarray(c16[e, :, 15]).view(np.int32)
        assert np.array_equal(gg >> 16, b['contact'][e, :, 15].astype(int)) and np.array_equal(gg & 0xffff, b['contact'][e, :, 16].astype(int))
    groups = _groups(m)
    ex = {k: S.ulp_excess(getattr(p.data, k).cpu().numpy(), a[k], groups[k]) for k in ('qpos', 'qvel', 'qacc')}
    ex['contact_pos'] = worst
    print('truncated at', P.TRUNCATED, 'error / bound:', {k: round(v, 3) for k, v in ex.items()})
    assert max(ex.values()) <= 1.0, ex
    p.step(1)      # not frozen: the next step moves the state
    torch.cuda.synchronize()
    assert not np.array_equal(p.data.qpos.cpu().numpy(), a['qpos'].astype(np.float32)) and float(p.data.time[0]) > 1.5*m.timestep


@pytest.mark.parametrize('which', P.NARROW)
def test_narrow_phase_branches_on_terrain(oracle, which):
    """Small hand-placed models on the terrain kernel through fmj_forward: the records (and everything else fmj_forward writes) against
    the oracle's; support_f64_contact_params.narrow_branch asserts from the numpy narrow phase which branch every env takes."""
    m, ins = P.narrow_case(which)
    ref = C.reference(oracle, m, ins)
    P.narrow_branch(which, m, ins, ref)
    print(which, 'ncon', ref['ncon'], 'dist', ref['dist'][0, :ref['ncon'][0]])
    _step_and_forward(m, ins, ref, 'terrain', which, forwards=(True,))
