"""The inputs of tests/test_gpu_f64_contact_trees.py, checked on the CPU oracle alone (no GPU): every case of
support_f64_contact_trees.CASES passes every check of fmj_create_ex2 with its family's flags, has at its seed what it is about
(support_f64_contact_trees.conditions: contacts with and without a force in every env, no narrow-phase decision within 1e-9, a solve
that ended below its budget, a reference that a 100 x tighter tolerance with 200 iterations moves by no more than 0.1 of the one-step
bound, and the structural facts of CLAIMS), and the headline facts are read once more here from dof_depth, body_dofnum, geom_bodyid
and the oracle's records without the support module's helpers.  The LDS arithmetic of the largest model is held to the byte."""
import numpy as np
import pytest

import support_f64_contacts as C
import support_f64_terrain as T
import support_f64_contact_trees as K
from support_capi import FMJ_ERR_UNSUPPORTED
from support_f64_interface import create_ex2, accepted, lds_bytes
from wide_trees import dof_depth


def _forced(m, ref):
    """(env, slot, geom, body, last dof) of every oracle contact with a normal force; the last dof by walking up body_parentid to the
    first body with a dof (the rule of the geom table), and how many bodies up that was."""
    out = []
    for e in range(len(ref['ncon'])):
        for c in range(int(ref['ncon'][e])):
            if not ref['contact'][e, c, 12] > 0:
                continue
            g = int(ref['geoms'][e, c, 1]); b = int(m.geom_bodyid[g])
            a, up = b, 0
            while m.body_dofnum[a] == 0:
                a, up = int(m.body_parentid[a]), up + 1
                assert a >= 1, 'a geom on a body without a jointed ancestor'
            out.append((e, c, g, b, int(m.body_dofadr[a] + m.body_dofnum[a] - 1), up))
    return out


def test_the_models_are_what_the_recipe_says():
    for name, (shape, family, integrator, what) in K.CASES.items():
        m = K.make(name)
        an = [g for g in range(m.ngeom) if g not in T.grounds(m)]
        assert T.grounds(m) == [0] and m.geom_bodyid[0] == 0 and m.ngeom <= 128 and m.max_contacts <= 128, name      # the ground first
        assert m.geom_friction[0, 0] == (K.GROUND_FRICTION if what == 'mu' else 0.0)
        assert m.geom_friction[an, 0].min() >= 0.5 and m.geom_friction[an, 0].max() <= 1.2
        anc, up = K.jointed_ancestor(m)
        assert all(anc[m.geom_bodyid[g]] >= 1 for g in an), name      # fmj_create_ex2 refuses a geom without a jointed ancestor
        assert (m.jnt_type[0] == 0) == (K.BASE[shape] == 'free') and (m.body_dofnum[1] == 0) == (K.BASE[shape] == 'fixed')
        assert bool(np.any(m.jnt_limited)) == (what == 'limits') and (m.geom_type[0] == T.GEOM_HFIELD) == (what == 'hfield')
        if what == 'limits':
            sj = int((m.jnt_type != 0).sum())
            assert int(np.sum(m.jnt_limited)) == max(3, sj//3)
        if shape == 11:
            assert (m.nbody, m.nv, m.ngeom) == (2, 1, 2) and m.geom_type[1] == C.GEOM_SPHERE
            continue
        assert np.all(np.abs(m.geom_pos[an]).max(axis=1) > 0) and np.all(np.abs(m.geom_quat[an, 0]) < 1), name      # off-centre, turned
        assert len(set(m.geom_bodyid[an])) < len(an) or what == 'lds', name             # some bodies carry two geoms (lds: all 127 carry one)
        assert any(m.body_dofnum[m.geom_bodyid[g]] == 0 for g in an) or not np.any(m.body_dofnum[2:] == 0), name      # some geoms on welded bodies
        kinds = set(int(t) for t in m.geom_type[an])
        assert {C.GEOM_CAPSULE, C.GEOM_BOX} <= kinds, (name, kinds)
        assert (T.GEOM_CYLINDER in kinds) == (family == 'terrain' or (what == 'lds' and family == 'elliptic')), (name, kinds)
        assert (K.GEOM_MESH in kinds) == (family in ('mesh', 'mesh_elliptic')), (name, kinds)
        if family in ('elliptic', 'mesh_elliptic'):
            assert (int(m.cone), m.impratio, m.solver_tolerance) == (1, 4.0, K.E.TOLERANCE)
        if what == 'lds':
            assert (m.nbody, m.nv, m.nq, m.ngeom, m.max_contacts) == (128, 128, 129, 128, K.LDS_MAX_CONTACTS[family])
    assert sum(1 for c in K.CASES.values() if c[3] == 'n5') == 2 and any(c[3] == 'mu' for c in K.CASES.values())
    assert {n for n, c in K.CASES.items() if c[1] == 'contacts' and c[3] in ('', 'n5', 'mu')} == {'contacts-%d' % s for s in range(1, 13)}
    for family in K.FAMILIES[1:]:
        assert {c[0] for c in K.CASES.values() if c[1] == family} >= {1, 3, 4, 7}


@pytest.mark.parametrize('name', list(K.CASES))
def test_the_case_has_what_it_is_about_and_the_reference_is_converged(oracle, name):
    m, ins, family = K.case(name)
    assert np.array_equal(ins['qpos'], ins['qpos'].astype(np.float32).astype(np.float64)) and len(ins['qpos']) == K.envs_of(name)
    rc, msg, prec, _ = create_ex2(m, flags=K.flags_of(m, family))
    assert accepted(rc, msg, prec), (name, rc, msg)
    ok, ref, what = K.conditions(oracle, name, m, ins)
    print(name, what)
    assert ok, (name, what)
    assert ref['iterations'].max() < m.solver_iterations and not ref['status'].any()
    assert max(what['moved_by_a_tighter_tolerance'].values()) <= 0.1


# the headline facts, per case: (what, argument)
HEADLINES = {'contacts-1': [('depth', 63), ('dof64', None), ('body64', None), ('on_body', 1)], 'contacts-8': [('depth', 63)], 'contacts-3': [('depth', 31)],
             'contacts-2': [('depth', 32)], 'contacts-4': [('slide', None), ('last_dof', 0)], 'contacts-5': [('body64', None), ('no_dof64', None), ('last_dof', 0)],
             'contacts-6': [('dof64', None), ('no_body64', None)], 'contacts-7': [('welded_up', 2)], 'lds-contacts': [('slot64', None), ('geom64', None)],
             'lds-terrain': [('slot64', None), ('geom64', None)]}


@pytest.mark.parametrize('name', list(HEADLINES))
def test_the_structural_claims_from_the_model_and_the_records(oracle, name):
    m, ins, _ = K.case(name)
    ref = C.reference(oracle, m, ins)
    f = _forced(m, ref)
    depth = dof_depth(m)
    assert f
    for what, arg in HEADLINES[name]:
        if what == 'depth':      # a chain of arg + 1 dofs ends in the contact's last dof
            hit = [x for x in f if depth[x[4]] == arg]
            assert hit and len(K.chain(m, hit[0][4])) == arg + 1, (name, what, arg)
        elif what == 'dof64':
            assert any(x[4] >= 64 for x in f)
        elif what == 'no_dof64':
            assert m.nv <= 64
        elif what == 'body64':
            assert any(x[3] >= 64 for x in f)
        elif what == 'no_body64':
            assert m.nbody <= 64
        elif what == 'on_body':
            assert any(x[3] == arg for x in f) and m.jnt_type[m.body_jntadr[arg]] == 0
        elif what == 'slide':
            on = {d for x in f for d in K.chain(m, x[4])}
            assert any(m.jnt_type[j] == 2 and m.jnt_dofadr[j] in on for j in range(m.njnt))
        elif what == 'last_dof':      # the hinged or sliding root itself
            assert m.body_dofnum[1] == 1 and m.body_dofadr[1] == arg and any(x[4] == arg for x in f)
        elif what == 'welded_up':
            assert any(x[5] >= arg for x in f)
        elif what == 'slot64':
            assert any(x[1] >= 64 for x in f) and ref['ncon'].min() > 64
        elif what == 'geom64':
            assert any(x[2] >= 64 for x in f)
        else:
            raise KeyError(what)


def test_the_smallest_model_has_envs_with_and_without_its_contact(oracle):
    m, ins, _ = K.case('contacts-11')
    ref = C.reference(oracle, m, ins)
    assert (m.nbody, m.nv, m.max_contacts) == (2, 1, 4) and sorted(ref['ncon']) == [0, 0, 1, 1] and m.geom_pos[0, 2] != 0
    assert [(ref['contact'][e, 0, 12] > 0) for e in range(4) if ref['ncon'][e]] == [True, True]


def test_the_seeds_are_the_first_that_satisfy_the_conditions(oracle):
    """first_seed on three of the cases whose seed is not the first tried (the others are 100: the first)."""
    assert all(K.SEEDS[n] == 100 for n in K.CASES if n not in K.NOT_THE_FIRST_TRIED) and all(K.SEEDS[n] > 100 for n in K.NOT_THE_FIRST_TRIED)
    for name in ('contacts-5', 'contacts-9', 'contacts-10-limits'):
        assert K.first_seed(oracle, name) == K.SEEDS[name], name


def test_the_lds_bytes_at_the_edge():
    """Shape 1 (128 bodies, 128 dofs, nq 129, row length 64): 163 024 bytes at 128 contacts on the contacts family, 163 792 at 120 on the
    terrain text - 48 under gfx950's 163 840 - and 121 refused with the bytes named."""
    assert lds_bytes('contacts', 128, 128, 129, 64, 128) == K.LDS_BYTES['contacts'] == 163024
    assert lds_bytes('terrain', 128, 128, 129, 64, 120) == K.LDS_BYTES['terrain'] == 163792 == 160*1024 - 48
    need = lds_bytes('terrain', 128, 128, 129, 64, 121)
    assert need > 160*1024
    for name in ('lds-terrain', 'lds-elliptic', 'lds-mesh', 'lds-mesh_elliptic'):
        m = K.make(name)
        family = K.CASES[name][1]
        rc, msg, prec, _ = create_ex2(m, flags=K.flags_of(m, family))
        assert accepted(rc, msg, prec), (name, rc, msg)
        m.max_contacts = 121
        rc, msg, prec, _ = create_ex2(m, flags=K.flags_of(m, family))
        assert rc == FMJ_ERR_UNSUPPORTED and 'needs %d bytes of LDS' % need in msg, (name, rc, msg)


def test_the_truncation_case_cuts_a_list_past_128(oracle):
    m, ins, family = K.truncated_case()
    full = K.full_list(oracle, m, ins)
    assert full['ncon'].min() > m.max_contacts == 128 and K.clear(m, ins)
    a = oracle.step(m, ins['qpos'], ins['qvel'], ctrl=ins['ctrl'])
    b = oracle.step_tf(m, ins['qpos'], ins['qvel'], ctrl=ins['ctrl'], want_AR=False)
    assert np.all(b['ncon'] == 128) and np.all(a['status'] == C.FMJ_WARN_CONTACTFULL) and b['iterations'].max() < m.solver_iterations
    for e in range(K.N):
        assert np.array_equal(b['contact'][e, :, :3], full['contact'][e, :128, :3])
        assert (b['contact'][e, 64:, 12] > 0).sum() >= 1


def test_the_trajectory_cases_keep_their_contacts(oracle):
    """More than half of the 60 steps have a contact force in every env, on a fixed and on a hinged base."""
    bases = set()
    for name in K.TRAJECTORIES:
        m, q0, v0, tape32 = K.trajectory_case(name)
        share = K.share_of_steps_with_a_force(oracle, m, q0, v0, tape32.astype(np.float64))
        print(name, 'share of steps with a contact force', share)
        assert share.min() > 0.5, (name, share)
        bases.add(K.BASE[K.CASES[name][0]])
    assert bases == {'fixed', 'hinge'}


def test_the_lifted_tree_is_clear_of_the_plane():
    a, b, ins = K.lifted()
    assert K.BASE[3] == 'fixed' and a.ngeom > 40 and b.ngeom == 0 and (a.nbody, a.nv) == (b.nbody, b.nv)
    assert min(d.min() for q in ins['qpos'] for _, d, _ in K.geom_candidates(a, q)) > 0.99
