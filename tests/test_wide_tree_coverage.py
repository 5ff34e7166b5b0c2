"""What the random trees of test_gpu_wide_random_trees.py exercise in the two-wave step kernel (csrc/fmj_wide.inc), checked from the
model arrays alone: the model-wide shortcuts and joint / actuator kinds the kernel branches on, both register-row builds, and the
workgroup machinery (rounds split across the two waves, pointer jumping past round 4, nq past 128).  And fmj_create accepts every tree;
it validates a model before it looks for a device, so this runs without a GPU."""
import numpy as np
import pytest

from wide_trees import WIDE_SHAPES, shape_tree, tree_properties, elimination_rounds
from support_capi import create as _create, no_gpu as _no_gpu, FMJ_ERR_NODEVICE


@pytest.fixture(scope='module')
def trees():
    return {s[0]: shape_tree(s[0]) for s in WIDE_SHAPES}


def test_wide_trees_have_the_shapes_they_were_drawn_at(trees):
    for seed, nbody, nv, base, chain in WIDE_SHAPES:
        p = tree_properties(trees[seed])
        assert (p['nbody'], p['nv'], p['chain']) == (nbody, nv, chain), (seed, p)
        assert p['base'] == {'free': 'free', 'fixed': 'fixed', 'hinge': 'hinged'}[base], (seed, p['base'])


def test_wide_trees_cover_the_two_wave_kernel(trees):
    """Every property below is hit by at least one tree; the table printed is the coverage of each seed."""
    props = {seed: tree_properties(m) for seed, m in trees.items()}
    need = {
        # the general branches of phases K and C, and the other per-model shortcuts
        'off-centre hinge anchors (any_jpos)': lambda p: p['any_jpos'],
        'rotated body frames (any_bquat)': lambda p: p['any_bquat'],
        'rotated inertial frames (any_iquat)': lambda p: p['any_iquat'],
        'hinge joints': lambda p: p['hinge'], 'slide joints': lambda p: p['slide'], 'welded bodies': lambda p: p['welded'],
        'free base': lambda p: p['base'] == 'free', 'fixed base': lambda p: p['base'] == 'fixed', 'hinged base': lambda p: p['base'] == 'hinged',
        'damping': lambda p: p['damping'], 'stiffness': lambda p: p['stiffness'], 'qpos0 offsets': lambda p: p['qpos0_offset'],
        'armature': lambda p: p['armature'],
        'position actuators': lambda p: p['position'], 'velocity actuators with a gain': lambda p: p['velocity_gain'],
        'motors': lambda p: p['motor'], 'ctrl ranges': lambda p: p['ctrlrange'], 'force ranges': lambda p: p['forcerange'],
        'vertical gravity': lambda p: not p['tilted_gravity'], 'tilted gravity': lambda p: p['tilted_gravity'],
        # size and shape
        'nbody > 64 with nv <= 64': lambda p: p['nbody'] > 64 and p['nv'] <= 64,
        'nbody <= 64 with nv > 64': lambda p: p['nbody'] <= 64 and p['nv'] > 64,
        'nbody 128, nv 128, nq 129': lambda p: (p['nbody'], p['nv'], p['nq']) == (128, 128, 129),
        'both counts within one wave': lambda p: p['nbody'] <= 64 and p['nv'] <= 64,
        'rs 32 build': lambda p: p['rs'] == 32, 'rs 64 build': lambda p: p['rs'] == 64,
        'dof chain of exactly 32': lambda p: p['chain'] == 32, 'dof chain of exactly 33': lambda p: p['chain'] == 33,
        'dof chain of exactly 64': lambda p: p['chain'] == 64,
        'nq > 128 (a second qpos entry on lane 0)': lambda p: p['nq_past_128'],
        'dofs in wave 1': lambda p: p['dofs_in_wave1'], 'bodies in wave 1': lambda p: p['bodies_in_wave1'],
        'a level of more than six dofs (split across rounds)': lambda p: p['wide_level'],
        'a round with dofs of both waves': lambda p: p['split_round_across_waves'],
        'pointer jumping past round 4 (JUMP_SRC from LDS)': lambda p: p['jump_src_from_lds'],
        'a body lane that is not its dof lane': lambda p: p['body_lane_not_dof_lane'],
    }
    for name, f in need.items():
        hit = [seed for seed, p in props.items() if f(p)]
        print(f'{name:55s} seeds {hit}')
        assert hit, name


def test_round_grouping_keeps_the_elimination_invariants(trees):
    """The rounds that elimination_rounds forms (its restatement of fmj_create's grouping, fmj_hip.hip, by reading: the uploaded table
    has no accessor) put every dof in exactly one round, a round's dofs at one depth, deepest first, at most six per round, and a dof's
    ancestors all eliminated after it."""
    for seed, m in trees.items():
        rounds = elimination_rounds(m)
        flat = [d for r in rounds for d in r]
        assert sorted(flat) == list(range(m.nv)), seed
        pos = {d: k for k, r in enumerate(rounds) for d in r}
        for k, r in enumerate(rounds):
            assert 1 <= len(r) <= 6 and r == sorted(r)
            for d in r:
                a = m.dof_parentid[d]
                while a >= 0:
                    assert pos[a] > k, (seed, d, a)
                    a = m.dof_parentid[a]


def test_wide_random_tree_draws_are_seeded():
    """The same seed draws the same tree."""
    a, b = shape_tree(6), shape_tree(6)
    for k in ('body_parentid', 'body_pos', 'body_quat', 'jnt_type', 'jnt_axis', 'jnt_pos', 'actuator_gain', 'gravity'):
        assert np.array_equal(getattr(a, k), getattr(b, k)), k


# sha1 of what random_tree(0..19) draws (tree structure, joint kinds, frames, axes, actuators, gravity), taken before the wide generator
# was added: test_random_tree_vs_oracle and its two-wave run in test_gpu_wide_random_trees.py must keep stepping these trees
RANDOM_TREE_DIGEST = '00dcf40a493afc37f913a6f2610ae325581e73e4'


def random_tree_digest():
    import hashlib
    from support_models import random_tree
    h = hashlib.sha1()
    for seed in range(20):
        m = random_tree(seed)
        for k in ('body_parentid', 'jnt_type', 'jnt_qposadr', 'dof_parentid', 'actuator_jntid'):
            h.update(np.ascontiguousarray(getattr(m, k), np.int64).tobytes())
        for k in ('body_pos', 'body_quat', 'body_mass', 'jnt_axis', 'jnt_pos', 'jnt_stiffness', 'dof_damping', 'dof_armature', 'qpos0',
                  'actuator_gain', 'actuator_bias', 'actuator_forcerange', 'gravity'):
            h.update(np.round(np.asarray(getattr(m, k), np.float64), 9).tobytes())
        h.update(repr(list(m.actuator_tags)).encode())
    return h.hexdigest()


def test_random_tree_draws_are_unchanged():
    assert random_tree_digest() == RANDOM_TREE_DIGEST


@pytest.mark.parametrize('seed', [s[0] for s in WIDE_SHAPES])
def test_fmj_create_accepts_every_wide_tree(trees, seed):
    rc, msg = _create(trees[seed])
    if _no_gpu():
        assert rc == FMJ_ERR_NODEVICE, (seed, rc, msg)
    else:
        assert rc == 0, (seed, rc, msg)
