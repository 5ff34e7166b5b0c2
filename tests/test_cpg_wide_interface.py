"""Oscillator networks of up to FMJ_CPG_MAX_OSC = 256 oscillators as far as they can be checked without a GPU: the limit through the
C ABI (decided before any device call), its Python mirror, the numpy checker of the GPU tests pinned to the oracle where the oracle
works (n_osc <= 64), and the network builder for bodies with any number of limbs (axial_limb_network)."""
import ctypes
import os
import re

import numpy as np
import pytest

from support_capi import lib as _lib, FMJ_ERR_ARG
from support_cpg import cpg_reference, ring_network, wrapped

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FMJ_OK, FMJ_ERR_HIP = 0, 3      # include/fmj.h


def _create(n_osc):
    """fmj_cpg_create of a ring of ``n_osc`` oscillators (and destroy): the return code and the library's message."""
    L, so = _lib()
    net = ring_network(max(n_osc, 1), 3)
    d = net.as_c(L.CCpgDesc)
    d.n_osc = n_osc
    ctx = ctypes.c_void_p()
    rc = so.fmj_cpg_create(ctypes.byref(d), 0, ctypes.byref(ctx))
    if rc == FMJ_OK:
        so.fmj_cpg_destroy(ctx)
    return rc, so.fmj_last_error().decode()


@pytest.mark.parametrize('n_osc', [65, 96, 256])
def test_create_accepts_more_than_one_wave(n_osc):
    rc, msg = _create(n_osc)
    assert rc in (FMJ_OK, FMJ_ERR_HIP), (rc, msg)      # FMJ_ERR_HIP: no device here; the size itself was accepted


@pytest.mark.parametrize('n_osc', [0, 257])
def test_create_refuses_past_the_limit_before_any_device_call(n_osc):
    rc, msg = _create(n_osc)
    assert rc == FMJ_ERR_ARG and '256' in msg, (rc, msg)


def test_python_mirrors_the_header_limit_and_the_abi_version_stays():
    from farms_mujoco_amd import _lib as L
    hdr = open(os.path.join(ROOT, 'include', 'fmj.h')).read()
    assert int(re.search(r'^#define FMJ_CPG_MAX_OSC (\d+)$', hdr, re.M).group(1)) == L.CPG_MAX_OSC == 256
    assert '#define FMJ_ABI_VERSION 6' in hdr and L.ABI_VERSION == 6


def test_reference_agrees_with_the_oracle_where_the_oracle_works(oracle):
    from farms_mujoco_amd.model import salamander33
    from farms_mujoco_amd.control import salamander_network
    m = salamander33()
    net = salamander_network(m)
    n, T = 4, 500
    rng = np.random.default_rng(3)
    ph0 = wrapped(net.initial_phase[None, :] + rng.uniform(-1.0, 1.0, (n, net.n_osc)))
    a0 = rng.uniform(0.0, 0.2, (n, net.n_osc)); d0 = rng.uniform(-0.1, 0.1, (n, net.n_osc))
    drive = (1.0 + 0.1*np.arange(n)/n).astype(np.float32)
    want = oracle.cpg_tape(net, T, m.timestep, ph0, a0, d0, drive=drive)
    got = cpg_reference(net, T, m.timestep, ph0, a0, d0, drive=drive)
    assert np.abs(want[0]).max() > 0.1
    for name, g, w in zip(('tape', 'phase', 'amp', 'damp'), got, want):
        err = np.abs(wrapped(g - w) if name == 'phase' else g - w).max()
        print(name, 'cpg_reference - oracle:', err)
        assert err < 1e-9, (name, err)


def _models():
    import farms_mujoco_amd.model as mm
    return {'centipede': (mm.centipede, 70), 'centipede_20_25': (lambda: mm.centipede(20, 25), 130), 'eel48': (lambda: mm.eel(48), 96)}


@pytest.mark.parametrize('name', ['centipede', 'centipede_20_25', 'eel48'])
def test_builder_sizes(name):
    from farms_mujoco_amd import _lib as L
    from farms_mujoco_amd.control import axial_limb_network
    make, n_osc = _models()[name]
    m = make()
    net = axial_limb_network(m)
    assert net.n_osc == n_osc <= L.CPG_MAX_OSC and net.nu == m.nu
    assert net.conn_to.max() < n_osc and net.conn_from.max() < n_osc and net.initial_phase.shape == (n_osc,)


def test_builder_on_the_salamander_differs_only_in_the_hind_girdle():
    """The same chain, pairs and outputs as salamander_network; the hind limbs hang on the joint of the segment that carries them
    (body_5: axial joint 4), where salamander_network takes the mid-body joint."""
    from farms_mujoco_amd.model import salamander33
    from farms_mujoco_amd.control import axial_limb_network, salamander_network
    m = salamander33()
    a, s = axial_limb_network(m), salamander_network(m)
    for k in ('frequency', 'rate', 'amplitude', 'conn_to', 'conn_weight', 'conn_bias', 'out_a', 'out_b', 'out_gain', 'out_offset'):
        assert np.array_equal(getattr(a, k), getattr(s, k)), k
    moved = np.nonzero(a.conn_from != s.conn_from)[0]
    assert len(moved) == 2 and sorted(a.conn_from[moved]) == [8, 9] and sorted(s.conn_from[moved]) == [10, 11]


@pytest.mark.parametrize('name', ['centipede', 'centipede_20_25'])
def test_builder_gait(name):
    """From a perturbed initial_phase the network locks into the travelling wave, every limb in antiphase to the axial oscillator of
    its own segment, on its own side."""
    from farms_mujoco_amd.control import axial_limb_network
    m = _models()[name][0]()
    net = axial_limb_network(m)
    axial = [j for j, n in enumerate(m.joint_names) if n.startswith('joint_body_')]
    na = len(axial)
    rng = np.random.default_rng(0)
    ph0 = net.initial_phase[None, :] + rng.uniform(-0.3, 0.3, (1, net.n_osc))
    tape, ph, amp, _ = cpg_reference(net, 8000, 1e-3, ph0, np.zeros((1, net.n_osc)), np.zeros((1, net.n_osc)))
    left = ph[0, 0:2*na:2]
    lag = wrapped(left[:-1] - left[1:])
    print(name, 'axial lag error', np.abs(lag - 2*np.pi/na).max())
    assert np.allclose(lag, 2*np.pi/na, atol=0.05), lag
    # the segment of every limb, from the model's tree and not from the builder
    names = list(m.joint_names)
    limbs = sorted({n.rsplit('_', 1)[0] for n in names if n.startswith('joint_leg_')})
    assert len(limbs) == (net.n_osc - 2*na)//2 > 4
    worst, used = 0.0, set()
    for li, limb in enumerate(limbs):
        segment = m.body_names[m.body_parentid[m.jnt_bodyid[names.index(limb + '_0')]]]
        k = 0 if segment == 'body_0' else axial.index(names.index('joint_' + segment))      # the root segment: the first axial joint
        side = {'L': 0, 'R': 1}[limb[-1]]
        used.add(k)
        worst = max(worst, abs(wrapped(ph[0, 2*na + 2*li] - ph[0, 2*k + side] - np.pi)))
    print(name, 'limb antiphase error', worst)
    assert worst < 0.05 and len(used) >= len(limbs)//2 - 1      # the limbs are spread over the segments, not hung on one
    pos = [a for a in range(m.nu) if m.actuator_tags[a] == 'position' and m.joint_names[m.actuator_jntid[a]].startswith('joint_body_')]
    swing = tape[-1000:, 0, pos].max(0) - tape[-1000:, 0, pos].min(0)
    print(name, 'axial swing', swing.min(), swing.max())
    assert np.all(swing > 0.5) and np.all(swing < 0.7)                 # 2 * 2 * 0.15 = 0.6 rad peak to peak
