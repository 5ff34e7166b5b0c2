"""The lean build of the two-env step kernel (csrc/fmj_dual2.inc, LEAN): a fused launch of the flagship shape runs an instantiation
with its launch options folded in at compile time.  It removes tests, not arithmetic, so it must agree BITWISE with the generic
build (FMJ_DUAL_LEAN=0) in every register tier, and a launch shape it does not cover must still run the generic build."""
import numpy as np
import pytest

from support_sims import swim_sim, outputs, assert_bitwise as _assert_bitwise

pytestmark = pytest.mark.gpu

N, T, RING = 7, 120, 40      # odd batch: the last wave has an idle half; more steps than ring rows: the ring wraps


def _run(monkeypatch, fused=True, **env):
    """The workload under the FMJ_* switches of ``env`` (read at fmj_create); returns its outputs and the context's kernel_info
    after the run, and - for the per-iteration host path - the build every single launch ran."""
    for k in ('FMJ_WPS', 'FMJ_DUAL_LEAN'):
        monkeypatch.delenv(k, raising=False)
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    sim = swim_sim(N, T, RING, water_kwargs=dict(height=-0.11, velocity=[0.03, 0.0, -0.01]))[0]      # the surface cuts the animal, a current
    launches = set()
    if fused:
        sim.run(fused=True)
    else:
        for _ in range(T):
            sim._env_step()
            launches.add(sim.physics.kernel_info()['dual_last_launch'])
        sim.physics.check_invalid_state()
    out = outputs(sim, ('qpos', 'qvel', 'sensordata', 'xpos', 'xquat'))
    assert int(sim.physics.data.status.abs().sum()) == 0
    return out, sim.physics.kernel_info(), launches


@pytest.mark.parametrize('wps', ['2', '3', '4'])
def test_lean_build_is_bitwise_the_generic_build(wps, monkeypatch):
    lean, info, _ = _run(monkeypatch, FMJ_WPS=wps)
    assert info['threads_per_env'] == 32 and info['dual_wps'] == int(wps)
    assert info['dual_build'] == 'lean' and info['dual_last_launch'] == 'lean', info      # the default, and the fused run really took it
    generic, ginfo, _ = _run(monkeypatch, FMJ_WPS=wps, FMJ_DUAL_LEAN='0')
    assert ginfo['dual_build'] == 'generic' and ginfo['dual_last_launch'] == 'generic', ginfo
    _assert_bitwise(lean, generic, f'WPS={wps} lean vs generic')


def test_launch_shape_the_lean_build_refuses_runs_the_generic_build(monkeypatch):
    """The per-iteration host path: one-step launches with rows_ahead (and a last one without readout), none of which the lean
    build covers.  A context with the lean build enabled runs the generic build for every one of them, to the same bits as a
    context that has it turned off."""
    a, info, launches = _run(monkeypatch, fused=False)
    assert info['dual_build'] == 'lean' and launches == {'generic'}, (info, launches)
    b, ginfo, glaunches = _run(monkeypatch, fused=False, FMJ_DUAL_LEAN='0')
    assert ginfo['dual_build'] == 'generic' and glaunches == {'generic'}, (ginfo, glaunches)
    _assert_bitwise(a, b, 'host path, lean enabled vs forced generic')


def test_register_tiers_agree_bitwise(monkeypatch):
    """The three register tiers compute the same bits on the fused workload (the property the per-tier instruction orders - resident
    constants, the order of independent chains - have to keep)."""
    w2, i2, _ = _run(monkeypatch, FMJ_WPS='2')
    w4, i4, _ = _run(monkeypatch, FMJ_WPS='4')
    assert i2['dual_wps'] == 2 and i4['dual_wps'] == 4
    _assert_bitwise(w2, w4, 'WPS=2 vs WPS=4')
    w3, _, _ = _run(monkeypatch, FMJ_WPS='3')
    _assert_bitwise(w3, w4, 'WPS=3 vs WPS=4')
