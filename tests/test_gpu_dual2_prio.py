"""Issue priority in the two-env step kernel (csrc/fmj_dual2.inc, FMJ_DUAL_PRIO_POLICY): fused launches let the waves that share a SIMD
take turns at s_setprio 1.  That changes which wave wins arbitration and nothing a wave computes, so a run with it must agree BITWISE
with a run of a context created under FMJ_DUAL_PRIO=0, in every register tier and on the per-iteration host path.
Only the builds of the WPS = 2 and 3 tiers carry the policy (FMJ_DUAL_PRIO_MAX_WPS): kernel_info() reports it there and False in the other
tier, whose cases check the plumbing only - the switch must change nothing where there is nothing to switch."""
import pytest

from support_sims import swim_sim, outputs, assert_bitwise

pytestmark = pytest.mark.gpu

N, T, RING = 7, 120, 40      # odd batch: the last wave has an idle half; more steps than ring rows: the ring wraps
PRIO_TIERS = ('2', '3')      # register tiers whose builds carry the policy: FMJ_WPS <= FMJ_DUAL_PRIO_MAX_WPS of csrc/fmj_dual2.inc (keep in step)
FIELDS = ('qpos', 'qvel', 'sensordata', 'xpos', 'xquat')      # outputs() adds the three rings (links, joints, xfrc)


def _run(monkeypatch, fused=True, **env):
    """The workload under the FMJ_* switches of ``env`` (read at fmj_create): its outputs and the context's kernel_info after the run."""
    for k in ('FMJ_WPS', 'FMJ_DUAL_LEAN', 'FMJ_DUAL_PRIO'):
        monkeypatch.delenv(k, raising=False)
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    sim = swim_sim(N, T, RING, water_kwargs=dict(height=-0.11, velocity=[0.03, 0.0, -0.01]))[0]      # the surface cuts the animal, a current
    if fused:
        sim.run(fused=True)
    else:
        for _ in range(T):      # one-step launches (rows_ahead): the generic build, whose every launch sets the priority at its step 0
            sim._env_step()
        sim.physics.check_invalid_state()
    out = outputs(sim, FIELDS)
    assert {'links', 'joints', 'xfrc'} <= set(out)
    assert int(sim.physics.data.status.abs().sum()) == 0
    return out, sim.physics.kernel_info()


@pytest.mark.parametrize('wps', ['2', '3', '4'])
def test_priority_policy_is_bitwise_the_plain_run(wps, monkeypatch):
    on, info = _run(monkeypatch, FMJ_WPS=wps)
    assert info['threads_per_env'] == 32 and info['dual_wps'] == int(wps)
    assert info['dual_prio'] is (wps in PRIO_TIERS) and info['dual_last_launch'] == 'lean', info          # the default, on the kernel of the headline
    off, oinfo = _run(monkeypatch, FMJ_WPS=wps, FMJ_DUAL_PRIO='0')
    assert oinfo['dual_prio'] is False and oinfo['dual_last_launch'] == 'lean', oinfo
    assert oinfo['dual_wps'] == int(wps) and oinfo['dual_build'] == info['dual_build'] == 'lean'      # the switch moved nothing else
    assert_bitwise(on, off, f'WPS={wps} priority on vs FMJ_DUAL_PRIO=0')


@pytest.mark.parametrize('wps', ['2', '3', '4'])
def test_priority_policy_in_the_generic_build(wps, monkeypatch):
    on, info = _run(monkeypatch, FMJ_WPS=wps, FMJ_DUAL_LEAN='0')
    assert info['dual_prio'] is (wps in PRIO_TIERS) and info['dual_last_launch'] == 'generic', info
    off, oinfo = _run(monkeypatch, FMJ_WPS=wps, FMJ_DUAL_LEAN='0', FMJ_DUAL_PRIO='0')
    assert oinfo['dual_prio'] is False and oinfo['dual_last_launch'] == 'generic', oinfo
    assert_bitwise(on, off, f'WPS={wps} generic build, priority on vs FMJ_DUAL_PRIO=0')


def test_host_path_is_bitwise_with_and_without_the_switch(monkeypatch):
    a, info = _run(monkeypatch, fused=False, FMJ_WPS='2')      # (seven envs would pick this tier anyway)
    assert info['dual_prio'] is True and info['dual_last_launch'] == 'generic', info
    b, oinfo = _run(monkeypatch, fused=False, FMJ_WPS='2', FMJ_DUAL_PRIO='0')
    assert oinfo['dual_prio'] is False and oinfo['dual_last_launch'] == 'generic', oinfo
    assert_bitwise(a, b, 'host path, priority on vs FMJ_DUAL_PRIO=0')
