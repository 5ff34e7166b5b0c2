"""Config 4 (walking, limits + contacts, PGS) step by step: is the looser rollout parity of walking a real per-step error or
the amplification of fp32 rounding by the dynamics?

A teacher trajectory (the fp64 oracle, 1000 steps of the trot) is followed; at EVERY step the teacher's state - qpos, qvel and
the solver's warm start qacc - is rounded to fp32 and handed to the HIP path, both step once from that identical rounded state
(the oracle in fp64), and everything the step produces is compared: contact list, constraint rows, constraint forces, new
velocity.  Errors cannot accumulate, so what is measured is the per-step error of the HIP step, contact solve included.
Steps whose active sets differ (an fp32 `dist < 0` or `dist < margin` flip of a grazing contact / limit) are counted and
reported, and must be rare; on every other step the per-step bounds hold.

The same run checks oracle-independent properties of the HIP solve: f >= 0, the dual cost does not increase in any sweep, and
- with A, b of the SAME rounded state in fp64 - the residual A f + b, complementarity and the dual cost of the HIP forces are
as good as those of the fp64 PGS after the same 50 sweeps, and bracketed by the exact minimum (Newton)."""
import copy

import numpy as np
import pytest

from parity_metrics import group_relerr, qvel_groups
from support_models import walker as _walker, trot_tape as _trot_tape

pytestmark = pytest.mark.gpu


def test_teacher_forced_walk_per_step_parity_and_kkt(oracle):
    import torch
    from farms_mujoco_amd.physics import BatchedPhysics
    from farms_mujoco_amd.model import SOLVERS
    m = _walker()
    n, T = 8, 1000
    tape = _trot_tape(m, n, T)
    m_newton = copy.copy(m); m_newton.solver = SOLVERS['newton']; m_newton.solver_iterations = 100; m_newton.solver_tolerance = 1e-12
    phys = BatchedPhysics(m, n)
    d = phys.data
    f32 = lambda a: torch.as_tensor(np.asarray(a), dtype=torch.float32, device=d.qpos.device)
    r64 = lambda t: t.cpu().numpy().astype(np.float64)
    q = np.tile(m.qpos0, (n, 1)); v = np.zeros((n, m.nv)); w = np.zeros((n, m.nv))
    groups = qvel_groups(m)
    stat = dict(flips=0, steps=0, qvel=[], qvel_floor=[], force_floor=[], force=[], b=[], R=[], kkt_hip=[], kkt_ref=[], dcost=[], gap_hip=[], gap_ref=[], imp_min=[],
                ncon=[], sweeps=[], pos=[])
    for t in range(T):
        d.qpos[:] = f32(q); d.qvel[:] = f32(v); d.qacc_warmstart[:] = f32(w); d.ctrl[:] = f32(tape[t])
        q32, v32, w32, c32 = r64(d.qpos), r64(d.qvel), r64(d.qacc_warmstart), r64(d.ctrl)
        rows, imp = phys.step_debug()
        torch.cuda.synchronize()
        o = oracle.step_tf(m, q32, v32, ctrl=c32, warmstart=w32)               # the probe: fp64 step from the same rounded state
        with oracle.fp32_storage():                                           # the floor: the same step with M / H stored in fp32, nothing else
            fl = oracle.step_tf(m, q32, v32, ctrl=c32, warmstart=w32, want_AR=False)
        rows = r64(rows); imp = r64(imp)
        ncon_h = d.ncon.cpu().numpy(); con_h = oracle.contacts_from_hip(d.contact.cpu().numpy())
        qv_h = r64(d.qvel)
        assert int(d.status.abs().sum()) == 0 and int(o['status'].sum()) == 0
        for e in range(n):
            stat['steps'] += 1
            ne = int(o['nefc'][e]); nc = int(o['ncon'][e])
            kinds_h = rows[e, :, 6].astype(np.float32).view(np.int32)
            nlim = ne - 4*nc
            same = ncon_h[e] == nc and np.array_equal(con_h[e, :nc, 16], o['contact'][e, :nc, 16])
            # limit rows: the HIP rows before the first contact row must be the oracle's limit rows (same joints)
            if same and nlim:
                same = bool(np.all((kinds_h[:nlim] & 0x40000000) == 0)) and (ne == nlim or bool(kinds_h[nlim] & 0x40000000))
            if same and ne > nlim:
                same = bool(np.all(kinds_h[nlim:ne] & 0x40000000))
            if not same:
                stat['flips'] += 1
                continue
            stat['ncon'].append(nc)
            stat['qvel'].append(group_relerr(qv_h[e], o['qvel'][e], groups))
            stat['qvel_floor'].append(group_relerr(fl['qvel'][e], o['qvel'][e], groups))
            if ne == 0:
                continue
            f_h = rows[e, :ne, 4]; f_o = o['efc'][e, :ne, 0]; b = o['efc'][e, :ne, 1]; AR = o['AR'][e, :ne, :ne]
            fs = max(np.abs(f_o).max(), 1e-2)
            stat['force'].append(np.abs(f_h - f_o).max()/fs)
            stat['force_floor'].append(np.abs(fl['efc'][e, :ne, 0] - f_o).max()/fs if fl['nefc'][e] == ne else 0.0)
            stat['b'].append(np.abs(rows[e, :ne, 3] - b).max()/max(np.abs(b).max(), 1.0))
            stat['R'].append(np.abs(rows[e, :ne, 2]/o['efc'][e, :ne, 2] - 1).max())
            stat['pos'].append(np.abs(con_h[e, :nc, :3] - o['contact'][e, :nc, :3]).max() if nc else 0.0)
            assert f_h.min() >= 0.0                                               # PGS clamps: exactly non-negative
            # residuals of the HIP forces and of the oracle's forces in the SAME fp64 problem
            bs = max(np.abs(b).max(), 1.0)
            for key, f in (('kkt_hip', f_h), ('kkt_ref', f_o)):
                r = AR @ f + b
                stat[key].append(max(-min(r.min(), 0.0)/bs, np.abs(f*r).max()/(fs*bs)))
            cost = lambda f: float(f @ (0.5*AR @ f + b))
            nw = oracle.step_tf(m_newton, q32[e:e+1], v32[e:e+1], ctrl=c32[e:e+1], warmstart=w32[e:e+1], want_AR=False)
            cmin = cost(nw['efc'][0, :ne, 0])
            stat['dcost'].append((cost(f_h) - cost(f_o))/max(abs(cmin), 1e-6))
            stat['gap_hip'].append((cost(f_h) - cmin)/max(abs(cmin), 1e-6)); stat['gap_ref'].append((cost(f_o) - cmin)/max(abs(cmin), 1e-6))
            ran = imp[e][~np.isnan(imp[e])]
            stat['sweeps'].append(len(ran))
            if len(ran):
                stat['imp_min'].append(ran.min()/max(abs(cmin), 1e-6))
        tch = oracle.step_tf(m, q, v, ctrl=tape[t], warmstart=w, want_AR=False)    # the teacher moves on, unrounded
        q, v, w = tch['qpos'], tch['qvel'], tch['warmstart']
    S = {k: np.asarray(x) for k, x in stat.items() if isinstance(x, list)}
    pct = lambda x, p: float(np.percentile(x, p)) if len(x) else 0.0
    print(f"teacher-forced walk: {stat['steps']} env-steps, active-set flips {stat['flips']}, contacts per step median {np.median(S['ncon'])} max {S['ncon'].max()}")
    for k in ('qvel', 'qvel_floor', 'force', 'force_floor', 'b', 'R', 'pos', 'kkt_hip', 'kkt_ref', 'gap_hip', 'gap_ref'):
        print(f"  {k:8s} median {pct(S[k], 50):.3e}  99% {pct(S[k], 99):.3e}  max {S[k].max():.3e}")
    print(f"  dcost (HIP - oracle, / |min|) min {S['dcost'].min():.3e} max {S['dcost'].max():.3e}; worst sweep improvement / |min| {S['imp_min'].min():.3e}; "
          f"sweeps median {np.median(S['sweeps'])}")
    # ---- the statement ----
    assert stat['flips'] <= 0.002*stat['steps']                                  # grazing contacts / limits: rare
    assert S['ncon'].max() >= 4 and np.median(S['ncon']) >= 2                    # the animal does stand on its feet
    # per-step velocity, per component: typically 6e-5; its tail is the (M + hB) solve of an ill-conditioned matrix and is held to
    # the floor that fp32 storage of that matrix alone sets on the same steps (oracle.fp32_storage), not to a fitted number
    assert np.median(S['qvel']) < 1e-4
    for p_ in (50, 99, 100):
        assert pct(S['qvel'], p_) < 6*pct(S['qvel_floor'], p_) + 1e-6, (p_, pct(S['qvel'], p_), pct(S['qvel_floor'], p_))
    assert S['force'].max() < 1e-3 and pct(S['force'], 99) < 3e-4                # constraint forces / largest force of the env
    assert S['b'].max() < 3e-4 and pct(S['b'], 99) < 3e-5 and S['R'].max() < 5e-5 and S['pos'].max() < 1e-6
    # oracle-independent: no sweep raises the dual cost (fp32 rounding of a ~0 improvement aside) ...
    assert S['imp_min'].min() > -1e-5
    # ... and in the fp64 problem of the same state the HIP forces are as feasible, as complementary and as cheap as the fp64
    # PGS after the same number of sweeps, both above the exact minimum
    assert S['kkt_hip'].max() < 2*S['kkt_ref'].max() + 1e-4
    assert S['gap_hip'].min() > -1e-6 and np.abs(S['dcost']).max() < 1e-4
