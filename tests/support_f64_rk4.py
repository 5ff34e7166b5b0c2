"""What the tests of RK4 on the fp64 step kernel share (test_f64_rk4_interface.py, test_gpu_f64_rk4.py): models that integrate with RK4,
contexts made with fp64_rk4=True, and the oracle's read-outs of a step's first pass and of its stage states.  torch and the GPU test
modules are imported inside the functions, so importing this module needs no GPU."""
import numpy as np

from support_sims import f64 as _f64, load_batch

RK4 = 1      # FMJ_CREATE_F64_RK4 is 8; FMJ_INT_RK4 is 1
CREATE_F64_LIMITS, CREATE_F64_RK4 = 1, 8
FIELDS = ('qpos', 'qvel', 'qacc', 'xpos', 'xquat', 'xipos', 'sensordata')


def rk4_model(name):
    """A model of test_gpu_f64_step.MODELS, unconstrained, integrating with RK4."""
    import support_f64_step as S
    m = S._make(name)
    m.integrator = RK4
    return m


def rk4_limited(name, *args, **kw):
    """support_limits.limited(name, ...) integrating with RK4."""
    from support_limits import limited
    m = limited(name, *args, **kw)
    m.integrator = RK4
    return m


def as_euler(m):
    """The same model object's Euler twin (a shallow copy with the integrator changed)."""
    import copy
    e = copy.copy(m)
    e.integrator = 0
    return e


def phys(m, n, qpos, qvel, ctrl=None, xf=None, qs=None, limits=False, rk4=True):
    """BatchedPhysics(precision='fp64', fp64_rk4=rk4, fp64_limits=limits) with the inputs stored in fp32; returns it and the inputs as
    the device holds them, in fp64."""
    import torch
    from farms_mujoco_amd.physics import BatchedPhysics
    p = BatchedPhysics(m, n, precision='fp64', fp64_limits=limits, fp64_rk4=rk4)
    assert p.precision == 'fp64' and p.kernel_info()['threads_per_env'] == 128 and 0 < p.kernel_info()['lds_bytes_per_env'] <= 160*1024
    d = p.data
    f32 = lambda a: torch.as_tensor(np.asarray(a), dtype=torch.float32)
    d.qpos[:] = f32(qpos); d.qvel[:] = f32(qvel)
    if xf is not None:
        d.xfrc_applied[:] = f32(xf)
    if qs is not None:
        d.qpos_spring[:] = f32(qs)
    if ctrl is not None and m.nu:
        d.ctrl[:] = f32(ctrl)
    return p, dict(qpos=_f64(d.qpos), qvel=_f64(d.qvel), ctrl=_f64(d.ctrl) if m.nu else None, xfrc_applied=_f64(d.xfrc_applied),
                   qpos_spring=_f64(d.qpos_spring))


def oracle_kw(ins):
    return dict(ctrl=ins['ctrl'], qpos_spring=ins['qpos_spring'], xfrc_applied=ins['xfrc_applied'])


def first_pass(oracle, m, ins):
    """The oracle's forward pass at the inputs, per env: what fmj_forward leaves on an RK4 context (no implicit damping: qacc is the
    constrained M^-1 (...)), and the poses a step's first pass sees."""
    n = len(ins['qpos'])
    fds = [oracle.forward_debug(m, ins['qpos'][e], ins['qvel'][e], ctrl=ins['ctrl'][e] if m.nu else None, qpos_spring=ins['qpos_spring'][e],
                                xfrc_applied=ins['xfrc_applied'][e]) for e in range(n)]
    out = {k: np.array([fd[k] for fd in fds]) for k in ('qacc', 'xpos', 'xquat', 'xipos', 'sensordata')}
    return dict(out, qpos=ins['qpos'], qvel=ins['qvel'])


def integrate_pos(m, q0, vel, h):
    """mj_integratePos (oracle integrate_pos) for one env, in numpy."""
    q = np.array(q0, float)
    for j in range(m.njnt):
        qa, da = int(m.jnt_qposadr[j]), int(m.jnt_dofadr[j])
        if m.jnt_type[j] == 0:
            q[qa:qa + 3] += h*vel[da:da + 3]
            w = np.array(vel[da + 3:da + 6], float)
            nrm = np.sqrt(w @ w)
            ax = w/nrm if nrm >= 1e-15 else np.array([1.0, 0.0, 0.0])
            ang = h*nrm if nrm >= 1e-15 else 0.0
            qr = np.concatenate([[np.cos(ang/2)], np.sin(ang/2)*ax])
            a = q[qa + 3:qa + 7]/np.linalg.norm(q[qa + 3:qa + 7])
            q[qa + 3:qa + 7] = [a[0]*qr[0] - a[1:] @ qr[1:], *(a[0]*qr[1:] + qr[0]*a[1:] + np.cross(a[1:], qr[1:]))]
        else:
            q[qa] += h*vel[da]
    return q


def second_stage(oracle, m, ins, e):
    """X[1] of env e's step, built on the host from the oracle's first pass: q0 (+) h/2 v0, v0 + h/2 qacc."""
    fd = oracle.forward_debug(m, ins['qpos'][e], ins['qvel'][e], ctrl=ins['ctrl'][e] if m.nu else None, qpos_spring=ins['qpos_spring'][e],
                              xfrc_applied=ins['xfrc_applied'][e])
    h = m.timestep
    return fd, integrate_pos(m, ins['qpos'][e], ins['qvel'][e], 0.5*h), ins['qvel'][e] + 0.5*h*fd['qacc']


def rk4_swim_sim(n_envs, n_iterations, m, seed=9, controller_of=None, water_kwargs=None, **sim_kw):
    """support_sims.swim_sim for a model that integrates with RK4: SimulationOptions(integrator='RK4'), fp64_rk4=True."""
    from farms_mujoco_amd.model import synthetic_batch
    from farms_mujoco_amd.options import SimulationOptions, ArenaOptions, AnimatOptions, WaterOptions
    from farms_mujoco_amd.control import WaveController
    from farms_mujoco_amd.simulation.simulation import Simulation
    assert m.integrator == RK4
    qpos, qvel, psi = synthetic_batch(m, n_envs, seed=seed)
    opts = SimulationOptions(timestep=1e-3, n_iterations=n_iterations, integrator='RK4')
    arena = ArenaOptions(water=WaterOptions(**(water_kwargs or {})))
    sim = Simulation.from_sdf(opts, AnimatOptions.from_model(m), arena, model=m, n_envs=n_envs, controller=(controller_of or WaveController)(m, psi),
                              buffer_size=n_iterations, precision='fp64', fp64_rk4=True, **sim_kw)
    load_batch(sim, qpos, qvel)
    return sim
