"""Models, contexts and the ulp metric that the fp64 step's GPU tests share (test_gpu_f64_step.py and the tests of the kernel families
built on it).  torch is imported inside the functions, so importing this module needs no GPU."""
import numpy as np

from parity_metrics import qpos_groups, qvel_groups
from wide_trees import WIDE_SHAPES, shape_tree
from support_models import random_tree
from support_sims import f64 as _f64

MODELS = (['salamander33', 'eel20', 'eel48', 'eel58', 'centipede', 'centipede_20_25', 'centipede_12_50'] +
          [f'shape{s[0]}' for s in WIDE_SHAPES] + [f'tree{s}' for s in range(20)])


def _make(name, integrator='Euler'):
    import farms_mujoco_amd.model as mm
    if name.startswith('shape'):
        m = shape_tree(int(name[5:]))
    elif name.startswith('tree'):
        m = random_tree(int(name[4:]))
    else:
        m = {'salamander33': mm.salamander33, 'eel20': lambda: mm.eel(n_joints=20), 'eel48': lambda: mm.eel(n_joints=48),
             'eel58': lambda: mm.eel(n_joints=58), 'centipede': mm.centipede, 'centipede_20_25': lambda: mm.centipede(20, 25),
             'centipede_12_50': lambda: mm.centipede(12, 50)}[name]()
    m.integrator = mm.INTEGRATORS['implicitfast' if integrator == 'implicitfast' else 'euler']
    return m


def _phys(m, n, qpos, qvel, ctrl=None, xf=None, qs=None, precision='fp64'):
    """BatchedPhysics with the inputs stored in fp32; returns it and the inputs as the device holds them, in fp64."""
    import torch
    from farms_mujoco_amd.physics import BatchedPhysics
    phys = BatchedPhysics(m, n, precision=precision)
    assert phys.precision == precision
    d = phys.data
    f32 = lambda a: torch.as_tensor(np.asarray(a), dtype=torch.float32)
    d.qpos[:] = f32(qpos); d.qvel[:] = f32(qvel)
    if xf is not None:
        d.xfrc_applied[:] = f32(xf)
    if qs is not None:
        d.qpos_spring[:] = f32(qs)
    if ctrl is not None and m.nu:
        d.ctrl[:] = f32(ctrl)
    return phys, dict(qpos=_f64(d.qpos), qvel=_f64(d.qvel), ctrl=_f64(d.ctrl) if m.nu else None, xfrc_applied=_f64(d.xfrc_applied),
                      qpos_spring=_f64(d.qpos_spring))


def _ulp32(x):
    return np.spacing(np.abs(np.asarray(x, np.float64)).astype(np.float32)).astype(np.float64)


def _sensor_groups(m):
    """Columns of one physical kind: link linear velocities, link angular velocities, joint positions, joint velocities, joint limit
    forces, actuator forces (the sensordata layout of include/fmj.h)."""
    nl, njs = 6*(m.nbody - 1), m.n_sensor_joints
    lin = np.array([6*b + k for b in range(m.nbody - 1) for k in range(3)], int)
    return [lin, lin + 3, nl + 3*np.arange(njs), nl + 3*np.arange(njs) + 1, nl + 3*np.arange(njs) + 2, np.arange(nl + 3*njs, nl + 3*njs + m.nu)]


def ulp_excess(got, ref, groups=None):
    """Worst |got - ref| / (ulp32(ref_i) + ulp32(max |ref| of the component's group in its env)); got, ref: [n_envs, ...]."""
    got = np.asarray(got, np.float64).reshape(len(ref), -1); ref = np.asarray(ref, np.float64).reshape(len(ref), -1)
    worst = 0.0
    for g in (groups if groups is not None else [slice(None)]):
        r = ref[:, g]
        if r.size == 0:
            continue
        bound = _ulp32(r) + _ulp32(np.abs(r).max(axis=1, keepdims=True))
        worst = max(worst, float((np.abs(got[:, g] - r)/bound).max()))
    return worst


def _field_groups(m):
    return dict(qpos=qpos_groups(m), qvel=qvel_groups(m), qacc=qvel_groups(m), xpos=None, xquat=None, xipos=None, sensordata=_sensor_groups(m))
