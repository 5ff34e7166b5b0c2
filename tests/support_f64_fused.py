"""Swimming simulations on an fp64 context that fuses, their oracle references and the checks of a run, shared by the GPU tests of
fmj_step_fused_f64 (test_gpu_f64_fused.py and the fused cases of the limits, RK4 and wide-CPG tests).  torch is imported inside the
functions, so importing this module needs no GPU."""
import numpy as np

from parity_metrics import relerr, link_row_groups
from support_sims import f64 as _f64, swim_sim, wave_at, swim_water, rows as _rows
from support_f64_step import ulp_excess

FMJ_WARN_BADQPOS = 1


CURRENT = [0.03, 0.0, -0.01]


# the surface per model, so that over the run some link is above it and some link partly submerged (checked in the test from the
# reference's rows): the salamander's limbs hang below its trunk; the eel lies flat at z = -0.1 and falls through a surface 4 mm
# below it; the centipede's legs straddle z = -0.1
SURFACE = {'salamander33': -0.11, 'eel48': -0.104, 'centipede_20_25': -0.1, 'eel20': -0.095}      # (eel20: every link partly submerged)


STATE = ('qpos', 'qvel', 'xpos', 'xquat', 'xipos', 'sensordata')


RING = ('links', 'joints', 'xfrc')


def _model(name, substeps=1):
    import farms_mujoco_amd.model as mm
    h = 1e-3/substeps
    return {'salamander33': lambda: mm.salamander33(timestep=h), 'eel20': lambda: mm.eel(n_joints=20, timestep=h),
            'eel48': lambda: mm.eel(n_joints=48, timestep=h), 'centipede_20_25': lambda: mm.centipede(20, 25, timestep=h)}[name]()


def _scaled_units():
    """Units of which none is 1, a power of two or exact in fp32: fmj_units then holds rounded values, the reciprocal of each differs
    between fp32 and double, and no two of velocity (0.54), angular_velocity (0.77), newtons (0.79) and torques (0.55) can be swapped."""
    from farms_mujoco_amd.units import SimulationUnitScaling
    return SimulationUnitScaling(meters=0.7, seconds=1.3, kilograms=1.9)


def _sim(name, n, T, ring=None, substeps=1, surface=None, units=None, **kw):
    """``units``: a SimulationUnitScaling; the rows are then in its units, and so is the surface (the model's height / meters)."""
    kw.setdefault('controller_of', wave_at(1.5))
    water = dict(height=(SURFACE.get(name, -0.11) if surface is None else surface)/(units.meters if units else 1.0), velocity=CURRENT)
    if units is not None:
        kw['units'] = units
    return swim_sim(n, T, ring, m=_model(name, substeps), seed=9, water_kwargs=water, substeps=substeps, precision='fp64', fp64_fused=True, **kw)[0]


def _f32(a):
    return np.asarray(a, np.float32).astype(np.float64)


def _oracle_args(sim, envs=slice(None)):
    """swim, water and wave of oracle.run_fused as the device holds them: fp32 values, widened."""
    swim, water, wave = swim_water(sim, wave=True, envs=envs)
    water = dict(water, surface=float(np.float32(water['surface'])), velocity=_f32(water['velocity']), viscosity=float(np.float32(water['viscosity'])),
                 gravity=float(np.float32(water['gravity'])))
    c = sim.task._controller
    freq = c.frequency[envs].cpu().numpy().astype(np.float64) if hasattr(c.frequency, 'cpu') else float(np.float32(c.frequency))
    wave = dict(amplitude=_f64(c.amplitude), phase_lag=_f64(c.phase_lag), env_phase=_f64(c.env_phase[envs]), frequency=freq)
    return swim, water, wave


def _units(sim):
    """``units`` of oracle.run_fused as fmj_units holds them: fp32 values, widened."""
    c = sim.task.units.as_c()
    return tuple(float(x) for x in (c.meters, c.newtons, c.torques, c.velocity, c.angular_velocity))


def _device_state(sim, envs=slice(None)):
    """The state a launch starts from as the device holds it: qpos, qvel and the poses and sensors of the last forward pass, fp32, widened."""
    return {k: _f64(getattr(sim.physics.data, k)[envs]) for k in STATE}


def _floor_state(oracle, m, st, T, **kw):
    """The run as T launches of one iteration, the state rounded to fp32 between them; the ring rows of every launch gathered."""
    ring = None
    for k in range(T):
        o = oracle.run_fused(m, st, 1, iteration0=k, buffer_size=T, **kw)
        if ring is None:
            ring = {r: np.zeros_like(o[r]) for r in RING}
        for r in RING:
            ring[r][k % T] = o[r][k % T]
        st = {s: _f32(o[s]) for s in STATE}
    return dict(st, **ring)


def _references(oracle, sim, m, T, substeps=1, substep_links=False, n_iterations=0):
    swim, water, wave = _oracle_args(sim)
    st = _device_state(sim)
    kw = dict(swim=swim, water=water, controller=1, wave=wave, n_threads=8, substeps=substeps, substep_links=substep_links, n_iterations=n_iterations,
              units=_units(sim))
    ref = oracle.run_fused(m, st, T, buffer_size=T, **kw)
    with oracle.fp32_storage():
        fst = oracle.run_fused(m, st, T, buffer_size=T, **kw)
    return ref, _floor_state(oracle, m, st, T, **kw), fst


def _row_groups(kind, n_rows):
    """Columns of one physical kind over all rows of a ring row [n_envs, n_rows, width], flattened per env."""
    width, kinds = {'links': (20, link_row_groups()), 'joints': (12, [slice(0, 1), slice(1, 2), slice(2, 8), slice(8, 9), slice(9, 12)]),
                    'xfrc': (6, [slice(0, 3), slice(3, 6)])}[kind]
    cols = np.arange(n_rows*width).reshape(n_rows, width)
    return [cols[:, k].ravel() for k in kinds]


def _got(sim):
    import torch
    torch.cuda.synchronize()
    d = sim.physics.data
    return dict({k: getattr(d, k).cpu().numpy() for k in STATE + ('ctrl', 'status')}, **_rows(sim))


def _check_one_pass_rows(got, ref, its, what):
    for it in its:
        for r in RING:
            ex = ulp_excess(got[r][it], ref[r][it], _row_groups(r, ref[r].shape[2]))
            print(what, 'row', it, r, 'error / one-step bound', round(ex, 3))
            assert ex <= 1.0, (what, it, r, ex)


def _check_run(got, ref, floor, fst, what):
    err = {k: relerr(got[k], ref[k]) for k in ('qpos', 'qvel') + RING}
    fl = {k: relerr(floor[k], ref[k]) for k in err}
    fs = {k: relerr(fst[k], ref[k]) for k in err}
    for k in err:
        print(what, k, 'kernel %.3g  floor_state %.3g  fp32_storage %.3g' % (err[k], fl[k], fs[k]))
    for k in err:
        assert err[k] <= fl[k], (what, k, err[k], fl[k])
    for k in ('links', 'xfrc'):
        assert err[k] <= fs[k]/10, (what, k, err[k], fs[k])
    return err
