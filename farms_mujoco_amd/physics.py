"""Batched physics: the object behind ``Simulation.physics``.

Replaces ``dm_control.mjcf.Physics`` (reference farms_mujoco/simulation/simulation.py:53) for a
batch of independent environments.  ``physics.data.<field>`` are PyTorch tensors on the GPU, fp32,
batch-first (``[n_envs, ...]``); ``physics.model`` is the shared :class:`~farms_mujoco_amd.model.Model`.
All arithmetic happens in the HIP library (``_lib``); this file only owns memory and marshals pointers.
"""
from __future__ import annotations

import ctypes
from types import SimpleNamespace
from typing import Optional

import numpy as np
import torch

from . import _lib
from .model import Model, JNT_FREE
from .options import KernelOptions


class PhysicsError(RuntimeError):
    """Bad simulation state (dm_control.rl.control.PhysicsError role, reference simulation.py:13,157-161)."""


def _ptr(t: Optional[torch.Tensor]):
    return None if t is None else ctypes.c_void_p(t.data_ptr())


class _MjData(SimpleNamespace):
    """``physics.data``: rebinding a field (``data.qpos = tensor``) is seen by the cached pointer struct of the per-step host path;
    in-place writes (``data.qpos[:] = ...``) never move a tensor."""
    _cdata_cache = None

    def __setattr__(self, name, value):
        object.__setattr__(self, '_cdata_cache', None)
        object.__setattr__(self, name, value)


# The opt-in keywords of an fp64 context, in the order they are checked; mirrors f64_flags[] of csrc/fmj_hip.hip (include/fmj.h:
# fmj_create_ex2, fmj_step_fused_f64).  Per keyword: its CREATE_F64_* bit of fmj_create_ext.flags (0: no create flag), the other keywords
# it needs next to precision='fp64', what the ValueError says it needs, and the keywords it does not go with -> why.
#   fp64_fused     fused launches go through fmj_step_fused_f64: rows and drag in double, the state rounded to fp32 only where a
#                  launch ends, so results differ from the per-iteration fp64 path's
#   fp64_limits    joint limits, solved by the kernel's primal Newton solve: limited swimmers past the sizes of the fp32 constraint path
#   fp64_rk4       integrator = RK4, the four forward passes of a step inside the kernel, one launch for all steps of fmj_step; with
#                  fp64_fused such a run fuses too
#   fp64_contacts  ground contacts (sphere / capsule / box geoms against world planes, pyramidal cone) as more rows of the same Newton
#                  solve: walking models past the sizes of the fp32 constraint path; fmj_step only, no fused launch, RK4 only with
#                  fp64_contacts_rk4
#   fp64_terrain   the contacts context also takes the world's heightfield as ground and cylinder geoms on the animat: its own
#                  kernels, whose narrow phase carries a normal per contact; opt-in, also on flat ground
#   fp64_mesh      the contacts context also takes convex mesh geoms on the animat (what Simulation.from_sdf makes of every mesh
#                  collision): up to four contacts at a mesh's deepest vertices, on kernels of their own; a model without a mesh
#                  runs what it runs without the keyword
#   fp64_elliptic  the contacts context also takes a model whose cone is elliptic (three rows per contact, kernels of their own); a
#                  pyramidal model runs what it runs without the keyword.  The elliptic cone's regulariser does not depend on the
#                  friction, so a model with friction-0 feet (1e-5 after the clamp), which the pyramid refuses, is accepted
#   fp64_contacts_rk4  the contacts context also takes integrator = RK4 on a walking model: the four passes of a step, each with its own
#                  narrow phase and solve, inside kernels of their own (terrain text, also on planes); an Euler or implicitfast model
#                  runs what it runs without the keyword.  It is not fp64_rk4, which admits RK4 on a model without contacts and still
#                  does not go with fp64_contacts; RK4 with mesh geoms stays refused
_NEEDS_FP64 = "precision='fp64', not {precision!r}: "
_CONTACTS_EXCLUDE = {'fp64_fused': 'fused contact rows are not built for the fp64 step', 'fp64_rk4': 'the fp64 contact solve integrates with Euler or implicitfast'}
FP64_OPTIONS = {
    'fp64_fused': (0, (), _NEEDS_FP64 + 'an fp32 context fuses through fmj_step_fused', {}),
    'fp64_limits': (_lib.CREATE_F64_LIMITS, (), _NEEDS_FP64 + 'an fp32 context solves limits on its constraint path', {}),
    'fp64_rk4': (_lib.CREATE_F64_RK4, (), _NEEDS_FP64 + 'an fp32 context integrates RK4 with four launches per step', {}),
    'fp64_contacts': (_lib.CREATE_F64_CONTACTS, (), _NEEDS_FP64 + 'an fp32 context solves contacts on its constraint path',
                      _CONTACTS_EXCLUDE),
    'fp64_terrain': (_lib.CREATE_F64_TERRAIN, ('fp64_contacts',), "precision='fp64' and fp64_contacts=True (not precision={precision!r}, "
                     'fp64_contacts={fp64_contacts}): it widens the narrow phase of the fp64 contact solve', {}),
    'fp64_mesh': (_lib.CREATE_F64_MESH, ('fp64_contacts',), "precision='fp64' and fp64_contacts=True (not precision={precision!r}, "
                  'fp64_contacts={fp64_contacts}): it lets the fp64 contact solve take convex mesh geoms', _CONTACTS_EXCLUDE),
    'fp64_contacts_rk4': (_lib.CREATE_F64_CONTACTS_RK4, ('fp64_contacts',), "precision='fp64' and fp64_contacts=True (not precision={precision!r}, "
                          'fp64_contacts={fp64_contacts}): it lets the fp64 contact solve integrate with RK4', _CONTACTS_EXCLUDE),
    'fp64_elliptic': (_lib.CREATE_F64_ELLIPTIC, ('fp64_contacts',), "precision='fp64' and fp64_contacts=True (not precision={precision!r}, "
                      'fp64_contacts={fp64_contacts}): it lets the fp64 contact solve take the elliptic cone', _CONTACTS_EXCLUDE),
}


class BatchedPhysics:
    """Device-resident mjData for ``n_envs`` copies of one model + the HIP step context."""

    def __init__(self, model: Model, n_envs: int, device='cuda:0', precision: str = 'fp32', kernel=None, fp64_fused: bool = False,
                 fp64_limits: bool = False, fp64_rk4: bool = False, fp64_contacts: bool = False, fp64_terrain: bool = False,
                 fp64_elliptic: bool = False, fp64_mesh: bool = False, fp64_contacts_rk4: bool = False):
        # precision='fp64': the fp64 step kernel (fmj_create_ex, include/fmj.h) - unconstrained models, Euler / implicitfast; the
        # tensors of physics.data stay fp32.  kernel: a KernelOptions (options.py) states this context's kernel selection in full;
        # None leaves it to the library, which then also hears the FMJ_* variables (include/fmj.h, "Kernel selection").
        # fp64_*: the opt-in keywords of an fp64 context (FP64_OPTIONS above).
        if precision not in _lib.PRECISIONS:
            raise ValueError(f'precision must be one of {sorted(_lib.PRECISIONS)}, not {precision!r}')
        on = dict(fp64_fused=bool(fp64_fused), fp64_limits=bool(fp64_limits), fp64_rk4=bool(fp64_rk4), fp64_contacts=bool(fp64_contacts),
                  fp64_terrain=bool(fp64_terrain), fp64_elliptic=bool(fp64_elliptic), fp64_mesh=bool(fp64_mesh),
                  fp64_contacts_rk4=bool(fp64_contacts_rk4))
        ext_flags = 0
        for name, (flag, needs, needs_text, excludes) in FP64_OPTIONS.items():
            if on[name] and (precision != 'fp64' or not all(on[n] for n in needs)):
                raise ValueError(f'{name}=True needs ' + needs_text.format(precision=precision, **on))
            for other, reason in excludes.items():
                if on[name] and on[other]:
                    raise ValueError(f'{name}=True does not go with {other}=True: {reason}')
            ext_flags |= flag if on[name] else 0
        vars(self).update(on)      # self.fp64_fused, self.fp64_limits, ...
        if kernel is not None and not isinstance(kernel, KernelOptions):
            raise TypeError(f'kernel must be a KernelOptions or None, not {kernel!r}')
        if not torch.cuda.is_available():
            raise _lib.FmjError('BatchedPhysics needs a GPU (torch.cuda.is_available() is False); '
                                'there is no CPU fallback for the product path.')
        self.model = model
        self.n_envs = int(n_envs)
        self.device = torch.device(device)
        self._lib = _lib.load()
        self._cmodel = model.as_c()
        ctx = ctypes.c_void_p()
        if precision == 'fp32' and kernel is None:
            _lib.check(self._lib.fmj_create(ctypes.byref(self._cmodel), self.n_envs, self.device.index or 0,
                                            ctypes.byref(ctx)))
        else:
            asked = f'precision={precision!r}' if kernel is None else f'kernel={kernel!r}'
            if not _lib.has('fmj_create_ex'):      # an A/B base build (FMJ_SO)
                raise _lib.FmjError(f'this libfmj_hip.so has no fmj_create_ex: {asked} needs a current build')
            k = kernel or KernelOptions()
            flags = (k.two_wave * _lib.KERNEL_TWO_WAVE | (not k.two_env) * _lib.KERNEL_ONE_ENV_PER_WAVE |
                     (not k.lean) * _lib.KERNEL_NO_LEAN | (not k.prio) * _lib.KERNEL_NO_PRIO)
            opts = _lib.CCreateOptions(ctypes.sizeof(_lib.CCreateOptions), _lib.PRECISIONS[precision], flags, k.wps or 0)
            if ext_flags:
                if not _lib.has('fmj_create_ex2'):      # an A/B base build (FMJ_SO)
                    raise _lib.FmjError('this libfmj_hip.so has no fmj_create_ex2: fp64_limits=True / fp64_rk4=True / fp64_contacts=True need a current build')
                ext = _lib.CCreateExt(ctypes.sizeof(_lib.CCreateExt), ext_flags)
                rc = self._lib.fmj_create_ex2(ctypes.byref(self._cmodel), self.n_envs, self.device.index or 0,
                                              ctypes.byref(opts), ctypes.byref(ext), ctypes.byref(ctx))
            else:
                rc = self._lib.fmj_create_ex(ctypes.byref(self._cmodel), self.n_envs, self.device.index or 0,
                                             ctypes.byref(opts), ctypes.byref(ctx))
            if rc and b'fmj_create_options.size' in self._lib.fmj_last_error():      # an A/B base build from before the kernel fields
                raise _lib.FmjError(f'this libfmj_hip.so has no kernel fields in fmj_create_options: {asked} needs a current build')
            _lib.check(rc)
        self._ctx = ctx
        code = self._lib.fmj_precision(self._ctx) if _lib.has('fmj_precision') else 0
        self.precision = {v: k for k, v in _lib.PRECISIONS.items()}[code]      # what the context reports
        lay = _lib.CSensorLayout()
        _lib.check(self._lib.fmj_get_sensor_layout(self._ctx, ctypes.byref(lay)))
        self.sensor_layout = lay
        assert lay.nsensordata == model.nsensordata
        n, m, dev = self.n_envs, model, self.device
        z = lambda *s, dtype=torch.float32: torch.zeros(*s, dtype=dtype, device=dev)
        self.data = _MjData(
            qpos=z(n, m.nq), qvel=z(n, m.nv), ctrl=z(n, m.nu), qpos_spring=z(n, m.nq),
            xfrc_applied=z(n, m.nbody, 6), xpos=z(n, m.nbody, 3), xquat=z(n, m.nbody, 4), xipos=z(n, m.nbody, 3),
            sensordata=z(n, m.nsensordata), qacc=z(n, m.nv), time=z(n), status=z(n, dtype=torch.int32))
        self.has_constraints = bool(np.any(m.jnt_limited)) or m.ngeom > 0
        # FMJ_INT_RK4: fmj_step runs four forward launches per step and fmj_step_fused refuses - or, in an fp64_rk4 context, the fp64
        # kernel runs the four passes itself (one launch for all steps; fmj_step_fused_f64 fuses); so does an fp64_contacts_rk4 context
        # on a walking model, through fmj_step alone
        self.rk4 = int(getattr(m, 'integrator', 0)) == 1
        self.max_contacts = max(int(m.max_contacts), 1)
        self.data.qacc_warmstart = z(n, m.nv)
        self.data.contact = z(n, self.max_contacts, 16)
        self.data.ncon = z(n, dtype=torch.int32)
        self.data.xquat[:, :, 0] = 1.0
        self.data.qpos_spring[:] = torch.as_tensor(m.qpos_spring, dtype=torch.float32)
        # the solver that actually runs (fmj_solver_info): fmj_create swaps a primal solver for the dual one on near-frictionless contacts
        rq, ef, it = _lib.ints(self._lib.fmj_solver_info, self._ctx) if _lib.has('fmj_solver_info') else (0, 0, 0)     # absent only from an A/B base build (FMJ_SO)
        names = {0: 'PGS', 1: 'CG', 2: 'Newton'}
        self.solver_requested, self.solver_effective, self.solver_budget = names[rq], names[ef], it
        if rq != ef and (self.fp64_limits or self.fp64_contacts):      # (raised only when the model asked for PGS or CG: Newton is what runs)
            import warnings
            what = 'joint limits' if not self.fp64_contacts else 'limits and contacts'
            warnings.warn(f'solver={self.solver_requested!r} was requested, but the fp64 step solves {what} with its primal Newton solve: '
                          f'{self.solver_effective}, until the active set stops changing or {self.solver_budget} iterations per step '
                          '(same minimiser; include/fmj.h: fmj_create_ex2)', stacklevel=2)
        elif rq != ef:
            import warnings
            why = ('the noslip post-pass works on the dual matrices, which a primal solver never forms' if int(getattr(model, 'noslip_iterations', 0)) > 0 else
                   'explicit pairs under the elliptic cone have the dual block update only' if (int(getattr(model, 'cone', 0)) == 1 and int(getattr(model, 'npair', 0)) > 0) else
                   'some ground contact has friction / sqrt(impratio) < 1e-3 (rows an fp32 primal iteration cannot resolve)')
            warnings.warn(f'solver={self.solver_requested!r} was requested, but {why}: the model is solved on the dual problem instead - {self.solver_effective} to the '
                          f'solver tolerance, up to {self.solver_budget} sweeps per step (same minimiser; include/fmj.h: fmj_solver_info)', stacklevel=2)
        self.links_body = np.arange(1, m.nbody, dtype=np.int32)
        self.joints_jnt = np.nonzero(m.jnt_type != JNT_FREE)[0].astype(np.int32)
        self.reset()

    def __del__(self):
        ctx = getattr(self, '_ctx', None)
        if ctx:
            self._lib.fmj_destroy(ctx)
            self._ctx = None

    # ---- marshalling ----------------------------------------------------------------------------
    def _cdata(self, ctrl: Optional[torch.Tensor] = None) -> _lib.CData:
        """fmj_data of ``physics.data`` (``ctrl``: a ctrl tape in the place of ``data.ctrl``): built once per binding of the fields
        (_MjData), and handed out as a private copy - callers edit single fields."""
        d = self.data
        if d._cdata_cache is None:
            object.__setattr__(d, '_cdata_cache', _lib.CData(*[getattr(d, name).data_ptr() for name, _ in _lib.CData._fields_]))
        c = _lib.CData.from_buffer_copy(d._cdata_cache)
        if ctrl is not None:
            c.ctrl = ctrl.data_ptr()
        return c

    # ---- dm_control Physics surface -----------------------------------------------------------------
    def reset(self, keyframe_id: int = 0):
        """physics.reset(keyframe_id=0) (reference task.py:137): keyframe state, then mj_forward with
        actuation disabled."""
        m, d = self.model, self.data
        d.qpos[:] = torch.as_tensor(m.key_qpos, dtype=torch.float32)
        d.qvel[:] = torch.as_tensor(m.key_qvel, dtype=torch.float32)
        d.ctrl.zero_(); d.xfrc_applied.zero_(); d.time.zero_(); d.status.zero_(); d.qacc.zero_()
        d.sensordata.zero_(); d.qacc_warmstart.zero_(); d.contact.zero_(); d.ncon.zero_()
        self.forward(disable_actuation=True)

    def forward(self, disable_actuation: bool = False):
        _lib.check(self._lib.fmj_forward(self._ctx, ctypes.byref(self._cdata()), int(disable_actuation), _lib.stream_ptr(self.device)))

    def step(self, nstep: int = 1, ctrl_tape: Optional[torch.Tensor] = None):
        """mujoco.mj_step x nstep for every env (reference simulation.py:156 via Physics.step).
        ``ctrl_tape`` [nstep, n_envs, nu] supplies a different ctrl row per step."""
        if ctrl_tape is not None:
            assert ctrl_tape.shape == (nstep, self.n_envs, self.model.nu) and ctrl_tape.is_contiguous()
        stride = 0 if ctrl_tape is None else self.n_envs*self.model.nu
        _lib.check(self._lib.fmj_step(self._ctx, ctypes.byref(self._cdata(ctrl_tape)), int(nstep), stride, _lib.stream_ptr(self.device)))

    def step_debug(self, want_pgs: bool = True):
        """One mj_step through ``fmj_step_debug``: returns ``(efc_rows [n_envs, maxefc, 8], pgs_improvement [n_envs,
        solver_iterations] or None)`` next to the usual state update (tests of the constraint solve; not the product path)."""
        maxefc, _, iterations = _lib.ints(self._lib.fmj_constraint_info, self._ctx)
        rows = torch.zeros(self.n_envs, max(maxefc, 1), 8, device=self.device)
        imp = torch.full((self.n_envs, max(iterations, 1)), float('nan'), device=self.device) if want_pgs else None
        _lib.check(self._lib.fmj_step_debug(self._ctx, ctypes.byref(self._cdata()), _ptr(rows), _ptr(imp), _lib.stream_ptr(self.device)))
        return rows, imp

    def forward_debug(self, disable_actuation: bool = False):
        """mj_forward through ``fmj_forward_debug``: returns ``(H [n_envs, nv, row_stride], qfrc_smooth [n_envs, nv])`` next to the
        usual derived fields - the packed rows of H = M + diag(armature + h damping) as the step assembles them (include/fmj.h; tests
        of the stages, not the product path).  The library names its row stride in the call that fills the rows, so they land in a
        buffer of the longest row any build has (64, _lib.build) and H is the view of its packed head: ``H._base`` is the whole
        buffer, zero past the rows."""
        n, nv, rs = self.n_envs, self.model.nv, ctypes.c_int32()
        buf = torch.zeros(n*nv*64, device=self.device)
        qfrc = torch.zeros(n, nv, device=self.device)
        _lib.check(self._lib.fmj_forward_debug(self._ctx, ctypes.byref(self._cdata()), int(disable_actuation), _ptr(buf), ctypes.byref(rs),
                                               _ptr(qfrc), _lib.stream_ptr(self.device)))
        return buf[:n*nv*rs.value].view(n, nv, rs.value), qfrc

    # ---- checkpoint / resume ---------------------------------------------------------
    STATE_FIELDS = ('qpos', 'qvel', 'ctrl', 'qpos_spring', 'xfrc_applied', 'xpos', 'xquat', 'xipos', 'sensordata', 'qacc',
                    'time', 'status', 'qacc_warmstart', 'contact', 'ncon')

    def get_state(self):
        """Every mjData field as a host array: the integrated state (qpos, qvel, qpos_spring, time, status), the solver's warm
        start, and the derived fields of the last step (poses, sensordata, contacts) that the NEXT step's row readout reports
        (mj_step lag).  ``set_state`` of this dict on a context of the same model and batch resumes bitwise."""
        return {k: getattr(self.data, k).detach().cpu().numpy().copy() for k in self.STATE_FIELDS}

    def set_state(self, state):
        for k in self.STATE_FIELDS:
            t = getattr(self.data, k)
            a = np.asarray(state[k])
            if tuple(a.shape) != tuple(t.shape):
                raise ValueError(f'state field {k}: shape {a.shape}, this context holds {tuple(t.shape)}')
            t.copy_(torch.as_tensor(a, dtype=t.dtype))

    def check_invalid_state(self):
        """Raise PhysicsError if any env reported a bad-state warning (lazy, one sync)."""
        bad = torch.nonzero(self.data.status).flatten()
        if bad.numel():
            e = int(bad[0])
            raise PhysicsError(f'bad simulation state in {bad.numel()} env(s); first env {e} '
                               f'status bits {int(self.data.status[e])}')

    def timestep(self):
        return self.model.timestep

    # ---- operators the API layer calls ---------------------------------------------------------------
    def set_readout_maps(self, links_body, joints_jnt):
        self.links_body = np.ascontiguousarray(links_body, np.int32)
        self.joints_jnt = np.ascontiguousarray(joints_jnt, np.int32)
        I = ctypes.POINTER(ctypes.c_int32)
        _lib.check(self._lib.fmj_set_readout_maps(self._ctx, len(self.links_body), self.links_body.ctypes.data_as(I),
                                                  len(self.joints_jnt), self.joints_jnt.ctypes.data_as(I)))

    def set_swimming(self, n_xfrc_rows, links_index, xfrc_index, body_index, coefficients, masses, heights, densities):
        """``n_xfrc_rows`` = len(data.sensors.xfrc.names): the per-env row count of the xfrc tensor."""
        I, D = ctypes.POINTER(ctypes.c_int32), ctypes.POINTER(ctypes.c_double)
        a = [np.ascontiguousarray(x, np.int32) for x in (links_index, xfrc_index, body_index)]
        b = [np.ascontiguousarray(x, np.float64) for x in (coefficients, masses, heights, densities)]
        _lib.check(self._lib.fmj_set_swimming(self._ctx, len(a[0]), int(n_xfrc_rows), *[x.ctypes.data_as(I) for x in a],
                                              *[x.ctypes.data_as(D) for x in b]))

    def set_actuator_forcerange(self, forcelimited, forcerange):
        """Rewrite ``model.actuator_forcelimited`` / ``actuator_forcerange`` and refresh the device tables (the
        run-time edit of reference task.py:279-286)."""
        m = self.model
        m.actuator_forcelimited = np.ascontiguousarray(forcelimited, np.int32).reshape(m.nu)
        m.actuator_forcerange = np.ascontiguousarray(forcerange, np.float64).reshape(m.nu, 2)
        _lib.check(self._lib.fmj_set_actuator_forcerange(
            self._ctx, m.nu, m.actuator_forcelimited.ctypes.data_as(ctypes.POINTER(ctypes.c_int32)),
            m.actuator_forcerange.ctypes.data_as(ctypes.POINTER(ctypes.c_double))))

    def set_contact_maps(self, n_rows, geom_sensor, pairs=()):
        """geompair2data (reference physics.py:360-382): geom -> contact sensor row for keys (geom, -1), plus explicit
        (geom1, geom2, row) pairs."""
        I = ctypes.POINTER(ctypes.c_int32)
        gs = np.ascontiguousarray(geom_sensor, np.int32)
        pr = np.ascontiguousarray(np.asarray(pairs, np.int32).reshape(-1, 3))
        _lib.check(self._lib.fmj_set_contact_maps(self._ctx, int(n_rows), gs.ctypes.data_as(I), len(pr),
                                                  pr.ctypes.data_as(I) if len(pr) else None))

    def kernel_info(self):
        lds, thr = _lib.ints(self._lib.fmj_kernel_info, self._ctx)
        info = dict(lds_bytes_per_env=lds, threads_per_env=thr)
        if self.precision == 'fp64':
            # which text of csrc/fmj_f64_step.inc every launch of the context runs: an fp64 context reports contacts (fmj_constraint_info's
            # max_contacts) only where its model has ground contacts and the contact solve was asked for
            contacts = self.fp64_contacts and _lib.ints(self._lib.fmj_constraint_info, self._ctx)[1] > 0
            elliptic = contacts and self.fp64_elliptic and int(getattr(self.model, 'cone', 0)) == 1      # (FMJ_CONE_ELLIPTIC; one family on flat ground and terrain)
            mesh = contacts and self.fp64_mesh and bool((np.asarray(self.model.geom_type) == 7).any())      # (FMJ_GEOM_MESH: kernels of their own)
            rk4 = contacts and self.fp64_contacts_rk4 and self.rk4      # (the four passes inside the terrain / elliptic text; no mesh builds)
            info['fp64_step_kernel'] = ('fmj_step_f64_elliptic_rk4_kernel' if rk4 and elliptic else 'fmj_step_f64_terrain_rk4_kernel' if rk4 else
                                        'fmj_step_f64_mesh_elliptic_kernel' if mesh and elliptic else 'fmj_step_f64_mesh_kernel' if mesh else
                                        'fmj_step_f64_elliptic_kernel' if elliptic else 'fmj_step_f64_terrain_kernel' if contacts and self.fp64_terrain else 'fmj_step_f64_contacts_kernel' if contacts else
                                        'fmj_step_f64_rk4_kernel' if self.fp64_rk4 and self.rk4 else 'fmj_step_f64_kernel')
        if _lib.has('fmj_dual_build_info'):     # absent only from an A/B base build (FMJ_SO)
            # the two-env step kernel's build (include/fmj.h: fmj_dual_build_info): register tier, whether fused launches of the
            # flagship shape run the lean build, what the last step launch ran, and whether fused launches alternate the issue
            # priority of the waves of a SIMD and by which policy (csrc/fmj_dual2.inc, FMJ_DUAL_PRIO_PHASE; 0 = none).  An A/B base build
            # from before either argument leaves it at 0
            wps, lean, last, prio, pol = _lib.ints(self._lib.fmj_dual_build_info, self._ctx)
            if wps:
                info.update(dual_wps=wps, dual_build='lean' if lean else 'generic', dual_last_launch=(None, 'generic', 'rare', 'lean')[last],
                            dual_prio=bool(prio), dual_prio_policy=pol)
        return info
