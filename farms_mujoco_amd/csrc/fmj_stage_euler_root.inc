// fmj_stage_euler_root.inc - step stage shared by fmj_step_kernel (fmj_hip.hip) and fmj_step_wide_kernel (fmj_wide.inc): a block of
// statements on the including kernel's locals.
// Euler, part 3 (after the barrier): position and quaternion of a free root (lane = root body); the kernel's BADQPOS vote follows.
// reads  jtype, qadr, dadr, frozen, QV;  writes QP;  updates warn
    if (jtype == FMJ_JNT_FREE && A.integrate && !frozen) {     // free joint position update (lane = root body)
      // the new root position is tested before it is committed: a frozen env keeps its last finite state (include/fmj.h)
      const float nx = QP[qadr] + M.h * QV[dadr], ny = QP[qadr + 1] + M.h * QV[dadr + 1], nz = QP[qadr + 2] + M.h * QV[dadr + 2];
      if (!(fabsf(nx) <= 1e10f) || !(fabsf(ny) <= 1e10f) || !(fabsf(nz) <= 1e10f)) warn |= FMJ_WARN_BADQPOS;
      else {
        QP[qadr] = nx; QP[qadr + 1] = ny; QP[qadr + 2] = nz;
        const v3 w = mk3(QV[dadr + 3], QV[dadr + 4], QV[dadr + 5]);
        const float n2 = dot3(w, w), rn = rsqrt_nr(n2), n = n2 * rn;
        q4 qo = {QP[qadr + 3], QP[qadr + 4], QP[qadr + 5], QP[qadr + 6]};
        qo = qnormalize(qo);
        if (n2 >= 1e-30f) qo = qmul(qo, axisangle_small(scl3(w, rn), M.h * n));
        QP[qadr + 3] = qo.w; QP[qadr + 4] = qo.x; QP[qadr + 5] = qo.y; QP[qadr + 6] = qo.z;
      }
    }
