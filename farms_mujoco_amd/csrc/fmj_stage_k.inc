// fmj_stage_k.inc - step stage shared by fmj_step_kernel (fmj_hip.hip) and fmj_step_wide_kernel (fmj_wide.inc): a block of
// statements on the including kernel's locals.
// K: the body's local transform, before the chain composition.
// reads  blo, isb, jtype, qadr, c_axis_q0, c_jpos_k, any_jpos, any_bquat, QP
// writes xp, xq (declared by the kernel: they live on past the pointer-jumping rounds that follow)
      const float4 c_pos_mass = BTAB(blo, 0);
      const float4 c_quat = BTAB(blo, 1);
      xp = mk3(c_pos_mass.x, c_pos_mass.y, c_pos_mass.z);
      xq.w = c_quat.x; xq.x = c_quat.y; xq.y = c_quat.z; xq.z = c_quat.w;
      if (jtype == FMJ_JNT_FREE) {
        xp = mk3(QP[qadr], QP[qadr + 1], QP[qadr + 2]);
        q4 rq = {QP[qadr + 3], QP[qadr + 4], QP[qadr + 5], QP[qadr + 6]};
        xq = qnormalize(rq);
      } else if (jtype == FMJ_JNT_HINGE) {
        const float q = QP[qadr] - c_axis_q0.w;
        const v3 ax = mk3(c_axis_q0.x, c_axis_q0.y, c_axis_q0.z);
        const q4 ql = axisangle_mid(ax, q);       // half-angle sin / cos by polynomial for |q| <= pi
        if (any_jpos) {                           // anchor off the body origin: the body turns about the anchor
          const v3 jp = mk3(c_jpos_k.x, c_jpos_k.y, c_jpos_k.z);
          xp = add3(xp, qrot(xq, sub3(jp, qrot(ql, jp))));
        }
        xq = any_bquat ? qmul(xq, ql) : ql;       // body frames aligned with their parents': the local rotation is the joint's
      } else if (jtype == FMJ_JNT_SLIDE) {
        const float q = QP[qadr] - c_axis_q0.w;
        xp = add3(xp, qrot(xq, scl3(mk3(c_axis_q0.x, c_axis_q0.y, c_axis_q0.z), q)));
      }
      if (!isb) { xp = mk3(0.f, 0.f, 0.f); xq.w = 1.f; xq.x = xq.y = xq.z = 0.f; }
