// fmj_stage2_k.inc - step stage shared by the two-env kernel (fmj_dual2.inc) and the two-env constraint kernel (fmj_cons2.inc): a block
// of statements on the including kernel's locals.
// K: the body's local transform, composed along the chain by pointer jumping inside the half (partner poses pulled with ds_bpermute).
// reads  c_pos_mass, c_quat, c_axis_q0, c_jpos_k, jtype, qadr, isb, sl, hb, jm, max_bdepth, any_jpos, any_bquat, QP, JMP
// writes xp, xq (declared by the kernel)
      xp = mk3(c_pos_mass.x, c_pos_mass.y, c_pos_mass.z);
      xq.w = c_quat.x; xq.x = c_quat.y; xq.y = c_quat.z; xq.z = c_quat.w;
      if (jtype == FMJ_JNT_FREE) {
        xp = mk3(QP[qadr], QP[qadr + 1], QP[qadr + 2]);
        q4 rq = {QP[qadr + 3], QP[qadr + 4], QP[qadr + 5], QP[qadr + 6]};
        xq = qnormalize(rq);
      } else if (jtype == FMJ_JNT_HINGE) {
        const float q = QP[qadr] - c_axis_q0.w;
        const v3 ax = mk3(c_axis_q0.x, c_axis_q0.y, c_axis_q0.z);
        const q4 ql = axisangle_mid(ax, q);
        if (any_jpos) {                          // anchor off the body origin: the body turns about the anchor
          const v3 jp = mk3(c_jpos_k.x, c_jpos_k.y, c_jpos_k.z);
          xp = add3(xp, qrot(xq, sub3(jp, qrot(ql, jp))));
        }
        xq = any_bquat ? qmul(xq, ql) : ql;      // body frames aligned with their parents': the local rotation is the joint's
      } else if (jtype == FMJ_JNT_SLIDE) {
        const float q = QP[qadr] - c_axis_q0.w;
        xp = add3(xp, qrot(xq, scl3(mk3(c_axis_q0.x, c_axis_q0.y, c_axis_q0.z), q)));
      }
      if (!isb) { xp = mk3(0.f, 0.f, 0.f); xq.w = 1.f; xq.x = xq.y = xq.z = 0.f; }
      for (int r = 0; r < max_bdepth; r++) {
        const int a = r < 4 ? (int)((jm >> (8 * r)) & 0xff) : (sl < nb ? (int)JMP[sl * M.anc_stride + r] : 0);
        const int src = (hb + a) << 2;
#define PULL(v_) __int_as_float(__builtin_amdgcn_ds_bpermute(src, __float_as_int(v_)))
        const v3 ap = mk3(PULL(xp.x), PULL(xp.y), PULL(xp.z));
        const q4 aqq = {PULL(xq.w), PULL(xq.x), PULL(xq.y), PULL(xq.z)};
#undef PULL
        xp = add3(ap, qrot(aqq, xp));
        xq = qmul(aqq, xq);
      }
      xq = qnormalize(xq);
