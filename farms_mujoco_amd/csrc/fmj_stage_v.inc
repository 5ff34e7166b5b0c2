// fmj_stage_v.inc - step stage shared by fmj_step_kernel (fmj_hip.hip) and fmj_step_wide_kernel (fmj_wide.inc): a block of
// statements on the including kernel's locals.
// V: the joint's motion axes (cdof, about the tree CoM) into CD and the joint velocity, before the chain sums.
// reads  jtype, dadr, xp, xq, com, c_axis_q0, c_jpos_k, any_jpos, QV;  writes CD
// defines vJ (joint velocity), vt (translational part of a free root)
      s6 vJ = {mk3(0.f, 0.f, 0.f), mk3(0.f, 0.f, 0.f)};
      s6 vt = {mk3(0.f, 0.f, 0.f), mk3(0.f, 0.f, 0.f)};       // translational part of a free root
      if (jtype == FMJ_JNT_HINGE || jtype == FMJ_JNT_SLIDE) {
        const v3 axw = qrot(xq, mk3(c_axis_q0.x, c_axis_q0.y, c_axis_q0.z));
        s6 cd;
        if (jtype == FMJ_JNT_HINGE) {
          const v3 anchor = any_jpos ? add3(xp, qrot(xq, mk3(c_jpos_k.x, c_jpos_k.y, c_jpos_k.z))) : xp;
          cd.r = axw; cd.l = cross(axw, sub3(com, anchor));
        } else { cd.r = mk3(0.f, 0.f, 0.f); cd.l = axw; }
        lds_put6(CD + dadr * 8, cd);
        vJ = s6scl(cd, QV[dadr]);
      } else if (jtype == FMJ_JNT_FREE) {
        const v3 off = sub3(com, xp);
        const m33 R = q2m(xq);
        vt.l = mk3(QV[dadr], QV[dadr + 1], QV[dadr + 2]);
#pragma unroll
        for (int k = 0; k < 3; k++) {
          s6 ct = {mk3(0.f, 0.f, 0.f), mk3(k == 0 ? 1.f : 0.f, k == 1 ? 1.f : 0.f, k == 2 ? 1.f : 0.f)};
          lds_put6(CD + (dadr + k) * 8, ct);
          const v3 col = mk3(R.a[k], R.a[k + 3], R.a[k + 6]);
          s6 cr = {col, cross(col, off)};
          lds_put6(CD + (dadr + 3 + k) * 8, cr);
          vJ = s6add(vJ, s6scl(cr, QV[dadr + 3 + k]));
        }
      }
