// fmj_stage2_v.inc - step stage shared by the two-env kernel (fmj_dual2.inc) and the two-env constraint kernel (fmj_cons2.inc): a block
// of statements on the including kernel's locals.  STAGE2_REC is the kernel's stride of the CD / F records in floats.
// V: joint velocity, cvel = chain sum of joint velocities, cacc = chain sum of cvel_parent x vJ - g.
// reads  jtype, dadr, c_info, c_axis_q0, c_jpos_k, xp, xq, com, isb, sl, hb, jm, max_bdepth, any_jpos, QV, JMP;  writes CD
// defines cv, ca
    s6 cv, ca;
    {
      s6 vJ = {mk3(0.f, 0.f, 0.f), mk3(0.f, 0.f, 0.f)};
      s6 vt = {mk3(0.f, 0.f, 0.f), mk3(0.f, 0.f, 0.f)};
      if (jtype == FMJ_JNT_HINGE || jtype == FMJ_JNT_SLIDE) {
        const v3 axw = qrot(xq, mk3(c_axis_q0.x, c_axis_q0.y, c_axis_q0.z));
        s6 cd;
        if (jtype == FMJ_JNT_HINGE) {
          const v3 anchor = any_jpos ? add3(xp, qrot(xq, mk3(c_jpos_k.x, c_jpos_k.y, c_jpos_k.z))) : xp;
          cd.r = axw; cd.l = cross(axw, sub3(com, anchor));
        } else { cd.r = mk3(0.f, 0.f, 0.f); cd.l = axw; }
        lds_put6(CD + dadr * STAGE2_REC, cd);
        vJ = s6scl(cd, QV[dadr]);
      } else if (jtype == FMJ_JNT_FREE) {
        const v3 off = sub3(com, xp);
        const m33 R = q2m(xq);
        vt.l = mk3(QV[dadr], QV[dadr + 1], QV[dadr + 2]);
#pragma unroll
        for (int k = 0; k < 3; k++) {              // the translational cdof are unit vectors: never read back
          const v3 col = mk3(R.a[k], R.a[k + 3], R.a[k + 6]);
          s6 cr = {col, cross(col, off)};
          lds_put6(CD + (dadr + 3 + k) * STAGE2_REC, cr);
          vJ = s6add(vJ, s6scl(cr, QV[dadr + 3 + k]));
        }
      }
      cv = s6add(vJ, vt);
#define PULL6(dst_, src_, v_) do { \
        dst_.r = mk3(__int_as_float(__builtin_amdgcn_ds_bpermute(src_, __float_as_int(v_.r.x))), __int_as_float(__builtin_amdgcn_ds_bpermute(src_, __float_as_int(v_.r.y))), \
                     __int_as_float(__builtin_amdgcn_ds_bpermute(src_, __float_as_int(v_.r.z)))); \
        dst_.l = mk3(__int_as_float(__builtin_amdgcn_ds_bpermute(src_, __float_as_int(v_.l.x))), __int_as_float(__builtin_amdgcn_ds_bpermute(src_, __float_as_int(v_.l.y))), \
                     __int_as_float(__builtin_amdgcn_ds_bpermute(src_, __float_as_int(v_.l.z)))); } while (0)
      for (int r = 0; r < max_bdepth; r++) {
        const int a = r < 4 ? (int)((jm >> (8 * r)) & 0xff) : (sl < nb ? (int)JMP[sl * M.anc_stride + r] : 0);
        s6 o; PULL6(o, (hb + a) << 2, cv);
        cv = s6add(cv, o);
      }
      s6 cpar; PULL6(cpar, (hb + (isb ? c_info.x : 0)) << 2, cv);
      cpar = s6add(cpar, vt);
      ca = cross_motion(cpar, vJ);
      if (!isb) { ca.r = ca.l = mk3(0.f, 0.f, 0.f); }
      for (int r = 0; r < max_bdepth; r++) {
        const int a = r < 4 ? (int)((jm >> (8 * r)) & 0xff) : (sl < nb ? (int)JMP[sl * M.anc_stride + r] : 0);
        s6 o; PULL6(o, (hb + a) << 2, ca);
        ca = s6add(ca, o);
      }
#undef PULL6
      ca.l = sub3(ca.l, mk3(M.gx, M.gy, M.gz));
      if (!isb) { cv.r = cv.l = mk3(0.f, 0.f, 0.f); }
    }
