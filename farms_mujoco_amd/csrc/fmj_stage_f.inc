// fmj_stage_f.inc - step stage shared by fmj_step_kernel (fmj_hip.hip) and fmj_step_wide_kernel (fmj_wide.inc): a block of
// statements on the including kernel's locals.
// F: body force about the common point, then what the last forward pass leaves behind: the links row and drag of the next
// before_step, and on the launch's last step the poses and the velocimeter sensors.
// reads  xi, com, mass, iw, ca, cv, xf, xp, xq, isb, blo, lane, nb, env, last, nfull, nit;  emit_links_and_drag updates xf
// defines fbody
    // ---- F: body force (inertial minus external), about the common point
    s6 fbody;
    {
      // cinert * v with cinert = {Iw, d = xi - com, m} (MuJoCo's cinert about the tree CoM, never materialised):
      // lin = p = m (u + w x d),  rot = Iw w + d x p
      const v3 d = sub3(xi, com);
      s6 ia, iv;
      ia.l = scl3(add3(ca.l, cross(ca.r, d)), mass);
      ia.r = add3(mk3(iw[0] * ca.r.x + iw[3] * ca.r.y + iw[4] * ca.r.z, iw[3] * ca.r.x + iw[1] * ca.r.y + iw[5] * ca.r.z,
                      iw[4] * ca.r.x + iw[5] * ca.r.y + iw[2] * ca.r.z), cross(d, ia.l));
      iv.l = scl3(add3(cv.l, cross(cv.r, d)), mass);
      iv.r = add3(mk3(iw[0] * cv.r.x + iw[3] * cv.r.y + iw[4] * cv.r.z, iw[3] * cv.r.x + iw[1] * cv.r.y + iw[5] * cv.r.z,
                      iw[4] * cv.r.x + iw[5] * cv.r.y + iw[2] * cv.r.z), cross(d, iv.l));
      s6 f = s6add(ia, cross_force(cv, iv));
      const v3 fw = mk3(xf[0], xf[1], xf[2]), tw = mk3(xf[3], xf[4], xf[5]);
      f.r = sub3(f.r, add3(tw, cross(sub3(xi, com), fw)));
      f.l = sub3(f.l, fw);
      if (!isb) { f.r = f.l = mk3(0.f, 0.f, 0.f); }
      fbody = f;
    }
    // ---- sensors of this (pre-integration) state; they are next iteration's link data (mj_step lag)
    {
      const v3 linvel = add3(cv.l, cross(cv.r, sub3(xi, com)));
      if (FUSED && !last && (nfull || (A.sub_links && !(A.n_it_total > 0 && nit >= A.n_it_total)))) {      // the next before_step's links row and drag (xf is consumed above, in this step's F);
        const int4 ci2 = BTABI(blo, 8);                     // a sub-step that writes no row keeps the drag force it has
        emit_links_and_drag(M, A, env, nit, isb, false, ci2.z, ci2.w, xp, xq, xi, linvel, cv.r, xf);
      }
      if (last && lane < nb) {
        float* p = glob(A.xpos) + (size_t)env * nb * 3 + lane * 3; p[0] = xp.x; p[1] = xp.y; p[2] = xp.z;
        *(float4*)(glob(A.xquat) + (size_t)env * nb * 4 + lane * 4) = make_float4(xq.w, xq.x, xq.y, xq.z);
        float* ip = glob(A.xipos) + (size_t)env * nb * 3 + lane * 3; ip[0] = xi.x; ip[1] = xi.y; ip[2] = xi.z;
        if (isb) {
          float* sp = glob(A.sensordata) + (size_t)env * M.nsensordata + 6 * (lane - 1);
          *(float2*)(sp) = make_float2(linvel.x, linvel.y);
          *(float2*)(sp + 2) = make_float2(linvel.z, cv.r.x);
          *(float2*)(sp + 4) = make_float2(cv.r.y, cv.r.z);
        }
      }
    }
