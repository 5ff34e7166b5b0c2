// fmj_stage_q.inc - step stage shared by fmj_step_kernel (fmj_hip.hip) and fmj_step_wide_kernel (fmj_wide.inc): a block of
// statements on the including kernel's locals.
// Q: qfrc_smooth of the lane's dof: bias force, damping, joint stiffness, mj_fwdActuation (tape or wave controller); on the
// launch's last step the wave controller's ctrl and the actuatorfrc sensors.
// reads  dlo, isd, lane, env, it, itm, S_sub, last, com, CD, CI, F, QP, QV;  updates cy_actsum
// defines qfrc, dvel, cd, bf, sc, d_prm, d_act, d_qadr, d_scalar
    // ---- Q: qfrc_smooth, buf = (I_s w, m v(s))  (lane = dof)
    float qfrc = 0.f;
    float dvel = 0.f;                               // implicitfast: velocity gains of this dof's unclamped actuators
    float af0 = 0.f, af1 = 0.f, af2 = 0.f, af3 = 0.f;
    const float4 d_prm = DTAB(dlo, 1);             // armature, damping, qposadr bits, hinge/slide flag
    const int4 d_act = DTABI(dlo, 2);               // first actuator, count, joint sensor slot
    const int d_qadr = __float_as_int(d_prm.z);
    const bool d_scalar = isd && d_prm.w != 0.f;
    s6 cd = {mk3(0.f, 0.f, 0.f), mk3(0.f, 0.f, 0.f)}, bf = cd;     // this dof's cdof; (I_s w_i, m v_i(s)), s = CoM of the subtree it moves
    v3 sc = mk3(0.f, 0.f, 0.f);                                    // s relative to the tree CoM
    if (isd) {
      const int body = DTABI(dlo, 0).x;
      cd = lds_get6(CD + lane * 8);
      {
        const float4 a = *(const float4*)(CI + body * 12), b = *(const float4*)(CI + body * 12 + 4);
        const float2 c = *(const float2*)(CI + body * 12 + 8);
        sc = sub3(mk3(b.z, b.w, c.x), com);
        const v3 vs = add3(cd.l, cross(cd.r, sc));                 // velocity of the subtree CoM per unit dof rate
        bf.r = mk3(a.x * cd.r.x + a.w * cd.r.y + b.x * cd.r.z, a.w * cd.r.x + a.y * cd.r.y + b.y * cd.r.z, b.x * cd.r.x + b.y * cd.r.y + a.z * cd.r.z);
        bf.l = scl3(vs, c.y);
      }
      const float qd = QV[lane];
      qfrc = -d_prm.y * qd - s6dot(cd, lds_get6(F + body * 8));
      if (d_scalar) {
        const float qj = QP[d_qadr];
        if (M.any_stiffness) {
          const float kst = BTAB(body, 6).w;
          if (kst != 0.f) qfrc -= kst * (qj - gptr(A.qpos_spring)[(size_t)env * nq + d_qadr]);
        }
        float asum = 0.f;
        float cbase = 0.f;
        const float AS1* const w_amp = gptr(A.w_amp) + (size_t)env * A.w_amp_stride;      // the env's rows (stride 0: the shared row)
        const float AS1* const w_lag = gptr(A.w_lag) + (size_t)env * A.w_lag_stride;
        if (FUSED && A.controller == 1) {
          // phase in cycles kept in fp64 so long runs keep the argument exact (task.py:290: time = iteration*timestep)
          const float wfreq = A.w_freq_env ? gptr(A.w_freq_env)[env] : A.w_freq;      // the env's own frequency (fmj_fused_ext), else the shared one
          double cyc = (double)wfreq * ((double)it * ((double)M.h * (double)S_sub));   // task.py:290: time = iteration * timestep (of an iteration)
          cyc -= floor(cyc);
          cbase = 6.283185307179586f * (float)cyc + gptr(A.w_env)[env];
        }
#pragma unroll
        for (int a = 0; a < 4; a++) {                 // mj_fwdActuation, joint transmission
          if (a < d_act.y) {
            const int ai = d_act.x + a, src = __float_as_int(ATAB(ai, 2).x);
            const float4 p = ATAB(ai, 0), lim = ATAB(ai, 1);
            float c;
            if (FUSED && A.controller == 1) { const float amp = w_amp[src]; c = amp != 0.f ? amp * sinf(cbase - w_lag[src]) : 0.f; }
            else c = A.ctrl ? gptr(A.ctrl)[(size_t)itm * A.ctrl_step_stride + (size_t)env * nu + src] : 0.f;      // one ctrl row per iteration
            c = fminf(fmaxf(c, lim.x), lim.y);
            float f = p.x * c + p.y + p.z * qj + p.w * qd;
            if (M.implicitfast && !A.disable_actuation && f > lim.z && f < lim.w) dvel -= p.w;      // d force / d qvel of an unclamped actuator (mjd_actuator_vel)
            f = fminf(fmaxf(f, lim.z), lim.w);
            if (A.disable_actuation) f = 0.f;
            if (a == 0) af0 = f; else if (a == 1) af1 = f; else if (a == 2) af2 = f; else af3 = f;
            asum += f;
          }
        }
        qfrc += asum;
        cy_actsum = asum * A.inv_torques;
        if (FUSED && A.controller == 1 && last && A.ctrl_out) {     // what task.py:288-346 leaves in physics.data.ctrl
#pragma unroll
          for (int a = 0; a < 4; a++) if (a < d_act.y) {
            const int src = __float_as_int(ATAB(d_act.x + a, 2).x);
            const float amp = w_amp[src];
            gptr(A.ctrl_out)[(size_t)env * nu + src] = amp != 0.f ? amp * sinf(cbase - w_lag[src]) : 0.f;
          }
        }
        if (last) {
          float* sa = glob(A.sensordata) + (size_t)env * M.nsensordata + 6 * (nb - 1) + 3 * M.njs;   // actuatorfrc
          if (0 < d_act.y) sa[__float_as_int(ATAB(d_act.x + 0, 2).x)] = af0;
          if (1 < d_act.y) sa[__float_as_int(ATAB(d_act.x + 1, 2).x)] = af1;
          if (2 < d_act.y) sa[__float_as_int(ATAB(d_act.x + 2, 2).x)] = af2;
          if (3 < d_act.y) sa[__float_as_int(ATAB(d_act.x + 3, 2).x)] = af3;
        }
      }
    }
