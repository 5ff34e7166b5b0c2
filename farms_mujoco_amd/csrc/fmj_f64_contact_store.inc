// fmj_f64_contact_store.inc - the contact list a step leaves in fmj_data, included by fmj_f64_step.inc where the launch's last step commits
// (the Euler branch; the fourth pass of an RK4 step, after the workgroup's freeze decision): lane = contact writes pos, frame and the
// force in the contact frame (mju_decodePyramid; under the elliptic cone the rows are the frame's axes) and geom1 << 16 | geom2 from
// its registers and its normal in LDS; lane 0 writes ncon
    if (is_c) {
#if F64_STEP_TERRAIN
      const double* cp = TM.tg + (size_t)c_plane * F64_TG;
      float* o = A.contact + ((size_t)env * CM.max_contacts + lane) * 16;
      o[0] = (float)c_pos.x; o[1] = (float)c_pos.y; o[2] = (float)c_pos.z;
      const d3 n = dmk(CN[lane * F64_TN], CN[lane * F64_TN + 1], CN[lane * F64_TN + 2]);
      d3 t1 = dmk(cp[15], cp[16], cp[17]), t2 = dmk(cp[18], cp[19], cp[20]);
      if (cp[14] != 0.0) f64_contact_frame(n, t1, t2);
      o[3] = (float)n.x; o[4] = (float)n.y; o[5] = (float)n.z;
      o[6] = (float)t1.x; o[7] = (float)t1.y; o[8] = (float)t1.z; o[9] = (float)t2.x; o[10] = (float)t2.y; o[11] = (float)t2.z;
#else
      const double* cp = CM.pd + (size_t)c_plane * F64_PD;
      float* o = A.contact + ((size_t)env * CM.max_contacts + lane) * 16;
      o[0] = (float)c_pos.x; o[1] = (float)c_pos.y; o[2] = (float)c_pos.z;
      o[3] = (float)cp[0]; o[4] = (float)cp[1]; o[5] = (float)cp[2];
      for (int k = 0; k < 6; k++) o[6 + k] = (float)cp[6 + k];
#endif
#if F64_STEP_ELLIPTIC
      o[12] = (float)c_f0; o[13] = (float)c_f1; o[14] = (float)c_f2;      // the rows are the frame's axes (oracle export_contacts)
#else
      o[12] = (float)(c_f0 + c_f1 + c_f2 + c_f3); o[13] = (float)(c_mu * (c_f0 - c_f1)); o[14] = (float)(c_mu * (c_f2 - c_f3));
#endif
      o[15] = __int_as_float(((int)cp[13] << 16) | c_geom);
    }
    if (lane == 0) A.ncon[env] = ncon;
