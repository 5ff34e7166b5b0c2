// fmj_stage_c.inc - step stage shared by fmj_step_kernel (fmj_hip.hip) and fmj_step_wide_kernel (fmj_wide.inc): a block of
// statements on the including kernel's locals.
// C: world-frame inertia of the body about its own CoM.
// reads  blo, isb, xq, any_iquat
// defines iw[6] (xx, yy, zz, xy, xz, yz; zero on lanes without a body)
    float iw[6];     // world-frame inertia about the body's own CoM
    {
      const float4 c_iquat = BTAB(blo, 3);
      const float4 c_inertia = BTAB(blo, 4);
      q4 iq = {c_iquat.x, c_iquat.y, c_iquat.z, c_iquat.w};
      const m33 Ri = q2m(any_iquat ? qmul(xq, iq) : xq);
      const float i0 = c_inertia.x, i1 = c_inertia.y, i2 = c_inertia.z;
      iw[0] = Ri.a[0] * Ri.a[0] * i0 + Ri.a[1] * Ri.a[1] * i1 + Ri.a[2] * Ri.a[2] * i2;
      iw[1] = Ri.a[3] * Ri.a[3] * i0 + Ri.a[4] * Ri.a[4] * i1 + Ri.a[5] * Ri.a[5] * i2;
      iw[2] = Ri.a[6] * Ri.a[6] * i0 + Ri.a[7] * Ri.a[7] * i1 + Ri.a[8] * Ri.a[8] * i2;
      iw[3] = Ri.a[0] * Ri.a[3] * i0 + Ri.a[1] * Ri.a[4] * i1 + Ri.a[2] * Ri.a[5] * i2;
      iw[4] = Ri.a[0] * Ri.a[6] * i0 + Ri.a[1] * Ri.a[7] * i1 + Ri.a[2] * Ri.a[8] * i2;
      iw[5] = Ri.a[3] * Ri.a[6] * i0 + Ri.a[4] * Ri.a[7] * i1 + Ri.a[5] * Ri.a[8] * i2;
      if (!isb) {
#pragma unroll
        for (int k = 0; k < 6; k++) iw[k] = 0.f;
      }
    }
