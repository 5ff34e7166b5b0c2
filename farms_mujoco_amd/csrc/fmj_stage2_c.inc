// fmj_stage2_c.inc - step stage shared by the two-env kernel (fmj_dual2.inc) and the two-env constraint kernel (fmj_cons2.inc): a block
// of statements on the including kernel's locals.
// C: world-frame inertia of the body about its own CoM.
// reads  c_iquat, c_inertia, xq, any_iquat, isb
// writes iw[6] (declared by the kernel; zero on lanes without a body)
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
