// fmj_stage_carry_in.inc - step stage shared by fmj_step_kernel (fmj_hip.hip) and fmj_step_wide_kernel (fmj_wide.inc): a block of
// statements on the including kernel's locals.
// Before the first step: what the previous launch left for this one.
// reads  dl, bl, isd, isb, env, nb
// defines xf (the caller's xfrc_applied unless the fused drag writes it), cy_actsum (the motor torque of the joints row)
  float xf[6] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f};     // world-frame external force / torque on this body
  float cy_actsum = 0.f;                            // carried motor torque (physics.py:510-524)
  if (FUSED) {
    const float4 dp = DTAB(dl, 1);
    if (isd && dp.w != 0.f) {
      const int4 da = DTABI(dl, 2);
      const float* sa = glob(A.sensordata) + (size_t)env * M.nsensordata + 6 * (nb - 1) + 3 * M.njs;
#pragma unroll
      for (int a = 0; a < 4; a++) if (a < da.y) cy_actsum += sa[__float_as_int(ATAB(da.x + a, 2).x)] * A.inv_torques;
    }
  }
  if (!(FUSED && A.do_drag) && A.xfrc_applied && isb) {
    const float* x = glob(A.xfrc_applied) + (size_t)env * nb * 6 + bl * 6;
#pragma unroll
    for (int k = 0; k < 6; k++) xf[k] = x[k];
  }
