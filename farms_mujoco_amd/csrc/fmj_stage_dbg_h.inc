// fmj_stage_dbg_h.inc - step stage shared by fmj_step_kernel (fmj_hip.hip) and fmj_step_wide_kernel (fmj_wide.inc): a block of
// statements on the including kernel's locals.
// dbg_H dump (fmj_forward_debug).
// reads  hrow, hdg_h, qfrc, ddepth, isd, lane, env, nv
    if (!FUSED && A.dbg_H) {      // fmj_forward_debug: the assembled rows of H and the right-hand side, before any factorisation
      if (isd) {
#pragma unroll
        for (int d = 0; d < MAXD; d++) {
          const float v = (d & 1) ? hrow[d / 2].y : hrow[d / 2].x;
          gptr(A.dbg_H)[((size_t)env * nv + lane) * RS + d] = d < ddepth ? v : (d == ddepth ? hdg_h : 0.f);
        }
        gptr(A.dbg_qfrc)[(size_t)env * nv + lane] = qfrc;
      }
    }
