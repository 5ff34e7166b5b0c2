// fmj_rows_chain.inc - the chain of one constraint row, shared by fmj_cons_rows.inc (one-env kernel) and fmj_cons2_rows.inc
// (two-env constraint kernel), lane = row: a block of statements on the including code's locals.
// The chain's dof at each depth comes from the model's ancestor table (ancl1: byte = 4 * dof of the ancestor at that depth,
// the dof itself beyond its own depth), five words per row instead of a pointer chase of 19 dependent ds_bpermute.  Slots
// beyond the chain name the chain's last dof: J is zero there, so whatever finite value is read is multiplied by 0.
// reads  M, YC, e, isr (the lane's row, if it has one), chain (the row's last dof, -1: no row), QV / XS / QW of the row's env
// defines y[MAXD] (the row of J by depth, read from YC), atab (the chain's dofs, four bytes a word), vel = J qvel,
//         jxs = J qacc_smooth, jqw = J qacc_warmstart, and the macros ANC4 / LDSF, which the includer uses for its walks to
//         the root and #undefs after the last of them
// the includer supplies ROW_ENV(a_): the name under which it holds array a_ of the row's env (QV, XS, QW)
        float y[MAXD];
        {
          const float* yr = YC + (isr ? e : 0) * RS;
#pragma unroll
          for (int g4 = 0; g4 < MAXD / 4; g4++) { const float4 v = *(const float4*)(yr + 4 * g4); y[4 * g4] = v.x; y[4 * g4 + 1] = v.y; y[4 * g4 + 2] = v.z; y[4 * g4 + 3] = v.w; }
        }
#define ANC4(tab_, dd_) ((int)((tab_[(dd_) >> 2] >> (8 * ((dd_) & 3))) & 0xffu))      /* 4 * dof: the byte offset into a float array */
#define LDSF(base_, off4_) (*(const float*)((const char*)(base_) + (off4_)))
        uint32_t atab[MAXD / 4];
        {
          const unsigned crow = (unsigned)(chain < 0 ? 0 : chain) * (MAXD / 4);
#pragma unroll
          for (int g4 = 0; g4 < MAXD / 4; g4++) atab[g4] = gptr(M.ancl1)[crow + g4];
        }
        float vel = 0.f, jxs = 0.f, jqw = 0.f;
#pragma unroll
        for (int dd = 0; dd < MAXD; dd++) {
          const int o4 = ANC4(atab, dd);
          const float j = y[dd];
          vel = fmaf(j, LDSF(ROW_ENV(QV), o4), vel); jxs = fmaf(j, LDSF(ROW_ENV(XS), o4), jxs); jqw = fmaf(j, LDSF(ROW_ENV(QW), o4), jqw);
        }
