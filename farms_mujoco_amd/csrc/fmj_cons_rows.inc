// fmj_cons_rows.inc - constraint rows, PGS and constraint forces of the one-env kernel (included twice by
// fmj_hip.hip inside fmj_step_kernel<.., CONS = true>): once with YC / EP in LDS and `small` = true (<= LL.na rows,
// A in registers), once with YC / EP in the per-env HBM scratch and `small` = false.  Including the code twice keeps
// every access in its own address space: no flat pointers, and the branch on `small` folds away in each copy.
// Rows of explicit geom-pair contacts (both bodies move) have a second part, the FORK: the first body's branch of the tree
// beyond the deepest dof both bodies share, kept in YF (row e - e_p0) with its chain end in CHF; `hasp` (uniform) says
// that the env has such rows, every fork block is skipped otherwise.
      uint8_t* CHN = (uint8_t*)CH;
      uint8_t* CHF = (uint8_t*)CF;
      const int8_t* LCB0 = (const int8_t*)LC;
      const bool haspx = !small && hasp;       // envs with an active pair contact take the HBM copy of this code: the on-chip copy has no fork code
      // Primal solvers and explicit pairs.  The reference declares its self-collision pairs with friction 0 (mjcf.py:1026: mjMINMU = 1e-5
      // after MuJoCo's clamp), so their pyramid rows carry R = 2 mu^2 R0 ~ 1e-10 R0: a force of 1 N is a residual J qacc - aref of 1e-11,
      // far below what fp32 can resolve next to the terms of that sum - no fp32 primal iteration can find it.  The dual variables have
      // no such scale, so an env whose step has an ACTIVE pair contact is solved by PGS on the dual problem, run to the solver's
      // tolerance (up to 10 x solver_iterations sweeps): the same convex problem, the same minimiser (tests/test_oracle_solvers.py holds
      // the two to 1e-8 in fp64).  Every other env of the batch takes the solver that was asked for - except that in a model with
      // pairs the whole HBM copy of this code is the dual one (so also an env with more rows than the chip holds): with both solvers
      // in it that copy spilled 260 VGPRs and the common path paid 13 KB of scratch traffic per env-step for it.
      constexpr bool primal = NEWTON && !(PAIRS && !small);
#define RSYNC() do { if (!small) __threadfence(); WSYNC(); } while (0)
      for (int i = lane; i < nefc * RS; i += 64) YC[i] = 0.f;
      if (haspx) {
        for (int i = lane; i < (nefc - e_p0) * RS; i += 64) YF[i] = 0.f;
        for (int i = lane; i < nefc; i += 64) CHF[i] = 0;
      }
      RSYNC();
      if (act_lo) { YC[e_lo * RS + ddepth] = 1.f;  CHN[e_lo] = (uint8_t)(lane + 1); float* ep = EP + e_lo * 8; ep[0] = dist_lo; ep[1] = lim.w; ep[6] = __int_as_float(lane); ep[7] = 0.f; }
      if (act_hi) { YC[e_hi * RS + ddepth] = -1.f; CHN[e_hi] = (uint8_t)(lane + 1); float* ep = EP + e_hi * 8; ep[0] = dist_hi; ep[1] = lim.w; ep[6] = __int_as_float(lane); ep[7] = 0.f; }
      {
        const s6 cd = isd ? lds_get6(CD + lane * 8) : s6{mk3(0.f, 0.f, 0.f), mk3(0.f, 0.f, 0.f)};
        for (int c = 0; c < ncon; c++) {
          const float* ct = CT + c * 16;
          const float4 c0 = *(const float4*)(ct), c1 = *(const float4*)(ct + 4), c2 = *(const float4*)(ct + 8), c3 = *(const float4*)(ct + 12);
          const int last = (__float_as_int(c3.z) >> 16) - 1;    // last dof on the contact body's chain (packed next to the geom at the collision stage)
          const bool on = isd && last >= 0 && lane <= last && last < lane + dsub;
          // explicit pair: the first geom's body moves too, J = J(body2) - J(body1); the dofs both chains share cancel
          const int last1 = c >= ncg ? GTABI(__float_as_int(c3.w) & 0xffff, 0).z : -1;
          const bool on1 = isd && last1 >= 0 && lane <= last1 && last1 < lane + dsub;
          if (on != on1) {
            const v3 jp = add3(cd.l, cross(cd.r, sub3(mk3(c0.x, c0.y, c0.z), com)));
            const float sg = on ? 1.f : -1.f;
            const float jn = sg * dot3(jp, mk3(c0.w, c1.x, c1.y));
            const float j1 = sg * c3.y * dot3(jp, mk3(c1.z, c1.w, c2.x));
            const float j2 = sg * c3.y * dot3(jp, mk3(c2.y, c2.z, c2.w));
            float* y = (on ? YC + (nlim + crs * c) * RS : YF + (nlim + crs * c - e_p0) * RS) + ddepth;
            if (crs == 3) {                 // elliptic (mj_instantiateContact): the rows are the axes of the contact frame
              y[0] = jn; y[RS] = sg * dot3(jp, mk3(c1.z, c1.w, c2.x)); y[2 * RS] = sg * dot3(jp, mk3(c2.y, c2.z, c2.w));
            } else { y[0] = jn + j1; y[RS] = jn - j1; y[2 * RS] = jn + j2; y[3 * RS] = jn - j2; }
          }
          if (lane < crs) {
            CHN[nlim + crs * c + lane] = (uint8_t)(last + 1);
            if (c >= ncg) CHF[nlim + crs * c + lane] = (uint8_t)(last1 + 1);
            float* ep = EP + (nlim + crs * c + lane) * 8; ep[0] = (crs == 4 || lane == 0) ? c3.x : 0.f;   // elliptic friction rows: pos = margin = 0
            ep[1] = 0.f; ep[6] = __int_as_float(0x40000000 | c); ep[7] = c3.y;
          }
        }
      }
      RSYNC();
      STAMP(14);  // J rows
      // (5) per row (lane = row, 64 rows per pass): R, aref (mj_makeImpedance / mj_referenceConstraint),
      //     b = J qacc_smooth - aref, warm-start jar from the previous qacc (mj_fwdConstraint), then
      // (6) Z = J L^-1 D^-1/2 with the row in registers: walking the chain from its last dof i to the root,
      //     y[dd2] -= L[i][dd2] y[depth(i)] for dd2 < depth(i); A = J M^-1 J' = Z Z'.
      for (int e0 = 0; e0 < nefc; e0 += 64) {
        const int e = e0 + lane;
        const bool isr = e < nefc;
        float* ep = EP + (isr ? e : 0) * 8;
        const int tid = __float_as_int(ep[6]);
        const bool is_con = (tid & 0x40000000) != 0;
        const int chain = isr ? (int)CHN[e] - 1 : -1;
        float sr0, sr1, si0, si1, si2, si3, si4, dapx;
        const float mu = ep[7];
        if (is_con) {
          const float4 c3 = *(const float4*)(CT + (tid & 0xff) * 16 + 12);
          const int g = __float_as_int(c3.z) & 0xffff;
          const int gp = __float_as_int(c3.w);                   // ground contact: the ground geom; pair: geom1 | (pair + 1) << 16
          const bool is_pair = (tid & 0xff) >= ncg;
          float4 a = GTAB(g, 4), b = GTAB(g, 5);
          float tran = GTAB(g, 2).w;                             // invweight0 of the body (+ 0 for the world's ground)
          if (is_pair) { const int pr = (gp >> 16) - 1; a = QTAB(pr, 1); b = QTAB(pr, 2); tran += GTAB(gp & 0xffff, 2).w; }
          sr0 = a.x; sr1 = a.y; si0 = a.z; si1 = a.w; si2 = b.x; si3 = b.y; si4 = b.z;
          dapx = crs == 4 ? tran + mu * mu * tran : tran;
        } else {
          const float4 a = DTAB(tid & 0xff, 4), b = DTAB(tid & 0xff, 5);
          sr0 = a.x; sr1 = a.y; si0 = a.z; si1 = a.w; si2 = b.x; si3 = b.y; si4 = b.z; dapx = b.w;
        }
        float R, kimp, bb;
        row_params(sr0, sr1, si0, si1, si2, si3, si4, ep[0], ep[1], dapx, h, &R, &kimp, &bb);
#define ROW_ENV(a_) a_
#include "fmj_rows_chain.inc"      // y: the row of J by depth; ANC4, LDSF, atab: the chain's dof at each depth; vel, jxs, jqw
#undef ROW_ENV
        // fork part of a pair row: the first body's chain beyond lcae, the depth of the deepest dof both chains share
        const int fchain = (haspx && isr && e >= e_p0) ? (int)CHF[e] - 1 : -1;
        const int lcae = (fchain >= 0 && chain >= 0) ? (int)LCB0[chain * nv + fchain] : -1;
        if (haspx) {       // everything the fork needs lives and dies inside this block: the rows without a fork keep the register budget
          // the row of the main part is NOT held in registers across this block (it is re-read below): what the fork adds to the
          // main part's shared depths is collected in ycor and added to the stored row
          float yf[MAXD], ycor[MAXD];
#pragma unroll
          for (int dd = 0; dd < MAXD; dd++) { yf[dd] = 0.f; ycor[dd] = 0.f; }
          if (fchain >= 0) {
            const float* yr = YF + (e - e_p0) * RS;
#pragma unroll
            for (int g4 = 0; g4 < MAXD / 4; g4++) { const float4 v = *(const float4*)(yr + 4 * g4); yf[4 * g4] = v.x; yf[4 * g4 + 1] = v.y; yf[4 * g4 + 2] = v.z; yf[4 * g4 + 3] = v.w; }
          }
          uint32_t ftab[MAXD / 4];       // the fork chain's dofs (shared depths <= lcae carry yf = 0)
          {
            const unsigned frow = (unsigned)(fchain < 0 ? 0 : fchain) * (MAXD / 4);
#pragma unroll
            for (int g4 = 0; g4 < MAXD / 4; g4++) ftab[g4] = gptr(M.ancl1)[frow + g4];
          }
#pragma unroll
          for (int dd = 0; dd < MAXD; dd++) {
            const int o4 = ANC4(ftab, dd);
            const float j = yf[dd];
            vel = fmaf(j, LDSF(QV, o4), vel); jxs = fmaf(j, LDSF(XS, o4), jxs); jqw = fmaf(j, LDSF(QW, o4), jqw);
          }
          // the fork's dofs first (none of them is an ancestor of a dof of the main branch below lcae): their ancestors are
          // the fork's own dofs above them and, from lcae up, the dofs both chains share, which live in the main part
          // (PGS only: Newton / CG keep the rows of J)
          if (!primal) {
#pragma unroll
          for (int dd = MAXD - 1; dd >= 1; dd--) {
            const float yi = yf[dd];
            const float* lr = (const float*)((const char*)HM + ANC4(ftab, dd) * RS);
#pragma unroll
            for (int g4 = 0; g4 < (dd + 3) / 4; g4++) {
              const float4 l4 = *(const float4*)(lr + 4 * g4);
#pragma unroll
              for (int k = 0; k < 4; k++) {
                const int sl_ = 4 * g4 + k;
                if (sl_ < dd) {
                  const float lv = (k == 0 ? l4.x : k == 1 ? l4.y : k == 2 ? l4.z : l4.w) * yi;
                  yf[sl_] = sl_ > lcae ? yf[sl_] - lv : yf[sl_];
                  ycor[sl_] = sl_ <= lcae ? ycor[sl_] - lv : ycor[sl_];
                }
              }
            }
          }
#pragma unroll
          for (int dd = 0; dd < MAXD; dd++) yf[dd] *= LDSF(SD, ANC4(ftab, dd));
          if (fchain >= 0) {
            float* yr2 = YF + (e - e_p0) * RS;
#pragma unroll
            for (int g4 = 0; g4 < MAXD / 4; g4++) *(float4*)(yr2 + 4 * g4) = make_float4(yf[4 * g4], yf[4 * g4 + 1], yf[4 * g4 + 2], yf[4 * g4 + 3]);
            float* yr1 = YC + e * RS;                  // the lane's own row: no other lane touches it
#pragma unroll
            for (int g4 = 0; g4 < MAXD / 4; g4++) {
              const float4 v = *(const float4*)(yr1 + 4 * g4);
              *(float4*)(yr1 + 4 * g4) = make_float4(v.x + ycor[4 * g4], v.y + ycor[4 * g4 + 1], v.z + ycor[4 * g4 + 2], v.w + ycor[4 * g4 + 3]);
            }
          }
          }
        }
        const float aref = -bb * vel - kimp * (ep[0] - ep[1]);
        if (PAIRS && haspx) {                           // the row again, with what the fork added to it
          const float* yr = YC + (isr ? e : 0) * RS;
#pragma unroll
          for (int g4 = 0; g4 < MAXD / 4; g4++) { const float4 v = *(const float4*)(yr + 4 * g4); y[4 * g4] = v.x; y[4 * g4 + 1] = v.y; y[4 * g4 + 2] = v.z; y[4 * g4 + 3] = v.w; }
        }
        if (!primal) {                                 // PGS works on Z = J L^-1 D^-1/2; Newton keeps the rows of J
#pragma unroll
        for (int dd = MAXD - 1; dd >= 1; dd--) {
          const float yi = y[dd];
          const float* lr = (const float*)((const char*)HM + ANC4(atab, dd) * RS);
#pragma unroll
          for (int g4 = 0; g4 < (dd + 3) / 4; g4++) {
            const float4 l4 = *(const float4*)(lr + 4 * g4);
            if (4 * g4 + 0 < dd) y[4 * g4 + 0] = fmaf(-l4.x, yi, y[4 * g4 + 0]);
            if (4 * g4 + 1 < dd) y[4 * g4 + 1] = fmaf(-l4.y, yi, y[4 * g4 + 1]);
            if (4 * g4 + 2 < dd) y[4 * g4 + 2] = fmaf(-l4.z, yi, y[4 * g4 + 2]);
            if (4 * g4 + 3 < dd) y[4 * g4 + 3] = fmaf(-l4.w, yi, y[4 * g4 + 3]);
          }
        }
#pragma unroll
        for (int dd = 0; dd < MAXD; dd++) y[dd] *= LDSF(SD, ANC4(atab, dd));
        }
#undef ANC4
#undef LDSF
        if (isr) {
          if (!primal) {
            float* yr = YC + e * RS;
#pragma unroll
            for (int g4 = 0; g4 < MAXD / 4; g4++) *(float4*)(yr + 4 * g4) = make_float4(y[4 * g4], y[4 * g4 + 1], y[4 * g4 + 2], y[4 * g4 + 3]);
          }
          ep[1] = aref; ep[2] = R; ep[3] = jxs - aref; ep[4] = jqw - aref; ep[5] = R;   // ep[4]: jar for the warm start; ep[5]: R before the pyramidal fix
        }
      }
      RSYNC();
      // pyramidal: the 4 rows of a contact share R = 2 mu^2 R_first (mu scaled by 1/sqrt(impratio))
      for (int e = lane; e < nefc; e += 64) {
        float* ep = EP + e * 8;
        const int tid = __float_as_int(ep[6]);
        if (tid & 0x40000000) {
          const int e0 = nlim + crs * (tid & 0xff);
          const float mu = ep[7] * M.impratio_isqrt;
          if (crs == 4) ep[2] = fmaxf(1e-15f, 2.f * mu * mu * EP[e0 * 8 + 5]);
          else if (e != e0) ep[2] = fmaxf(1e-15f, EP[e0 * 8 + 5] * M.impratio_isqrt * M.impratio_isqrt);   // elliptic: R_normal mu^2 / friction^2, mu = friction / sqrt(impratio)
        }
        if (!primal && !(crs == 3 && (tid & 0x40000000))) { const float jar = ep[4]; ep[4] = jar < 0.f ? -jar / ep[2] : 0.f; }      // PGS: warm-start force; Newton keeps jar = J qacc_warmstart - aref
      }
      RSYNC();
      if (crs == 3 && !primal) {      // PGS with elliptic cones: the warm-start forces of a contact are its cone's at the warm-start residuals (mj_constraintUpdate)
        for (int c = lane; c < ncon; c += 64) {
          float* e0 = EP + (nlim + 3 * c) * 8;
          float f0, f1, f2;
          ell_zone_forces(e0[4], e0[12], e0[20], 1.0f / e0[2], e0[7], M.impratio_isqrt, &f0, &f1, &f2);
          e0[4] = f0; e0[12] = f1; e0[20] = f2;
        }
        RSYNC();
      }
      STAMP(16);  // row params + Z
      float w = 0.f;
      if (primal) {
#include "fmj_newton.inc"
      } else {
      if (small) {
        // (7a) explicit A = Z Z' + diag(R), lane = row: lane j keeps row j of A in FMJ_NA registers (A is symmetric, so
        //      this is also column j).  Rows e and f couple through the dofs their chains share.
        const bool isr = lane < nefc;
        const int je = isr ? lane : 0;
        const int chain = isr ? (int)CHN[je] - 1 : -1;
        const int fchain = (haspx && isr && je >= e_p0) ? (int)CHF[je] - 1 : -1;
        float areg[FMJ_NA];
        {
          // on the matrix cores, by the text the two-env kernel's SOLO mode runs (fmj_cons2_rows.inc (7)): an env gets the same A from either kernel
          const int8_t* LCB = (const int8_t*)LC;
#define MFMA_A_NEFC nefc
#include "fmj_rows_mfma_a.inc"      // areg = the lane's row of Z Z'
#undef MFMA_A_NEFC
#undef ZOP
#undef SWAP32
          const float Rj = isr ? EP[je * 8 + 2] : 0.f;
#pragma unroll
          for (int f = 0; f < FMJ_NA; f++) areg[f] += (f == lane && isr) ? Rj : 0.f;
        }
        STAMP(17);  // A
        // warm start: keep it only if its dual cost beats f = 0 (mj_fwdConstraint)
        float fj = isr ? EP[je * 8 + 4] : 0.f;
        const float bj = isr ? EP[je * 8 + 3] : 0.f;
        float diag = 1.f;                                            // A_jj + R_j: the lane's own column of its row
#pragma unroll
        for (int f = 0; f < FMJ_NA; f++) diag = (f == lane && isr) ? areg[f] : diag;
        const float ainv = 1.0f / diag;
        float afj = 0.f;
        {
          const int nefc_w = opaque_s(nefc);
#pragma unroll
          for (int k = 0; k < FMJ_NA; k++) if (k < nefc_w) afj = fmaf(areg[k], bcast(fj, k), afj);
        }
        {
          const float cost = wave_sum_fast(fj * (0.5f * afj + bj));
          if (cost > 0.f) { fj = 0.f; afj = 0.f; }
        }
        float res = bj + afj;                                        // residual of row j: b + (A + R) f
        STAMP(18);  // warm start
        // (8a) PGS on the explicit matrix (mj_solPGS: rows in order, f_e <- max(0, f_e - res_e / A_ee)).  Every lane
        //      keeps the update its own row would make from its current residual (delta_j = max(-f_j, -res_j / A_jj));
        //      row e's turn is then one v_readlane of that value and one FMA of every residual with the lane's
        //      register e: no reduction, no LDS, no address arithmetic, a dependent chain of 4 VALU ops per row.
        //      mj_solPGS reverts a row whose cost change delta * (0.5 A_ee delta + res) exceeds 1e-10; for these scalar
        //      rows the two factors never have the same sign, in floating point too (delta = -res/A_ee gives
        //      t = res/2; the clamped delta = -f gives t >= res/2 > 0), so the revert cannot fire and is not
        //      evaluated; the product still feeds the improvement that stops the sweeps.
        const float hdiag = 0.5f * diag;
        const float nainv = -ainv;
        float nf = -fj;
        // The sweep works on the scaled residual r_j = -res_j / A_jj (the unclamped update of row j): the lane's
        // registers are scaled by -1 / A_jj once per step, so a row costs v_max (its update), v_cndmask (lane e keeps
        // the r it was made from), v_readlane and one FMA of every lane's r with its register e.
#pragma unroll
        for (int k = 0; k < FMJ_NA; k++) areg[k] *= nainv;
        res *= nainv;
        // Rows past nefc are no-ops by construction (their lanes hold r = 0, f = 0 and a zero row), so the sweep is
        // straight-line code for the next multiple of 12 rows: static register indices, one branch per step.
#define PGS_SWEEPS(NR_) \
        for (int itp = 0; itp < M.solver_iterations; itp++) { \
          float capr = 0.f;                 /* lane e: the scaled residual its own row's update was made from */ \
          _Pragma("unroll") for (int e = 0; e < NR_; e++) { \
            /* the turn as ONE asm block (round 5; see fmj_cons2_rows.inc): v_max (no NaN canonicalisation), lane e's bit made where it is used (60 hoisted \
               masks were 120 SGPRs, all spilled), v_readlane, the capture in the shadow of the v_readlane -> v_fmac wait, one s_nop, v_fmac */ \
            float cand_, upd_; unsigned long long bit_; \
            asm volatile("v_max_f32_e32 %[cand], %[nf], %[res]\n\t" \
                         "s_lshl_b64 %[bit], 1, %[e]\n\t" \
                         "v_readlane_b32 %[sa], %[cand], %[e]\n\t" \
                         "v_cndmask_b32_e64 %[capr], %[capr], %[res], %[bit]\n\t" \
                         "s_nop 0\n\t" \
                         "v_fmac_f32_e32 %[res], %[sa], %[a0]" \
                         : [cand] "=&v"(cand_), [bit] "=&s"(bit_), [sa] "=&s"(upd_), [capr] "+v"(capr), [res] "+v"(res) \
                         : [nf] "v"(nf), [e] "n"(e), [a0] "v"(areg[e]) : "scc"); \
          } \
          float capc; asm("v_max_f32_e32 %0, %1, %2" : "=v"(capc) : "v"(nf), "v"(capr));   /* the update row j made */ \
          capc = isr ? capc : 0.f; \
          nf -= capc;                                                 /* f_j += delta_j */ \
          const float imp = capc * fmaf(hdiag, capc, -diag * capr);   /* cost change of row j = delta (0.5 A_jj delta + res) */ \
          const float improvement = -wave_sum_fast(imp); \
          if (!FUSED && A.dbg_pgs && lane == 0) gptr(A.dbg_pgs)[(size_t)env * M.solver_iterations + itp] = improvement; \
          if (improvement * M.pgs_scale < M.solver_tolerance) break; \
        }
        // one instantiation per 4 rows (a contact's pyramid): walking has 16 .. 48 rows, median 24 (blocks of 12 wasted ~15 % of the sweep)
        switch ((nefc + 3) >> 2) {
          case 0: case 1: case 2: PGS_SWEEPS(8) break;
          case 3: PGS_SWEEPS(12) break;
          case 4: PGS_SWEEPS(16) break;
          case 5: PGS_SWEEPS(20) break;
          case 6: PGS_SWEEPS(24) break;
          case 7: PGS_SWEEPS(28) break;
          case 8: PGS_SWEEPS(32) break;
          case 9: PGS_SWEEPS(36) break;
          case 10: PGS_SWEEPS(40) break;
          case 11: PGS_SWEEPS(44) break;
          case 12: PGS_SWEEPS(48) break;
          case 13: PGS_SWEEPS(52) break;
          case 14: PGS_SWEEPS(56) break;
          case 15: PGS_SWEEPS(60) break;
          default: PGS_SWEEPS(FMJ_NA) break;
        }
#undef PGS_SWEEPS
        fj = -nf;
        if (isr) EP[je * 8 + 4] = fj;
        if (isd) {
          int e = 0;
          for (; e + 4 <= nefc; e += 4) {                   // four rows at a time: their LDS reads are issued together
            float yv[4]; int ce[4];
#pragma unroll
            for (int u = 0; u < 4; u++) { yv[u] = YC[(e + u) * RS + ddepth]; ce[u] = (int)CHN[e + u] - 1; }
#pragma unroll
            for (int u = 0; u < 4; u++) w = fmaf((lane <= ce[u] && ce[u] < lane + dsub) ? yv[u] : 0.f, bcast(fj, e + u), w);
          }
          for (; e < nefc; e++) {
            const int ce = (int)CHN[e] - 1;
            const bool on = lane <= ce && ce < lane + dsub;
            w = fmaf(on ? YC[e * RS + ddepth] : 0.f, bcast(fj, e), w);
          }
          w *= sqrtf(dinv_m);
        }
        WSYNC();
      } else {
        // (7b) more rows than the LDS matrix holds: A = Z Z' + diag(R) goes to the global scratch, full rows of
        //      AG_LD floats (row f is written by the lanes that own rows e: A is symmetric, so the stores coalesce),
        //      and each lane owns up to three rows (e = lane + 64 s).
        float* AG = M.cons_a + (size_t)env * M.maxefc * AG_LD;
        const int ns = (nefc + 63) >> 6;
        const int8_t* LCB = (const int8_t*)LC;
        for (int c0 = 0; c0 < nefc; c0 += LL.na) {       // columns c0 .. c0 + nc - 1: their rows of Z are staged in LDS
          const int nc = nefc - c0 < LL.na ? nefc - c0 : LL.na;
          WSYNC();
          for (int i = lane; i < nc * RS; i += 64) YJ[i] = YC[c0 * RS + i];
          WSYNC();
          for (int sl = 0; sl < ns; sl++) {
            const int e = 64 * sl + lane;
            const bool isr = e < nefc;
            const int chain = isr ? (int)CHN[e] - 1 : -1;
            const int fchain = (haspx && isr && e >= e_p0) ? (int)CHF[e] - 1 : -1;
            const float Rj = isr ? EP[e * 8 + 2] : 0.f;
            float zr[MAXD], zm[MAXD];
            {
              const float* yr = YC + (isr ? e : 0) * RS;
#pragma unroll
              for (int g4 = 0; g4 < MAXD / 4; g4++) { const float4 v = *(const float4*)(yr + 4 * g4); zr[4 * g4] = v.x; zr[4 * g4 + 1] = v.y; zr[4 * g4 + 2] = v.z; zr[4 * g4 + 3] = v.w; }
            }
#pragma unroll
            for (int dd = 0; dd < MAXD; dd++) zm[dd] = 0.f;
            int cprev = -2;
            if (!haspx) {
            for (int f = 0; f < nc; f++) {
              const int cf = (int)CHN[c0 + f] - 1;
              if (cf != cprev) {
                cprev = cf;
                const int l = (cf >= 0 && chain >= 0) ? (int)LCB[chain * nv + cf] : -1;
#pragma unroll
                for (int dd = 0; dd < MAXD; dd++) zm[dd] = dd <= l ? zr[dd] : 0.f;
              }
              const float* yf = YJ + f * RS;
              float a0 = 0.f, a1 = 0.f, a2 = 0.f, a3 = 0.f;
#pragma unroll
              for (int g4 = 0; g4 < MAXD / 4; g4++) {
                const float4 v = *(const float4*)(yf + 4 * g4);
                a0 = fmaf(zm[4 * g4], v.x, a0); a1 = fmaf(zm[4 * g4 + 1], v.y, a1); a2 = fmaf(zm[4 * g4 + 2], v.z, a2); a3 = fmaf(zm[4 * g4 + 3], v.w, a3);
              }
              AG[(size_t)(c0 + f) * AG_LD + 64 * sl + lane] = (a0 + a1) + (a2 + a3) + (c0 + f == e ? Rj : 0.f);
            }
            } else {     // rows with fork parts (see the on-chip variant); the fork part of a column is read from the scratch
            float zrf[MAXD], zm2[MAXD];
#pragma unroll
            for (int dd = 0; dd < MAXD; dd++) { zrf[dd] = 0.f; zm2[dd] = 0.f; }
            if (fchain >= 0) {
              const float* yr = YF + (e - e_p0) * RS;
#pragma unroll
              for (int g4 = 0; g4 < MAXD / 4; g4++) { const float4 v = *(const float4*)(yr + 4 * g4); zrf[4 * g4] = v.x; zrf[4 * g4 + 1] = v.y; zrf[4 * g4 + 2] = v.z; zrf[4 * g4 + 3] = v.w; }
            }
            int fprev = -2;
            for (int f = 0; f < nc; f++) {
              const int cf = (int)CHN[c0 + f] - 1;
              const int cff = c0 + f >= e_p0 ? (int)CHF[c0 + f] - 1 : -1;
              if (cf != cprev || cff != fprev) {
                cprev = cf; fprev = cff;
                const int l1 = (cf >= 0 && chain >= 0) ? (int)LCB[chain * nv + cf] : -1;
                const int l3 = (cf >= 0 && fchain >= 0) ? (int)LCB[fchain * nv + cf] : -1;
                const int l2 = (cff >= 0 && chain >= 0) ? (int)LCB[chain * nv + cff] : -1;
                const int l4 = (cff >= 0 && fchain >= 0) ? (int)LCB[fchain * nv + cff] : -1;
#pragma unroll
                for (int dd = 0; dd < MAXD; dd++) {
                  zm[dd] = (dd <= l1 ? zr[dd] : 0.f) + (dd <= l3 ? zrf[dd] : 0.f);
                  zm2[dd] = (dd <= l2 ? zr[dd] : 0.f) + (dd <= l4 ? zrf[dd] : 0.f);
                }
              }
              float a0 = 0.f, a1 = 0.f, a2 = 0.f, a3 = 0.f;
              {
                const float* yf = YJ + f * RS;
#pragma unroll
                for (int g4 = 0; g4 < MAXD / 4; g4++) {
                  const float4 v = *(const float4*)(yf + 4 * g4);
                  a0 = fmaf(zm[4 * g4], v.x, a0); a1 = fmaf(zm[4 * g4 + 1], v.y, a1); a2 = fmaf(zm[4 * g4 + 2], v.z, a2); a3 = fmaf(zm[4 * g4 + 3], v.w, a3);
                }
              }
              if (cff >= 0) {
                const float* yf2 = YF + (c0 + f - e_p0) * RS;
#pragma unroll
                for (int g4 = 0; g4 < MAXD / 4; g4++) {
                  const float4 v = *(const float4*)(yf2 + 4 * g4);
                  a0 = fmaf(zm2[4 * g4], v.x, a0); a1 = fmaf(zm2[4 * g4 + 1], v.y, a1); a2 = fmaf(zm2[4 * g4 + 2], v.z, a2); a3 = fmaf(zm2[4 * g4 + 3], v.w, a3);
                }
              }
              AG[(size_t)(c0 + f) * AG_LD + 64 * sl + lane] = (a0 + a1) + (a2 + a3) + (c0 + f == e ? Rj : 0.f);
            }
            }
          }
        }
        __threadfence();
        WSYNC();
        STAMP(17);  // A
        // The block solvers below (elliptic PGS, noslip) keep the forces, b, R and mu of every row in LDS - FL / BL / RL / ML overlay the staging
        // area of (7b), free again (fmj_create checks that it holds 4 maxefc floats) - so that an update costs a wave barrier, not a memory
        // fence; A is read-only by now.  (A f)_e at the forces as they stand, the same number in every lane (A is symmetric: row e is read
        // as a contiguous run).
        float* const FL = YJ; float* const BL = YJ + M.maxefc; float* const RL = YJ + 2 * M.maxefc; float* const ML = YJ + 3 * M.maxefc;
        auto rows_to_lds = [&]() {
          WSYNC();
          for (int e = lane; e < nefc; e += 64) { FL[e] = EP[e * 8 + 4]; BL[e] = EP[e * 8 + 3]; RL[e] = EP[e * 8 + 2]; ML[e] = EP[e * 8 + 7]; }
          WSYNC();
        };
        auto forces_to_rows = [&]() {
          WSYNC();
          for (int e = lane; e < nefc; e += 64) EP[e * 8 + 4] = FL[e];
        };
        auto row_dot = [&](const int e) {
          float p_ = 0.f;
          for (int k = lane; k < nefc; k += 64) p_ = fmaf(AG[(size_t)e * AG_LD + k], FL[k], p_);
          return wave_sum_fast(p_);
        };
        if (crs == 3) {
          // (8c) PGS with ELLIPTIC cones (mj_solPGS; oracle: solve_constraints + pgs_elliptic_block).  Limit rows are scalar updates; a
          //      contact's three rows move together: first along the ray of their own force vector (or, from f_n = 0, the normal alone),
          //      then the friction forces solve their QCQP inside the cone of the new normal force.  The forces stay in EP; every lane
          //      computes the (uniform) update, lane 0 stores it.  One block costs three row products with A: an order of magnitude
          //      more than a pyramid's four scalar rows on chip - this is the rare option, the walk's default is the pyramid.
          rows_to_lds();
          {     // warm start: keep it only if its dual cost beats f = 0 (mj_fwdConstraint)
            float cst = 0.f;
            for (int e = lane; e < nefc; e += 64) {
              float s_ = 0.f;
              for (int k = 0; k < nefc; k++) s_ = fmaf(AG[(size_t)e * AG_LD + k], FL[k], s_);
              cst += FL[e] * (0.5f * s_ + BL[e]);
            }
            cst = wave_sum_fast(cst);
            WSYNC();
            if (cst > 0.f) for (int e = lane; e < nefc; e += 64) FL[e] = 0.f;
            WSYNC();
          }
          for (int itp = 0; itp < M.solver_iterations; itp++) {
            float improvement = 0.f;
            for (int e = 0; e < nefc;) {
              if (e < nlim) {
                const float Aee = AG[(size_t)e * AG_LD + e];
                const float res = BL[e] + row_dot(e);
                const float old = FL[e];
                float f = fmaxf(0.f, old - res / Aee);
                const float dl = f - old;
                float change = 0.5f * dl * dl * Aee + dl * res;
                if (change > 1e-10f) { f = old; change = 0.f; }
                WSYNC();
                if (lane == 0) FL[e] = f;
                WSYNC();
                improvement -= change;
                e++;
                continue;
              }
              const float r0 = BL[e] + row_dot(e), r1 = BL[e + 1] + row_dot(e + 1), r2 = BL[e + 2] + row_dot(e + 2);
              const float* a0_ = AG + (size_t)e * AG_LD + e; const float* a1_ = a0_ + AG_LD; const float* a2_ = a1_ + AG_LD;
              const float A00 = a0_[0], A01 = a0_[1], A02 = a0_[2], A11 = a1_[1], A12 = a1_[2], A22 = a2_[2];
              const float o0 = FL[e], o1 = FL[e + 1], o2 = FL[e + 2], mu = ML[e];
              float f0 = o0, f1 = o1, f2 = o2;
              if (f0 < 1e-15f) { f0 = fmaxf(0.f, f0 - r0 / A00); f1 = 0.f; f2 = 0.f; }
              else {
                const float w0 = A00 * o0 + A01 * o1 + A02 * o2, w1 = A01 * o0 + A11 * o1 + A12 * o2, w2 = A02 * o0 + A12 * o1 + A22 * o2;
                const float denom = o0 * w0 + o1 * w1 + o2 * w2, num = o0 * r0 + o1 * r1 + o2 * r2;
                if (denom >= 1e-15f) {
                  float x = -num / denom;
                  if (o0 + x * o0 < 0.f) x = -1.f;
                  f0 = fmaf(x, o0, o0); f1 = fmaf(x, o1, o1); f2 = fmaf(x, o2, o2);
                }
              }
              if (f0 < 1e-15f) { f1 = 0.f; f2 = 0.f; }
              else {
                const float bc1 = r1 - A11 * o1 - A12 * o2 + A01 * (f0 - o0), bc2 = r2 - A12 * o1 - A22 * o2 + A02 * (f0 - o0);
                float x1, x2;
                if (qcqp2_dev(A11, A12, A22, bc1, bc2, mu, f0, &x1, &x2)) {
                  float sv = (x1 / mu) * (x1 / mu) + (x2 / mu) * (x2 / mu);
                  sv = sqrtf(f0 * f0 / fmaxf(1e-15f, sv));
                  x1 *= sv; x2 *= sv;
                }
                f1 = x1; f2 = x2;
              }
              const float d0 = f0 - o0, d1 = f1 - o1, d2 = f2 - o2;
              float change = d0 * r0 + d1 * r1 + d2 * r2
                           + 0.5f * (d0 * (A00 * d0 + A01 * d1 + A02 * d2) + d1 * (A01 * d0 + A11 * d1 + A12 * d2) + d2 * (A02 * d0 + A12 * d1 + A22 * d2));
              if (change > 1e-10f) { f0 = o0; f1 = o1; f2 = o2; change = 0.f; }
              WSYNC();
              if (lane == 0) { FL[e] = f0; FL[e + 1] = f1; FL[e + 2] = f2; }
              WSYNC();
              improvement -= change;
              e += 3;
            }
            if (!FUSED && A.dbg_pgs && lane == 0) gptr(A.dbg_pgs)[(size_t)env * M.solver_iterations + itp] = improvement;
            if (improvement * M.pgs_scale < M.solver_tolerance) break;
          }
          forces_to_rows();
        } else {
        // per-lane row state (slot s = row lane + 64 s)
        float res[3], nf[3], nainv[3], hdiag[3], bj[3];
#pragma unroll
        for (int sl = 0; sl < 3; sl++) {
          const int e = 64 * sl + lane;
          const bool isr = e < nefc;
          const float dg = isr ? AG[(size_t)e * AG_LD + e] : 1.f;
          bj[sl] = isr ? EP[e * 8 + 3] : 0.f;
          res[sl] = bj[sl]; nf[sl] = 0.f; nainv[sl] = -1.0f / dg; hdiag[sl] = 0.5f * dg;
        }
        // one pass over the rows: mode 0 applies the warm-start forces as given deltas (builds res = b + (A + R) f),
        // mode 1 is a PGS sweep.  Rows of A are fetched PB rows ahead of their use.
        constexpr int PB = 8;
        float imp = 0.f;
        float fw[3];
#pragma unroll
        for (int sl = 0; sl < 3; sl++) { const int e = 64 * sl + lane; fw[sl] = e < nefc ? EP[e * 8 + 4] : 0.f; }
        const int nsweep = NEWTON ? 10 * M.solver_iterations : M.solver_iterations;     // NEWTON: this is the fallback of an env with an active pair contact
        for (int pass = -1; pass < nsweep; pass++) {
          const int mode = pass < 0 ? 0 : 1;
          imp = 0.f;

          // rows in order, one slot (64 rows, one per lane) after the other so that the slot is static in the row code;
          // rows of A are fetched one block of PB rows ahead
#define PGS_SLOT(S_) \
          if (S_ < ns) { \
            const int ebeg = 64 * S_, eend = nefc < 64 * S_ + 64 ? nefc : 64 * S_ + 64; \
            float cur[PB][3], nxt[PB][3]; \
            _Pragma("unroll") for (int r = 0; r < PB; r++) { \
              const int e = ebeg + r < eend ? ebeg + r : eend - 1; \
              _Pragma("unroll") for (int sl = 0; sl < 3; sl++) cur[r][sl] = sl < ns ? AG[(size_t)e * AG_LD + 64 * sl + lane] : 0.f; \
            } \
            for (int e0 = ebeg; e0 < eend; e0 += PB) { \
              _Pragma("unroll") for (int r = 0; r < PB; r++) { \
                const int e = e0 + PB + r < eend ? e0 + PB + r : eend - 1; \
                _Pragma("unroll") for (int sl = 0; sl < 3; sl++) nxt[r][sl] = sl < ns ? AG[(size_t)e * AG_LD + 64 * sl + lane] : 0.f; \
              } \
              _Pragma("unroll") for (int r = 0; r < PB; r++) { \
                const int e = e0 + r; \
                if (e < eend) { \
                  float dj, t = 0.f; \
                  if (mode == 0) dj = fw[S_]; \
                  else { dj = fmaxf(nf[S_], res[S_] * nainv[S_]); t = fmaf(hdiag[S_], dj, res[S_]); }   /* no revert: see (8a) */ \
                  const float delta = bcast(dj, e & 63); \
                  _Pragma("unroll") for (int sl = 0; sl < 3; sl++) res[sl] = fmaf(cur[r][sl], delta, res[sl]); \
                  const float md = lane == (e & 63) ? dj : 0.f; \
                  nf[S_] -= md; imp = fmaf(md, t, imp); \
                } \
              } \
              _Pragma("unroll") for (int r = 0; r < PB; r++) \
                _Pragma("unroll") for (int sl = 0; sl < 3; sl++) cur[r][sl] = nxt[r][sl]; \
            } \
          }
          PGS_SLOT(0) PGS_SLOT(1) PGS_SLOT(2)
#undef PGS_SLOT
          if (mode == 0) {   // dual cost of the warm start; start from f = 0 if that is better
            float cost = 0.f;
#pragma unroll
            for (int sl = 0; sl < 3; sl++) cost += (-nf[sl]) * (0.5f * (res[sl] - bj[sl]) + bj[sl]);
            cost = wave_sum_fast(cost);
            if (cost > 0.f) {
#pragma unroll
              for (int sl = 0; sl < 3; sl++) { nf[sl] = 0.f; res[sl] = bj[sl]; }
            }
          } else {
            const float improvement = -wave_sum_fast(imp);
            if (!FUSED && A.dbg_pgs && lane == 0 && pass < M.solver_iterations) gptr(A.dbg_pgs)[(size_t)env * M.solver_iterations + pass] = improvement;
            if (improvement * M.pgs_scale < M.solver_tolerance) break;
          }
        }
#pragma unroll
        for (int sl = 0; sl < 3; sl++) { const int e = 64 * sl + lane; if (e < nefc) EP[e * 8 + 4] = -nf[sl]; }
        }
        // (8d) noslip post-pass (mj_solNoSlip, option.noslip_iterations; oracle: noslip()): Gauss-Seidel on the dual problem WITHOUT the
        //      regulariser over the friction dimensions alone - normal forces and limit rows keep the main solver's values.  Pyramid: the
        //      rows come in opposing pairs (j, j + 1); their sum stays, their difference is minimised exactly and clamped to [-mid, mid].
        //      Elliptic: the friction forces solve their QCQP inside the cone of the (fixed) normal force.
        if (M.noslip_iterations > 0 && ncon > 0) {
          __threadfence();
          rows_to_lds();
          for (int itn = 0; itn < M.noslip_iterations; itn++) {
            float improvement = 0.f;
            if (itn == 0) {
              float p_ = 0.f;
              for (int e = lane; e < nefc; e += 64) { const float f = FL[e]; p_ = fmaf(0.5f * f * f, RL[e], p_); }
              improvement += wave_sum_fast(p_);
            }
            for (int c = 0; c < ncon; c++) {
              const int i = nlim + crs * c;
              if (crs == 3) {
                const float fn = FL[i], o1 = FL[i + 1], o2 = FL[i + 2], mu = ML[i];
                const float* a1_ = AG + (size_t)(i + 1) * AG_LD + i; const float* a2_ = a1_ + AG_LD;
                const float A11 = a1_[1] - RL[i + 1], A12 = a1_[2], A22 = a2_[2] - RL[i + 2];
                const float r1 = BL[i + 1] + row_dot(i + 1) - RL[i + 1] * o1, r2 = BL[i + 2] + row_dot(i + 2) - RL[i + 2] * o2;
                float f1 = 0.f, f2 = 0.f;
                if (fn >= 1e-15f) {
                  const float bc1 = r1 - A11 * o1 - A12 * o2, bc2 = r2 - A12 * o1 - A22 * o2;
                  if (qcqp2_dev(A11, A12, A22, bc1, bc2, mu, fn, &f1, &f2)) {
                    float sv = (f1 / mu) * (f1 / mu) + (f2 / mu) * (f2 / mu);
                    sv = sqrtf(fn * fn / fmaxf(1e-15f, sv));
                    f1 *= sv; f2 *= sv;
                  }
                }
                const float d1 = f1 - o1, d2 = f2 - o2;
                float change = d1 * r1 + d2 * r2 + 0.5f * (d1 * (A11 * d1 + A12 * d2) + d2 * (A12 * d1 + A22 * d2));
                if (change > 1e-10f) { f1 = o1; f2 = o2; change = 0.f; }
                WSYNC();
                if (lane == 0) { FL[i + 1] = f1; FL[i + 2] = f2; }
                WSYNC();
                improvement -= change;
              } else {
                for (int j = i; j < i + 4; j += 2) {
                  const float o0 = FL[j], o1 = FL[j + 1];
                  const float* a0_ = AG + (size_t)j * AG_LD + j;
                  const float A00 = a0_[0] - RL[j], A01 = a0_[1], A11 = a0_[AG_LD + 1] - RL[j + 1];
                  const float r0 = BL[j] + row_dot(j) - RL[j] * o0, r1 = BL[j + 1] + row_dot(j + 1) - RL[j + 1] * o1;
                  const float bc0 = r0 - A00 * o0 - A01 * o1, bc1 = r1 - A01 * o0 - A11 * o1;
                  const float mid = 0.5f * (o0 + o1);
                  const float K1 = A00 + A11 - 2.f * A01, K0 = mid * (A00 - A11) + bc0 - bc1;
                  float f0, f1;
                  if (K1 < 1e-15f) { f0 = mid; f1 = mid; }
                  else {
                    const float y = -K0 / K1;
                    if (y < -mid) { f0 = 0.f; f1 = 2.f * mid; }
                    else if (y > mid) { f0 = 2.f * mid; f1 = 0.f; }
                    else { f0 = mid + y; f1 = mid - y; }
                  }
                  const float d0 = f0 - o0, d1 = f1 - o1;
                  float change = d0 * r0 + d1 * r1 + 0.5f * (d0 * (A00 * d0 + A01 * d1) + d1 * (A01 * d0 + A11 * d1));
                  if (change > 1e-10f) { f0 = o0; f1 = o1; change = 0.f; }
                  WSYNC();
                  if (lane == 0) { FL[j] = f0; FL[j + 1] = f1; }
                  WSYNC();
                  improvement -= change;
                }
              }
            }
            if (improvement * M.pgs_scale < M.noslip_tolerance) break;
          }
          forces_to_rows();
        }
        __threadfence();
        WSYNC();
        if (isd) {
          for (int e = 0; e < nefc; e++) {
            const int ce = (int)CHN[e] - 1;
            const bool on = lane <= ce && ce < lane + dsub;
            w = fmaf(on ? YC[e * RS + ddepth] : 0.f, EP[e * 8 + 4], w);
          }
          if (haspx) for (int e = e_p0; e < nefc; e++) {
            const int ce = (int)CHF[e] - 1;
            const bool on = lane <= ce && ce < lane + dsub;
            w = fmaf(on ? YF[(e - e_p0) * RS + ddepth] : 0.f, EP[e * 8 + 4], w);
          }
          w *= sqrtf(dinv_m);
        }
        WSYNC();
      }
      }
      STAMP(19);  // PGS
      if (!FUSED && A.dbg_efc) {     // fmj_step_debug: the rows of this step as the solver left them (EP layout) + the row count
        RSYNC();
        float AS1* o = gptr(A.dbg_efc) + (size_t)env * M.maxefc * 8;
        for (int i = lane; i < nefc * 8; i += 64) o[i] = EP[i];
      }
      // (9) qfrc_constraint = J' f = L'(Y' f) ; qacc = qacc_smooth + L^-1 w  (saved as next step's warm start)
      if (!primal) {
        const float u = isd ? w / dinv_m : 0.f;                      // (Y' f)_d
        float q = u;                                                 // q_a = u_a + sum over descendants i of L[i][a] u_i: no chain, LDS reads batched
        {
          int i = nv - 1;
          for (; i >= 8; i -= 8) {
            float l[8];
#pragma unroll
            for (int k = 0; k < 8; k++) l[k] = HM[(i - k) * RS + ddepth];
#pragma unroll
            for (int k = 0; k < 8; k++) { const bool anc = lane < i - k && i - k < lane + dsub; q = fmaf(anc ? l[k] : 0.f, bcast(u, i - k), q); }
          }
#pragma unroll 1
          for (; i >= 1; i--) { const bool anc = lane < i && i < lane + dsub; q = fmaf(anc ? HM[i * RS + ddepth] : 0.f, bcast(u, i), q); }
        }
        qfrc_c = q;
        const float xa = ldl_pull_sweep<MAXD>(HM, w, isd ? lane : 0, isd, ddepth, M.ancl1, M.maxdep1);   // xa = L^-1 w
        if (isd) { const float qa = xs + xa; QW[lane] = qa; if (!(fabsf(qa) <= 1e10f)) warn |= FMJ_WARN_BADQACC; }
      }
      STAMP(20);  // qfrc_constraint + warm start
      // (10) sensors: joint limit force; contact forces in the contact frame (mj_contactForce, pyramidal)
      {
        float lf = 0.f;
        if (act_lo) lf += EP[e_lo * 8 + 4];
        if (act_hi) lf += EP[e_hi * 8 + 4];
        cy_limfrc = lf * A.inv_torques;
        cy_ncon = ncon;
        WSYNC();
        for (int c = lane; c < ncon; c += 64) {                   // complete the LDS records: force(3) + geom1 << 16 | geom2
          const float* ep = EP + (nlim + crs * c) * 8;
          const float f0 = ep[4], f1 = ep[12], f2 = ep[20], f3 = crs == 4 ? ep[28] : 0.f, mu = ep[7];
          float* ct = CT + c * 16;
          const int g2 = __float_as_int(ct[14]) & 0xffff, g1 = __float_as_int(ct[15]) & 0xffff;   // geom2 = the animat geom, geom1 = the ground geom or the pair's first geom
          if (crs == 4) { ct[12] = f0 + f1 + f2 + f3; ct[13] = mu * (f0 - f1); ct[14] = mu * (f2 - f3); }
          else { ct[12] = f0; ct[13] = f1; ct[14] = f2; }                                  // elliptic: the rows are the frame axes
          ct[15] = __int_as_float((g1 << 16) | g2);
        }
        WSYNC();
        if (last && d_scalar) gptr(A.sensordata)[(size_t)env * M.nsensordata + 6 * (nb - 1) + 3 * d_act.z + 2] = lf;
        if (last) {
          for (int i = lane; i < ncon * 16; i += 64) gptr(A.contact)[(size_t)env * M.max_contacts * 16 + i] = CT[i];
          if (lane == 0) gptr(A.ncon)[env] = ncon;
        }
      }
      WSYNC();
#undef RSYNC
