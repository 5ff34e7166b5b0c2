// fmj_cons2_rows.inc - constraint rows, PGS and constraint forces of the two-env constraint kernel (fmj_cons2.inc), included twice:
//   CR_PAIR 1  both envs of the wave at once: lane = row inside each half (<= 32 rows per env), row scratch per half;
//   CR_PAIR 0  env `xenv` (0: lanes 0..31 own it, 1: lanes 32..63) alone on all 64 lanes (lane = row, <= 64 rows); the lanes of its
//              half do the lane = dof parts, the other half idles through them.
// Same steps and arithmetic as the on-chip copy of fmj_cons_rows.inc (MuJoCo's mj_makeConstraint / mj_projectConstraint /
// mj_solPGS for limit and pyramidal contact rows, restated by oracle make_constraints / solve_constraints), with the translational
// dofs of a free root as scalars: a row's entries at depths 0..2 are its direction's world components, the chain walk ends in
// the 3 x 3 factor of the translational block, and the J' products add that block's share by reductions over the rows.
// Every sum over rows is a DPP reduction in which absent rows contribute exact zeros, and every per-row operation is the lane's
// own: an env's numbers do not depend on the mode, nor on the other env of the wave.
    {
#if CR_PAIR
      constexpr int NAR = 32;                              // rows per env = registers of the lane's row of A
      const int RL = sl;                                   // the lane's row
      float* const eb = base;                              // persistent arrays of the env whose rows this lane works on
      float* const rb = lds + LL.SCR + (upper ? LL.rowsz : 0);
      const int nefc_r = nefc, ncon_r = ncon, nlim_r = nlim;
      const int nefc_u = nefcA > nefcB ? nefcA : nefcB, ncon_u = nconA > nconB ? nconA : nconB;      // uniform loop bounds
      const bool dofon = !retired;                         // a retired half (fmj_cons2.inc) has no rows and must keep its warm start
      const int env_r = env;
#define BCR(v_, i_) bcast2(v_, i_, upper)
#define BCD(v_, i_) bcast2(v_, i_, upper)
#define RSUM(v_) half_sum_dpp(v_, upper)
      const bool run_rows = true;
#else
      constexpr int NAR = 64;
      const int RL = lane;
      const int xoff = xenv ? 32 : 0;
      float* const eb = lds + (xenv ? LL.env_total : 0);
      float* const rb = lds + LL.SCR;
      const int nefc_r = xenv ? nefcB : nefcA, ncon_r = xenv ? nconB : nconA;
      const int nlim_r = __builtin_amdgcn_readlane(nlim, xoff);
      const int nefc_u = nefc_r, ncon_u = ncon_r;
      const bool dofon = upper == (xenv != 0) && !retired;
      const int env_r = __builtin_amdgcn_readlane(env, xoff);
#define BCR(v_, i_) bcast(v_, i_)
#define BCD(v_, i_) __int_as_float(__builtin_amdgcn_readlane(__float_as_int(v_), (i_) + xoff))
#define RSUM(v_) wave_sum_fast(v_)
      const bool run_rows = nefc_r > 0;
      if (!run_rows && dofon) { if (isd) QW[mydof] = xsm; if (T0 && sl == 0) { QW[0] = XS[0]; QW[1] = XS[1]; QW[2] = XS[2]; } }
#endif
      if (run_rows) {
      // a value per lane = row -> the values of rows l and l + 16 in lanes l and l + 16 alike (the builtin, not asm: the compiler pads its hazards)
#define ROWS_L_L16(x_, y_) { const auto sw_ = __builtin_amdgcn_permlane16_swap(__float_as_uint(x_), __float_as_uint(x_), false, false); \
                             x_ = __uint_as_float(sw_[0]); y_ = __uint_as_float(sw_[1]); }
      float* const eQV = eb + LL.QV; float* const eXS = eb + LL.XS; float* const eQW = eb + LL.QW; float* const eSD = eb + LL.SD;
      float* const eTS = eb + LL.TS; float* const eHM = eb + LL.HM; float* const eCT = eb + LL.CT;
      float* const YC = rb;                                // compact rows [NAR][RS]: entry at the chain's dof of each depth
      float* const EP = rb + NAR * RS;                     // per row: pos, margin -> aref, R, b, force, R0, type | id, mu
      uint8_t* const CHN = (uint8_t*)(rb + NAR * RS + NAR * 8);   // per row: last dof of its chain + 1
      float* const UU = rb + NAR * RS + NAR * 8 + NAR / 4;           // D^1/2 Z' f of the lane dofs (32 floats)
      const int8_t* const LCB = (const int8_t*)(lds + LL.LC);
      for (int i = RL * 4; i < NAR * RS + NAR * 8 + NAR / 4 + 32; i += NAR * 4) *(float4*)(rb + i) = make_float4(0.f, 0.f, 0.f, 0.f);
      WSYNC();
      // (4) Jacobian rows.  Limit rows: +-1 at the dof.  Contact rows: n.Jp +- mu t.Jp, Jp column of dof d = cdof_lin + cdof_rot x (p - com);
      //     the columns of the translational dofs are the direction's world components
      if (dofon && act_lo) { YC[e_lo * RS + ddepth] = 1.f;  CHN[e_lo] = (uint8_t)(mydof + 1); float* ep = EP + e_lo * 8; ep[0] = dist_lo; ep[1] = lim.w; ep[6] = __int_as_float(mydof); ep[7] = 0.f; }
      if (dofon && act_hi) { YC[e_hi * RS + ddepth] = -1.f; CHN[e_hi] = (uint8_t)(mydof + 1); float* ep = EP + e_hi * 8; ep[0] = dist_hi; ep[1] = lim.w; ep[6] = __int_as_float(mydof); ep[7] = 0.f; }
      for (int c = 0; c < ncon_u; c++) {
        const bool cvalid = c < ncon_r;
        const float* ct = eCT + (cvalid ? c : 0) * 16;
        const float4 c0 = *(const float4*)(ct), c1 = *(const float4*)(ct + 4), c2 = *(const float4*)(ct + 8), c3 = *(const float4*)(ct + 12);
        const int lastd = (__float_as_int(c3.z) >> 16) - 1;     // last dof on the contact body's chain
        const bool on = dofon && cvalid && isd && lastd >= 0 && mydof <= lastd && lastd < mydof + dsub;
        const v3 nrm = mk3(c0.w, c1.x, c1.y), t1 = mk3(c1.z, c1.w, c2.x), t2 = mk3(c2.y, c2.z, c2.w);
        if (on) {
          const v3 jp = add3(cdme.l, cross(cdme.r, sub3(mk3(c0.x, c0.y, c0.z), com)));
          const float jn = dot3(jp, nrm), j1 = c3.y * dot3(jp, t1), j2 = c3.y * dot3(jp, t2);
          float* y = YC + (nlim_r + 4 * c) * RS + ddepth;
          y[0] = jn + j1; y[RS] = jn - j1; y[2 * RS] = jn + j2; y[3 * RS] = jn - j2;
        }
        if (dofon && cvalid && T0 && sl < 3) {      // translational dof sl of the free root: cdof = the unit translation
          const float jn = sl == 0 ? nrm.x : (sl == 1 ? nrm.y : nrm.z);
          const float j1 = c3.y * (sl == 0 ? t1.x : (sl == 1 ? t1.y : t1.z)), j2 = c3.y * (sl == 0 ? t2.x : (sl == 1 ? t2.y : t2.z));
          float* y = YC + (nlim_r + 4 * c) * RS + sl;
          y[0] = jn + j1; y[RS] = jn - j1; y[2 * RS] = jn + j2; y[3 * RS] = jn - j2;
        }
        if (cvalid && RL < 4) {
          const int r_ = nlim_r + 4 * c + RL;
          CHN[r_] = (uint8_t)(lastd + 1);
          float* ep = EP + r_ * 8; ep[0] = c3.x; ep[1] = 0.f; ep[6] = __int_as_float(0x40000000 | c); ep[7] = c3.y;
        }
      }
      WSYNC();
      STAMP(14);  // J rows
      // (5) per row (lane = row): R, aref (mj_makeImpedance / mj_referenceConstraint), b = J qacc_smooth - aref, warm-start jar, then
      // (6) Z = J L^-1 D^-1/2 with the row in registers, walking the chain from its last dof to the root
      const int e = RL;
      const bool isr = e < nefc_r;
      const int chain = isr ? (int)CHN[e] - 1 : -1;
      {
        float* ep = EP + (isr ? e : 0) * 8;
        const int tid = __float_as_int(ep[6]);
        const bool is_con = (tid & 0x40000000) != 0;
        float sr0, sr1, si0, si1, si2, si3, si4, dapx;
        const float mu = ep[7];
        if (is_con) {
          const float4 c3 = *(const float4*)(eCT + (tid & 0xff) * 16 + 12);
          const int g = __float_as_int(c3.z) & 0xffff;
          const float4 a = GTAB(g, 4), b = GTAB(g, 5);
          const float tran = GTAB(g, 2).w;                       // invweight0 of the body (+ 0 for the world's ground)
          sr0 = a.x; sr1 = a.y; si0 = a.z; si1 = a.w; si2 = b.x; si3 = b.y; si4 = b.z;
          dapx = tran + mu * mu * tran;
        } else {
          const float4 a = DTAB(tid & 0xff, 4), b = DTAB(tid & 0xff, 5);
          sr0 = a.x; sr1 = a.y; si0 = a.z; si1 = a.w; si2 = b.x; si3 = b.y; si4 = b.z; dapx = b.w;
        }
        float R, kimp, bb;
        row_params(sr0, sr1, si0, si1, si2, si3, si4, ep[0], ep[1], dapx, hstepc, &R, &kimp, &bb);
#define ROW_ENV(a_) e##a_
#include "fmj_rows_chain.inc"      // y: the row of J by depth; ANC4, LDSF, atab: the chain's dof at each depth; vel, jxs, jqw
#undef ROW_ENV
        const float aref = -bb * vel - kimp * (ep[0] - ep[1]);
        const float tl10 = eTS[0], tl20 = eTS[1], tl21 = eTS[2];
        const char* const HMb = (const char*)eHM - (size_t)T0 * RS * 4;      // rows of the lane dofs, addressed by dof
#pragma unroll
        for (int dd = MAXD - 1; dd >= 1; dd--) {
          const float yi = y[dd];
          if (dd >= 3 || T0 == 0) {
            const float* lr = (const float*)(HMb + ANC4(atab, dd) * RS);
#pragma unroll
            for (int g4 = 0; g4 < (dd + 3) / 4; g4++) {
              const float4 l4 = *(const float4*)(lr + 4 * g4);
              if (4 * g4 + 0 < dd) y[4 * g4 + 0] = fmaf(-l4.x, yi, y[4 * g4 + 0]);
              if (4 * g4 + 1 < dd) y[4 * g4 + 1] = fmaf(-l4.y, yi, y[4 * g4 + 1]);
              if (4 * g4 + 2 < dd) y[4 * g4 + 2] = fmaf(-l4.z, yi, y[4 * g4 + 2]);
              if (4 * g4 + 3 < dd) y[4 * g4 + 3] = fmaf(-l4.w, yi, y[4 * g4 + 3]);
            }
          } else if (dd == 2) { y[1] = fmaf(-tl21, yi, y[1]); y[0] = fmaf(-tl20, yi, y[0]); }
          else y[0] = fmaf(-tl10, yi, y[0]);
        }
#pragma unroll
        for (int dd = 0; dd < MAXD; dd++) y[dd] *= LDSF(eSD, ANC4(atab, dd));
#undef ANC4
#undef LDSF
        if (isr) {
          float* yr = YC + e * RS;
#pragma unroll
          for (int g4 = 0; g4 < MAXD / 4; g4++) *(float4*)(yr + 4 * g4) = make_float4(y[4 * g4], y[4 * g4 + 1], y[4 * g4 + 2], y[4 * g4 + 3]);
          ep[1] = aref; ep[2] = R; ep[3] = jxs - aref; ep[4] = jqw - aref; ep[5] = R;
        }
      }
      WSYNC();
      if (isr) {      // pyramidal: the 4 rows of a contact share R = 2 mu^2 R_first (mu scaled by 1/sqrt(impratio)); warm-start force
        float* ep = EP + e * 8;
        const int tid = __float_as_int(ep[6]);
        if (tid & 0x40000000) {
          const int e0 = nlim_r + 4 * (tid & 0xff);
          const float mu = ep[7] * M.impratio_isqrt;
          ep[2] = fmaxf(1e-15f, 2.f * mu * mu * EP[e0 * 8 + 5]);
        }
        const float jar = ep[4]; ep[4] = jar < 0.f ? -jar / ep[2] : 0.f;
      }
      WSYNC();
      STAMP(16);  // row params + Z
      // (7) explicit A = Z Z' + diag(R) on the matrix cores (round 5): with every row of Z spread over the dofs (entry k = the row's entry
      //     at the depth of dof k if dof k lies on the row's chain, else 0) A is a plain product, no depth masks - 32 x 32 x 2 fp32 MFMA
      //     steps over pairs of dofs.  Operand of a step: lane i = row i & 31 of the block, dof 2t + (i >> 5).  The result leaves column j in
      //     lanes j and j + 32 (rows 8g .. 8g + 3 of every eight in the first, 8g + 4 .. 8g + 7 in the second); A is symmetric, so that is row j,
      //     and v_permlane32_swap of two results puts both halves of one into lanes 0 .. 31 and of the other into lanes 32 .. 63:
      //     PAIR: env A's and env B's; SOLO: the row blocks 0 .. 31 and 32 .. 63 of the env, once per block of 32 columns.
      //     Sums run over the dofs in the same order in every mode: an env's numbers do not depend on it.
      float areg[64];
      float diag = 1.f;                                      // A_jj + R_j
      {
#define MFMA_A_NEFC nefc_r
#define MFMA_A_OPERANDS_ONLY CR_PAIR      // PAIR assembles one 32-row matrix per env in its own loop below
#include "fmj_rows_mfma_a.inc"      // kh, r32, nsteps, ZOP, SWAP32; SOLO: areg = the lane's row of Z Z'
#undef MFMA_A_NEFC
#undef MFMA_A_OPERANDS_ONLY
#if CR_PAIR
        const float* const ycA = lds + LL.SCR + r32 * RS;
        const float* const ycB = ycA + LL.rowsz;
        const int chA = r32 < nefcA ? (int)((const uint8_t*)(lds + LL.SCR + 32 * RS + 32 * 8))[r32] - 1 : -1;
        const int chB = r32 < nefcB ? (int)((const uint8_t*)(lds + LL.SCR + LL.rowsz + 32 * RS + 32 * 8))[r32] - 1 : -1;
        f16_t accA, accB;
#pragma unroll
        for (int v = 0; v < 16; v++) { accA[v] = 0.f; accB[v] = 0.f; }
        for (int t = 0; t < nsteps; t++) {
          const int k = 2 * t + kh;
          const int dk = k < nv ? (int)LCB[k * nv + k] : -1;
          const float za = ZOP(ycA, chA, dk, k), zb = ZOP(ycB, chB, dk, k);
          accA = __builtin_amdgcn_mfma_f32_32x32x2f32(za, za, accA, 0, 0, 0);
          accB = __builtin_amdgcn_mfma_f32_32x32x2f32(zb, zb, accB, 0, 0, 0);
        }
#pragma unroll
        for (int v = 0; v < 16; v++) {
          float x_ = accA[v], y_ = accB[v];
          SWAP32(x_, y_);
          areg[8 * (v >> 2) + (v & 3)] = x_; areg[8 * (v >> 2) + 4 + (v & 3)] = y_;
        }
#pragma unroll
        for (int f = 32; f < 64; f++) areg[f] = 0.f;
#endif
#undef ZOP
#undef SWAP32
        const float Rj = isr ? EP[e * 8 + 2] : 0.f;
#pragma unroll
        for (int f = 0; f < NAR; f++) {
          const bool own = f == e && isr;
          areg[f] += own ? Rj : 0.f;
          diag = own ? areg[f] : diag;
        }
      }
      STAMP(17);  // A
      // warm start: keep it only if its dual cost beats f = 0 (mj_fwdConstraint); the forces of the other rows come as LDS broadcasts
      float fj = isr ? EP[e * 8 + 4] : 0.f;
      const float bj = isr ? EP[e * 8 + 3] : 0.f;
      const float ainv = 1.0f / diag;
      float afj = 0.f;
      {
        const int nefc_w = opaque_s(nefc_u);      // one uniform test per four columns: the registers past nefc hold exact zeros, their EP slots the zero fill
#pragma unroll
        for (int k4 = 0; k4 < NAR; k4 += 4)
          if (k4 < nefc_w) {
#pragma unroll
            for (int k = k4; k < k4 + 4; k++) afj = fmaf(areg[k], EP[k * 8 + 4], afj);
          }
      }
      {
        const float cost = RSUM(fj * (0.5f * afj + bj));
        if (cost > 0.f) { fj = 0.f; afj = 0.f; }
      }
      float res = bj + afj;
      STAMP(18);  // warm start
      // (8) PGS on the explicit matrix on the scaled residual r_j = -res_j / A_jj (fmj_cons_rows.inc (8a)).  PAIR: turn e serves row e of
      //     both envs.  An env whose rows are not finite is solved as if it had none (and flagged).  A half whose sweeps have converged
      //     keeps its forces of that moment and idles through the other half's remaining sweeps.
      const float hdiag = 0.5f * diag;
      const float nainv = -ainv;
      float nf = -fj;
#pragma unroll
      for (int k = 0; k < NAR; k++) areg[k] *= nainv;
      res *= nainv;
#if CR_PAIR
      {
        // A is positive semidefinite: |A_jf| <= sqrt(A_jj A_ff) - finite diagonals of all rows bound every entry
        const bool rbad = !(fabsf(res) + fabsf(nf) + fabsf(diag) + fabsf(nainv) <= 1e30f);
        if (__any(rbad)) {
          const bool hbad = HALF_ANY(rbad);
          if (hbad) {
            warn |= FMJ_WARN_BADQACC; res = 0.f; nf = 0.f;
#pragma unroll
            for (int k = 0; k < NAR; k++) areg[k] = 0.f;
          }
        }
      }
#endif
      // Two rows per lane (PAIR always; SOLO for an env of <= 32 rows - the light partner of a heavy env): lanes l and l + 16 of a group of 32
      // both get rows l (areg[0, 32), res, nf) and l + 16 (areg[32, 64), res1, nf1).  v_permlane16_swap (gfx950) trades the odd groups of 16
      // lanes of its first operand for the even ones of its second.  SOLO: the lanes past 31 hold no rows - zeros in, zeros out.
      const bool two_rows = CR_PAIR || nefc_r <= 32;
      float res1 = 0.f, nf1 = 0.f;
      if (two_rows) {
#pragma unroll
        for (int k = 0; k < 32; k++) { float y_; ROWS_L_L16(areg[k], y_); areg[32 + k] = y_; }
        ROWS_L_L16(res, res1);
        ROWS_L_L16(nf, nf1);
      }
      const bool hi16 = (RL & 16) != 0;                    // the lane's OWN row is the second of its two
      const bool isr0 = RL < 32 && (RL & 15) < nefc_r, isr1 = RL < 32 && (RL & 15) + 16 < nefc_r;
      const int q3 = RL & 3;
      bool pgs_done = false; float f_done = 0.f;
      // Two rows per lane (round 5): the update reaches the lanes as the DPP operand of the fmacs (row_newbcast: lane e of every group of 16 lanes
      // to its group) - no v_readlane, no scalar, no zero-padded multiplicand - and THREE vector instructions make a turn (with two waves per
      // SIMD the sweeps are bound by those): v_max_f32_dpp under the bank mask of lane e (an immediate) latches the update itself - register
      // e & 3 of the row set is the lane's own for lane & 3 == e & 3, junk elsewhere, never read there -, the fmac of the PREVIOUS turn for the
      // row set this turn does not read (one turn late), the fmac for the row set the next turn reads.  The force a row gains in the sweep is
      // its latched update; the residual it was made from is not kept, and the sweep's improvement (below) does not need it.  The four turns of
      // a bank are one asm statement (the compiler pads every boundary between statements); a DPP read of a latched register comes two wait
      // states after its v_max (the late fmac and an s_nop), v_max_dpp's own DPP operand is -f, last written in the previous sweep's tail.
      // Both groups of a half run the same numbers, so each lane ends with its own row's; every row sees the same fmacs in the same order as
      // with v_readlane (scripts/ubench/pgs2.hip, variant 10: identical residuals and forces, 34.2 -> 21.5 ticks per turn).
      float dq[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
#define T3S_N(i, lp_, dp_) \
            "v_max_f32_dpp %[d" #i "], %[nf], %[S] quad_perm:[0,1,2,3] row_mask:0xf bank_mask:%[bm]\n\t" \
            "v_fmac_f32_dpp %[O], %[" dp_ "], %[l" #i "] row_newbcast:%[" lp_ "] row_mask:0xf bank_mask:0xf\n\t" \
            "s_nop 0\n\t" \
            "v_fmac_f32_dpp %[S], %[d" #i "], %[a" #i "] row_newbcast:%[e" #i "] row_mask:0xf bank_mask:0xf\n\t"
      // a turn whose own fmac goes to the OTHER set (the next turn reads that one: turn 15 of more than 16, the last turn of more than 16)
#define T3S_X(i, lp_, dp_) \
            "v_max_f32_dpp %[d" #i "], %[nf], %[S] quad_perm:[0,1,2,3] row_mask:0xf bank_mask:%[bm]\n\t" \
            "v_fmac_f32_dpp %[O], %[" dp_ "], %[l" #i "] row_newbcast:%[" lp_ "] row_mask:0xf bank_mask:0xf\n\t" \
            "s_nop 1\n\t" \
            "v_fmac_f32_dpp %[O], %[d" #i "], %[a" #i "] row_newbcast:%[e" #i "] row_mask:0xf bank_mask:0xf\n\t"
      // the sweep's first turn: nothing is late yet; whatever the compiler put in front of the statement is two wait states away
#define T3S_FIRST \
            "s_nop 1\n\t" \
            "v_max_f32_dpp %[d0], %[nf], %[S] quad_perm:[0,1,2,3] row_mask:0xf bank_mask:%[bm]\n\t" \
            "s_nop 1\n\t" \
            "v_fmac_f32_dpp %[S], %[d0], %[a0] row_newbcast:%[e0] row_mask:0xf bank_mask:0xf\n\t"
#define T3S_OPS(E0_, s_, XL_, dprev_) \
            : [S] "+v"(s_ ? res1 : res), [O] "+v"(s_ ? res : res1), \
              [d0] "+v"(dq[4 * s_]), [d1] "+v"(dq[4 * s_ + 1]), [d2] "+v"(dq[4 * s_ + 2]), [d3] "+v"(dq[4 * s_ + 3]) \
            : [nf] "v"(s_ ? nf1 : nf), [dp] "v"(dprev_), [bm] "n"(1 << (((E0_) & 15) >> 2)), \
              [a0] "v"(areg[32 * s_ + (E0_)]), [a1] "v"(areg[32 * s_ + (E0_) + 1]), [a2] "v"(areg[32 * s_ + (E0_) + 2]), \
              [a3] "v"(areg[32 * (XL_ ? 1 - s_ : s_) + (E0_) + 3]), \
              [l0] "v"(areg[32 * (1 - s_) + ((E0_) > 0 ? (E0_) - 1 : 0)]), [l1] "v"(areg[32 * (1 - s_) + (E0_)]), [l2] "v"(areg[32 * (1 - s_) + (E0_) + 1]), \
              [l3] "v"(areg[32 * (1 - s_) + (E0_) + 2]), \
              [em] "n"(((E0_) + 15) & 15), [e0] "n"((E0_) & 15), [e1] "n"(((E0_) + 1) & 15), [e2] "n"(((E0_) + 2) & 15), [e3] "n"(((E0_) + 3) & 15)
      // the bank of turns E0_ .. E0_ + 3 of a sweep of NR_ turns (both multiples of 4; a bank never straddles the two row sets)
#define PGS_QUAD_D(E0_, NR_) { \
            const int s_ = (E0_) < 16 ? 0 : 1; \
            const bool xl_ = ((E0_) == 12 && (NR_) > 16) || ((E0_) == (NR_) - 4 && (NR_) > 16);      /* the bank's last turn hands over to the other set */ \
            if ((E0_) == 0) \
              asm volatile(T3S_FIRST T3S_N(1, "e0", "d0") T3S_N(2, "e1", "d1") T3S_N(3, "e2", "d2") "" T3S_OPS(E0_, s_, 0, dq[0])); \
            else if (xl_) \
              asm volatile(T3S_N(0, "em", "dp") T3S_N(1, "e0", "d0") T3S_N(2, "e1", "d1") T3S_X(3, "e2", "d2") "" T3S_OPS(E0_, s_, 1, dq[(E0_) == 16 ? 3 : 4 * s_ + 3])); \
            else \
              asm volatile(T3S_N(0, "em", "dp") T3S_N(1, "e0", "d0") T3S_N(2, "e1", "d1") T3S_N(3, "e2", "d2") "" T3S_OPS(E0_, s_, 0, dq[(E0_) == 16 ? 3 : 4 * s_ + 3])); \
            if ((E0_) == (NR_) - 4)      /* the sweep's last late fmac: the second row set (the last turn's own fmac went to the first, which turn 0 reads) */ \
              asm volatile("s_nop 1\n\tv_fmac_f32_dpp %[rp], %[cp], %[ap] row_newbcast:%[elp] row_mask:0xf bank_mask:0xf" \
                           : [rp] "+v"(res1) : [cp] "v"(dq[4 * s_ + 3]), [elp] "n"(((NR_) - 1) & 15), [ap] "v"(areg[32 + (NR_) - 1])); }
      // the sweep's improvement against the tolerance (mj_solPGS).  PAIR: the half's total sits in its last lane after the DPP steps; the
      // test is made there and read off the ballot - no broadcast of the sum
#if CR_PAIR
#define PGS_CONVERGED(imp_) \
        const float tot_ = -half_sum_last(imp_); \
        if (!FUSED && A.dbg_pgs && !pgs_done && sl == 31) gptr(A.dbg_pgs)[(size_t)env_r * M.solver_iterations + itp] = tot_; \
        const unsigned long long sm_ = __ballot(tot_ * M.pgs_scale < M.solver_tolerance); \
        const bool conv_ = upper ? (sm_ >> 63) != 0ull : ((sm_ >> 31) & 1ull) != 0ull;
#else
#define PGS_CONVERGED(imp_) \
        const float improvement = -RSUM(imp_); \
        if (!FUSED && A.dbg_pgs && !pgs_done && RL == 0) gptr(A.dbg_pgs)[(size_t)env_r * M.solver_iterations + itp] = improvement; \
        const bool conv_ = improvement * M.pgs_scale < M.solver_tolerance;
#endif
      // The sweep's improvement (mj_solPGS sums the cost change of every row, delta (A_ee delta / 2 + r_e) with r_e the residual the row's
      // update was made from): the sum over a sweep telescopes to C(f + d) - C(f) = d' (r_start + r_end) / 2 for the dual cost C = f' A f / 2 + b' f
      // (A d = r_end - r_start), which needs the residuals at the two ENDS of the sweep and the forces gained - nothing from inside the turns.
      // Same number up to rounding, terms of the size of the per-row ones (r ~ delta near the solution).
      float rs0 = res, rs1 = res1;                          // the (scaled) residuals at the start of the sweep
#define PGS_SWEEPS_D(NR_) \
      for (int itp = 0; itp < M.solver_iterations; itp++) { \
        _Pragma("unroll") for (int e_ = 0; e_ < NR_; e_ += 4) { PGS_QUAD_D(e_, NR_) } \
        const float d0_ = q3 == 0 ? dq[0] : (q3 == 1 ? dq[1] : (q3 == 2 ? dq[2] : dq[3]));      /* rows past NR_ read stale or zero registers: isr0 / isr1 */ \
        const float d1_ = q3 == 0 ? dq[4] : (q3 == 1 ? dq[5] : (q3 == 2 ? dq[6] : dq[7])); \
        const float capc = isr0 ? d0_ : 0.f, capc1 = isr1 ? d1_ : 0.f; \
        nf -= capc; nf1 -= capc1; \
        const float capc_o = hi16 ? capc1 : capc, rsum_o = hi16 ? rs1 + res1 : rs0 + res;      /* the lane's own row */ \
        rs0 = res; rs1 = res1; \
        const float imp = -hdiag * capc_o * rsum_o; \
        PGS_CONVERGED(imp) \
        if (!pgs_done && conv_) { pgs_done = true; f_done = -(hi16 ? nf1 : nf); } \
        if (__all(pgs_done)) break; \
      }
      if (two_rows) {
        switch ((nefc_u + 3) >> 2) {
          case 0: case 1: case 2: PGS_SWEEPS_D(8) break;
          case 3: PGS_SWEEPS_D(12) break;
          case 4: PGS_SWEEPS_D(16) break;
          case 5: PGS_SWEEPS_D(20) break;
          case 6: PGS_SWEEPS_D(24) break;
          case 7: PGS_SWEEPS_D(28) break;
          default: PGS_SWEEPS_D(32) break;
        }
      }
#if !CR_PAIR
      // SOLO, 33 .. 64 rows: lane = row on the whole wave, the update crosses the groups of 16 lanes through v_readlane.  Three vector
      // instructions here too: v_max_f32_dpp under the row and bank masks of lane e latches the update (register e & 3), v_readlane takes it
      // from there, one fmac; the waits around v_readlane are s_nops.  The improvement comes from the two ends of the sweep, as above.
      float dqs[4] = {0.f, 0.f, 0.f, 0.f};
#define PGS_TS_STR \
            "v_max_f32_dpp %[dq], %[nf], %[res] quad_perm:[0,1,2,3] row_mask:%[rm] bank_mask:%[bm]\n\t" \
            "s_nop 0\n\t" \
            "v_readlane_b32 %[sa], %[dq], %[e]\n\t" \
            "s_nop 1\n\t" \
            "v_fmac_f32_e32 %[res], %[sa], %[a0]"
#define PGS_TS_OPS(e_) \
            : [dq] "+v"(dqs[(e_) & 3]), [sa] "=&s"(upd_), [res] "+v"(res) \
            : [nf] "v"(nf), [e] "n"(e_), [rm] "n"(1 << ((e_) >> 4)), [bm] "n"(1 << (((e_) & 15) >> 2)), [a0] "v"(areg[e_])
      // (-f is the DPP operand of every turn: whatever wrote it last - the sweep's tail, a copy the compiler makes - is two wait states away)
#define PGS_TURN_S(e_, NR_) { \
            float upd_; \
            if ((e_) == 0) asm volatile("s_nop 1\n\t" PGS_TS_STR PGS_TS_OPS(e_)); \
            else asm volatile(PGS_TS_STR PGS_TS_OPS(e_)); }
#define PGS_SWEEPS_S(NR_) \
      for (int itp = 0; itp < M.solver_iterations; itp++) { \
        _Pragma("unroll") for (int e_ = 0; e_ < NR_; e_++) { PGS_TURN_S(e_, NR_) } \
        const float d_ = q3 == 0 ? dqs[0] : (q3 == 1 ? dqs[1] : (q3 == 2 ? dqs[2] : dqs[3]));      /* rows past NR_ read stale or zero registers: isr */ \
        const float capc = isr ? d_ : 0.f; \
        nf -= capc; \
        const float imp = -hdiag * capc * (rs0 + res); \
        rs0 = res; \
        PGS_CONVERGED(imp) \
        if (!pgs_done && conv_) { pgs_done = true; f_done = -nf; } \
        if (__all(pgs_done)) break; \
      }
      if (!two_rows) {
        switch ((nefc_u + 3) >> 2) {
          case 9: PGS_SWEEPS_S(36) break;
          case 10: PGS_SWEEPS_S(40) break;
          case 11: PGS_SWEEPS_S(44) break;
          case 12: PGS_SWEEPS_S(48) break;
          case 13: PGS_SWEEPS_S(52) break;
          case 14: PGS_SWEEPS_S(56) break;
          case 15: PGS_SWEEPS_S(60) break;
          default: PGS_SWEEPS_S(64) break;
        }
      }
#undef PGS_SWEEPS_S
#undef PGS_TURN_S
#undef PGS_TS_STR
#undef PGS_TS_OPS
#endif
#undef PGS_SWEEPS_D
#undef PGS_QUAD_D
#undef T3S_N
#undef T3S_X
#undef T3S_FIRST
#undef T3S_OPS
#undef PGS_CONVERGED
#undef ROWS_L_L16
      fj = pgs_done ? f_done : (two_rows ? -(hi16 ? nf1 : nf) : -nf);
      if (isr) EP[e * 8 + 4] = fj;
      STAMP(19);  // PGS
      // translational dofs: (Z' f)_t over all rows of the env (every chain runs through the free root)
      float wt0 = 0.f, wt1 = 0.f, wt2 = 0.f;
      if (T0) {
        const float4 z4 = *(const float4*)(YC + (isr ? e : 0) * RS);
        const float fz = isr ? fj : 0.f;
        wt0 = RSUM(z4.x * fz); wt1 = RSUM(z4.y * fz); wt2 = RSUM(z4.z * fz);
      }
      WSYNC();
      // (9) qfrc_constraint = J' f = L' D^1/2 (Z' f);  qacc = qacc_smooth + L^-1 D^-1/2 (Z' f)  (saved as the next warm start).  Lane = dof
      //     of the env's own half; the forces come as LDS broadcasts (EP), D^1/2 Z' f goes through LDS (UU) for the L' product.
      if (dofon) {
        const int ddq = opaque(ddepth), dsq = opaque(dsub);     // their own copies: see the laundering notes of fmj_hip.hip
        float w = 0.f;
        if (isd) {
          int e2 = 0;
          for (; e2 + 4 <= nefc_u; e2 += 4) {
            float yv[4], fv[4]; int ce[4];
            const unsigned ch4 = *(const unsigned*)(CHN + e2);
#pragma unroll
            for (int u = 0; u < 4; u++) { yv[u] = YC[(e2 + u) * RS + ddq]; fv[u] = EP[(e2 + u) * 8 + 4]; ce[u] = (int)((ch4 >> (8 * u)) & 0xffu) - 1; }
#pragma unroll
            for (int u = 0; u < 4; u++) w = fmaf((mydof <= ce[u] && ce[u] < mydof + dsq) ? yv[u] : 0.f, fv[u], w);
          }
          for (; e2 < nefc_u; e2++) {
            const int ce = (int)CHN[e2] - 1;
            w = fmaf((mydof <= ce && ce < mydof + dsq) ? YC[e2 * RS + ddq] : 0.f, EP[e2 * 8 + 4], w);
          }
          w *= sqrtf(dinv_m);
        }
        const float u = isd ? w / dinv_m : 0.f;                       // (D^1/2 Z' f)_d
        if (isd) UU[sl] = u;
        const float sd0 = T0 ? SD[0] : 1.f, sd1 = T0 ? SD[1] : 1.f, sd2 = T0 ? SD[2] : 1.f;      // the translational block of M, parked in LDS by the factorisation
        const float ml10 = TS[0], ml20 = TS[1], ml21 = TS[2];
        const float ut0 = T0 ? wt0 / sd0 : 0.f, ut1 = T0 ? wt1 / sd1 : 0.f, ut2 = T0 ? wt2 / sd2 : 0.f;
        float4 myrow[MAXD / 4];                                       // this dof's row of L
#pragma unroll
        for (int g = 0; g < MAXD / 4; g++) myrow[g] = *(const float4*)(HM + (isd ? sl : 0) * RS + 4 * g);
        const float lmx = isd ? myrow[0].x : 0.f, lmy = isd ? myrow[0].y : 0.f, lmz = isd ? myrow[0].z : 0.f;
        WSYNC();
        float q = u;                                                  // q_a = u_a + sum over descendants i of L[i][a] u_i: independent terms
        {
          int i = ND - 1;
          for (; i >= 8; i -= 8) {
            float l[8], uv[8];
#pragma unroll
            for (int k = 0; k < 8; k++) { l[k] = HM[(i - k) * RS + ddq]; uv[k] = UU[i - k]; }
#pragma unroll
            for (int k = 0; k < 8; k++) { const bool anc = isd && sl < i - k && i - k < sl + dsq; q = fmaf(anc ? l[k] : 0.f, uv[k], q); }
          }
#pragma unroll 1
          for (; i >= 1; i--) { const bool anc = isd && sl < i && i < sl + dsq; q = fmaf(anc ? HM[i * RS + ddq] : 0.f, UU[i], q); }
        }
        qfrc_c = q;
        float xa0 = 0.f, xa1 = 0.f, xa2 = 0.f;
        float xa = w;                                                 // xa = L^-1 D^-1/2 (Z' f), root first
        if (T0) {
          qc0 = ut0 + half_sum_dpp(lmx * u, upper) + ml10 * ut1 + ml20 * ut2;
          qc1 = ut1 + half_sum_dpp(lmy * u, upper) + ml21 * ut2;
          qc2 = ut2 + half_sum_dpp(lmz * u, upper);
          xa0 = wt0 * sd0; xa1 = fmaf(-ml10, xa0, wt1 * sd1); xa2 = fmaf(-ml21, xa1, fmaf(-ml20, xa0, wt2 * sd2));
          xa = fmaf(-lmx, xa0, xa); xa = fmaf(-lmy, xa1, xa); xa = fmaf(-lmz, xa2, xa);
        }
        {
          const unsigned lmask = (unsigned)opaque_s((int)((1u << M.dual_maxdep) - (1u << T0)));      // levels T0 .. maxdep - 1 (fmj_dual2.inc)
#pragma unroll
          for (int g = 0; g < MAXD / 4; g++) {
            const unsigned aw_ = (unsigned)opaque((int)ancl[g]);      // its own copy per sweep: shared, the 17 lane addresses stay live across the whole step and spill
#pragma unroll
            for (int k = 0; k < 4; k++) {
              const int lvl = 4 * g + k;
              if (__builtin_expect((lmask & (1u << lvl)) != 0u, 1)) {
                const int src = (int)((aw_ >> (8 * k)) & 0xffu) + 4 * hb;
                const float xs_ = __int_as_float(__builtin_amdgcn_ds_bpermute(src, __float_as_int(xa)));
                const float rl_ = k == 0 ? myrow[g].x : (k == 1 ? myrow[g].y : (k == 2 ? myrow[g].z : myrow[g].w));
                xa = fmaf((isd && lvl < opaque(ddq)) ? -rl_ : 0.f, xs_, xa);
              }
            }
          }
        }
        if (isd) { const float qa = xsm + xa; QW[mydof] = qa; if (!(fabsf(qa) <= 1e10f)) warn |= FMJ_WARN_BADQACC; }
        if (T0 && sl == 0) {
          const float q0 = XS[0] + xa0, q1 = XS[1] + xa1, q2 = XS[2] + xa2;
          QW[0] = q0; QW[1] = q1; QW[2] = q2;
          if (!(fabsf(q0) <= 1e10f) || !(fabsf(q1) <= 1e10f) || !(fabsf(q2) <= 1e10f)) warn |= FMJ_WARN_BADQACC;
        }
        // (10) sensors: joint limit force
        if (act_lo) lf += EP[e_lo * 8 + 4];
        if (act_hi) lf += EP[e_hi * 8 + 4];
      }
      if (!FUSED && A.dbg_efc) {     // fmj_step_debug: the rows of this step as the solver left them
        float AS1* o = gptr(A.dbg_efc) + (size_t)env_r * M.maxefc * 8;
        for (int i = RL; i < nefc_r * 8; i += NAR) o[i] = EP[i];
      }
      STAMP(20);  // qfrc_constraint + warm start
      // contact forces in the contact frame (mj_contactForce, pyramidal) complete the records: force(3) + geom1 << 16 | geom2
      for (int c = RL; c < ncon_r; c += NAR) {
        const float* ep = EP + (nlim_r + 4 * c) * 8;
        const float f0 = ep[4], f1 = ep[12], f2 = ep[20], f3 = ep[28], mu = ep[7];
        float* ct = eCT + c * 16;
        const int g2 = __float_as_int(ct[14]) & 0xffff, g1 = __float_as_int(ct[15]) & 0xffff;
        ct[12] = f0 + f1 + f2 + f3; ct[13] = mu * (f0 - f1); ct[14] = mu * (f2 - f3);
        ct[15] = __int_as_float((g1 << 16) | g2);
      }
      WSYNC();
      }
#undef BCR
#undef BCD
#undef RSUM
    }
