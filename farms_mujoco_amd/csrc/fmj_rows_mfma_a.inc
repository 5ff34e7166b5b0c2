// fmj_rows_mfma_a.inc - A = Z Z' of up to 64 constraint rows on the matrix cores, shared by fmj_cons_rows.inc (one-env kernel, on-chip
// copy) and fmj_cons2_rows.inc (two-env constraint kernel): a block of statements on the including code's locals.
// Every row of Z spread over the dofs (entry k = the row's entry at the depth of dof k if dof k lies on its chain, else 0) makes A a
// plain product: 32 x 32 x 2 fp32 MFMA steps over pairs of dofs, operand lane i = row i & 31 of the block of 32 rows, dof 2t + (i >> 5).
// The result leaves column j (= row j, A is symmetric) in lanes j and j + 32, half of its entries each, and v_permlane32_swap of two
// results puts both halves of the first into lanes 0 .. 31 and of the second into lanes 32 .. 63.  Same operands and the same order of
// the sums for both kernels: an env gets the same A from either.
// reads  lane, nv, RS, LCB (depth of the deepest dof two chains share), YC (rows of Z, [64][RS]), CHN (per row: last dof of its chain + 1)
// defines kh, r32, nsteps, f16_t and the macros ZOP (operand of one step) / SWAP32, which the includer #undefs;
//         writes areg[0 .. 63]: lane j's row j of A (rows 32 .. 63 exact zeros with at most 32 rows)
// the includer supplies MFMA_A_NEFC (the number of rows) and may set MFMA_A_OPERANDS_ONLY to stop after the definitions
    typedef float f16_t __attribute__((ext_vector_type(16)));
    const int kh = lane >> 5, r32 = lane & 31;
    const int nsteps = (nv + 1) >> 1;
#define ZOP(YC_, CH_, DK_, K_) ({ const int ch_ = (CH_); const int lc_ = ch_ >= 0 && (K_) < nv ? (int)LCB[(K_) * nv + ch_] : -2; \
                                   lc_ == (DK_) ? (YC_)[(DK_)] : 0.f; })
#define SWAP32(x_, y_) { const auto sw_ = __builtin_amdgcn_permlane32_swap(__float_as_uint(x_), __float_as_uint(y_), false, false); \
                         x_ = __uint_as_float(sw_[0]); y_ = __uint_as_float(sw_[1]); }
#if !MFMA_A_OPERANDS_ONLY
    const float* const yc0 = YC + r32 * RS;
    const float* const yc1 = yc0 + 32 * RS;
    const int ch0 = r32 < MFMA_A_NEFC ? (int)CHN[r32] - 1 : -1;
    const int ch1 = r32 + 32 < MFMA_A_NEFC ? (int)CHN[r32 + 32] - 1 : -1;
    f16_t a00, a01, a10, a11;
#pragma unroll
    for (int v = 0; v < 16; v++) { a00[v] = 0.f; a01[v] = 0.f; a10[v] = 0.f; a11[v] = 0.f; }
    if (MFMA_A_NEFC > 32) {
      for (int t = 0; t < nsteps; t++) {
        const int k = 2 * t + kh;
        const int dk = k < nv ? (int)LCB[k * nv + k] : -1;
        const float z0 = ZOP(yc0, ch0, dk, k), z1 = ZOP(yc1, ch1, dk, k);
        a00 = __builtin_amdgcn_mfma_f32_32x32x2f32(z0, z0, a00, 0, 0, 0);      // rows (operand 1) x columns (operand 2): the lane keeps a column = a row of A
        a01 = __builtin_amdgcn_mfma_f32_32x32x2f32(z0, z1, a01, 0, 0, 0);
        a10 = __builtin_amdgcn_mfma_f32_32x32x2f32(z1, z0, a10, 0, 0, 0);
        a11 = __builtin_amdgcn_mfma_f32_32x32x2f32(z1, z1, a11, 0, 0, 0);
      }
    } else {
      for (int t = 0; t < nsteps; t++) {
        const int k = 2 * t + kh;
        const int dk = k < nv ? (int)LCB[k * nv + k] : -1;
        const float z0 = ZOP(yc0, ch0, dk, k);
        a00 = __builtin_amdgcn_mfma_f32_32x32x2f32(z0, z0, a00, 0, 0, 0);
      }
      // swapped with the zeros of a01: both halves of every column to lanes 0 .. 31, exact zeros to the lanes without rows
    }
#pragma unroll
    for (int v = 0; v < 16; v++) {
      float x_ = a00[v], y_ = a01[v];
      SWAP32(x_, y_);
      areg[8 * (v >> 2) + (v & 3)] = x_; areg[8 * (v >> 2) + 4 + (v & 3)] = y_;
      float x1_ = a10[v], y1_ = a11[v];
      SWAP32(x1_, y1_);
      areg[32 + 8 * (v >> 2) + (v & 3)] = x1_; areg[32 + 8 * (v >> 2) + 4 + (v & 3)] = y1_;
    }
#endif
