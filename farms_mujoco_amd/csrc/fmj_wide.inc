// fmj_wide.inc — the two-wave step kernel: one workgroup of 128 threads (two wavefronts) per environment, for unconstrained models
// of up to 128 bodies and 128 dofs (included from fmj_hip.hip).
//
// Lane t of the workgroup is body t and dof t, as in fmj_step_kernel<FUSED, MAXD, false>, and each dof lane keeps its row of H in
// registers (MAXD = rs <= FMJ_MAXD_DEEP: the dof chain still fits one register row).  What changes is every cross-lane step, because
// the partner of a lane (a parent body, an ancestor dof, a pivot of the factorisation) may live in the other wave:
//   K / V   pointer jumping along the body chains: each round publishes the lane's value in LDS (two buffers, alternating), one
//           workgroup barrier per round, and reads the partner's
//   C       tree CoM: DPP reduction inside each wave, the two partial sums combined through LDS (wave 0 + wave 1, on every lane)
//   S       subtree sums: the fp64 DPP prefix inside each wave is stored in LDS for all twelve sums, one barrier, then every lane
//           forms P[last] - P[lane - 1] with wave 0's total added to the prefixes of wave 1
//   L       L'DL by rounds of unrelated dofs (WideRoundW: lane masks of 128 bits, one 64-bit word per wave); the pivot rows, 1 / D
//           and the swept right-hand side are published through LDS, two barriers per round
//   X       the root-first sweep: the dofs at depth lvl publish their final x, one barrier, their descendants pull it
//   freeze  decided by a workgroup OR (wg_or: wave OR, LDS, barrier) before any lane commits a store; every barrier is reached by
//           all 128 threads (uniform loop bounds, no early return)
// Results do not depend on the partner wave's timing: every LDS value is read only after the barrier that follows its write, and
// no slot is rewritten before a barrier that follows its last read.

#define FMJ_WIDE_LANES 128
#define FMJ_WIDE_XCH (12 * FMJ_WIDE_LANES * 2)   // exchange area in floats: 12 fp64 prefix rows (S), or 2 x 128 x 8 floats (K / V)

struct LdsLayoutW {
  LdsLayout L;        // the unconstrained one-env layout for nb, nv (<= 128)
  int XCH, XW, RED, FLG, total;
};
__host__ __device__ inline LdsLayoutW ldsw_layout(int nb, int nv, int nq, int rs, int anc_stride) {
  LdsLayoutW W;
  W.L = lds_layout(nb, nv, nq, rs, anc_stride);
  int o = W.L.total;
  W.XCH = o; o += FMJ_WIDE_XCH;
  W.XW = o; o += FMJ_WIDE_LANES;       // x of the factorisation / the sweep, published per lane
  W.RED = o; o += 8;                   // partial CoM sums of the two waves
  W.FLG = o; o += 8;                   // wg_or slots: two words per call site
  W.total = r4(o);
  return W;
}

// OR of v over the workgroup, on every lane.  slot: two ints of LDS owned by one call site; a call site is reached again only after
// later barriers, so a slot is never rewritten while a lane may still read it.
__device__ __forceinline__ int wg_or(int v, int* slot) {
  int w = v;
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) w |= __shfl_xor(w, o, 64);
  if ((threadIdx.x & 63) == 0) slot[threadIdx.x >> 6] = w;
  __syncthreads();
  return slot[0] | slot[1];
}

// L'DL of H with the right-hand side swept leaves-first in the rounds (ldl_factor of the one-env kernel, workgroup form).  On return
// HR holds L (unit diagonal, rows scaled by 1 / D), dinv_mine = 1 / D_lane and x the swept right-hand side.
template <int MAXD>
__device__ __forceinline__ void ldl_factor_wg(float* HR, float* DV, float* XW, const WideRoundW* rounds, int nround, int lane, int wv, bool isd,
                                              int ddepth, f2_t (&r)[MAXD / 2], float diag, float& dinv_mine, float& x) {
  constexpr int RS = MAXD;
  typedef const WideRoundW __attribute__((address_space(4)))* wround_p;
  const wround_p RND = (wround_p)rounds;
#define APPLY_PIVOT_W(NG_, p_, am_) do { \
    const float tk_ = HR[(p_) * RS + ddepth]; const float dki_ = DV[p_]; const float xk_ = XW[p_]; \
    float4 rk_[NG_]; \
    _Pragma("unroll") for (int g = 0; g < NG_; g++) rk_[g] = *(const float4*)(HR + (p_) * RS + 4 * g); \
    const float t_ = mask_select(tk_ * dki_, am_); \
    const f2_t tt_ = f2_t{t_, t_}; \
    _Pragma("unroll") for (int g = 0; g < NG_; g++) { \
      pk_fnma(r[2 * g], tt_, f2_t{rk_[g].x, rk_[g].y}); \
      pk_fnma(r[2 * g + 1], tt_, f2_t{rk_[g].z, rk_[g].w}); } \
    diag = fmaf(-t_, tk_, diag); \
    x = fmaf(-t_, xk_, x); } while (0)
#define ROUND_BODY_W(NG_) do { \
    if (isd) { \
      _Pragma("unroll") for (int d = 0; d < 4 * NG_; d += 4) *(float4*)(HR + lane * RS + d) = make_float4(r[d / 2].x, r[d / 2].y, r[d / 2 + 1].x, r[d / 2 + 1].y); \
      DV[lane] = __builtin_amdgcn_rcpf(diag); XW[lane] = x; \
    } \
    __syncthreads(); \
    APPLY_PIVOT_W(NG_, p0, a0); \
    if (np > 1) { APPLY_PIVOT_W(NG_, p1, a1); APPLY_PIVOT_W(NG_, p2, a2); } \
    if (np > 3) { APPLY_PIVOT_W(NG_, p3, a3); APPLY_PIVOT_W(NG_, p4, a4); APPLY_PIVOT_W(NG_, p5, a5); } \
    __syncthreads(); } while (0)
  {
    int p0 = RND[0].p[0], p1 = RND[0].p[1], p2 = RND[0].p[2], p3 = RND[0].p[3], p4 = RND[0].p[4], p5 = RND[0].p[5], dep = RND[0].depth, np = RND[0].np;
    unsigned long long a0 = RND[0].anc[0][wv], a1 = RND[0].anc[1][wv], a2 = RND[0].anc[2][wv], a3 = RND[0].anc[3][wv], a4 = RND[0].anc[4][wv], a5 = RND[0].anc[5][wv];
    int rd = 0;
#define ROUNDS_AT_W(NG_, COND_) \
    _Pragma("unroll 1") while (rd < nround && (COND_)) { \
      const int rn = rd + 1 < nround ? rd + 1 : rd; \
      const int np0 = RND[rn].p[0], np1 = RND[rn].p[1], np2 = RND[rn].p[2], np3 = RND[rn].p[3], np4 = RND[rn].p[4], np5 = RND[rn].p[5], ndep = RND[rn].depth, nnp = RND[rn].np; \
      const unsigned long long na0 = RND[rn].anc[0][wv], na1 = RND[rn].anc[1][wv], na2 = RND[rn].anc[2][wv], na3 = RND[rn].anc[3][wv], na4 = RND[rn].anc[4][wv], na5 = RND[rn].anc[5][wv]; \
      ROUND_BODY_W(NG_); \
      p0 = np0; p1 = np1; p2 = np2; p3 = np3; p4 = np4; p5 = np5; a0 = na0; a1 = na1; a2 = na2; a3 = na3; a4 = na4; a5 = na5; dep = ndep; np = nnp; rd++; \
    }
    DEPTH_LADDER(ROUNDS_AT_W, true)
#undef ROUNDS_AT_W
  }
#undef ROUND_BODY_W
#undef APPLY_PIVOT_W
  dinv_mine = isd ? __builtin_amdgcn_rcpf(diag) : 0.f;
  if (isd) {
#pragma unroll
    for (int d = 0; d < MAXD; d += 4)
      *(float4*)(HR + lane * RS + d) = make_float4(r[d / 2].x * dinv_mine, r[d / 2].y * dinv_mine, r[d / 2 + 1].x * dinv_mine, r[d / 2 + 1].y * dinv_mine);
  }
  __syncthreads();
}

// Root-first sweep x_d -= L[d][a] x_a over the proper ancestors a of d, a tree level at a time: at level lvl the dofs of depth lvl
// (whose x is final) publish it, and every deeper dof pulls its ancestor's.  ancw: per dof and depth, the lane of the ancestor at that
// depth (one byte each; the dof's own lane where there is none).  A slot of XW is written once, at its dof's own level.
template <int MAXD>
__device__ __forceinline__ float ldl_pull_sweep_wg(const float* HR, float* XW, float x, int lane, int dli, bool isd, int ddepth, const uint32_t* ancw, int maxdep) {
  constexpr int RS = MAXD;
  maxdep = opaque_s(maxdep);
  float4 row[MAXD / 4];
#pragma unroll
  for (int g = 0; g < MAXD / 4; g++) row[g] = *(const float4*)(HR + dli * RS + 4 * g);
#pragma unroll
  for (int g = 0; g < MAXD / 4; g++) {
    const uint32_t ab = gptr(ancw)[(unsigned)dli * (MAXD / 4) + g];
#pragma unroll
    for (int k = 0; k < 4; k++) {
      const int lvl = 4 * g + k;
      if (lvl < maxdep) {                       // uniform
        if (isd && ddepth == lvl) XW[lane] = x;
        __syncthreads();
        const float xs = XW[(ab >> (8 * k)) & 0xffu];
        const float rl = k == 0 ? row[g].x : (k == 1 ? row[g].y : (k == 2 ? row[g].z : row[g].w));
        x = fmaf((isd && lvl < ddepth) ? -rl : 0.f, xs, x);
      }
    }
  }
  return x;
}

// Subtree sum of scan j over [lane, last] from the per-wave inclusive prefixes PS[j][*] (fp64): wave 0's total joins the prefixes of
// wave 1.  The sum is P(last) - P(lane - 1).
__device__ __forceinline__ double wg_subtree(const double* PS, int j, int lane, int last) {
  const double* P = PS + j * FMJ_WIDE_LANES;
  const double t0 = P[63];
  const double hi = P[last] + (last >= 64 ? t0 : 0.0);
  const double lo = lane > 0 ? P[lane - 1] + (lane - 1 >= 64 ? t0 : 0.0) : 0.0;
  return hi - lo;
}

template <bool FUSED, int MAXD>
__global__ void __launch_bounds__(FMJ_WIDE_LANES, MAXD > 32 ? 2 : 3) fmj_step_wide_kernel(const DevModel M_by_value, const StepArgs A_by_value) {
  extern __shared__ __align__(16) float lds[];
  const char AS4* const karg = (const char AS4*)__builtin_amdgcn_kernarg_segment_ptr();
  const DevModel AS4* Mp = (const DevModel AS4*)karg;
  const StepArgs AS4* Ap = (const StepArgs AS4*)(karg + FMJ_KARG_A_OFF);
#define M (*Mp)
#define A (*Ap)
  const int env = A.env_order ? gptr(A.env_order)[blockIdx.x] : blockIdx.x;
  const int lane = threadIdx.x;
  const int wv = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);     // this lane's wave (uniform inside it)
  const int nb = M.nbody, nv = M.nv, nq = M.nq, nu = M.nu;
  constexpr int RS = MAXD;                     // row stride of H == register row length (dispatch guarantees M.rs == MAXD)
  constexpr bool CONS = false;                 // the shared stages (fmj_stage_*.inc) test it: this kernel has no constraints
  const LdsLayoutW LW = ldsw_layout(nb, nv, nq, RS, M.anc_stride);
  const LdsLayout& LL = LW.L;
  float* F = lds + LL.P1;
  float* CI = lds + LL.CI;
  float* CD = lds + LL.CD;
  float* HR = lds + LL.HR;
  float* QP = lds + LL.QP;
  float* QV = lds + LL.QV;
  float* XV = lds + LL.XV;
  float* XCH = lds + LW.XCH;
  float* XW = lds + LW.XW;
  float* RED = lds + LW.RED;
  int* FLG = (int*)(lds + LW.FLG);
  const uint8_t* JMP = (const uint8_t*)(lds + LL.ANC);

  const bool isb = lane > 0 && lane < nb;
  const int bl = isb ? lane : 0;
  const bool isd = lane < nv;
  const int dl = isd ? lane : 0;
  const int4 d_info0 = DTABI(dl, 0);
  const int ddepth_o = isd ? d_info0.y : 0;

  // ---- load tables + state -------------------------------------------------------------------------
  int warn = 0;
  for (int i = lane * 4; i < LW.total; i += 4 * FMJ_WIDE_LANES) *(float4*)(lds + i) = make_float4(0.f, 0.f, 0.f, 0.f);
  __syncthreads();
  {
    uint32_t* jw = (uint32_t*)(lds + LL.ANC);
    const int nw = r4(nb * M.anc_stride) / 4;
    for (int i = lane; i < nw; i += FMJ_WIDE_LANES) jw[i] = ((const uint32_t*)M.b_anc)[i];
  }
  {
    const float* gq = glob(A.qpos) + (size_t)env * nq;
    const float* gv = glob(A.qvel) + (size_t)env * nv;
    for (int i = lane; i < nq; i += FMJ_WIDE_LANES) { const float v = gq[i]; QP[i] = v; if (!(fabsf(v) <= 1e10f)) warn |= FMJ_WARN_BADQPOS; }   // mj_checkPos
    for (int i = lane; i < nv; i += FMJ_WIDE_LANES) { const float v = gv[i]; QV[i] = v; if (!(fabsf(v) <= 1e10f)) warn |= FMJ_WARN_BADQVEL; }   // mj_checkVel
  }
#include "fmj_stage_carry_in.inc"      // xf, cy_actsum
  // frozen (include/fmj.h): decided for the whole workgroup
  bool frozen = (gptr(A.status)[env] & FMJ_WARN_FREEZE) != 0;
  frozen = wg_or(warn & FMJ_WARN_FREEZE, FLG + 0) != 0 || frozen;
  int steps_done = 0;
  if (FUSED && !frozen && A.n_steps > 0) {
    const int cl = lane < nb ? lane : 0;
    const float* p = glob(A.xpos) + (size_t)env * nb * 3 + cl * 3;
    const float4 q = *(const float4*)(glob(A.xquat) + (size_t)env * nb * 4 + cl * 4);
    const float* ip = glob(A.xipos) + (size_t)env * nb * 3 + cl * 3;
    const float* sd = glob(A.sensordata) + (size_t)env * M.nsensordata + 6 * (isb ? lane - 1 : 0);
    const int4 ci2 = BTABI(bl, 8);
    const q4 cq = {q.x, q.y, q.z, q.w};
    emit_links_and_drag(M, A, env, A.iteration0, isb, false, ci2.z, ci2.w, mk3(p[0], p[1], p[2]), cq, mk3(ip[0], ip[1], ip[2]),
                        mk3(sd[0], sd[1], sd[2]), mk3(sd[3], sd[4], sd[5]), xf);
  }
  __syncthreads();

  const int lane_outer = lane;
  int sub = 0, itm = 0;
#pragma unroll 1
  for (int step = 0; step < A.n_steps; step++) {
    if (frozen) break;                          // uniform: every freeze decision is a workgroup OR
#include "fmj_stage_step_head.inc"      // lane, it, last, S_sub, full, nsub, nfull, nit, blo, dlo
    const int ddepth = opaque(ddepth_o);
    // ============ before_step: joints row (physics.py:500-524) ============
    if (FUSED && A.do_readout && full) {
      const int4 di = DTABI(dlo, 0);
      const float4 dp = DTAB(dlo, 1);
      if (isd && dp.w != 0.f && di.w >= 0) {
        const int index = it % A.buffer_size;
        float AS1* row = gptr(A.joints) + ((size_t)index * A.row_stride_joints + (size_t)env * M.n_joints * FMJ_JOINT_SIZE) + di.w * FMJ_JOINT_SIZE;
        stg4(row + 0, QP[__float_as_int(dp.z)], QV[lane] * A.inv_angvel, 0.f, 0.f);
        stg4(row + 4, 0.f, 0.f, 0.f, 0.f);
        stg4(row + 8, cy_actsum, 0.f, 0.f, 0.f);
      }
    }
    // ============ mj_step ============
    const int4 c_info = BTABI(blo, 7);        // parent, jtype, qadr, dadr
    const int jtype = isb ? c_info.y : -1;
    const int qadr = c_info.z, dadr = c_info.w;
    const float4 c_axis_q0 = BTAB(blo, 5);
    const float4 c_jpos_k = BTAB(blo, 6);
    const bool any_jpos = M.any_jpos != 0, any_bquat = M.any_bquat != 0, any_iquat = M.any_iquat != 0;
    const uint32_t jm = lane < nb ? *(const uint32_t*)(JMP + lane * M.anc_stride) : 0u;   // jumping rounds 0..3
#define JUMP_SRC(r_) ((r_) < 4 ? (int)((jm >> (8 * (r_))) & 0xff) : (lane < nb ? (int)JMP[lane * M.anc_stride + (r_)] : 0))
    // ---- K: local transforms, composed along the chains by pointer jumping through LDS (buffer r & 1)
    v3 xp; q4 xq;
    {
#include "fmj_stage_k.inc"      // the body's local transform (xp, xq)
      for (int r = 0; r < M.max_bdepth; r++) {
        float* X = XCH + (r & 1) * (FMJ_WIDE_LANES * 8);
        *(float4*)(X + lane * 8) = make_float4(xp.x, xp.y, xp.z, 0.f);
        *(float4*)(X + lane * 8 + 4) = make_float4(xq.w, xq.x, xq.y, xq.z);
        __syncthreads();
        const int a = JUMP_SRC(r);
        const float4 pa = *(const float4*)(X + a * 8), qa = *(const float4*)(X + a * 8 + 4);
        const q4 aqq = {qa.x, qa.y, qa.z, qa.w};
        xp = add3(mk3(pa.x, pa.y, pa.z), qrot(aqq, xp));
        xq = qmul(aqq, xq);
      }
      xq = qnormalize(xq);
    }
    v3 xi;
    {
      const float4 c_ipos = BTAB(blo, 2);
      xi = add3(xp, qrot(xq, mk3(c_ipos.x, c_ipos.y, c_ipos.z)));
    }
    // ---- C: tree CoM: a DPP reduction per wave, the two partial sums through LDS (the barrier also closes K's last reads)
    const float mass = isb ? BTAB(blo, 0).w : 0.f;
    v3 com;
    {
      const float sx = wave_sum_fast(mass * xi.x), sy = wave_sum_fast(mass * xi.y), sz = wave_sum_fast(mass * xi.z);
      if ((lane & 63) == 0) *(float4*)(RED + 4 * wv) = make_float4(sx, sy, sz, 0.f);
      __syncthreads();
      const float4 r0 = *(const float4*)RED, r1 = *(const float4*)(RED + 4);
      com = mk3((r0.x + r1.x) * M.mtot_inv, (r0.y + r1.y) * M.mtot_inv, (r0.z + r1.z) * M.mtot_inv);
    }
#include "fmj_stage_c.inc"      // iw: world-frame inertia about the body's own CoM
    // ---- V: vJ, cvel = chain sum of vJ, cacc = a0 + chain sum of cvel_parent x vJ (exchanges alternate between the two buffers)
    s6 cv, ca;
    {
#include "fmj_stage_v.inc"      // cdof into CD, joint velocity vJ, vt
      int xb = 0;
#define XPULL6(dst_, src_, v_) do { \
        float* X_ = XCH + xb * (FMJ_WIDE_LANES * 8); \
        lds_put6(X_ + lane * 8, v_); \
        __syncthreads(); \
        dst_ = lds_get6(X_ + (src_) * 8); \
        xb ^= 1; } while (0)
      cv = s6add(vJ, vt);
      for (int r = 0; r < M.max_bdepth; r++) {
        s6 o; XPULL6(o, JUMP_SRC(r), cv);
        cv = s6add(cv, o);
      }
      s6 cpar; XPULL6(cpar, isb ? c_info.x : 0, cv);
      cpar = s6add(cpar, vt);
      ca = cross_motion(cpar, vJ);
      if (!isb) { ca.r = ca.l = mk3(0.f, 0.f, 0.f); }
      for (int r = 0; r < M.max_bdepth; r++) {
        s6 o; XPULL6(o, JUMP_SRC(r), ca);
        ca = s6add(ca, o);
      }
#undef XPULL6
      ca.l = sub3(ca.l, mk3(M.gx, M.gy, M.gz));
      if (!isb) { cv.r = cv.l = mk3(0.f, 0.f, 0.f); }
    }
#undef JUMP_SRC
#include "fmj_stage_f.inc"      // F: fbody; the next links row and drag; on the last step the pose and velocimeter stores
    __syncthreads();                                // V's last reads of XCH are done: S overwrites it
    // ---- S: subtree sums over the contiguous DFS range [lane, last], fp64: twelve per-wave prefixes into LDS, one barrier, then
    // differences of workgroup prefixes; the composite inertia is moved to the subtree's own CoM as in the one-env kernel
    {
      double* PS = (double*)XCH;
      const int lastb = isb ? lane + BTABI(blo, 8).y - 1 : lane;
      const double dm = (double)mass;
      const double dx = (double)xi.x - (double)com.x, dy = (double)xi.y - (double)com.y, dz = (double)xi.z - (double)com.z;
#define SCAN_W(j_, expr) do { PS[(j_) * FMJ_WIDE_LANES + lane] = wave_prefix_f64(expr); } while (0)
      SCAN_W(0, dm * dx); SCAN_W(1, dm * dy); SCAN_W(2, dm * dz);
      SCAN_W(3, (double)pinf(iw[0]) + dm * (dy * dy + dz * dz));
      SCAN_W(4, (double)pinf(iw[1]) + dm * (dx * dx + dz * dz));
      SCAN_W(5, (double)pinf(iw[2]) + dm * (dx * dx + dy * dy));
      SCAN_W(6, (double)pinf(iw[3]) - dm * dx * dy);
      SCAN_W(7, (double)pinf(iw[4]) - dm * dx * dz);
      SCAN_W(8, (double)pinf(iw[5]) - dm * dy * dz);
      SCAN_W(9, (double)pinf(fbody.r.x)); SCAN_W(10, (double)pinf(fbody.r.y)); SCAN_W(11, (double)pinf(fbody.r.z));
#undef SCAN_W
      // the linear force sums need three more rows: they reuse rows 0..2 after the CoM sums are read
      __syncthreads();
      const double ms = (double)BTAB(blo, 2).w;
      const double minv = ms > 0.0 ? rcp_f64_nr(ms) : 0.0;
      const double ex = wg_subtree(PS, 0, lane, lastb) * minv, ey = wg_subtree(PS, 1, lane, lastb) * minv, ez = wg_subtree(PS, 2, lane, lastb) * minv;
      const float i0 = pinf((float)(wg_subtree(PS, 3, lane, lastb) - ms * (ey * ey + ez * ez)));
      const float i1 = pinf((float)(wg_subtree(PS, 4, lane, lastb) - ms * (ex * ex + ez * ez)));
      const float i2 = pinf((float)(wg_subtree(PS, 5, lane, lastb) - ms * (ex * ex + ey * ey)));
      const float i3 = pinf((float)(wg_subtree(PS, 6, lane, lastb) + ms * ex * ey));
      const float i4 = pinf((float)(wg_subtree(PS, 7, lane, lastb) + ms * ex * ez));
      const float i5 = pinf((float)(wg_subtree(PS, 8, lane, lastb) + ms * ey * ez));
      s6 fs;
      fs.r.x = pinf((float)wg_subtree(PS, 9, lane, lastb));
      fs.r.y = pinf((float)wg_subtree(PS, 10, lane, lastb));
      fs.r.z = pinf((float)wg_subtree(PS, 11, lane, lastb));
      __syncthreads();
      PS[0 * FMJ_WIDE_LANES + lane] = wave_prefix_f64((double)pinf(fbody.l.x));
      PS[1 * FMJ_WIDE_LANES + lane] = wave_prefix_f64((double)pinf(fbody.l.y));
      PS[2 * FMJ_WIDE_LANES + lane] = wave_prefix_f64((double)pinf(fbody.l.z));
      __syncthreads();
      fs.l.x = pinf((float)wg_subtree(PS, 0, lane, lastb));
      fs.l.y = pinf((float)wg_subtree(PS, 1, lane, lastb));
      fs.l.z = pinf((float)wg_subtree(PS, 2, lane, lastb));
      if (lane < nb) {
        *(float4*)(CI + lane * 12) = make_float4(i0, i1, i2, i3);
        *(float4*)(CI + lane * 12 + 4) = make_float4(i4, i5, (float)((double)com.x + ex), (float)((double)com.y + ey));
        *(float2*)(CI + lane * 12 + 8) = make_float2((float)((double)com.z + ez), (float)ms);
        lds_put6(F + lane * 8, fs);
      }
    }
    __syncthreads();
#include "fmj_stage_q.inc"      // Q: qfrc_smooth with actuation (lane = dof); defines qfrc, dvel, cd, bf, sc, d_prm, d_act, d_qadr, d_scalar
    __syncthreads();
    // ---- M (ancestor lanes from the wide table: one byte = one lane)
#define MROW_ANCL M.anclw
#define MROW_LANE(byte_) ((int)(byte_))
#include "fmj_stage_m.inc"
#undef MROW_ANCL
#undef MROW_LANE
    __syncthreads();                                // the published rows overlay CD / F / CI from here
#include "fmj_stage_dbg_h.inc"      // fmj_forward_debug: the rows of H and the right-hand side
    // ---- L + X
    float my_qacc;
    {
      float dinv_h = 0.f;
      float xr = isd ? qfrc : 0.f;
      ldl_factor_wg<MAXD>(HR, XV, XW, M.roundsw, M.nroundw, lane, wv, isd, ddepth, hrow, hdg_h, dinv_h, xr);
      my_qacc = ldl_pull_sweep_wg<MAXD>(HR, XW, xr * dinv_h, lane, isd ? lane : 0, isd, ddepth, M.anclw, M.maxdep1);
    }
#include "fmj_stage_euler_check.inc"      // semi-implicit Euler: nvel and the warn tests ...
    if (wg_or(warn & FMJ_WARN_FREEZE, FLG + 2) != 0) frozen = true;      // the freeze is decided for the workgroup before any lane commits
#include "fmj_stage_euler_commit.inc"      // ... the commit of XV / QV / QP and the joint sensors ...
    __syncthreads();
#include "fmj_stage_euler_root.inc"      // ... and the free root's position and quaternion
    if (wg_or(warn & FMJ_WARN_BADQPOS, FLG + 4) != 0) frozen = true;   // (its barrier also orders the root update before the next step)
    sub = nsub; itm += nfull ? 1 : 0;
  }

  // ---- store state ---------------------------------------------------------------------------------------
  float* oq = glob(A.qpos) + (size_t)env * nq;
  float* ov = glob(A.qvel) + (size_t)env * nv;
  for (int i = lane; i < nq; i += FMJ_WIDE_LANES) oq[i] = QP[i];
  for (int i = lane; i < nv; i += FMJ_WIDE_LANES) ov[i] = QV[i];
  if (A.qacc && steps_done > 0) for (int i = lane; i < nv; i += FMJ_WIDE_LANES) gptr(A.qacc)[(size_t)env * nv + i] = XV[i];
  if (A.time && lane == 0 && A.integrate) gptr(A.time)[env] += M.h * steps_done;
  const int w = wg_or(warn, FLG + 6);
  if (w != 0 && lane == 0) gptr(A.status)[env] |= w;
#undef M
#undef A
}
