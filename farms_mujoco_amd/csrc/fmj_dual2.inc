// fmj_dual2.inc - the "two environments per wavefront" step kernel (included by fmj_hip.hip).
//
// Why: with one env per wave only ~half of the 64 lanes carry data (29 bodies / 33 dofs for the salamander) and the
// kernel is VALU-issue bound, so packing two envs into one wave halves the instructions per env.  Lanes 0..31
// serve env 2*blockIdx.x, lanes 32..63 env 2*blockIdx.x + 1; every cross-lane operation is confined to a half
// (DPP rows stop at row_bcast:15, v_readlane pairs, ds_bpermute inside the half).
//
// The 32-lane budget holds the bodies (nbody <= 32) and the dofs EXCEPT the three translational dofs of a free root
// (nv - 3 <= 32): those sit at depths 0..2 of the dof tree, are the last three pivots of the factorisation and
// update nothing else, so they are carried as per-half uniform scalars: their columns live in slots 0..2 of every
// row as usual, their 3x3 Schur complement is accumulated next to the pivot loop and factored in scalar code, and
// the triangular sweeps treat them the same way.  Not for the constraint path - those models keep the one-env kernel.
//
// This is the second generation of the kernel.  Round 1's ran at 256 VGPRs + 47 spilled, 247 spilled SGPRs (every kernel
// argument lived in an SGPR for the whole launch) and 19.4 KB of LDS per workgroup, i.e. 2 waves per SIMD whatever
// the batch size (DESIGN.md section 2).  Here:
//   * kernel arguments are read where they are used, through the kernarg segment (scalar loads, scalar cache), and the
//     pointer is laundered once per step so that nothing is hoisted out of the step loop: no argument is held, or
//     spilled, across the loop;
//   * the rows of H are born in registers: lane = dof i walks its own ancestor chain by depth (static register index)
//     and computes H[i][anc_d(i)] from its own (I_s w_i, m v_i) and the ancestor's cdof; the entry table, the BUF array,
//     the zero fill, the scatter into the LDS rows and the read-back of the factorisation's first round are gone;
//   * the fields of the last forward pass are not carried through LDS: the links row of iteration it + 1 and its drag are
//     emitted by the step that computes them (step it), the row of a launch's first iteration by the prologue;
//   * only the first live actuator slot of a joint is resident; further live slots and the last step's sensor outputs
//     take a cold path that re-reads the tables;
//   * the LDS rows of the factorisation overlay cdof / subtree inertia / subtree force, dead by then.
// Result: <= 128 VGPRs, < 10 KB LDS per workgroup -> 4 waves per SIMD when the batch provides them.

__device__ __forceinline__ float bcast2(float v, int i, bool upper) {      // lane (half*32 + i) of v, for every lane of the half
  const float a = bcast(v, i), b = bcast(v, i + 32);
  return upper ? b : a;
}
__device__ __forceinline__ float half_sum(float v) {                         // sum over the 32 lanes of the half, in every lane
#pragma unroll
  for (int o = 16; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
  return v;
}
// sum over the 32 lanes of the half with DPP (no LDS traffic); the total lands in every lane
__device__ __forceinline__ float half_sum_dpp(float v, bool upper) {
  int x = __float_as_int(v);
  v += __int_as_float(__builtin_amdgcn_update_dpp(0, x, 0xB1, 0xF, 0xF, true));  x = __float_as_int(v);   // quad_perm [1,0,3,2]
  v += __int_as_float(__builtin_amdgcn_update_dpp(0, x, 0x4E, 0xF, 0xF, true));  x = __float_as_int(v);   // quad_perm [2,3,0,1]
  v += __int_as_float(__builtin_amdgcn_update_dpp(0, x, 0x141, 0xF, 0xF, true)); x = __float_as_int(v);   // row_half_mirror
  v += __int_as_float(__builtin_amdgcn_update_dpp(0, x, 0x140, 0xF, 0xF, true)); x = __float_as_int(v);   // row_mirror
  v += __int_as_float(__builtin_amdgcn_update_dpp(0, x, 0x142, 0xA, 0xF, true));                          // row_bcast:15 -> rows 1, 3
  return bcast2(v, 31, upper);
}
// the same sum where EVERY lane of the wave is active (uniform control flow): after the four in-row steps every lane holds its row's
// total; gfx950's v_permlane16_swap exchanges row 1 (3) of one copy with row 0 (2) of another, so the sum of the two copies is the
// half's total in every lane - a move, the swap and an add instead of the row_bcast step, two v_readlane, two moves and a select.
// Same two addends: bitwise the same total (+ 1 % on the headline, round 4 A/B).  Not under a per-half or per-lane condition: the
// swap leaves the rows of inactive lanes alone.
__device__ __forceinline__ float half_sum_all(float v) {
  int x = __float_as_int(v);
  v += __int_as_float(__builtin_amdgcn_update_dpp(0, x, 0xB1, 0xF, 0xF, true));  x = __float_as_int(v);   // quad_perm [1,0,3,2]
  v += __int_as_float(__builtin_amdgcn_update_dpp(0, x, 0x4E, 0xF, 0xF, true));  x = __float_as_int(v);   // quad_perm [2,3,0,1]
  v += __int_as_float(__builtin_amdgcn_update_dpp(0, x, 0x141, 0xF, 0xF, true)); x = __float_as_int(v);   // row_half_mirror
  v += __int_as_float(__builtin_amdgcn_update_dpp(0, x, 0x140, 0xF, 0xF, true));                          // row_mirror
  const unsigned u = __float_as_uint(v);
  const auto sw = __builtin_amdgcn_permlane16_swap(u, u, false, false);
  return __uint_as_float(sw[0]) + __uint_as_float(sw[1]);
}

__device__ __forceinline__ double half_prefix_f64(double v) {               // inclusive prefix inside each 32-lane half
  v += dpp_f64<0x111, 0xF>(v);
  v += dpp_f64<0x112, 0xF>(v);
  v += dpp_f64<0x114, 0xF>(v);
  v += dpp_f64<0x118, 0xF>(v);
  v += dpp_f64<0x142, 0xA>(v);      // row_bcast:15 into rows 1 and 3: row0 -> row1, row2 -> row3
  return v;
}
__device__ __forceinline__ double half_subtree_sum_f64(double x, int src_lane) {
  const double P = half_prefix_f64(x);
  return lane_gather_f64(P, src_lane) - P + x;
}

// LDS layout of one env of the dual2 kernel, in floats (every region 16-byte aligned)
// floats between the published rows of the factorisation: the row, its (1 / D, rhs) pair, rounded to float4s - and never a multiple of
// 8 floats, which would put the 16-byte row writes of a half's 32 lanes on 8 bank groups (4-way conflicts; 2-way at odd multiples of 4)
__host__ __device__ constexpr int dual_row_stride(int rs) { return ((rs + 2 + 3) / 4 * 4) % 8 == 0 ? (rs + 2 + 3) / 4 * 4 + 4 : (rs + 2 + 3) / 4 * 4; }
constexpr int D2S = 12;
struct Lds2 { int QP, QV, XV, CD, F, CI, HR, total; };
__host__ __device__ inline Lds2 lds2_layout(int nb, int nv, int nq, int rs, int t0) {
  Lds2 L; int o = 0;
  L.QP = o; o += r4(nq);
  L.QV = o; o += r4(nv);
  L.XV = o; o += r4(nv);                 // qacc of the last step
  const int r1 = o;
  L.CD = o; o += nv * D2S;               // cdof      (six floats per record, records D2S = 12 floats apart: at 8 the 16-byte
  L.F = o; o += nb * D2S;                // subtree force       accesses of a half fall on 4 bank groups, at 12 on 8)
  L.CI = o; o += nb * 12;                // subtree inertia about its own CoM (6), subtree CoM (3), subtree mass
  L.HR = r1;                             // rows of the lane dofs, from the factorisation on: CD / F / CI are dead by then
  const int hr_end = r1 + 32 * dual_row_stride(rs);  // a row per lane of the half (the rounds publish without a test for 'lane has a dof'), each followed by its (1 / D, rhs)
  if (hr_end > o) o = hr_end;
  L.total = r4(o);
  return L;
}

struct DragEnv { float surface, viscosity, wvx, wvy, wvz, wgravity; int use_buoyancy; };

// drag_link_same_frames with the water constants passed by value (see fmj_hip.hip for the derivation)
__device__ __forceinline__ bool drag_same_frames2(v3 com_pos, q4 q_wxyz, v3 lin_w, v3 ang_w, float4 c0, float4 c1, float mass_over_density,
                                                  float inv_height, const DragEnv W, v3* force_link, v3* force_w, v3* torque_link, v3* torque_w) {
  if (com_pos.z > W.surface) return false;                     // drag.pyx:192-194
  const m33 R = q2m(q_wxyz);
  v3 lin = mk3(R.a[0] * lin_w.x + R.a[3] * lin_w.y + R.a[6] * lin_w.z, R.a[1] * lin_w.x + R.a[4] * lin_w.y + R.a[7] * lin_w.z,
               R.a[2] * lin_w.x + R.a[5] * lin_w.y + R.a[8] * lin_w.z);
  const v3 ang = mk3(R.a[0] * ang_w.x + R.a[3] * ang_w.y + R.a[6] * ang_w.z, R.a[1] * ang_w.x + R.a[4] * ang_w.y + R.a[7] * ang_w.z,
                     R.a[2] * ang_w.x + R.a[5] * ang_w.y + R.a[8] * ang_w.z);
  v3 buoy = mk3(0.f, 0.f, 0.f);
  if (W.use_buoyancy && c0.w > 0.f && com_pos.z < W.surface) {  // drag.pyx:139-146, mass / density and 1 / height from the table
    const float fz = -1000.f * W.wgravity * mass_over_density * fminf(fmaxf(W.surface - com_pos.z, 0.f) * inv_height, 1.f);
    buoy = mk3(R.a[6] * fz, R.a[7] * fz, R.a[8] * fz);
  }
  if (W.wvx != 0.f || W.wvy != 0.f || W.wvz != 0.f) {
    lin.x -= R.a[0] * W.wvx + R.a[3] * W.wvy + R.a[6] * W.wvz;
    lin.y -= R.a[1] * W.wvx + R.a[4] * W.wvy + R.a[7] * W.wvz;
    lin.z -= R.a[2] * W.wvx + R.a[5] * W.wvy + R.a[8] * W.wvz;
  }
  v3 f, t;
  f.x = fabsf(lin.x) * lin.x * (W.viscosity * c0.x) + buoy.x;   // drag.pyx:83-88
  f.y = fabsf(lin.y) * lin.y * (W.viscosity * c0.y) + buoy.y;
  f.z = fabsf(lin.z) * lin.z * (W.viscosity * c0.z) + buoy.z;
  t.x = fabsf(ang.x) * ang.x * c1.x; t.y = fabsf(ang.y) * ang.y * c1.y; t.z = fabsf(ang.z) * ang.z * c1.z;   // :104-108
  *force_link = f; *torque_link = t;
  *force_w = mrot(R, f); *torque_w = mrot(R, t);
  return true;
}

// WPS = waves per SIMD the build is registered for: 4 (128 VGPRs, ~40 values spilled around the fp64 scans) when the batch
// provides more than three waves per SIMD, else 3 (<= 168 VGPRs: 157 used, nothing spilled).
// SUBS: the launch runs sub-steps (fmj_fused_args::substeps > 1).  Its own instantiation: the bookkeeping of sub-steps - two more
// loop-carried scalars, two argument loads and a dozen scalar instructions per step - cost the headline configuration (no
// sub-steps) 1.7 % when it was decided at run time (same-box A/B, round 4).  The same instantiation carries the other rarely used
// option, the implicitfast integrator (one compare pair per actuator and one more live register: 1.4 % of the headline when every
// build had it), so a launch with substeps = 1 of an implicitfast model also runs it.
// LEAN: the launch has the shape of a fused Simulation.run() with the device wave controller - rows written by the launch itself
// (no rows_ahead), readout and drag on, controller 1, actuation enabled, integrating, no joint stiffness, none of the SUBS options -
// which launch_step checks on the host before it picks this instantiation.  Every OPT_* below is then a constant instead of a scalar
// load through the laundered argument pointer plus a compare and a branch inside each step (the rows_ahead tests alone were 0.8 % of
// the headline, round 5), and the tail pass and the xfrc_applied hand-over of rows_ahead are not compiled.  The arithmetic is the
// generic build's: the two are bitwise equal on the same launch (tests/test_gpu_dual2_lean.py).
// Issue priority of the fused builds (DESIGN.md section 2, "The two waves of a SIMD": measurements and candidates).  The waves of a
// headline launch are all resident from its first cycle and run the same step loop; at equal priority a SIMD's VALU issue goes to its
// older wave, which finishes early and leaves the younger one to run the tail of the launch alone.  FMJ_DUAL_PRIO_POLICY decides, at
// compile time, what a launch with StepArgs::dual_prio set does about it: 0 nothing; P > 0 (a power of two) the waves of a SIMD swap
// s_setprio 1 / 0 every P steps, told apart by the parity of their wave slot; FMJ_DUAL_PRIO_PHASE (below) adds what they do inside
// a step.  Scheduling only: no arithmetic is involved, and FMJ_DUAL_PRIO=0 at fmj_create (dual_prio = 0) executes no s_setprio
// and gives the same bits.
// FMJ_DUAL_PRIO_MAX_WPS: the register tiers (waves per SIMD) whose builds carry the policy.  Two waves sit in slots 0 and 1; with
// three, two share a parity and take turns against the third, which still pays (measured at 6144 envs).  The 128-register builds
// (WPS = 4) have no scalar to spare (DESIGN.md section 2).
#ifndef FMJ_DUAL_PRIO_POLICY
#define FMJ_DUAL_PRIO_POLICY 1
#endif
#ifndef FMJ_DUAL_PRIO_MAX_WPS
#define FMJ_DUAL_PRIO_MAX_WPS 3
#endif
static_assert(FMJ_DUAL_PRIO_POLICY >= 0 && (FMJ_DUAL_PRIO_POLICY & (FMJ_DUAL_PRIO_POLICY - 1)) == 0, "priority policy: 0 or a power of two");
// FMJ_DUAL_PRIO_PHASE: what s_setprio a wave executes at which point INSIDE a step (DESIGN.md section 2, "Issue priority by phase").
// A step is not uniform: L and X are chains of dependent LDS round trips with little VALU between them, S and M dense VALU streams.
// The switch points are phase boundaries of the step loop (the STAMP sites); a policy is one row of levels per point, first for the
// wave whose turn the step is (((step / P) ^ slot) & 1, the "winner"), then for the other one, -1 = no instruction there:
//   1 (A) alternate at the top of the step, nothing inside it (round 8)
//   2 (B) alternate at the top; both waves at 2 from L's entry to the end of X, then back to the step's level
//   3 (C) no alternation: 1 at the top, 0 from S's entry, 2 from L's entry to the end of X
//   4 (D) alternate at the top; the step's winner gives way (0) from S's entry to L's entry
//   5 (E) alternate at the top and flip again at L's entry
//   6 (F) B, and both waves at 2 inside V (its pointer-jumping rounds) as well
//   7 (G) B with the turn kept inside L ... X: the step's winner at 3, the other wave at 2
//   8 (H) B without the way back: both waves stay at 2 through Euler, until the top of the next step
// Every point is a uniform scalar branch on prio_sw and the step's parity around literal s_setprio, as the top of the step is.
// H is the default: the best of the eight in a same-box A/B against A (+ 3.5 %; B + 1.9, C + 0.9, G + 1.1, F - 0.5, E - 1.4,
// D - 3.1 %); the others stay for measurements (-DFMJ_DUAL_PRIO_PHASE=<id>, scripts/build_variant.sh).  With 1 the generated code
// is round 8's, instruction for instruction.
#ifndef FMJ_DUAL_PRIO_PHASE
#define FMJ_DUAL_PRIO_PHASE 8
#endif
enum { FMJ_PRIO_TOP = 0, FMJ_PRIO_V = 1, FMJ_PRIO_VEND = 2, FMJ_PRIO_S = 3, FMJ_PRIO_L = 4, FMJ_PRIO_XEND = 5, FMJ_PRIO_NPOINTS = 6 };
#if FMJ_DUAL_PRIO_PHASE == 1
#define FMJ_PRIO_LEVELS { 1, 0,  -1, -1,  -1, -1,  -1, -1,  -1, -1,  -1, -1}
#elif FMJ_DUAL_PRIO_PHASE == 2
#define FMJ_PRIO_LEVELS { 1, 0,  -1, -1,  -1, -1,  -1, -1,   2,  2,   1,  0}
#elif FMJ_DUAL_PRIO_PHASE == 3
#define FMJ_PRIO_LEVELS { 1, 1,  -1, -1,  -1, -1,   0,  0,   2,  2,   1,  1}
#elif FMJ_DUAL_PRIO_PHASE == 4
#define FMJ_PRIO_LEVELS { 1, 0,  -1, -1,  -1, -1,   0, -1,   1, -1,  -1, -1}
#elif FMJ_DUAL_PRIO_PHASE == 5
#define FMJ_PRIO_LEVELS { 1, 0,  -1, -1,  -1, -1,  -1, -1,   0,  1,  -1, -1}
#elif FMJ_DUAL_PRIO_PHASE == 6
#define FMJ_PRIO_LEVELS { 1, 0,   2,  2,   1,  0,  -1, -1,   2,  2,   1,  0}
#elif FMJ_DUAL_PRIO_PHASE == 7
#define FMJ_PRIO_LEVELS { 1, 0,  -1, -1,  -1, -1,  -1, -1,   3,  2,   1,  0}
#elif FMJ_DUAL_PRIO_PHASE == 8
#define FMJ_PRIO_LEVELS { 1, 0,  -1, -1,  -1, -1,  -1, -1,   2,  2,  -1, -1}
#else
#error "FMJ_DUAL_PRIO_PHASE: 1 (A) .. 8 (H)"
#endif
// (PRIO, PRIO_P, prio_sw and step are the step loop's; the period P gates the top of the step only)
#define FMJ_PRIO_AT(PT_) do { \
    constexpr int lv_[2 * FMJ_PRIO_NPOINTS] = FMJ_PRIO_LEVELS; \
    constexpr int w_ = lv_[2 * (PT_)], l_ = lv_[2 * (PT_) + 1]; \
    if (PRIO > 0 && (w_ >= 0 || l_ >= 0) && prio_sw && ((PT_) != FMJ_PRIO_TOP || (step & (PRIO_P - 1)) == 0)) { \
      if (w_ == l_) __builtin_amdgcn_s_setprio(w_ >= 0 ? w_ : 0); \
      else if (((step / PRIO_P) ^ prio_sw) & 1) { if (w_ >= 0) __builtin_amdgcn_s_setprio(w_ >= 0 ? w_ : 0); } \
      else { if (l_ >= 0) __builtin_amdgcn_s_setprio(l_ >= 0 ? l_ : 0); } \
    } } while (0)
#define FMJ_HWREG_WAVE_SLOT (4 | (0 << 6) | (3 << 11))      // s_getreg operand: HW_REG_HW_ID, bits 3:0 = the wave's slot on its SIMD
#define FMJ_HWREG_HW_ID (4 | (0 << 6) | (31 << 11))         // the whole register: slot, SIMD, pipe, CU, SH, SE, ...
#define FMJ_HWREG_XCC_ID (20 | (0 << 6) | (31 << 11))       // HW_REG_XCC_ID: bits 3:0 = the XCC
template <bool FUSED, int MAXD, int WPS, bool SUBS = false, bool LEAN = false>
__global__ void __launch_bounds__(64, WPS) fmj_step_dual2_kernel(const DevModel M_by_value, const StepArgs A_by_value) {
  static_assert(!LEAN || (FUSED && !SUBS), "the lean build is a fused launch without the rare options");
  extern __shared__ __align__(16) float lds[];
#ifdef FMJ_STAMPS
  const unsigned long long life_t0 = __builtin_amdgcn_s_memtime();      // the wave's entry (scripts/wave_lifetimes.py)
#endif
  // the two arguments, addressed in the kernarg segment instead of being held in SGPRs
  const char AS4* const karg = (const char AS4*)__builtin_amdgcn_kernarg_segment_ptr();
  const DevModel AS4* Mp = (const DevModel AS4*)karg;
  const StepArgs AS4* Ap = (const StepArgs AS4*)(karg + FMJ_KARG_A_OFF);
#define M (*Mp)
#define A (*Ap)
#define BT2(b, k) ldg4(M.btab, (unsigned)(b) * BT_STRIDE + (k))
#define DT2(d, k) ldg4(M.dtab, (unsigned)(d) * DT_STRIDE + (k))
#define AT2(a, k) ldg4(M.atab, (unsigned)(a) * AT_STRIDE + (k))
#define ST2(i, k) ldg4(M.stab, (unsigned)(i) * ST_STRIDE + (k))
#define STAGE2_REC D2S      // stride of the CD / F records, for the shared stages (fmj_stage2_*.inc)
  // launch options that never change during a launch: read where they are used, constants in the LEAN build
#define OPT_ROWS_AHEAD (!LEAN && A.rows_ahead)
#define OPT_READOUT (LEAN || A.do_readout)
#define OPT_DRAG (LEAN || A.do_drag)
#define OPT_CONTROLLER (LEAN ? 1 : (FUSED ? A.controller : 0))
#define OPT_TAPE (LEAN ? (const float*)nullptr : A.ctrl)
#define OPT_NO_ACT (!LEAN && A.disable_actuation != 0)
#define OPT_STIFFNESS (!LEAN && M.any_stiffness)
#define OPT_INTEGRATE (LEAN || A.integrate)
  // per-env wave parameters (fmj_fused_ext): never in a LEAN launch, whose wave controller reads the shared row and A.w_freq
#define OPT_WFREQ_ENV (LEAN ? (const float*)nullptr : A.w_freq_env)
#define OPT_WAMP_STRIDE (LEAN ? 0ll : A.w_amp_stride)
#define OPT_WLAG_STRIDE (LEAN ? 0ll : A.w_lag_stride)
  const int lane = threadIdx.x;
  const bool upper = lane >= 32;
  const int sl = lane & 31;
  const int hb = lane & 32;
  const int env_raw = 2 * blockIdx.x + (upper ? 1 : 0);
  const int n_envs = A.n_envs;
  const bool exists = env_raw < n_envs;        // odd batch: the last wave's upper half computes a copy, stores nothing
  const int env = exists ? env_raw : n_envs - 1;
  const int nb = M.nbody, nv = M.nv, nq = M.nq, nu = M.nu;
  const int T0 = M.dual_t0;                    // 3 with a free root, else 0
  const int ND = nv - T0;
  constexpr int RS = MAXD;
  const Lds2 LL = lds2_layout(nb, nv, nq, RS, T0);
  float* const base = lds + (upper ? LL.total : 0);
  float* const QP = base + LL.QP;
  float* const QV = base + LL.QV;
  float* const XV = base + LL.XV;
  float* const CD = base + LL.CD;
  float* const F = base + LL.F;
  float* const CI = base + LL.CI;
  float* const HR = base + LL.HR;
  const uint8_t* const JMP = (const uint8_t*)(lds + 2 * LL.total);   // pointer-jumping table, shared by both halves

  const bool isb = sl > 0 && sl < nb;
  const int bl = isb ? sl : 0;
  const bool isd = sl < ND;
  const int mydof = isd ? sl + T0 : T0;
  const int4 d_info0 = as_int4(DT2(mydof, 0));
  const int ddepth = isd ? d_info0.y : 0;      // absolute depth: slots 0..T0-1 are the translational columns
  const int dsub = isd ? d_info0.z : 0;
  const int dbody = d_info0.x;

  // ---- load tables + state
  int warn = 0;
  {
    // The step reads LDS words it never wrote: the pad floats of the 8- and 12-float records, the translational cdof
    // slots, row slots past a lane's depth.  Their values are multiplied by an exact 0 or discarded by a select, which is
    // only harmless while they are finite: start from zeros, after which only finite values are ever stored.
    for (int i = sl; i < LL.total; i += 32) base[i] = 0.f;
    uint32_t* jw = (uint32_t*)(lds + 2 * LL.total);
    const int nw = r4(nb * M.anc_stride) / 4;
    const uint32_t AS1* ga = gptr((const uint32_t*)M.b_anc);
    for (int i = lane; i < nw; i += 64) jw[i] = ga[i];
    const float AS1* gq = gptr(A.qpos) + (size_t)env * nq;
    const float AS1* gv = gptr(A.qvel) + (size_t)env * nv;
    for (int i = sl; i < nq; i += 32) { const float v = gq[i]; QP[i] = v; if (!(fabsf(v) <= 1e10f)) warn |= FMJ_WARN_BADQPOS; }   // mj_checkPos
    for (int i = sl; i < nv; i += 32) { const float v = gv[i]; QV[i] = v; if (!(fabsf(v) <= 1e10f)) warn |= FMJ_WARN_BADQVEL; }   // mj_checkVel
  }
#define HALF_ANY(pred_) ({ const unsigned long long b_ = __ballot(pred_); upper ? (unsigned)(b_ >> 32) != 0u : (unsigned)b_ != 0u; })
  // A half whose env carries a bad-state bit is frozen (include/fmj.h): it keeps computing alongside the other half but
  // stores nothing and is not integrated, from the step that finds the bad value on.  `live` gates every store.
  bool frozen = (gptr(A.status)[env] & FMJ_WARN_FREEZE) != 0;
  frozen = frozen || HALF_ANY((warn & FMJ_WARN_FREEZE) != 0);
  bool live = exists && !frozen;
  int steps_done = 0;

  // Actuators of this lane's joint (<= 4, sorted by model order).  A slot is dead in this launch when it cannot produce
  // a force: no bias and either no gain or nothing driving it (wave controller: zero amplitude IN THIS LANE'S ENV - with per-env
  // amplitudes the halves of a wave may disagree, live_mask is a per-lane fact and a dead slot adds an exact 0; tape: no tape).  The
  // first live slot stays in registers; more live slots (wave-uniform count NL) are re-read from the tables each step.
  const int4 d_act = as_int4(DT2(mydof, 2));              // first actuator, count, joint sensor slot, dof parent
  const int act_n = isd ? d_act.y : 0;
  float4 a0_p = make_float4(0.f, 0.f, 0.f, 0.f), a0_lim = make_float4(0.f, 0.f, 0.f, 0.f); int a0_src = 0; float a0_amp = 0.f, a0_lag = 0.f;
  unsigned live_mask = 0;                                   // bit a: slot a of this lane is live
  {
    const int controller = OPT_CONTROLLER;
    const bool have_tape = OPT_TAPE != nullptr;
#pragma unroll
    for (int a = 3; a >= 0; a--) {
      if (a < act_n) {
        const int ai = d_act.x + a;
        const float4 p = AT2(ai, 0), lim = AT2(ai, 1);
        const int src = __float_as_int(AT2(ai, 2).x);
        float amp = 0.f, lag = 0.f;
        if (controller == 1) { amp = gptr(A.w_amp)[(size_t)env * OPT_WAMP_STRIDE + src]; lag = gptr(A.w_lag)[(size_t)env * OPT_WLAG_STRIDE + src]; }
        const bool biased = p.y != 0.f || p.z != 0.f || p.w != 0.f;
        const bool driven = controller == 1 ? amp != 0.f : have_tape;
        const bool clamp0 = lim.x > 0.f || lim.y < 0.f || lim.z > 0.f || lim.w < 0.f;   // a range without 0
        const bool zero_range = lim.z == 0.f && lim.w == 0.f;                             // forcerange [0, 0]: task.py:279-286
        if ((biased || clamp0 || (driven && p.x != 0.f)) && !zero_range) {
          live_mask |= 1u << a;
          a0_p = p; a0_lim = lim; a0_src = src; a0_amp = amp; a0_lag = lag;   // ends up holding the lowest live slot
        }
      }
    }
  }
  const int first_live = live_mask ? __ffs((int)live_mask) - 1 : 4;
  const bool more_slots = __any((live_mask & (live_mask - 1u)) != 0u);        // some lane has a second live slot

  float xf[6] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f};       // world-frame external force / torque on this body
  float cy_actsum = 0.f;                              // motor torque of the last forward pass (physics.py:510-524)
  const int it0 = A.iteration0;
  // links row of iteration `it` + drag (ExperimentTask.before_step, reference task.py:168-186; physics.py:449-466,
  // drag.pyx:389-411) from a pose / velocity of the last forward pass; leaves the world-frame drag of the body in xf
  // resident copies for the 256-register build (declared here: the row / drag emitter below uses them)
  constexpr bool RES2_ = WPS <= 2;
  // element offsets of the lane's link / xfrc / joint rows inside one ring row (the ring index adds a uniform multiple of the stride)
  const long long r_offl_ = (long long)env * M.n_links * FMJ_LINK_SIZE, r_offx_ = (long long)env * M.n_xfrc * FMJ_XFRC_SIZE,
                  r_offj_ = (long long)env * M.n_joints * FMJ_JOINT_SIZE;
  const float r_wenv_ = (FUSED && OPT_CONTROLLER == 1) ? gptr(A.w_env)[env] : 0.f;
  const float r_wfreq_ = (RES2_ && FUSED && OPT_CONTROLLER == 1 && OPT_WFREQ_ENV) ? gptr(A.w_freq_env)[env] : 0.f;      // the env's own frequency: resident in the 256-register build only
  // the env phase in revolutions, rounded once per launch in EVERY build (pinf keeps the product from being contracted into the
  // add of a step in the builds that would otherwise reload the phase there: the register builds must agree bitwise)
  const float r_wturn_ = pinf(0.15915494309189535f * r_wenv_);
  const int4 r_ci2_ = as_int4(BT2(bl, 8));
  const int r_sw_ = (isb && r_ci2_.w >= 0) ? r_ci2_.w : 0;
  const float4 r_s0_ = ST2(r_sw_, 0), r_s1_ = ST2(r_sw_, 1), r_s2_ = ST2(r_sw_, 2), r_s3_ = ST2(r_sw_, 3);
  auto emit_links_and_drag2 = [&](const int index, const v3 xp, const q4 xq, const v3 xi, const v3 linvel, const v3 angvel) {
    const int4 ci2 = RES2_ ? r_ci2_ : as_int4(BT2(bl, 8));        // depth, subtree size, link row, swim slot; index = iteration % buffer_size
    const float im = A.inv_meters;
    const v3 r_com = scl3(xi, im), r_urdf = scl3(xp, im);
    const v3 r_lin = scl3(linvel, A.inv_velocity), r_ang = scl3(angvel, A.inv_angvel);
    if (OPT_READOUT && isb && live && ci2.z >= 0) {      // quaternions: w,x,y,z -> x,y,z,w (physics.py:458)
      float AS1* row = gptr(A.links) + ((size_t)index * A.row_stride_links + (RES2_ ? (size_t)r_offl_ : (size_t)env * M.n_links * FMJ_LINK_SIZE)) + ci2.z * FMJ_LINK_SIZE;
      stg4(row + 0, r_com.x, r_com.y, r_com.z, xq.x);
      stg4(row + 4, xq.y, xq.z, xq.w, r_urdf.x);
      stg4(row + 8, r_urdf.y, r_urdf.z, xq.x, xq.y);
      stg4(row + 12, xq.z, xq.w, r_lin.x, r_lin.y);
      stg4(row + 16, r_lin.z, r_ang.x, r_ang.y, r_ang.z);
    }
    if (OPT_DRAG) {
#pragma unroll
      for (int k = 0; k < 6; k++) xf[k] = 0.f;
      if (isb && ci2.w >= 0) {
        const float4 s0 = RES2_ ? r_s0_ : ST2(ci2.w, 0), s1 = RES2_ ? r_s1_ : ST2(ci2.w, 1), s2 = RES2_ ? r_s2_ : ST2(ci2.w, 2), s3 = RES2_ ? r_s3_ : ST2(ci2.w, 3);
        const DragEnv W = {A.surface, A.viscosity, A.wvx, A.wvy, A.wvz, A.wgravity, A.use_buoyancy};
        v3 fo, to, fw, tw;
        if (drag_same_frames2(r_com, xq, r_lin, r_ang, s0, s1, s3.x, s3.y, W, &fo, &fw, &to, &tw)) {
          if (live) {
            float AS1* xr = gptr(A.xfrc) + ((size_t)index * A.row_stride_xfrc + (RES2_ ? (size_t)r_offx_ : (size_t)env * M.n_xfrc * FMJ_XFRC_SIZE)) + __float_as_int(s2.z) * FMJ_XFRC_SIZE;
            stg2(xr + 0, fo.x, fo.y);
            stg2(xr + 2, fo.z, to.x);
            stg2(xr + 4, to.y, to.z);
          }
          const float nw = A.newtons, tq = A.torques;
          xf[0] = fw.x * nw; xf[1] = fw.y * nw; xf[2] = fw.z * nw;
          xf[3] = tw.x * tq; xf[4] = tw.y * tq; xf[5] = tw.z * tq;
        }
      }
    }
  };
  // rows_ahead (fmj_fused_args::rows_ahead, the per-iteration host path): the rows, the drag and xfrc_applied of the launch's FIRST iteration
  // were written by the launch before (its tail, below) or by fmj_before_step - and host callbacks may have edited xfrc_applied since -,
  // so nothing of them is written here and the drag force comes from xfrc_applied; in exchange the launch writes everything
  // before_step would write for the iteration AFTER its last step
  const bool rows_ahead = FUSED && OPT_ROWS_AHEAD != 0;
  if (FUSED && !rows_ahead) {
    // the launch's first iteration logs the fields the previous launch (or the reset's mj_forward) left in mjData
    const float AS1* p = gptr(A.xpos) + (size_t)env * nb * 3 + bl * 3;
    const float4 q = ldg4f(A.xquat + (size_t)env * nb * 4 + bl * 4);     // w,x,y,z
    const float AS1* ip = gptr(A.xipos) + (size_t)env * nb * 3 + bl * 3;
    const float AS1* sd = gptr(A.sensordata) + (size_t)env * M.nsensordata + 6 * (isb ? sl - 1 : 0);
    const q4 cq = {q.x, q.y, q.z, q.w};
    emit_links_and_drag2(it0 % A.buffer_size, mk3(p[0], p[1], p[2]), cq, mk3(ip[0], ip[1], ip[2]), mk3(sd[0], sd[1], sd[2]), mk3(sd[3], sd[4], sd[5]));
    const float4 dp = DT2(mydof, 1);
    if (isd && dp.w != 0.f) {
      const float AS1* sa = gptr(A.sensordata) + (size_t)env * M.nsensordata + 6 * (nb - 1) + 3 * M.njs;
      const float itq = A.inv_torques;
#pragma unroll
      for (int a = 0; a < 4; a++) if (a < act_n) cy_actsum += sa[__float_as_int(AT2(d_act.x + a, 2).x)] * itq;
    }
  }
  if ((!(FUSED && OPT_DRAG) || rows_ahead) && A.xfrc_applied && isb) {
    const float AS1* x = gptr(A.xfrc_applied) + (size_t)env * nb * 6 + bl * 6;
#pragma unroll
    for (int k = 0; k < 6; k++) xf[k] = x[k];
  }
  WSYNC();

#ifdef FMJ_STAMPS
  float stamp_acc[NSTAMP];
#pragma unroll
  for (int i = 0; i < NSTAMP; i++) stamp_acc[i] = 0.f;
  unsigned long long stamp_prev = __builtin_amdgcn_s_memtime();
#endif
  const int n_steps = A.n_steps;
  // the priority switch and the slot parity in one loop-carried scalar: 0 = leave priorities alone, else 2 | parity
  constexpr int PRIO = (FUSED && WPS <= FMJ_DUAL_PRIO_MAX_WPS) ? FMJ_DUAL_PRIO_POLICY : 0, PRIO_P = PRIO > 0 ? PRIO : 1;
  int prio_sw = 0;
  if (PRIO != 0 && A.dual_prio) prio_sw = 2 | (int)(__builtin_amdgcn_s_getreg(FMJ_HWREG_WAVE_SLOT) & 1u);
  int ring = FUSED ? it0 % A.buffer_size : 0;      // ring index of the current iteration, advanced by wrap-around (no division per step)
  // what a lane carries across the steps: its index, (depth, subtree size, body, joint row) packed in one register, the
  // resident actuator slot (11), the drag on its body (6), the carried motor torque, the warning bits, the step count
  // WPS == 3 (batches of up to three waves per SIMD: 168 registers allowed, ~133 used): the model constants on the critical start
  // of a step stay resident instead of being re-read from the tables (an L2 round trip each, in front of the first joint transform)
  const bool RES = WPS <= 3;
  // WPS == 2 (batches of up to two waves per SIMD, e.g. 4096 envs on 256 CUs: 256 registers allowed): the swimming constants of
  // the lane's link and the ancestor-lane table stay resident too
  const bool RES2 = WPS <= 2;
  const float4 r_quat = BT2(bl, 1), r_iquat = BT2(bl, 3), r_jposk = BT2(bl, 6);
  uint32_t r_ancl[MAXD / 4];
#pragma unroll
  for (int g = 0; g < MAXD / 4; g++) r_ancl[g] = gptr(M.dual_ancl)[(unsigned)sl * (MAXD / 4) + g];
  const float4 r_info = BT2(bl, 7), r_axis = BT2(bl, 5), r_posm = BT2(bl, 0), r_ipos = BT2(bl, 2), r_inertia = BT2(bl, 4), r_dprm = DT2(mydof, 1);
  const int sl_o = lane;
  int sub = 0, itm = 0;       // sub-steps: index of this physics step inside its iteration (0 = the full step), iterations completed (fmj_hip.hip)
  const unsigned dpack_o = (unsigned)ddepth | ((unsigned)dsub << 6) | ((unsigned)dbody << 12) | ((unsigned)(d_info0.w + 1) << 18) |
                           ((unsigned)(first_live & 7) << 25) | ((unsigned)live_mask << 28);
  const int n_loop = n_steps + (rows_ahead ? 1 : 0);      // rows_ahead: one more pass that ends after the rows at its top (the joints row of the next iteration)
#pragma unroll 1
  for (int step = 0; step < n_loop; step++) {
    if (__all(frozen)) break;
    FMJ_PRIO_AT(FMJ_PRIO_TOP);      // (uniform) the waves of a SIMD swap priority every PRIO_P steps
    asm volatile("" : "+s"(Ap));                 // arguments are re-read inside the step, never carried across it
    asm volatile("" : "+s"(Mp));
    // per-lane indices, masks and LDS addresses are recomputed inside every step: hoisted out of the loop they would be
    // ~100 loop-invariant registers (one address and two lane masks per depth / per pivot), all of them spilled
    const int lane = opaque(sl_o);
    // uniform model constants are laundered too: the conditions made from them (d >= T0, lvl < maxdep for every depth) are
    // otherwise computed once, held as SGPR-pair masks across the whole loop and spilled (see opaque_s)
    const int T0 = opaque_s(M.dual_t0), ND = nv - T0;
    const bool upper = lane >= 32;
    const int sl = lane & 31, hb = lane & 32;
    const unsigned dpack = (unsigned)opaque((int)dpack_o);
    const int ddepth = dpack & 63, dsub = (dpack >> 6) & 63, dbody = (dpack >> 12) & 63, jrow = (int)((dpack >> 18) & 127) - 1;
    const int first_live = (dpack >> 25) & 7;
    const unsigned live_mask = dpack >> 28;
    const int env_raw = 2 * blockIdx.x + (upper ? 1 : 0);
    const int env = env_raw < n_envs ? env_raw : n_envs - 1;
    const bool isb = sl > 0 && sl < nb;
    const int bl = isb ? sl : 0;
    const bool isd = sl < ND;
    const int mydof = isd ? sl + T0 : T0;
    float* const base = lds + (upper ? LL.total : 0);
    float* const QP = base + LL.QP;
    float* const QV = base + LL.QV;
    float* const XV = base + LL.XV;
    float* const CD = base + LL.CD;
    float* const F = base + LL.F;
    float* const CI = base + LL.CI;
    float* const HR = base + LL.HR;
    // per dof, per depth: byte = 4 * (lane of the ancestor at that depth), own lane where there is none
    uint32_t ancl[MAXD / 4];
#pragma unroll
    for (int g = 0; g < MAXD / 4; g++) ancl[g] = RES2 ? r_ancl[g] : gptr(M.dual_ancl)[(unsigned)sl * (MAXD / 4) + g];
    if (!SUBS) itm = step;
    const int it = it0 + itm;
    const bool last = step == n_steps - 1;
    const int S_sub = SUBS ? A.substeps : 1;
    const bool full = sub == 0;
    const int nsub = sub + 1 >= S_sub ? 0 : sub + 1;           // the next physics step: sub index, full step or not, and whether its
    const bool nfull = nsub == 0;                               // before_step sees task.iteration = it + 1 (the reference advances it
    const bool nrow1 = nfull || (nsub >= 1 && nsub >= S_sub - 1);   // after sub-step S - 2 of a group: task.py:352-355) or still it
    const int ring_n1 = FUSED ? (ring + 1 == A.buffer_size ? 0 : ring + 1) : 0;
    // ============ before_step: joints row (reference physics.py:500-524), needs the CURRENT qpos / qvel ============
    const float4 d_prm = RES ? r_dprm : DT2(mydof, 1);          // armature, damping, qposadr bits, hinge/slide flag
    const int d_qadr = __float_as_int(d_prm.z);
    const bool d_scalar = isd && d_prm.w != 0.f;
    if (FUSED && OPT_READOUT && full && !(OPT_ROWS_AHEAD && step == 0)) {
      if (d_scalar && live && jrow >= 0) {
        const int index = ring;
        float AS1* row = gptr(A.joints) + ((size_t)index * A.row_stride_joints + (RES2_ ? (size_t)r_offj_ : (size_t)env * M.n_joints * FMJ_JOINT_SIZE)) + jrow * FMJ_JOINT_SIZE;
        // the whole 48-byte row as three aligned 16-byte stores, zeros in the columns nothing on this path writes (force / torque
        // sensors): the row's cache lines leave L2 fully written.  As two 8-byte stores the kernel was 0.9 % slower and WRITE_SIZE
        // counted the untouched columns anyway (partial lines; round 4 A/B, DESIGN section 5)
        stg4(row + 0, QP[d_qadr], QV[mydof] * A.inv_angvel, 0.f, 0.f);      // position, velocity
        stg4(row + 4, 0.f, 0.f, 0.f, 0.f);
        stg4(row + 8, cy_actsum, 0.f, 0.f, 0.f);                            // motor torque, limit force
      }
    }
    if (FUSED && OPT_ROWS_AHEAD && step == n_steps) break;        // the tail pass: the next iteration's rows are complete, nothing is stepped
    // ============ mj_step ============
    const int4 c_info = as_int4(RES ? r_info : BT2(bl, 7));     // parent, jtype, qadr, dadr
    const int jtype = isb ? c_info.y : -1;
    const int qadr = c_info.z, dadr = c_info.w;
    const float4 c_axis_q0 = RES ? r_axis : BT2(bl, 5);
    const float4 c_jpos_k = RES2 ? r_jposk : BT2(bl, 6);
    const uint32_t jm = sl < nb ? *(const uint32_t*)(JMP + sl * M.anc_stride) : 0u;
    const int max_bdepth = M.max_bdepth;
    const bool any_jpos = M.any_jpos != 0, any_bquat = M.any_bquat != 0, any_iquat = M.any_iquat != 0;   // model-wide (uniform) shortcuts
    STAMP(1);
    // ---- K: local transforms, composed along the chains by pointer jumping (partner poses pulled with ds_bpermute)
    v3 xp; q4 xq;
    {
      const float4 c_pos_mass = RES ? r_posm : BT2(bl, 0);
      const float4 c_quat = RES2 ? r_quat : BT2(bl, 1);
#include "fmj_stage2_k.inc"
    }
    v3 xi;
    {
      const float4 c_ipos = RES ? r_ipos : BT2(bl, 2);
      xi = add3(xp, qrot(xq, mk3(c_ipos.x, c_ipos.y, c_ipos.z)));
    }
    STAMP(2);
    // ---- C: tree CoM of this half's env, world inertia about the body's own CoM
    const float mass = isb ? (RES ? r_posm : BT2(bl, 0)).w : 0.f;
    v3 com;
    {
      const float mi = M.mtot_inv;
      com.x = half_sum_all(mass * xi.x) * mi; com.y = half_sum_all(mass * xi.y) * mi; com.z = half_sum_all(mass * xi.z) * mi;
    }
    float iw[6];
    {
      const float4 c_iquat = RES2 ? r_iquat : BT2(bl, 3);
      const float4 c_inertia = RES ? r_inertia : BT2(bl, 4);
#include "fmj_stage2_c.inc"
    }
    STAMP(3);
    FMJ_PRIO_AT(FMJ_PRIO_V);
    // ---- V: joint velocity, cvel = chain sum of joint velocities, cacc = chain sum of cvel_parent x vJ - g
#include "fmj_stage2_v.inc"
    STAMP(4);
    FMJ_PRIO_AT(FMJ_PRIO_VEND);
    // ---- F: body force (inertial minus external) about the tree CoM
    const v3 dcom = sub3(xi, com);
    s6 fbody;
    {
#include "fmj_stage2_f.inc"
      const v3 fw = mk3(xf[0], xf[1], xf[2]), tw = mk3(xf[3], xf[4], xf[5]);
      f.r = sub3(f.r, add3(tw, cross(dcom, fw)));
      f.l = sub3(f.l, fw);
      if (!isb) { f.r = f.l = mk3(0.f, 0.f, 0.f); }
      fbody = f;
    }
    STAMP(5);
    // ---- sensors of this (pre-integration) state: they are the link data of iteration it + 1 (mj_step lag); the row
    //      and its drag are emitted here, where the values are, instead of being carried to the next step through LDS
    {
      const v3 linvel = add3(cv.l, cross(cv.r, dcom));
      if (FUSED && (!last || OPT_ROWS_AHEAD) && (nfull || (SUBS && A.sub_links && !(A.n_it_total > 0 && it + (nrow1 ? 1 : 0) >= A.n_it_total)))) emit_links_and_drag2(nrow1 ? ring_n1 : ring, xp, xq, xi, linvel, cv.r);   // a sub-step without a row keeps its drag force
      if (FUSED && last && OPT_ROWS_AHEAD && OPT_DRAG && A.xfrc_applied_out && isb && live) {      // ... and the world-frame drag goes where the next launch (and the host callbacks before it) find it
        const int4 ci2x = as_int4(BT2(bl, 8));
        if (ci2x.w >= 0) {
          float AS1* xa = gptr(A.xfrc_applied_out) + (size_t)env * nb * 6 + bl * 6;
#pragma unroll
          for (int k = 0; k < 6; k++) xa[k] = xf[k];
        }
      }
      if (last && live && sl < nb) {
        float AS1* p = gptr(A.xpos) + (size_t)env * nb * 3 + sl * 3; p[0] = xp.x; p[1] = xp.y; p[2] = xp.z;
        stg4(gptr(A.xquat) + (size_t)env * nb * 4 + sl * 4, xq.w, xq.x, xq.y, xq.z);
        float AS1* ip = gptr(A.xipos) + (size_t)env * nb * 3 + sl * 3; ip[0] = xi.x; ip[1] = xi.y; ip[2] = xi.z;
        if (isb) {
          float AS1* sp = gptr(A.sensordata) + (size_t)env * M.nsensordata + 6 * (sl - 1);
          stg2(sp, linvel.x, linvel.y);
          stg2(sp + 2, linvel.z, cv.r.x);
          stg2(sp + 4, cv.r.y, cv.r.z);
        }
      }
    }
    STAMP(0);
    FMJ_PRIO_AT(FMJ_PRIO_S);
    // ---- S: subtree sums as prefix-sum differences inside the half (fp64 DPP scans, see fmj_hip.hip)
    {
      const float4 c_ipos = RES ? r_ipos : BT2(bl, 2);            // .w = subtree mass (model constant)
      const int lastl = hb | (isb ? sl + (RES2 ? r_ci2_ : as_int4(BT2(bl, 8))).y - 1 : sl);
#include "fmj_stage2_s.inc"
    }
    WSYNC();
    STAMP(6);
    // ---- Q (lane = dof T0 + sl; the translational dofs as per-half uniform scalars) and the rows of H in registers
    float qfrc = 0.f;
    float dvel = 0.f;                               // implicitfast: velocity gains of this dof's unclamped actuators
    float qt0 = 0.f, qt1 = 0.f, qt2 = 0.f;          // rhs of the translational dofs
    if (T0) {
      const float4 fl = *(const float4*)(F + 1 * D2S);        // root subtree force: rot xyz, lin x
      const float2 fl2 = *(const float2*)(F + 1 * D2S + 4);   // lin y, z
      qt0 = -DT2(0, 1).y * QV[0] - fl.w; qt1 = -DT2(1, 1).y * QV[1] - fl2.x; qt2 = -DT2(2, 1).y * QV[2] - fl2.y;
    }
    f2_t r[MAXD / 2];                                // row of H, then of its factor, indexed by depth
#pragma unroll
    for (int d = 0; d < MAXD / 2; d++) r[d] = f2_t{0.f, 0.f};
    float diag = 1.f;
    {
      const s6 cd = isd ? lds_get6(CD + mydof * D2S) : s6{mk3(0.f, 0.f, 0.f), mk3(0.f, 0.f, 0.f)};
      const float4 ia = *(const float4*)(CI + dbody * 12), ib = *(const float4*)(CI + dbody * 12 + 4);
      const float2 ic = *(const float2*)(CI + dbody * 12 + 8);
      const v3 sc = mk3(ib.z, ib.w, ic.x);                                      // subtree CoM - tree CoM
      // (I_s w_i, m v_i(s)): dof i's unit rate applied to the composite body it moves, about that body's own CoM
      s6 bf;
      bf.r = mk3(ia.x * cd.r.x + ia.w * cd.r.y + ib.x * cd.r.z, ia.w * cd.r.x + ia.y * cd.r.y + ib.y * cd.r.z, ib.x * cd.r.x + ib.y * cd.r.y + ia.z * cd.r.z);
      bf.l = scl3(add3(cd.l, cross(cd.r, sc)), ic.y);
      const float qd = QV[mydof];
      if (isd) qfrc = -d_prm.y * qd - s6dot(cd, lds_get6(F + dbody * D2S));
      if (d_scalar) {
        const float qj = QP[d_qadr];
        if (OPT_STIFFNESS) {
          const float kst = BT2(dbody, 6).w;
          if (kst != 0.f) qfrc -= kst * (qj - gptr(A.qpos_spring)[(size_t)env * nq + d_qadr]);
        }
        float asum = 0.f, cbase = 0.f, cturn = 0.f;
        const int controller = OPT_CONTROLLER;
        if (controller == 1) {
          const float wfreq = OPT_WFREQ_ENV ? (RES2_ ? r_wfreq_ : gptr(A.w_freq_env)[env]) : A.w_freq;      // the env's own frequency (fmj_fused_ext), else the shared one
          double cyc = (double)wfreq * ((double)it * ((double)M.h * (double)S_sub));   // task.py:290: time = iteration * timestep (of an iteration)
          cyc -= floor(cyc);
          const float wenv = RES2_ ? r_wenv_ : gptr(A.w_env)[env];
          cbase = fmaf(6.283185307179586f, (float)cyc, wenv);
          cturn = (float)cyc + r_wturn_;                         // the same phase in revolutions
        }
        const float AS1* ctrl_row = OPT_TAPE ? gptr(A.ctrl) + (size_t)itm * A.ctrl_step_stride + (size_t)env * nu : nullptr;      // one ctrl row per iteration
        const bool no_act = OPT_NO_ACT;
        if (first_live < 4) {                        // the resident slot
          float c;
          if (controller == 1) c = a0_amp != 0.f ? a0_amp * sin_turns(fmaf(-0.15915494309189535f, a0_lag, cturn)) : 0.f;
          else c = ctrl_row ? ctrl_row[a0_src] : 0.f;
          c = fminf(fmaxf(c, a0_lim.x), a0_lim.y);
          float f = a0_p.x * c + a0_p.y + a0_p.z * qj + a0_p.w * qd;
          if (SUBS && M.implicitfast && !no_act && f > a0_lim.z && f < a0_lim.w) dvel -= a0_p.w;      // d force / d qvel of an unclamped actuator (include/fmj.h: implicitfast)
          f = fminf(fmaxf(f, a0_lim.z), a0_lim.w);
          asum += no_act ? 0.f : f;
        }
        if (more_slots || last) {                    // cold path: the other live slots; on the last step every slot's sensor output
          const int4 d_act = as_int4(DT2(mydof, 2)); // first actuator, count, joint sensor slot, dof parent
          const int act_n = d_act.y;
          float AS1* sa = gptr(A.sensordata) + (size_t)env * M.nsensordata + 6 * (nb - 1) + 3 * M.njs;   // actuatorfrc
          for (int a = 0; a < act_n; a++) {
            const bool is_live = (live_mask >> a) & 1u;
            if (a == first_live && !last) continue;
            if (!is_live && !last) continue;
            const int ai = d_act.x + a;
            const float4 p = AT2(ai, 0), lim = AT2(ai, 1);
            const int src = __float_as_int(AT2(ai, 2).x);
            float c;
            if (controller == 1) { const float amp = gptr(A.w_amp)[(size_t)env * OPT_WAMP_STRIDE + src]; c = amp != 0.f ? amp * sinf(cbase - gptr(A.w_lag)[(size_t)env * OPT_WLAG_STRIDE + src]) : 0.f; }
            else c = ctrl_row ? ctrl_row[src] : 0.f;
            if (controller == 1 && last && live && A.ctrl_out) gptr(A.ctrl_out)[(size_t)env * nu + src] = c;   // what task.py:288-346 leaves in physics.data.ctrl
            c = fminf(fmaxf(c, lim.x), lim.y);
            float f = p.x * c + p.y + p.z * qj + p.w * qd;
            if (SUBS && M.implicitfast && !no_act && a != first_live && f > lim.z && f < lim.w) dvel -= p.w;
            f = fminf(fmaxf(f, lim.z), lim.w);
            if (no_act) f = 0.f;
            if (a != first_live) asum += f;           // a dead slot contributes exactly 0 by construction
            if (last && live) sa[src] = f;
          }
        }
        qfrc += asum;
        cy_actsum = asum * A.inv_torques;
      }
    STAMP(7);
      // ---- M: row i of H = M + diag(armature + h damping), one entry per depth of the chain root -> i:
      //      H[i][j] = w_j . (I_s w_i) + v_j(s) . (m v_i(s)), s = CoM of the subtree dof i moves, j = ancestor of i (or i)
      // (register-array elements are only assigned outside of branches: an assignment under a branch makes the compiler
      // carry the whole array through the join as copies)
      // the diagonal entry (the chain's last link is the dof itself) sits at the lane's own depth
      // H[i][j] = w_j . (I_s w_i) + (v_j + w_j x sc) . p_i = w_j . (I_s w_i + sc x p_i) + v_j . p_i with p_i = m v_i(s):
      // the bracket gi is the lane's own, so an entry costs two dot products
      const v3 gi = add3(bf.r, cross(sc, bf.l));
      diag = isd ? dot3(cd.r, gi) + dot3(cd.l, bf.l) + (d_prm.x + M.h * (SUBS ? d_prm.y + dvel : d_prm.y)) : 1.f;   // + armature + h (damping + implicitfast's actuator velocity gains)
      // the depths with lane dofs, T0 .. maxdep, as ONE uniform bit mask made inside the step: a level's test is s_bitcmp1 + branch
      // (the two compares per level it replaces were 7 scalar instructions each - 240 per step with the sweep below, round 4)
      const unsigned dmask = (unsigned)opaque_s((int)((2u << M.dual_maxdep) - (1u << T0)));
#pragma unroll
      for (int g = 0; g < MAXD / 4; g++) {
#pragma unroll
        for (int k = 0; k < 4; k++) {
          const int d = 4 * g + k;
          float mij = d == 0 ? bf.l.x : (d == 1 ? bf.l.y : bf.l.z);             // translational columns (d < T0): e_t . (m v_i(s))
          if (__builtin_expect((dmask & (1u << d)) != 0u, 1)) {                  // T0 <= d <= maxdep: the test is uniform, the register index static
            const int al = (int)((ancl[g] >> (8 * k)) & 0xffu) >> 2;            // lane of the ancestor at depth d (own lane beyond the chain)
            const s6 cdj = lds_get6(CD + (al + T0) * D2S);
            mij = dot3(cdj.r, gi) + dot3(cdj.l, bf.l);
          }
          if (k & 1) r[d / 2].y = mij; else r[d / 2].x = mij;
        }
      }
      // Slots at and past the lane's own depth hold finite values that are never read as matrix entries (beyond the chain
      // the table names the lane itself, so they repeat the undamped diagonal; the damped diagonal lives in `diag`).
      // Lanes without a dof have cd = 0: their rows are zero.
    }
    WSYNC();                                         // CD / F / CI are dead from here: the published rows overlay them
    STAMP(8);
    FMJ_PRIO_AT(FMJ_PRIO_L);
    // ---- L: L'DL over the lane dofs by rounds (as in ldl_factor); the 3x3 Schur complement of the translational dofs rides along
    // The leaves-first sweep of the solve rides in the rounds: when dof k is a pivot its right-hand side x_k is complete
    // (every descendant was a pivot before it) and t_ = row_k[depth_a] / D_k is exactly L[k][a], so each ancestor a does
    // x_a -= L[k][a] x_k next to its row update: no second pass over the factor, no extra LDS reads, no ancestor masks.
    float my_qacc, xt0 = 0.f, xt1 = 0.f, xt2 = 0.f;
    {
      float dinv_mine = 0.f;
      float x = qfrc;
      const cround_p RND = (cround_p)M.dual_rounds;
      // Published rows: RS entries + (1 / D, right-hand side) behind them, RS2 = RS + 4 floats apart; a round's descriptor carries the
      // byte offsets of its pivots' rows (DualRound::ro), so a pivot costs two address adds and no scalar multiply.
      constexpr int RS2 = dual_row_stride(RS);
      const char* const HRb = (const char*)HR;
      const char* const tkb = HRb + 4 * ddepth;        // the lane's own column in any row
      float* const myrow = HR + sl * RS2;
#define DECL_PIVOT(NG_, S_) float tk##S_ = 0.f, dki##S_ = 0.f, xk##S_ = 0.f; float4 rk##S_[NG_];
#define LOAD_PIVOT(NG_, ro_, S_) do { \
          tk##S_ = *(const float*)(tkb + (ro_)); { const float2 dx_ = *(const float2*)(HRb + (ro_) + 4 * RS); dki##S_ = dx_.x; xk##S_ = dx_.y; } \
          _Pragma("unroll") for (int g = 0; g < NG_; g++) rk##S_[g] = *(const float4*)(HRb + (ro_) + 16 * g); } while (0)
#define MATH_PIVOT(NG_, am_, S_) do { \
          const float t_ = mask_select(tk##S_ * dki##S_, am_); \
          const f2_t tt_ = f2_t{t_, t_}; \
          _Pragma("unroll") for (int g = 0; g < NG_; g++) { \
            pk_fnma(r[2 * g], tt_, f2_t{rk##S_[g].x, rk##S_[g].y}); \
            pk_fnma(r[2 * g + 1], tt_, f2_t{rk##S_[g].z, rk##S_[g].w}); } \
          diag = fmaf(-t_, tk##S_, diag); \
          x = fmaf(-t_, xk##S_, x); } while (0)
      // A pivot at depth d has entries in slots 0 .. d - 1 only, and so do the rows it updates: a round publishes, reads and
      // applies ceil(d / 4) float4 groups (the members of a round share their depth), picked by a uniform switch so that
      // every register index stays static.  Deep rounds move 4 groups, the rounds of the root's own dofs one.
      // The pivot's right-hand side travels with its 1 / D (one 8-byte LDS record behind the published row) instead of two v_readlane,
      // two moves and a select per pivot: + 3.6 % on the headline (round 4 A/B).  Tried with it and lost: reading the rows of a
      // round's second and third pivot before the first is applied (two rows in flight in the 256-register build): no gain alone,
      // - 2.8 % when it took registers from the resident model constants - the step is bound by instruction issue, not by these
      // latencies, which the other wave of the SIMD covers.
#define ROUND_BODY(NG_, R_) do { \
          _Pragma("unroll") for (int d = 0; d < 4 * NG_; d += 4) *(float4*)(myrow + d) = make_float4(r[d / 2].x, r[d / 2].y, r[d / 2 + 1].x, r[d / 2 + 1].y); \
          *(float2*)(myrow + RS) = make_float2(__builtin_amdgcn_rcpf(diag), x); \
          WSYNC(); \
          DECL_PIVOT(NG_, A) \
          LOAD_PIVOT(NG_, R_##o0, A); MATH_PIVOT(NG_, R_##a0, A); \
          if (R_##o1 >= 0) { LOAD_PIVOT(NG_, R_##o1, A); MATH_PIVOT(NG_, R_##a1, A); LOAD_PIVOT(NG_, R_##o2, A); MATH_PIVOT(NG_, R_##a2, A); } \
          WSYNC(); } while (0)
      {
        // Rounds come deepest level first, so the group count never grows from one round to the next: one loop per group
        // count, run one after the other (a switch inside one loop makes every join copy the whole register row).
        // The table ends with a terminator of depth -1 (fmj_create): a loop tests the depth alone and reads one round ahead without
        // a clamp.  Two descriptor sets, E and O, take turns (the loop body holds two rounds): the descriptor read one round ahead
        // lands in the set the next round uses, no scalar moves at the back edge.
#define GET_ROUND(R_, off_) \
        { const cround_p d_ = (cround_p)((const char __attribute__((address_space(4)))*)RND + (off_)); \
          R_##o0 = d_->ro[0]; R_##o1 = d_->ro[1]; R_##o2 = d_->ro[2]; R_##dep = d_->depth; R_##a0 = d_->anc[0]; R_##a1 = d_->anc[1]; R_##a2 = d_->anc[2]; }
        int Eo0, Eo1, Eo2, Edep, Oo0, Oo1, Oo2, Odep;
        unsigned long long Ea0, Ea1, Ea2, Oa0, Oa1, Oa2;
        GET_ROUND(E, 0)
        int ro = (int)sizeof(DualRound);             // byte offset of the round after the current one
#define ROUNDS_AT(NG_, LIM_) \
        _Pragma("unroll 1") while (Edep > (LIM_)) { \
          GET_ROUND(O, ro) \
          ROUND_BODY(NG_, E); \
          ro += (int)sizeof(DualRound); \
          if (Odep > (LIM_)) { \
            GET_ROUND(E, ro) \
            ROUND_BODY(NG_, O); \
            ro += (int)sizeof(DualRound); \
          } else { Eo0 = Oo0; Eo1 = Oo1; Eo2 = Oo2; Edep = Odep; Ea0 = Oa0; Ea1 = Oa1; Ea2 = Oa2; } \
        }
        if (MAXD >= 32) ROUNDS_AT((MAXD >= 32 ? 8 : 1), 28)
        if (MAXD >= 28) ROUNDS_AT((MAXD >= 28 ? 7 : 1), 24)
        if (MAXD >= 24) ROUNDS_AT((MAXD >= 24 ? 6 : 1), 20)
        if (MAXD >= 20) ROUNDS_AT((MAXD >= 20 ? 5 : 1), 16)
        if (MAXD >= 16) ROUNDS_AT((MAXD >= 16 ? 4 : 1), 12)
        if (MAXD >= 12) ROUNDS_AT((MAXD >= 12 ? 3 : 1), 8)
        if (MAXD >= 8) ROUNDS_AT((MAXD >= 8 ? 2 : 1), 4)
        ROUNDS_AT(1, -1)
#undef GET_ROUND
#undef ROUNDS_AT
      }
#undef ROUND_BODY
#undef LOAD_PIVOT
#undef DECL_PIVOT
#undef MATH_PIVOT
      dinv_mine = isd ? __builtin_amdgcn_rcpf(diag) : 0.f;      // (the factor stays in the registers: nothing of this kernel reads it from LDS)
      float l21 = 0.f, l20 = 0.f, l10 = 0.f, di0 = 0.f, di1 = 0.f, di2 = 0.f;
      if (T0) {
        const float c0 = isd ? r[0].x : 0.f, c1 = isd ? r[0].y : 0.f, c2 = isd ? r[1].x : 0.f;
        const float a0 = c0 * dinv_mine, a1 = c1 * dinv_mine, a2 = c2 * dinv_mine;
        float s00 = M.dual_tadd[0] - half_sum_all(a0 * c0), s11 = M.dual_tadd[1] - half_sum_all(a1 * c1);
        float s22 = M.dual_tadd[2] - half_sum_all(a2 * c2);
        float s10 = -half_sum_all(a1 * c0), s20 = -half_sum_all(a2 * c0), s21 = -half_sum_all(a2 * c1);
        di2 = rcp_nr(s22); l21 = s21 * di2; l20 = s20 * di2;
        s11 = fmaf(-l21, s21, s11); s10 = fmaf(-l21, s20, s10); s00 = fmaf(-l20, s20, s00);
        di1 = rcp_nr(s11); l10 = s10 * di1;
        s00 = fmaf(-l10, s10, s00);
        di0 = rcp_nr(s00);
      }
    STAMP(9);
      // ---- X: the translational block, then the root-first sweep
      if (T0) {
        const float lmx = isd ? r[0].x * dinv_mine : 0.f, lmy = isd ? r[0].y * dinv_mine : 0.f, lmz = isd ? r[1].x * dinv_mine : 0.f;
        qt0 -= half_sum_all(lmx * x); qt1 -= half_sum_all(lmy * x); qt2 -= half_sum_all(lmz * x);
        qt1 = fmaf(-l21, qt2, qt1); qt0 = fmaf(-l20, qt2, qt0); qt0 = fmaf(-l10, qt1, qt0);
        xt0 = qt0 * di0; xt1 = qt1 * di1; xt2 = qt2 * di2;
        xt1 = fmaf(-l10, xt0, xt1); xt2 = fmaf(-l20, xt0, xt2); xt2 = fmaf(-l21, xt1, xt2);
        x *= dinv_mine;
        x = fmaf(-lmx, xt0, x); x = fmaf(-lmy, xt1, x); x = fmaf(-lmz, xt2, x);
      } else x *= dinv_mine;
      {   // L part, root first, a tree level at a time (as in ldl_pull_sweep)
        const unsigned lmask = (unsigned)opaque_s((int)((1u << M.dual_maxdep) - (1u << T0)));      // levels T0 .. maxdep - 1
#pragma unroll
        for (int g = 0; g < MAXD / 4; g++) {
#pragma unroll
          for (int k = 0; k < 4; k++) {
            const int lvl = 4 * g + k;
            if (__builtin_expect((lmask & (1u << lvl)) != 0u, 1)) {     // (expected: the level's code falls through, a skipped level branches)
              const int src = (int)((ancl[g] >> (8 * k)) & 0xffu) + 4 * hb;
              const float xs = __int_as_float(__builtin_amdgcn_ds_bpermute(src, __float_as_int(x)));
              const float rl_ = (k & 2) ? ((k & 1) ? r[2 * g + 1].y : r[2 * g + 1].x) : ((k & 1) ? r[2 * g].y : r[2 * g].x);
              const float l = lvl < ddepth ? rl_ * dinv_mine : 0.f;      // (a lane without a dof has depth 0)
              x = fmaf(-l, xs, x);
            }
          }
        }
      }
      my_qacc = x;
    }
    STAMP(10);
    FMJ_PRIO_AT(FMJ_PRIO_XEND);
    // ---- Euler
    const float hstep = OPT_INTEGRATE ? M.h : 0.f;
    const float pre_qd = QV[mydof];
    const float nvel = pre_qd + hstep * my_qacc;
    if (isd) {
      if (!(fabsf(my_qacc) <= 1e10f)) warn |= FMJ_WARN_BADQACC;      // mj_checkAcc
      if (!(fabsf(nvel) <= 1e10f)) warn |= FMJ_WARN_BADQVEL;
    }
    if (T0 && sl == 1 && (!(fabsf(xt0) <= 1e10f) || !(fabsf(xt1) <= 1e10f) || !(fabsf(xt2) <= 1e10f))) warn |= FMJ_WARN_BADQACC;
    if (HALF_ANY((warn & FMJ_WARN_FREEZE) != 0)) { frozen = true; live = false; }   // the state stays at its last finite values
    float pre_q = 0.f;
    if (isd && !frozen) {
      XV[mydof] = my_qacc;
      QV[mydof] = nvel;
      if (d_scalar) {
        pre_q = QP[d_qadr];
        QP[d_qadr] = pre_q + hstep * nvel;
        if (last && live) {
          float AS1* s = gptr(A.sensordata) + (size_t)env * M.nsensordata + 6 * (nb - 1) + 3 * as_int4(DT2(mydof, 2)).z;
          s[0] = pre_q; s[1] = pre_qd; s[2] = 0.f;
        }
      }
    }
    bool posbad = false;
    if (T0 && sl == 1 && !frozen) {
      // translational dofs and the position of the free root: the root body lane applies the per-half scalars.  The new root position
      // is tested before it (and the translational velocity) is committed; the lanes of the other dofs commit theirs at the same
      // time and take them back below, so that a step that raises BADQPOS leaves qpos, qvel and time exactly as the previous step
      // left them (include/fmj.h: freeze contract) - at no cost to the steps that pass
      const float nv0 = QV[0] + hstep * xt0, nv1 = QV[1] + hstep * xt1, nv2 = QV[2] + hstep * xt2;
      const float nx = QP[0] + hstep * nv0, ny = QP[1] + hstep * nv1, nz = QP[2] + hstep * nv2;
      posbad = OPT_INTEGRATE && (!(fabsf(nx) <= 1e10f) || !(fabsf(ny) <= 1e10f) || !(fabsf(nz) <= 1e10f));
      if (posbad) warn |= FMJ_WARN_BADQPOS;
      else {
        XV[0] = xt0; XV[1] = xt1; XV[2] = xt2;
        QV[0] = nv0; QV[1] = nv1; QV[2] = nv2;
        QP[0] = nx; QP[1] = ny; QP[2] = nz;
      }
    }
    if (!frozen) steps_done++;
    WSYNC();
    if (T0 && sl == 1 && OPT_INTEGRATE && !frozen && !posbad) {      // orientation of the free root: needs the angular velocity the dof lanes just stored
      const float h = M.h;
      const v3 w = mk3(QV[3], QV[4], QV[5]);
      const float n2 = dot3(w, w), rn = rsqrt_nr(n2), n = n2 * rn;
      q4 qo = {QP[3], QP[4], QP[5], QP[6]};
      qo = qnormalize(qo);
      if (n2 >= 1e-30f) qo = qmul(qo, axisangle_small(scl3(w, rn), h * n));
      QP[3] = qo.w; QP[4] = qo.x; QP[5] = qo.y; QP[6] = qo.z;
    }
    if (HALF_ANY((warn & FMJ_WARN_BADQPOS) != 0) && !frozen) {   // no row of the next iteration from a bad position; the step is taken back
      if (isd) { QV[mydof] = pre_qd; if (d_scalar) QP[d_qadr] = pre_q; }
      steps_done--;
      frozen = true; live = false;
    }
    if (SUBS) { sub = nsub; if (nfull) { itm++; ring = ring_n1; } } else ring = ring_n1;
    WSYNC();
    STAMP(11);   // Euler
  }

  // ---- store state
  if (exists && steps_done > 0) {              // a frozen half leaves the last finite state it reached
    float AS1* oq = gptr(A.qpos) + (size_t)env * nq;
    float AS1* ov = gptr(A.qvel) + (size_t)env * nv;
    for (int i = sl; i < nq; i += 32) oq[i] = QP[i];
    for (int i = sl; i < nv; i += 32) ov[i] = QV[i];
    if (A.qacc) for (int i = sl; i < nv; i += 32) gptr(A.qacc)[(size_t)env * nv + i] = XV[i];
    if (A.time && sl == 0 && A.integrate) gptr(A.time)[env] += M.h * steps_done;
  }
  {
    int w = warn;
#pragma unroll
    for (int o = 16; o > 0; o >>= 1) w |= __shfl_xor(w, o, 64);
    if (w && sl == 0 && exists) gptr(A.status)[env] |= w;
  }
#ifdef FMJ_STAMPS
  if (env == 0 && lane == 0 && A.qacc) {     // stamp i = time up to marker i: 1 joints row, 2 K, 3 C, 4 V, 5 F, 0 row + drag, 6 S, 7 Q, 8 M, 9 L, 10 X, 11 Euler
#pragma unroll
    for (int i = 0; i < NSTAMP; i++) gptr(A.qacc)[i] = stamp_acc[i];
  }
  // this wave's entry and exit times and its placement, as raw words over the last six qacc slots of each of its envs (after the
  // qacc values other lanes stored there, in program order).  With nv - 6 < NSTAMP they also replace the tail of env 0's phase stamps:
  // scripts/stamps.py then reads slots >= nv - 6 of env 0 wrong (the eel, nv = 26)
  if (sl == 0 && exists && A.qacc && nv >= 6) {
    const unsigned long long life_t1 = __builtin_amdgcn_s_memtime();
    unsigned AS1* const w = (unsigned AS1*)(gptr(A.qacc) + (size_t)env * nv + nv - 6);
    w[0] = (unsigned)life_t0; w[1] = (unsigned)(life_t0 >> 32); w[2] = (unsigned)life_t1; w[3] = (unsigned)(life_t1 >> 32);
    w[4] = __builtin_amdgcn_s_getreg(FMJ_HWREG_HW_ID); w[5] = __builtin_amdgcn_s_getreg(FMJ_HWREG_XCC_ID);
  }
#endif
#undef HALF_ANY
#undef M
#undef A
#undef BT2
#undef DT2
#undef AT2
#undef ST2
#undef STAGE2_REC
#undef OPT_ROWS_AHEAD
#undef OPT_READOUT
#undef OPT_DRAG
#undef OPT_CONTROLLER
#undef OPT_TAPE
#undef OPT_NO_ACT
#undef OPT_STIFFNESS
#undef OPT_INTEGRATE
#undef OPT_WFREQ_ENV
#undef OPT_WAMP_STRIDE
#undef OPT_WLAG_STRIDE
}
