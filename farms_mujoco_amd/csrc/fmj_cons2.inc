// fmj_cons2.inc - the "two environments per wavefront" step kernel for models WITH constraints (included by fmj_hip.hip):
// joint limits and ground contacts, pyramidal cone, PGS - BASELINE configs[3], the reference's mj_step with
// option.solver = PGS (mjcf.py:1348-1353) and the contact readout of sensors.pyx:140-190.
//
// Why (round 4): the one-env constraint kernel runs at 2 waves per SIMD (244 VGPRs, 18.9 KB of LDS per env), so 4096 envs take
// TWO rounds of 2048 waves, each lane set half empty (29 bodies / 33 dofs / a median of 24 constraint rows on 64 lanes), and its
// PGS sweep is bound by the latency of the v_max -> v_readlane -> v_fmac chain of a row, not by issue (scripts/ubench/pgs.hip:
// 33.5 cycles per row whatever the occupancy, 23.7 per env-row with two envs per wave).  Here lanes 0..31 serve env A, lanes
// 32..63 env B of the wave, exactly as in fmj_dual2.inc for the unconstrained step (bodies, dofs minus the translational dofs of
// a free root, which are per-half scalars); 4096 envs are 2048 waves = ONE round at the same 2 waves per SIMD.
//
// The constraint rows of a step are handled in one of three ways, chosen per wave and per step from the two row counts:
//   PAIR  both envs have <= 32 rows (75 % of walking steps): lane = row inside each half, both envs at once - the rows of A in
//         32 registers per lane, PGS turns of the two halves interleaved (two readlanes and a select per turn);
//   SOLO  an env has 33..64 rows: the two envs take turns on all 64 lanes (lane = row), each exactly like the one-env kernel's
//         on-chip path; everything before and after the rows (kinematics ... the two factorisations, the final solve) stays
//         two-at-once;
//   RETIRE an env has more than 64 rows or more contacts than the on-chip list holds (animals dropping flat on the floor): ITS half
//         retires BEFORE this step changes anything of it - from here on it neither integrates nor stores rows, at the end of the
//         launch it stores its state as a launch boundary would and the number of steps it completed goes to StepArgs::resume -
//         while the other half of the wave steps on alone; the one-env kernel, launched right behind with the same arguments,
//         picks every retired env up where it stands (envs that completed cost it one early exit).  What an env computes
//         never depends on the env it shares its wave with.
// PAIR and SOLO run the same source (fmj_cons2_rows.inc, included once per mode): the arithmetic of an env does not depend on the
// mode it was solved in, nor on the env it shares its wave with.
//
// LDS (floats): per env  QP QV XS QW SD | HM (factor of M, lane dofs) | CT (16 contact records) | TS (3x3 factor of the
// translational block of M); per wave  SCR = scratch shared over time - { cdof, subtree force / inertia, poses } of both envs
// during kinematics .. M, the published rows of H during the factorisation and the final solve, the constraint rows (PAIR: 32
// compact rows + parameters per env; SOLO: 64 of one env) in between - + LC (chain-sharing table) + the pointer-jumping table.
// Salamander-33: 18.3 KB per wave = 8 waves per CU.

// sum over the 32 lanes of each half, valid in the half's LAST lane only (31 / 63): half_sum_dpp without the broadcast
__device__ __forceinline__ float half_sum_last(float v) {
  int x = __float_as_int(v);
  v += __int_as_float(__builtin_amdgcn_update_dpp(0, x, 0xB1, 0xF, 0xF, true));  x = __float_as_int(v);   // quad_perm [1,0,3,2]
  v += __int_as_float(__builtin_amdgcn_update_dpp(0, x, 0x4E, 0xF, 0xF, true));  x = __float_as_int(v);   // quad_perm [2,3,0,1]
  v += __int_as_float(__builtin_amdgcn_update_dpp(0, x, 0x141, 0xF, 0xF, true)); x = __float_as_int(v);   // row_half_mirror
  v += __int_as_float(__builtin_amdgcn_update_dpp(0, x, 0x140, 0xF, 0xF, true)); x = __float_as_int(v);   // row_mirror
  v += __int_as_float(__builtin_amdgcn_update_dpp(0, x, 0x142, 0xA, 0xF, true));                          // row_bcast:15 -> rows 1, 3
  return v;
}

struct Lds3 { int QP, QV, XS, QW, SD, HM, CT, TS, env_total; int CD, F, CI, PO, HRS, envscr; int SCR, LC, JMP, total; int nct; int rowsz; };
#define FMJ_C2_NCT 16      // contact records kept on chip per env: 16 contacts = 64 rows = what PAIR / SOLO hold; more is the BAIL case
__host__ __device__ inline Lds3 lds3_layout(int nb, int nv, int nq, int rs, int t0, int maxcon, int anc_stride) {
  Lds3 L; int o = 0;
  const int nd = nv - t0;
  L.nct = maxcon < FMJ_C2_NCT ? (maxcon > 0 ? maxcon : 1) : FMJ_C2_NCT;
  L.QP = o; o += r4(nq);
  L.QV = o; o += r4(nv);
  L.XS = o; o += r4(nv);                 // qacc_smooth; 1 / D of the published rows of M during the factorisation
  L.QW = o; o += r4(nv);                 // qacc_warmstart
  L.SD = o; o += r4(nv);                 // 1 / sqrt(D) of the factor of M; 1 / D of the published rows of H during the factorisation
  L.TS = o; o += 16;                     // translational blocks: l10 l20 l21 - of M; l10 l20 l21 di0 di1 di2 of H; qfrc_smooth of the three dofs
  L.HM = o; o += nd * rs;                // rows of the factor of M of the lane dofs (unit triangular: L itself)
  L.CT = o; o += L.nct * 16;             // contacts: pos(3) normal(3) t1(3) t2(3) dist mu geom|chain plane -> force(3), geoms
  L.env_total = r4(o);
  int s = 0;                             // per-env scratch of kinematics .. M
  L.CD = s; s += nv * 8;                 // cdof
  L.F = s; s += nb * 8;                  // subtree force
  L.CI = s; s += nb * 12;                // subtree inertia about its own CoM (6), subtree CoM (3), subtree mass
  L.PO = s; s += nb * 8;                 // body poses for the narrow phase
  L.HRS = L.F;                           // published rows of H (factorisation, final solve): F / CI / PO are dead by then
  if (L.HRS + nd * rs > s) s = L.HRS + nd * rs;
  L.envscr = r4(s);
  L.rowsz = 32 * rs + 32 * 8 + 8 + 32;   // PAIR: compact rows, row parameters, chain ends (bytes), D^1/2 Z' f of the lane dofs, of one env
  int scr = 2 * L.envscr;
  if (2 * L.rowsz > scr) scr = 2 * L.rowsz;
  if (64 * rs + 64 * 8 + 16 + 32 > scr) scr = 64 * rs + 64 * 8 + 16 + 32;      // SOLO: one env on all 64 lanes
  L.SCR = 2 * L.env_total;
  L.LC = L.SCR + r4(scr);
  L.JMP = L.LC + r4((nv * nv + 3) / 4);
  L.total = L.JMP + r4(r4(nb * anc_stride) / 4);
  return L;
}

template <bool FUSED, int MAXD>
#ifndef FMJ_C2_WPS      // development probes (scripts/kres.py 20 -DFMJ_DEV_CONS2_FUSED_ONLY -DFMJ_C2_WPS=1 [-DFMJ_X_NOPAIR] [-DFMJ_X_NOSOLO]): the register demand
#define FMJ_C2_WPS 2    // of the kernel with the 512-register budget of one wave per SIMD, with and without the two row pipelines (DESIGN section 2)
#endif
__global__ void __launch_bounds__(64, FMJ_C2_WPS) fmj_step_cons2_kernel(const DevModel M_by_value, const StepArgs A_by_value) {
  extern __shared__ __align__(16) float lds[];
  const char AS4* const karg = (const char AS4*)__builtin_amdgcn_kernarg_segment_ptr();
  const DevModel AS4* Mp = (const DevModel AS4*)karg;
  const StepArgs AS4* Ap = (const StepArgs AS4*)(karg + FMJ_KARG_A_OFF);
#define M (*Mp)
#define A (*Ap)
#define BT2(b, k) ldg4(M.btab, (unsigned)(b) * BT_STRIDE + (k))
#define DT2(d, k) ldg4(M.dtab, (unsigned)(d) * DT_STRIDE + (k))
#define AT2(a, k) ldg4(M.atab, (unsigned)(a) * AT_STRIDE + (k))
#define STAGE2_REC 8      // stride of the CD / F records, for the shared stages (fmj_stage2_*.inc)
  const int lane = threadIdx.x;
  const bool upper = lane >= 32;
  const int sl = lane & 31;
  const int hb = lane & 32;
  const int n_envs = A.n_envs;
  const int slot_raw = 2 * blockIdx.x + (upper ? 1 : 0);
  const bool exists = slot_raw < n_envs;        // odd batch: the last wave's upper half computes a copy of its partner, stores nothing
  const int slot = exists ? slot_raw : n_envs - 1;
  const int env = A.env_order ? gptr(A.env_order)[slot] : slot;
  const int nb = M.nbody, nv = M.nv, nq = M.nq, nu = M.nu;
  const int T0 = M.dual_t0;
  const int ND = nv - T0;
  constexpr int RS = MAXD;
  const Lds3 LL = lds3_layout(nb, nv, nq, RS, T0, M.max_contacts, M.anc_stride);
  float* const base = lds + (upper ? LL.env_total : 0);
  float* const scr = lds + LL.SCR + (upper ? LL.envscr : 0);
  float* const QP = base + LL.QP;
  float* const QV = base + LL.QV;
  float* const XS = base + LL.XS;
  float* const QW = base + LL.QW;
  float* const SD = base + LL.SD;
  float* const TS = base + LL.TS;
  float* const HM = base + LL.HM;
  float* const CT = base + LL.CT;
  float* const CD = scr + LL.CD;
  float* const F = scr + LL.F;
  float* const CI = scr + LL.CI;
  float* const PO = scr + LL.PO;
  float* const HRS = scr + LL.HRS;
  const uint8_t* const JMP = (const uint8_t*)(lds + LL.JMP);
  const int NCT = LL.nct;

  const bool isb = sl > 0 && sl < nb;
  const int bl = isb ? sl : 0;
  const bool isd = sl < ND;
  const int mydof = isd ? sl + T0 : T0;
  const int4 d_info0 = as_int4(DT2(mydof, 0));
  const int ddepth_o = isd ? d_info0.y : 0;
  const int dsub_o = isd ? d_info0.z : 0;
  const int dbody_o = d_info0.x;
  const int jrow_o = d_info0.w;

#define HALF_ANY(pred_) ({ const unsigned long long b_ = __ballot(pred_); upper ? (unsigned)(b_ >> 32) != 0u : (unsigned)b_ != 0u; })
#define HALF_BALLOT(pred_) ({ const unsigned long long b_ = __ballot(pred_); upper ? (unsigned)(b_ >> 32) : (unsigned)b_; })
  // ---- load tables + state
  int warn = 0;
  {
    for (int i = lane * 4; i < LL.total; i += 256) *(float4*)(lds + i) = make_float4(0.f, 0.f, 0.f, 0.f);   // see fmj_dual2.inc: finite everywhere
    WSYNC();
    uint32_t* jw = (uint32_t*)(lds + LL.JMP);
    const int nw = r4(nb * M.anc_stride) / 4;
    const uint32_t AS1* ga = gptr((const uint32_t*)M.b_anc);
    for (int i = lane; i < nw; i += 64) jw[i] = ga[i];
    uint32_t* lw = (uint32_t*)(lds + LL.LC);
    const uint32_t AS1* gl = gptr((const uint32_t*)M.lcad);
    for (int i = lane; i < (nv * nv + 3) / 4; i += 64) lw[i] = gl[i];
    const float AS1* gq = gptr(A.qpos) + (size_t)env * nq;
    const float AS1* gv = gptr(A.qvel) + (size_t)env * nv;
    const float AS1* gw = gptr(A.qacc_warmstart) + (size_t)env * nv;
    for (int i = sl; i < nq; i += 32) { const float v = gq[i]; QP[i] = v; if (!(fabsf(v) <= 1e10f)) warn |= FMJ_WARN_BADQPOS; }   // mj_checkPos
    for (int i = sl; i < nv; i += 32) { const float v = gv[i]; QV[i] = v; if (!(fabsf(v) <= 1e10f)) warn |= FMJ_WARN_BADQVEL; QW[i] = gw[i]; }   // mj_checkVel
  }
  bool frozen = (gptr(A.status)[env] & FMJ_WARN_FREEZE) != 0;
  frozen = frozen || HALF_ANY((warn & FMJ_WARN_FREEZE) != 0);
  bool live = exists && !frozen;
  int steps_done = 0;
  bool retired = false;                              // this half's env is handed to the one-env kernel (see the header): half-uniform
  int cy_ncon = 0;                                   // contacts of the last forward pass (records incl. forces stay in CT)
  bool retire_at_entry = false;                      // its contact list does not fit the chip: retired before step 0, AFTER the launch's first links row
  if (FUSED && A.contacts_rows) {
    cy_ncon = gptr(A.ncon)[env];
    if (cy_ncon > NCT) { retire_at_entry = true; cy_ncon = 0; }
    for (int i = sl; i < cy_ncon * 16; i += 32) CT[i] = gptr(A.contact)[(size_t)env * M.max_contacts * 16 + i];
  }
  const int4 d_act_o = as_int4(DT2(mydof, 2));       // first actuator, count, joint sensor slot, dof parent
  float lf_raw = 0.f;                                // joint-limit force of this dof's joint in the last forward pass (physics.py:484-487)
  float asum_raw = 0.f;                              // motor torque of the last forward pass (physics.py:510-524)
  {
    const float4 dp = DT2(mydof, 1);
    if (FUSED && isd && dp.w != 0.f) {
      const float AS1* sdp = gptr(A.sensordata) + (size_t)env * M.nsensordata + 6 * (nb - 1);
      lf_raw = sdp[3 * d_act_o.z + 2];
      const float AS1* sa = sdp + 3 * M.njs;
#pragma unroll
      for (int a = 0; a < 4; a++) if (a < d_act_o.y) asum_raw += sa[__float_as_int(AT2(d_act_o.x + a, 2).x)];
    }
  }
  const int it0 = A.iteration0;
  const long long r_offl = (long long)env * M.n_links * FMJ_LINK_SIZE, r_offj = (long long)env * M.n_joints * FMJ_JOINT_SIZE;
  const int link_row_o = as_int4(BT2(bl, 8)).z;
  // links row of a ring index from a pose / velocity of the last forward pass (physics.py:449-466,435-446)
  auto emit_links = [&](const int index, const v3 xp, const q4 xq, const v3 xi, const v3 linvel, const v3 angvel) {
    if (A.do_readout && isb && live && link_row_o >= 0) {
      const float im = A.inv_meters, iv = A.inv_velocity, ia = A.inv_angvel;
      float AS1* row = gptr(A.links) + ((size_t)index * A.row_stride_links + (size_t)r_offl) + link_row_o * FMJ_LINK_SIZE;
      stg4(row + 0, xi.x * im, xi.y * im, xi.z * im, xq.x);
      stg4(row + 4, xq.y, xq.z, xq.w, xp.x * im);
      stg4(row + 8, xp.y * im, xp.z * im, xq.x, xq.y);
      stg4(row + 12, xq.z, xq.w, linvel.x * iv, linvel.y * iv);
      stg4(row + 16, linvel.z * iv, angvel.x * ia, angvel.y * ia, angvel.z * ia);
    }
  };
  if (FUSED) {      // the launch's first iteration logs the fields the previous launch (or the reset's mj_forward) left in mjData
    const float AS1* p = gptr(A.xpos) + (size_t)env * nb * 3 + bl * 3;
    const float4 q = ldg4f(A.xquat + (size_t)env * nb * 4 + bl * 4);
    const float AS1* ip = gptr(A.xipos) + (size_t)env * nb * 3 + bl * 3;
    const float AS1* sdl = gptr(A.sensordata) + (size_t)env * M.nsensordata + 6 * (isb ? sl - 1 : 0);
    const q4 cq = {q.x, q.y, q.z, q.w};
    emit_links(it0 % A.buffer_size, mk3(p[0], p[1], p[2]), cq, mk3(ip[0], ip[1], ip[2]), mk3(sdl[0], sdl[1], sdl[2]), mk3(sdl[3], sdl[4], sdl[5]));
  }
  // an env retired at entry has its first links row now (the one-env kernel never writes the first row of an env it resumes: that row
  // belongs to whoever held the env when the launch began); nothing else of it is touched
  if (retire_at_entry) { retired = true; live = false; }
  WSYNC();

#ifdef FMJ_STAMPS
  float stamp_acc[NSTAMP];
#pragma unroll
  for (int i = 0; i < NSTAMP; i++) stamp_acc[i] = 0.f;
  unsigned long long stamp_prev = __builtin_amdgcn_s_memtime();
  const unsigned long long stamp_t0 = stamp_prev;
  int dbg_solo = 0, dbg_rows = 0;
#endif
  const int n_steps = A.n_steps;
  int ring = FUSED ? it0 % A.buffer_size : 0;
  int sub = 0, itm = 0;
  float my_qacc = 0.f, xq0 = 0.f, xq1 = 0.f, xq2 = 0.f;     // qacc of the last step (lane dof; translational dofs)
  int stop_step = retired ? 0 : n_steps;                      // what resume[] receives: the step this half retired in front of
  const int sl_o = lane;
  const unsigned dpack_o = (unsigned)ddepth_o | ((unsigned)dsub_o << 6) | ((unsigned)dbody_o << 12) | ((unsigned)(jrow_o + 1) << 18);
#pragma unroll 1
  for (int step = 0; step < n_steps; step++) {
    if (__all(frozen || retired)) break;
    asm volatile("" : "+s"(Ap));
    asm volatile("" : "+s"(Mp));
    const int lane = opaque(sl_o);
    const int T0 = opaque_s(M.dual_t0), ND = nv - T0;
    const bool upper = lane >= 32;
    const int sl = lane & 31, hb = lane & 32;
    const unsigned dpack = (unsigned)opaque((int)dpack_o);
    const int ddepth = dpack & 63, dsub = (dpack >> 6) & 63, dbody = (dpack >> 12) & 63, jrow = (int)((dpack >> 18) & 127) - 1;
    const bool isb = sl > 0 && sl < nb;
    const int bl = isb ? sl : 0;
    const bool isd = sl < ND;
    const int mydof = isd ? sl + T0 : T0;
    float* const base = lds + (upper ? LL.env_total : 0);
    float* const scr = lds + LL.SCR + (upper ? LL.envscr : 0);
    float* const QP = base + LL.QP;
    float* const QV = base + LL.QV;
    float* const XS = base + LL.XS;
    float* const QW = base + LL.QW;
    float* const SD = base + LL.SD;
    float* const TS = base + LL.TS;
    float* const HM = base + LL.HM;
    float* const CT = base + LL.CT;
    float* const CD = scr + LL.CD;
    float* const F = scr + LL.F;
    float* const CI = scr + LL.CI;
    float* const PO = scr + LL.PO;
    float* const HRS = scr + LL.HRS;
    uint32_t ancl[MAXD / 4];
#pragma unroll
    for (int g = 0; g < MAXD / 4; g++) ancl[g] = gptr(M.dual_ancl)[(unsigned)sl * (MAXD / 4) + g];
    const int it = it0 + itm;
    const bool last = step == n_steps - 1;
    const int S_sub = A.substeps;
    const bool full = sub == 0;
    const int nsub = sub + 1 >= S_sub ? 0 : sub + 1;
    const bool nfull = nsub == 0;
    const bool nrow1 = nfull || (nsub >= 1 && nsub >= S_sub - 1);      // see fmj_dual2.inc
    const int ring_n1 = FUSED ? (ring + 1 == A.buffer_size ? 0 : ring + 1) : 0;
    // ============ before_step (reference task.py:168-186) ============
    if (FUSED && A.do_readout && A.contacts_rows && full) {     // cycontacts2data from the carried contact list (sensors.pyx:140-190)
      if (live)
        for (int row = sl; row < A.n_contact_rows; row += 32)
          contact_row(CT, cy_ncon, row, glob(A.geom_sensor), A.n_pairs, glob(A.pairs), A.inv_newtons, A.inv_meters,
                      glob(A.contacts_rows) + ((size_t)ring * A.row_stride_contacts + ((size_t)env * A.n_contact_rows + row) * FMJ_CONTACT_SIZE));
      WSYNC();
    }
    STAMP(0);   // contact rows
    const float4 d_prm = DT2(mydof, 1);             // armature, damping, qposadr bits, hinge/slide flag
    const int d_qadr = __float_as_int(d_prm.z);
    const bool d_scalar = isd && d_prm.w != 0.f;
    if (FUSED && A.do_readout && full) {            // joints row (physics.py:500-524): the CURRENT qpos / qvel
      if (d_scalar && live && jrow >= 0) {
        float AS1* row = gptr(A.joints) + ((size_t)ring * A.row_stride_joints + (size_t)r_offj) + jrow * FMJ_JOINT_SIZE;
        stg4(row + 0, QP[d_qadr], QV[mydof] * A.inv_angvel, 0.f, 0.f);      // the whole row, as in fmj_dual2.inc
        stg4(row + 4, 0.f, 0.f, 0.f, 0.f);
        stg4(row + 8, asum_raw * A.inv_torques, lf_raw * A.inv_torques, 0.f, 0.f);
      }
    }
    STAMP(1);   // joints row
    // ============ mj_step ============
    const int4 c_info = as_int4(BT2(bl, 7));        // parent, jtype, qadr, dadr
    const int jtype = isb ? c_info.y : -1;
    const int qadr = c_info.z, dadr = c_info.w;
    const float4 c_axis_q0 = BT2(bl, 5);
    const float4 c_jpos_k = BT2(bl, 6);
    const uint32_t jm = sl < nb ? *(const uint32_t*)(JMP + sl * M.anc_stride) : 0u;
    const int max_bdepth = M.max_bdepth;
    const bool any_jpos = M.any_jpos != 0, any_bquat = M.any_bquat != 0, any_iquat = M.any_iquat != 0;
    // ---- K: local transforms, composed along the chains by pointer jumping
    v3 xp; q4 xq;
    {
      const float4 c_pos_mass = BT2(bl, 0);
      const float4 c_quat = BT2(bl, 1);
#include "fmj_stage2_k.inc"
      if (sl < nb) {
        *(float4*)(PO + sl * 8) = make_float4(xp.x, xp.y, xp.z, 0.f);
        *(float4*)(PO + sl * 8 + 4) = make_float4(xq.w, xq.x, xq.y, xq.z);
      }
    }
    STAMP(2);   // K
    v3 xi;
    {
      const float4 c_ipos = BT2(bl, 2);
      xi = add3(xp, qrot(xq, mk3(c_ipos.x, c_ipos.y, c_ipos.z)));
    }
    // ---- C: tree CoM of this half's env, world inertia about the body's own CoM
    const float mass = isb ? BT2(bl, 0).w : 0.f;
    v3 com;
    {
      const float mi = M.mtot_inv;
      com.x = half_sum_dpp(mass * xi.x, upper) * mi; com.y = half_sum_dpp(mass * xi.y, upper) * mi; com.z = half_sum_dpp(mass * xi.z, upper) * mi;
    }
    float iw[6];
    {
      const float4 c_iquat = BT2(bl, 3);
      const float4 c_inertia = BT2(bl, 4);
#include "fmj_stage2_c.inc"
    }
    STAMP(3);   // C
    // ---- V: joint velocity, cvel = chain sum of joint velocities, cacc = chain sum of cvel_parent x vJ - g
#include "fmj_stage2_v.inc"
    STAMP(4);   // V
    // ---- F: body force (inertial minus external) about the tree CoM
    const v3 dcom = sub3(xi, com);
    s6 fbody;
    {
#include "fmj_stage2_f.inc"
      float xf[6] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f};     // world-frame external force / torque on this body (the caller's xfrc_applied: this kernel
      if (A.xfrc_applied && isb) {                      // is not launched with the fused drag), re-read instead of carried across the steps
        const float AS1* x = gptr(A.xfrc_applied) + (size_t)env * nb * 6 + bl * 6;
#pragma unroll
        for (int k = 0; k < 6; k++) xf[k] = x[k];
      }
      const v3 fw = mk3(xf[0], xf[1], xf[2]), tw = mk3(xf[3], xf[4], xf[5]);
      f.r = sub3(f.r, add3(tw, cross(dcom, fw)));
      f.l = sub3(f.l, fw);
      if (!isb) { f.r = f.l = mk3(0.f, 0.f, 0.f); }
      fbody = f;
    }
    // ---- sensors of this (pre-integration) state: the link data of the next before_step (mj_step lag)
    const v3 linvel = add3(cv.l, cross(cv.r, dcom));
    if (FUSED && !last && (nfull || (A.sub_links && !(A.n_it_total > 0 && it + (nrow1 ? 1 : 0) >= A.n_it_total)))) emit_links(nrow1 ? ring_n1 : ring, xp, xq, xi, linvel, cv.r);
    if (last && live) {                                // fields of this (the last) forward pass: stored here, where they are (a step that then freezes or
                                                       // bails has stored the poses of its own state: a launch boundary's fields as well)
      if (sl < nb) {
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
    STAMP(5);   // F + rows
    // ---- S: subtree sums as prefix-sum differences inside the half (fp64 DPP scans, see fmj_hip.hip)
    {
      const float4 c_ipos = BT2(bl, 2);            // .w = subtree mass (model constant)
      const int lastl = hb | (isb ? sl + as_int4(BT2(bl, 8)).y - 1 : sl);
#include "fmj_stage2_s.inc"
    }
    WSYNC();
    STAMP(6);   // S
    // ---- Q (lane = dof T0 + sl; the translational dofs as per-half uniform scalars) and the rows of M in registers
    float qfrc = 0.f;
    float qt0 = 0.f, qt1 = 0.f, qt2 = 0.f;          // qfrc_smooth of the translational dofs
    if (T0) {
      const float4 fl = *(const float4*)(F + 1 * 8);
      const float2 fl2 = *(const float2*)(F + 1 * 8 + 4);
      qt0 = -DT2(0, 1).y * QV[0] - fl.w; qt1 = -DT2(1, 1).y * QV[1] - fl2.x; qt2 = -DT2(2, 1).y * QV[2] - fl2.y;
    }
    f2_t rh[MAXD / 2];                               // row of M, then of the factor of H, indexed by depth
#pragma unroll
    for (int d = 0; d < MAXD / 2; d++) rh[d] = f2_t{0.f, 0.f};
    float dgm = 1.f, dgh = 1.f;
    float dvel = 0.f;                                // implicitfast: velocity gains of this dof's unclamped actuators
    float asum_new = asum_raw;                       // this step's motor torque: committed once the half is known to keep the step
    s6 cdme = {mk3(0.f, 0.f, 0.f), mk3(0.f, 0.f, 0.f)};      // this lane's cdof: the Jacobian rows need it after CD has been overlaid
    {
      const s6 cd = isd ? lds_get6(CD + mydof * 8) : s6{mk3(0.f, 0.f, 0.f), mk3(0.f, 0.f, 0.f)};
      cdme = cd;
      const float4 ia = *(const float4*)(CI + dbody * 12), ib = *(const float4*)(CI + dbody * 12 + 4);
      const float2 ic = *(const float2*)(CI + dbody * 12 + 8);
      const v3 sc = mk3(ib.z, ib.w, ic.x);
      s6 bf;
      bf.r = mk3(ia.x * cd.r.x + ia.w * cd.r.y + ib.x * cd.r.z, ia.w * cd.r.x + ia.y * cd.r.y + ib.y * cd.r.z, ib.x * cd.r.x + ib.y * cd.r.y + ia.z * cd.r.z);
      bf.l = scl3(add3(cd.l, cross(cd.r, sc)), ic.y);
      const float qd = QV[mydof];
      if (isd) qfrc = -d_prm.y * qd - s6dot(cd, lds_get6(F + dbody * 8));
      if (d_scalar) {
        const float qj = QP[d_qadr];
        if (M.any_stiffness) {
          const float kst = BT2(dbody, 6).w;
          if (kst != 0.f) qfrc -= kst * (qj - gptr(A.qpos_spring)[(size_t)env * nq + d_qadr]);
        }
        float asum = 0.f, cbase = 0.f;
        const int controller = FUSED ? A.controller : 0;
        if (controller == 1) {
          const float wfreq = A.w_freq_env ? gptr(A.w_freq_env)[env] : A.w_freq;      // the env's own frequency (fmj_fused_ext), else the shared one
          double cyc = (double)wfreq * ((double)it * ((double)M.h * (double)S_sub));
          cyc -= floor(cyc);
          cbase = fmaf(6.283185307179586f, (float)cyc, gptr(A.w_env)[env]);
        }
        const float AS1* ctrl_row = A.ctrl ? gptr(A.ctrl) + (size_t)itm * A.ctrl_step_stride + (size_t)env * nu : nullptr;
        const bool no_act = A.disable_actuation != 0;
        const int4 d_act = as_int4(DT2(mydof, 2));
        const float AS1* const w_amp = gptr(A.w_amp) + (size_t)env * A.w_amp_stride;      // the env's rows (stride 0: the shared row)
        const float AS1* const w_lag = gptr(A.w_lag) + (size_t)env * A.w_lag_stride;
#pragma unroll
        for (int a = 0; a < 4; a++) {                 // mj_fwdActuation, joint transmission
          if (a < d_act.y) {
            const int ai = d_act.x + a;
            const float4 p = AT2(ai, 0), lim = AT2(ai, 1);
            const int src = __float_as_int(AT2(ai, 2).x);
            float c;
            if (controller == 1) { const float amp = w_amp[src]; c = amp != 0.f ? amp * sinf(cbase - w_lag[src]) : 0.f; }
            else c = ctrl_row ? ctrl_row[src] : 0.f;
            if (controller == 1 && last && live && A.ctrl_out) gptr(A.ctrl_out)[(size_t)env * nu + src] = c;
            c = fminf(fmaxf(c, lim.x), lim.y);
            float f = p.x * c + p.y + p.z * qj + p.w * qd;
            if (M.implicitfast && !no_act && f > lim.z && f < lim.w) dvel -= p.w;      // d force / d qvel of an unclamped actuator (include/fmj.h: implicitfast)
            f = fminf(fmaxf(f, lim.z), lim.w);
            if (no_act) f = 0.f;
            if (last && live) gptr(A.sensordata)[(size_t)env * M.nsensordata + 6 * (nb - 1) + 3 * M.njs + src] = f;      // actuatorfrc
            asum += f;
          }
        }
        qfrc += asum;
        asum_new = asum;
      }
      STAMP(7);   // Q
      // ---- M: row i of M (H differs on the diagonal only), one entry per depth of the chain root -> i (fmj_dual2.inc)
      const v3 gi = add3(bf.r, cross(sc, bf.l));
      const float mii = dot3(cd.r, gi) + dot3(cd.l, bf.l);
      dgm = isd ? mii + d_prm.x : 1.f;
      dgh = isd ? mii + (d_prm.x + M.h * (d_prm.y + dvel)) : 1.f;
      const unsigned dmask = (unsigned)opaque_s((int)((2u << M.dual_maxdep) - (1u << T0)));      // depths T0 .. maxdep as one uniform bit mask (fmj_dual2.inc)
#pragma unroll
      for (int g = 0; g < MAXD / 4; g++) {
#pragma unroll
        for (int k = 0; k < 4; k++) {
          const int d = 4 * g + k;
          float mij = d == 0 ? bf.l.x : (d == 1 ? bf.l.y : bf.l.z);
          if (__builtin_expect((dmask & (1u << d)) != 0u, 1)) {
            const int al = (int)((ancl[g] >> (8 * k)) & 0xffu) >> 2;
            const s6 cdj = lds_get6(CD + (al + T0) * 8);
            mij = dot3(cdj.r, gi) + dot3(cdj.l, bf.l);
          }
          if (k & 1) rh[d / 2].y = mij; else rh[d / 2].x = mij;
        }
      }
    }
    WSYNC();
    STAMP(8);   // M
    // ---- narrow phase (before the factorisation: the published rows of H overlay the poses): lane = geom of this half's env against
    //      the ground geom (one world-attached plane or heightfield: fmj_create), up to 4 contacts per geom, ordered by geom and point
    //      like the oracle's collide_ground; the records are written once the wave knows that it keeps the step
    const unsigned lt32 = (1u << sl) - 1u;
    int ncon = 0;
    int g_cnt = 0; v3 g_cq[4], g_nq[4]; float g_dq[4]; float g_rad = 0.f, g_mu = 0.f; int g_slot = 0;
    const float4 pn0 = M.nplane > 0 ? PTAB(0, 0) : make_float4(0.f, 0.f, 1.f, 0.f), pp0 = M.nplane > 0 ? PTAB(0, 1) : make_float4(0.f, 0.f, 0.f, 0.f);
#pragma unroll
    for (int k = 0; k < 4; k++) { g_cq[k] = mk3(0.f, 0.f, 0.f); g_nq[k] = mk3(0.f, 0.f, 1.f); g_dq[k] = 0.f; }
    if (M.nplane > 0) {
      const int g = sl;                              // fmj_create: ngeom <= 32 for this kernel
      const float4 pn = pn0, pp = pp0;
      int cnt = 0; float rad = 0.f, mu = 0.f;
#define NP_CQ g_cq
#define NP_NQ g_nq
#define NP_DQ g_dq
#define NP_PL 0
#include "fmj_narrow_ground.inc"      // sphere / capsule, box, cylinder: cnt, rad, mu and the first cnt entries of g_cq / g_nq / g_dq
#undef NP_CQ
#undef NP_NQ
#undef NP_DQ
#undef NP_PL
      int before = 0, total = 0;
#pragma unroll
      for (int k = 0; k < 4; k++) { const unsigned bk = HALF_BALLOT(cnt > k); before += __popc(bk & lt32); total += __popc(bk); }
      g_slot = before; ncon = total; g_cnt = cnt; g_rad = rad; g_mu = mu;
    }
    // joint limit rows (mj_instantiateLimit): lane = dof, rows ordered by joint then side (-1, +1)
    JOINT_LIMIT_ACT(DT2(mydof, 3));
    if (retired) { act_lo = false; act_hi = false; }
    const unsigned m_lo = HALF_BALLOT(act_lo), m_hi = HALF_BALLOT(act_hi);
    const int e_lo = __popc(m_lo & lt32) + __popc(m_hi & lt32);
    const int e_hi = e_lo + (act_lo ? 1 : 0);
    const int nlim = __popc(m_lo) + __popc(m_hi);
    bool cfull = false;
    if (ncon > M.max_contacts) { ncon = M.max_contacts; cfull = true; }
    int nefc = nlim + 4 * ncon;
    if (!retired && (nefc > 64 || ncon > NCT)) {      // RETIRE: nothing of this step has touched this env's state, warm start or contact list
      retired = true; live = false; stop_step = step; cfull = false;     // (the one-env kernel redoes the step and reports a full list)
    }
    if (retired) { nefc = 0; ncon = 0; }              // no rows: the other half of the wave has the step to itself
    else asum_raw = asum_new;
    if (cfull) warn |= FMJ_WARN_CONTACTFULL;
    // the two row counts, wave-uniform
    const int nefcA = __builtin_amdgcn_readlane(nefc, 0), nefcB = __builtin_amdgcn_readlane(nefc, 32);
    const int nconA = __builtin_amdgcn_readlane(ncon, 0), nconB = __builtin_amdgcn_readlane(ncon, 32);
    {   // contact records (CONTACT_RECORD of fmj_narrow.inc)
#pragma unroll
      for (int k = 0; k < 4; k++) {
        const int cslot = g_slot + k;
        if (k < g_cnt && cslot < ncon)
          CONTACT_RECORD(cslot, g_nq[k], sub3(g_cq[k], scl3(nrm, g_rad + 0.5f * g_dq[k])), g_dq[k], g_mu, __int_as_float(sl | ((GTABI(sl, 0).z + 1) << 16)), pp0.z);
      }
    }
    WSYNC();
    STAMP(13);  // limits + contacts
    // ---- L: M and H = M + diag(h damping) factored together by rounds (ldl_factor2 of fmj_hip.hip in the two-env layout), the
    //      leaves-first sweep of qacc_smooth = M^-1 qfrc_smooth riding in the rounds; the 3 x 3 Schur complements of the translational
    //      dofs of both matrices follow in scalar code (fmj_dual2.inc)
    float dinv_m, dinv_h;
    float xsm = qfrc;                                 // becomes qacc_smooth of this lane's dof
    {
      float ml10 = 0.f, ml20 = 0.f, ml21 = 0.f, mdi0 = 0.f, mdi1 = 0.f, mdi2 = 0.f;     // translational block of M (parked in TS / SD)
      float xst0 = 0.f, xst1 = 0.f, xst2 = 0.f;         // qacc_smooth of the translational dofs (parked in XS)
      f2_t rm[MAXD / 2];
#pragma unroll
      for (int d = 0; d < MAXD / 2; d++) rm[d] = rh[d];
      float* const PX3 = CD;        // per published row: 1 / D of M, 1 / D of H, the right-hand side (cdof is dead by now); see fmj_dual2.inc
      const cround_p RND = (cround_p)M.dual_rounds;
#define APPLY_PIVOT2(NG_, p_, am_) do { \
        const float tkm_ = HM[(p_) * RS + ddepth], tkh_ = HRS[(p_) * RS + ddepth]; const float4 px_ = *(const float4*)(PX3 + 4 * (p_)); const float dkm_ = px_.x, dkh_ = px_.y; \
        float4 km_[NG_], kh_[NG_]; \
        _Pragma("unroll") for (int g = 0; g < NG_; g++) { km_[g] = *(const float4*)(HM + (p_) * RS + 4 * g); kh_[g] = *(const float4*)(HRS + (p_) * RS + 4 * g); } \
        const float tm_ = mask_select(tkm_ * dkm_, am_), th_ = mask_select(tkh_ * dkh_, am_); \
        const f2_t ttm_ = f2_t{tm_, tm_}, tth_ = f2_t{th_, th_}; \
        _Pragma("unroll") for (int g = 0; g < NG_; g++) { \
          pk_fnma(rm[2 * g], ttm_, f2_t{km_[g].x, km_[g].y}); \
          pk_fnma(rm[2 * g + 1], ttm_, f2_t{km_[g].z, km_[g].w}); \
          pk_fnma(rh[2 * g], tth_, f2_t{kh_[g].x, kh_[g].y}); \
          pk_fnma(rh[2 * g + 1], tth_, f2_t{kh_[g].z, kh_[g].w}); } \
        dgm = fmaf(-tm_, tkm_, dgm); dgh = fmaf(-th_, tkh_, dgh); \
        xsm = fmaf(-tm_, px_.z, xsm); } while (0)
#define ROUND_BODY2(NG_) do { \
        if (isd) { \
          _Pragma("unroll") for (int d = 0; d < 4 * NG_; d += 4) { \
            *(float4*)(HM + sl * RS + d) = make_float4(rm[d / 2].x, rm[d / 2].y, rm[d / 2 + 1].x, rm[d / 2 + 1].y); \
            *(float4*)(HRS + sl * RS + d) = make_float4(rh[d / 2].x, rh[d / 2].y, rh[d / 2 + 1].x, rh[d / 2 + 1].y); } \
          *(float4*)(PX3 + 4 * sl) = make_float4(__builtin_amdgcn_rcpf(dgm), __builtin_amdgcn_rcpf(dgh), xsm, 0.f); \
        } \
        WSYNC(); \
        APPLY_PIVOT2(NG_, p0, a0); \
        if (p1 >= 0) { APPLY_PIVOT2(NG_, p1, a1); APPLY_PIVOT2(NG_, p2, a2); } \
        WSYNC(); } while (0)
      {
        // the table ends with a terminator of depth -1 (fmj_create): a loop tests the depth alone and reads one round ahead without a clamp
        int p0 = RND[0].p0, p1 = RND[0].p1, p2 = RND[0].p2, dep = RND[0].depth;
        unsigned long long a0 = RND[0].anc[0], a1 = RND[0].anc[1], a2 = RND[0].anc[2];
        int ro = (int)sizeof(DualRound);             // byte offset of the round after the current one
#define ROUNDS_AT(NG_, COND_) \
        _Pragma("unroll 1") while (COND_) { \
          const cround_p nx_ = (cround_p)((const char __attribute__((address_space(4)))*)RND + ro); \
          const int np0 = nx_->p0, np1 = nx_->p1, np2 = nx_->p2, ndep = nx_->depth; \
          const unsigned long long na0 = nx_->anc[0], na1 = nx_->anc[1], na2 = nx_->anc[2]; \
          ROUND_BODY2(NG_); \
          p0 = np0; p1 = np1; p2 = np2; a0 = na0; a1 = na1; a2 = na2; dep = ndep; ro += (int)sizeof(DualRound); \
        }
        DEPTH_LADDER(ROUNDS_AT, dep >= 0)
#undef ROUNDS_AT
      }
#undef ROUND_BODY2
#undef APPLY_PIVOT2
      dinv_m = isd ? __builtin_amdgcn_rcpf(dgm) : 0.f;
      dinv_h = isd ? __builtin_amdgcn_rcpf(dgh) : 0.f;
      if (isd) {        // the factor of M as the unit-triangular L itself: the rows' chain walks, J' products and sweeps read it
#pragma unroll
        for (int d = 0; d < MAXD; d += 4)
          *(float4*)(HM + sl * RS + d) = make_float4(rm[d / 2].x * dinv_m, rm[d / 2].y * dinv_m, rm[d / 2 + 1].x * dinv_m, rm[d / 2 + 1].y * dinv_m);
      }
      float hl10 = 0.f, hl20 = 0.f, hl21 = 0.f, hdi0 = 0.f, hdi1 = 0.f, hdi2 = 0.f;     // translational block of H
      if (T0) {
#define SCHUR3(r_, dinv_, tadd_, l10_, l20_, l21_, di0_, di1_, di2_) do { \
          const float c0_ = isd ? r_[0].x : 0.f, c1_ = isd ? r_[0].y : 0.f, c2_ = isd ? r_[1].x : 0.f; \
          const float a0_ = c0_ * dinv_, a1_ = c1_ * dinv_, a2_ = c2_ * dinv_; \
          float s00_ = tadd_[0] - half_sum_dpp(a0_ * c0_, upper), s11_ = tadd_[1] - half_sum_dpp(a1_ * c1_, upper); \
          float s22_ = tadd_[2] - half_sum_dpp(a2_ * c2_, upper); \
          float s10_ = -half_sum_dpp(a1_ * c0_, upper), s20_ = -half_sum_dpp(a2_ * c0_, upper), s21_ = -half_sum_dpp(a2_ * c1_, upper); \
          di2_ = rcp_nr(s22_); l21_ = s21_ * di2_; l20_ = s20_ * di2_; \
          s11_ = fmaf(-l21_, s21_, s11_); s10_ = fmaf(-l21_, s20_, s10_); s00_ = fmaf(-l20_, s20_, s00_); \
          di1_ = rcp_nr(s11_); l10_ = s10_ * di1_; \
          s00_ = fmaf(-l10_, s10_, s00_); \
          di0_ = rcp_nr(s00_); } while (0)
        SCHUR3(rm, dinv_m, M.dual_taddm, ml10, ml20, ml21, mdi0, mdi1, mdi2);
        SCHUR3(rh, dinv_h, M.dual_tadd, hl10, hl20, hl21, hdi0, hdi1, hdi2);      // parked in TS until the final solve
#undef SCHUR3
      }
      // qacc_smooth: the translational block, then the root-first sweep (ldl_pull_sweep in the two-env layout)
      const float lmx = isd ? rm[0].x * dinv_m : 0.f, lmy = isd ? rm[0].y * dinv_m : 0.f, lmz = isd ? rm[1].x * dinv_m : 0.f;
      if (T0) {
        float q0 = qt0 - half_sum_dpp(lmx * xsm, upper), q1 = qt1 - half_sum_dpp(lmy * xsm, upper), q2 = qt2 - half_sum_dpp(lmz * xsm, upper);
        q1 = fmaf(-ml21, q2, q1); q0 = fmaf(-ml20, q2, q0); q0 = fmaf(-ml10, q1, q0);
        xst0 = q0 * mdi0; xst1 = q1 * mdi1; xst2 = q2 * mdi2;
        xst1 = fmaf(-ml10, xst0, xst1); xst2 = fmaf(-ml20, xst0, xst2); xst2 = fmaf(-ml21, xst1, xst2);
        xsm *= dinv_m;
        xsm = fmaf(-lmx, xst0, xsm); xsm = fmaf(-lmy, xst1, xsm); xsm = fmaf(-lmz, xst2, xsm);
      } else xsm *= dinv_m;
      {
        const unsigned lmask = (unsigned)opaque_s((int)((1u << M.dual_maxdep) - (1u << T0)));      // levels T0 .. maxdep - 1 (fmj_dual2.inc)
        const int dds = opaque(ddepth);
#pragma unroll
        for (int g = 0; g < MAXD / 4; g++) {
          const unsigned aw_ = (unsigned)opaque((int)ancl[g]);      // its own copy per sweep: shared, the 17 lane addresses stay live across the whole step and spill
#pragma unroll
          for (int k = 0; k < 4; k++) {
            const int lvl = 4 * g + k;
            if (__builtin_expect((lmask & (1u << lvl)) != 0u, 1)) {
              const int src = (int)((aw_ >> (8 * k)) & 0xffu) + 4 * hb;
              const float xa_ = __int_as_float(__builtin_amdgcn_ds_bpermute(src, __float_as_int(xsm)));
              const float rl_ = (k & 2) ? ((k & 1) ? rm[2 * g + 1].y : rm[2 * g + 1].x) : ((k & 1) ? rm[2 * g].y : rm[2 * g].x);
              const float l = (isd && lvl < opaque(dds)) ? rl_ * dinv_m : 0.f;
              xsm = fmaf(-l, xa_, xsm);
            }
          }
        }
      }
      WSYNC();         // the last round's reads of XS / SD (1 / D of the published rows) are done
      if (isd) { XS[mydof] = xsm; SD[mydof] = sqrtf(dinv_m); }
      if (T0 && sl == 0) {
        XS[0] = xst0; XS[1] = xst1; XS[2] = xst2;
        SD[0] = sqrtf(mdi0); SD[1] = sqrtf(mdi1); SD[2] = sqrtf(mdi2);
        TS[0] = ml10; TS[1] = ml20; TS[2] = ml21;
        TS[4] = hl10; TS[5] = hl20; TS[6] = hl21; TS[7] = hdi0; TS[8] = hdi1; TS[9] = hdi2; TS[10] = qt0; TS[11] = qt1; TS[12] = qt2;
      }
    }
    WSYNC();
    STAMP(12);  // factor M + H, qacc_smooth
    // ---- constraint rows, PGS, constraint forces: both envs at once when each has at most 32 rows, else one after the other
    float qfrc_c = 0.f, qc0 = 0.f, qc1 = 0.f, qc2 = 0.f;      // qfrc_constraint of the lane dof / the translational dofs
    float lf = 0.f;                                            // joint-limit force of this dof's joint
    const float hstepc = M.h;
#ifdef FMJ_STAMPS
    dbg_solo += (nefcA > 32 || nefcB > 32) ? 1 : 0; dbg_rows += nefcA > nefcB ? nefcA : nefcB;
#endif
    if (nefcA <= 32 && nefcB <= 32) {
#ifndef FMJ_X_NOPAIR
      if (nefcA > 0 || nefcB > 0) {
#define CR_PAIR 1
#include "fmj_cons2_rows.inc"
#undef CR_PAIR
      } else
#endif
      if (!retired) { if (isd) QW[mydof] = xsm; if (T0 && sl == 0) { QW[0] = XS[0]; QW[1] = XS[1]; QW[2] = XS[2]; } }
    } else {
#ifndef FMJ_X_NOSOLO
#pragma unroll 1
      for (int xenv = 0; xenv < 2; xenv++) {
#define CR_PAIR 0
#include "fmj_cons2_rows.inc"
#undef CR_PAIR
      }
#endif
    }
    WSYNC();
    if (!retired) { lf_raw = lf; cy_ncon = ncon; }
    // ---- X: H qacc = qfrc_smooth + qfrc_constraint with the factor of H: its rows are published once more (scaled: L itself), the
    //      leaves-first sweep walks the lane dofs from the last to the first, then the translational block, then the root-first sweep
    float xt0 = 0.f, xt1 = 0.f, xt2 = 0.f;
    {
      if (isd) {
#pragma unroll
        for (int d = 0; d < MAXD; d += 4)
          *(float4*)(HRS + sl * RS + d) = make_float4(rh[d / 2].x * dinv_h, rh[d / 2].y * dinv_h, rh[d / 2 + 1].x * dinv_h, rh[d / 2 + 1].y * dinv_h);
      }
      WSYNC();
      float x = isd ? qfrc + qfrc_c : 0.f;
      {   // a right-hand side that is not finite must not reach the other env of the wave through the zero multiplicands below
        const bool xbad = HALF_ANY(!(fabsf(x) <= 1e30f));
        if (xbad) { warn |= FMJ_WARN_BADQACC; x = 0.f; }
      }
      {
        const int ddl = opaque(ddepth), dsl = opaque(dsub);
        int i = ND - 1;
        for (; i >= 8; i -= 8) {                       // batches of 8 pivots: the LDS reads do not depend on x
          float la[8], lb[8];
#pragma unroll
          for (int u = 0; u < 8; u++) {
            const float l_ = (isd && sl < i - u && i - u < sl + dsl) ? -HRS[(i - u) * RS + ddl] : 0.f;
            la[u] = upper ? 0.f : l_; lb[u] = upper ? l_ : 0.f;
          }
#pragma unroll
          for (int u = 0; u < 8; u++) { const float sa_ = bcast(x, i - u), sb_ = bcast(x, i - u + 32); x = fmaf(la[u], sa_, x); x = fmaf(lb[u], sb_, x); }
        }
#pragma unroll 1
        for (; i >= 1; i--) {
          const float l_ = (isd && sl < i && i < sl + dsl) ? -HRS[i * RS + ddl] : 0.f;
          const float sa_ = bcast(x, i), sb_ = bcast(x, i + 32);
          x = fmaf(upper ? 0.f : l_, sa_, x); x = fmaf(upper ? l_ : 0.f, sb_, x);
        }
      }
      const float lhx = isd ? rh[0].x * dinv_h : 0.f, lhy = isd ? rh[0].y * dinv_h : 0.f, lhz = isd ? rh[1].x * dinv_h : 0.f;
      if (T0) {
        const float hl10 = TS[4], hl20 = TS[5], hl21 = TS[6], hdi0 = TS[7], hdi1 = TS[8], hdi2 = TS[9], qt0 = TS[10], qt1 = TS[11], qt2 = TS[12];
        float q0 = qt0 + qc0 - half_sum_dpp(lhx * x, upper), q1 = qt1 + qc1 - half_sum_dpp(lhy * x, upper), q2 = qt2 + qc2 - half_sum_dpp(lhz * x, upper);
        q1 = fmaf(-hl21, q2, q1); q0 = fmaf(-hl20, q2, q0); q0 = fmaf(-hl10, q1, q0);
        xt0 = q0 * hdi0; xt1 = q1 * hdi1; xt2 = q2 * hdi2;
        xt1 = fmaf(-hl10, xt0, xt1); xt2 = fmaf(-hl20, xt0, xt2); xt2 = fmaf(-hl21, xt1, xt2);
        x *= dinv_h;
        x = fmaf(-lhx, xt0, x); x = fmaf(-lhy, xt1, x); x = fmaf(-lhz, xt2, x);
      } else x *= dinv_h;
      {
        const unsigned lmask = (unsigned)opaque_s((int)((1u << M.dual_maxdep) - (1u << T0)));      // levels T0 .. maxdep - 1 (fmj_dual2.inc)
        const int ddx = opaque(ddepth);
#pragma unroll
        for (int g = 0; g < MAXD / 4; g++) {
          const unsigned aw_ = (unsigned)opaque((int)ancl[g]);      // its own copy per sweep: shared, the 17 lane addresses stay live across the whole step and spill
#pragma unroll
          for (int k = 0; k < 4; k++) {
            const int lvl = 4 * g + k;
            if (__builtin_expect((lmask & (1u << lvl)) != 0u, 1)) {
              const int src = (int)((aw_ >> (8 * k)) & 0xffu) + 4 * hb;
              const float xa_ = __int_as_float(__builtin_amdgcn_ds_bpermute(src, __float_as_int(x)));
              const float rl_ = (k & 2) ? ((k & 1) ? rh[2 * g + 1].y : rh[2 * g + 1].x) : ((k & 1) ? rh[2 * g].y : rh[2 * g].x);
              const float l = (isd && lvl < opaque(ddx)) ? rl_ * dinv_h : 0.f;
              x = fmaf(-l, xa_, x);
            }
          }
        }
      }
      if (!(frozen || retired)) my_qacc = x;
    }
    STAMP(10);  // X
    // ---- Euler
    const float hstep = A.integrate ? M.h : 0.f;
    const float pre_qd = QV[mydof];
    const float nvel = pre_qd + hstep * my_qacc;
    if (isd) {
      if (!(fabsf(my_qacc) <= 1e10f)) warn |= FMJ_WARN_BADQACC;      // mj_checkAcc
      if (!(fabsf(nvel) <= 1e10f)) warn |= FMJ_WARN_BADQVEL;
    }
    if (T0 && sl == 1 && (!(fabsf(xt0) <= 1e10f) || !(fabsf(xt1) <= 1e10f) || !(fabsf(xt2) <= 1e10f))) warn |= FMJ_WARN_BADQACC;
    // the root position this step would commit is tested BEFORE anything is committed: a step that raises BADQPOS leaves qpos, qvel and
    // time exactly at the previous step's values
    if (T0 && sl == 1 && A.integrate) {
      const float h_ = M.h;
      if (!(fabsf(QP[0] + h_ * (QV[0] + h_ * xt0)) <= 1e10f) || !(fabsf(QP[1] + h_ * (QV[1] + h_ * xt1)) <= 1e10f) || !(fabsf(QP[2] + h_ * (QV[2] + h_ * xt2)) <= 1e10f)) warn |= FMJ_WARN_BADQPOS;
    }
    if (HALF_ANY((warn & FMJ_WARN_FREEZE) != 0)) { frozen = true; live = false; }
    const bool idle = frozen || retired;          // this half does not integrate
    if (!idle) { xq0 = xt0; xq1 = xt1; xq2 = xt2; }
    if (isd && !idle) {
      QV[mydof] = nvel;
      if (d_scalar) {
        const float pre_q = QP[d_qadr];
        QP[d_qadr] = pre_q + hstep * nvel;
        if (last && live) {
          const int4 d_act = as_int4(DT2(mydof, 2));
          float AS1* s = gptr(A.sensordata) + (size_t)env * M.nsensordata + 6 * (nb - 1) + 3 * d_act.z;   // jointpos, jointvel, jointlimitfrc
          s[0] = pre_q; s[1] = pre_qd; s[2] = lf;
        }
      }
    }
    if (T0 && sl == 1 && !idle) { QV[0] += hstep * xt0; QV[1] += hstep * xt1; QV[2] += hstep * xt2; }
    if (!idle) steps_done++;
    WSYNC();
    if (jtype == FMJ_JNT_FREE && A.integrate && !idle) {
      const float h = M.h;
      const float nx = QP[qadr] + h * QV[dadr], ny = QP[qadr + 1] + h * QV[dadr + 1], nz = QP[qadr + 2] + h * QV[dadr + 2];
      if (!(fabsf(nx) <= 1e10f) || !(fabsf(ny) <= 1e10f) || !(fabsf(nz) <= 1e10f)) warn |= FMJ_WARN_BADQPOS;
      else {
        QP[qadr] = nx; QP[qadr + 1] = ny; QP[qadr + 2] = nz;
        const v3 w = mk3(QV[dadr + 3], QV[dadr + 4], QV[dadr + 5]);
        const float n2 = dot3(w, w), rn = rsqrt_nr(n2), n = n2 * rn;
        q4 qo = {QP[qadr + 3], QP[qadr + 4], QP[qadr + 5], QP[qadr + 6]};
        qo = qnormalize(qo);
        if (n2 >= 1e-30f) qo = qmul(qo, axisangle_small(scl3(w, rn), h * n));
        QP[qadr + 3] = qo.w; QP[qadr + 4] = qo.x; QP[qadr + 5] = qo.y; QP[qadr + 6] = qo.z;
      }
    }
    if (HALF_ANY((warn & FMJ_WARN_BADQPOS) != 0)) { frozen = true; live = false; }
    sub = nsub; if (nfull) { itm++; ring = ring_n1; }
    WSYNC();
    STAMP(11);  // Euler
  }

  // ---- store state: what a launch boundary hands on (also to the one-env kernel after a BAIL)
  if (exists) {
    const bool wrote = steps_done > 0;
    if (wrote) {
      float AS1* oq = gptr(A.qpos) + (size_t)env * nq;
      float AS1* ov = gptr(A.qvel) + (size_t)env * nv;
      for (int i = sl; i < nq; i += 32) oq[i] = QP[i];
      for (int i = sl; i < nv; i += 32) ov[i] = QV[i];
      if (A.qacc) {
        if (isd) gptr(A.qacc)[(size_t)env * nv + mydof] = my_qacc;
        if (T0 && sl == 0) { float AS1* qa = gptr(A.qacc) + (size_t)env * nv; qa[0] = xq0; qa[1] = xq1; qa[2] = xq2; }
      }
      if (A.time && sl == 0 && A.integrate) gptr(A.time)[env] += M.h * steps_done;
      if (A.integrate && !frozen) for (int i = sl; i < nv; i += 32) gptr(A.qacc_warmstart)[(size_t)env * nv + i] = QW[i];     // mj_step saves qacc as the next warm start
      // contact list and forces of the last forward pass (mjData.contact, mj_contactForce)
      for (int i = sl; i < cy_ncon * 16; i += 32) gptr(A.contact)[(size_t)env * M.max_contacts * 16 + i] = CT[i];
      if (sl == 0) gptr(A.ncon)[env] = cy_ncon;
      if (retired && stop_step < n_steps) {
        // the one-env kernel resumes from mjData: it reads the limit force and the motor torque of the last forward pass there
        const float4 dp = DT2(mydof, 1);
        if (isd && dp.w != 0.f) {
          float AS1* sdp = gptr(A.sensordata) + (size_t)env * M.nsensordata + 6 * (nb - 1);
          sdp[3 * d_act_o.z + 2] = lf_raw;
          float AS1* sa = sdp + 3 * M.njs;
#pragma unroll
          for (int a = 0; a < 4; a++) if (a < d_act_o.y) sa[__float_as_int(AT2(d_act_o.x + a, 2).x)] = a == 0 ? asum_raw : 0.f;
        }
      }
    }
    if (A.resume && sl == 0) gptr(A.resume)[env] = (frozen || !retired) ? n_steps : stop_step;
  }
  {
    int w = warn;
#pragma unroll
    for (int o = 16; o > 0; o >>= 1) w |= __shfl_xor(w, o, 64);
    if (w && sl == 0 && exists) gptr(A.status)[env] |= w;
  }
#ifdef FMJ_STAMPS
  if (sl == 0 && exists && A.qacc) {      // lifetime of this wave in the launch (cycles) in the last qacc slot of its envs: the spread over the waves
    gptr(A.qacc)[(size_t)env * nv + nv - 1] = (float)(__builtin_amdgcn_s_memtime() - stamp_t0);
    gptr(A.qacc)[(size_t)env * nv + nv - 2] = (float)dbg_solo;      // steps this wave took one env at a time
    gptr(A.qacc)[(size_t)env * nv + nv - 3] = (float)dbg_rows;      // sum over the steps of the longer row count of the two envs
  }
  if (env == 0 && sl == 0 && exists && A.qacc) {
#pragma unroll
    for (int i = 0; i < NSTAMP; i++) gptr(A.qacc)[i] = stamp_acc[i];
  }
#endif
#undef HALF_ANY
#undef HALF_BALLOT
#undef M
#undef A
#undef BT2
#undef DT2
#undef AT2
#undef STAGE2_REC
}
