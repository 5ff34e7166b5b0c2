// fmj_f64_step.inc - the text of the fp64 step kernel, included twice by fmj_f64.inc (which has the description, the tables, the LDS map
// and the helpers): with F64_STEP_RK4 0 it is fmj_step_f64_kernel (one forward pass and the semi-implicit Euler commit per step), with
// F64_STEP_RK4 1 fmj_step_f64_rk4_kernel (the pass loop below runs four times per step; dynamic LDS is ldsd_total_bytes +
// F64_RK4_LDS_DOUBLES(nu)).  Every `RK4` condition is a compile-time constant: the first kernel compiles to what it was before the loop.
// With F64_STEP_CONTACTS 1 it is fmj_step_f64_contacts_kernel<LIMITS> (never fused; a fifth argument, F64Contacts; dynamic
// LDS is ldsd_contacts_bytes): ground contacts as four more unilateral rows each in the Newton solve of the LIMITS build.  Every
// `CONTACTS` condition is a compile-time constant, and CONS = LIMITS || CONTACTS is LIMITS in the other two texts.
// With F64_STEP_TERRAIN 1 on top of that it is fmj_step_f64_terrain_kernel<LIMITS> (a sixth argument, F64Terrain; dynamic LDS is
// ldsd_terrain_bytes): the ground entries are planes and the heightfield, the animat may carry cylinders, and a contact has its own normal.
// With F64_STEP_ELLIPTIC 1 on top of both it is fmj_step_f64_elliptic_kernel<LIMITS> (the terrain kernels' arguments and LDS): a contact
// is three rows under the elliptic cone (fmj_f64_elliptic.inc); every `#if F64_STEP_ELLIPTIC` keeps the pyramid's statements in its #else.
// With F64_STEP_MESH 1 on top of the terrain or the elliptic text it is fmj_step_f64_mesh_kernel<LIMITS> / fmj_step_f64_mesh_elliptic_kernel
// <LIMITS> (a seventh argument, F64Mesh): the narrow phase takes convex mesh geoms (fmj_f64_mesh.inc); every `#if F64_STEP_MESH` keeps
// the terrain kernels' statements in its #else.
// With F64_STEP_RK4 1 on top of the terrain or the elliptic text it is fmj_step_f64_terrain_rk4_kernel<LIMITS> / fmj_step_f64_elliptic_rk4_kernel
// <LIMITS> (dynamic LDS is ldsd_terrain_bytes + F64_RK4_LDS_DOUBLES(nu)): every pass runs the narrow phase and the solve; the contact
// list is stored with the fourth pass's commit (fmj_f64_contact_store.inc).
#if F64_STEP_MESH
template <bool LIMITS>
__global__ void __launch_bounds__(FMJ_F64_LANES) F64_STEP_KERNEL(const F64Model FM, const StepArgs A, const F64Fused U, const F64Limits LM, const F64Contacts CM,
                                                                 const F64Terrain TM, const F64Mesh MM) {
  constexpr bool FUSED = false;
#elif F64_STEP_TERRAIN
template <bool LIMITS>
__global__ void __launch_bounds__(FMJ_F64_LANES) F64_STEP_KERNEL(const F64Model FM, const StepArgs A, const F64Fused U, const F64Limits LM, const F64Contacts CM,
                                                                 const F64Terrain TM) {
  constexpr bool FUSED = false;
#elif F64_STEP_CONTACTS
template <bool LIMITS>
__global__ void __launch_bounds__(FMJ_F64_LANES) F64_STEP_KERNEL(const F64Model FM, const StepArgs A, const F64Fused U, const F64Limits LM, const F64Contacts CM) {
  constexpr bool FUSED = false;
#else
template <bool FUSED, bool LIMITS>
__global__ void __launch_bounds__(FMJ_F64_LANES) F64_STEP_KERNEL(const F64Model FM, const StepArgs A, const F64Fused U, const F64Limits LM) {
#endif
  constexpr bool RK4 = F64_STEP_RK4 != 0;
  constexpr bool CONTACTS = F64_STEP_CONTACTS != 0;
  constexpr bool CONS = LIMITS || CONTACTS;      // the step has a Newton solve
  extern __shared__ __align__(16) double ldsd[];
  const int env = blockIdx.x;
  const int lane = threadIdx.x;
  const int wv = lane >> 6;
  const int nb = FM.nbody, nv = FM.nv, nq = FM.nq, nu = FM.nu, rs = FM.rs;
  const LdsLayoutD L = ldsd_layout(nb, nv, nq, rs);
  double* QP = ldsd + L.QP; double* QV = ldsd + L.QV; double* XA = ldsd + L.XA; double* XCH = ldsd + L.XCH;
  double* CD = ldsd + L.CD; double* CI = ldsd + L.CI; double* CR = ldsd + L.CR; double* CF = ldsd + L.CF; double* CS = ldsd + L.CS;
  double* MX = ldsd + L.MX; double* HR = ldsd + L.HR; double* XW = ldsd + L.XW;
  int* FLG = (int*)(ldsd + L.FLG);
  double* SUM = ldsd + L.total_bytes / 8; int* FLX = (int*)(SUM + 16);      // LIMITS only: past the map (ldsd_total_bytes)
#if F64_STEP_CONTACTS && F64_STEP_RK4
  double* RKS = ldsd + ldsd_terrain_bytes(nb, nv, nq, rs, CM.max_contacts) / 8;      // RK4 with contacts (terrain text): past the records and the normals
#else
  double* RKS = ldsd + ldsd_total_bytes(nb, nv, nq, rs, LIMITS) / 8;      // RK4 only: past the map and the LIMITS block (F64_RK4_LDS_DOUBLES)
#endif
#if F64_STEP_CONTACTS
  double* CT = ldsd + ldsd_total_bytes(nb, nv, nq, rs, 1) / 8;            // the contact records (F64_CT doubles each), past the LIMITS block
#endif
#if F64_STEP_TERRAIN
  double* CN = CT + CM.max_contacts * F64_CT;                             // the contacts' normals (F64_TN doubles each), past the records
#endif
  int sumpar = 0;
#define WG_SUM4(a_, b_, c_, d_) do { wg_sum4(a_, b_, c_, d_, SUM + sumpar * 8); sumpar ^= 1; } while (0)

  const bool isb = lane > 0 && lane < nb;
  const int bl = isb ? lane : 0;
  const bool isd = lane < nv;
  const int dl = isd ? lane : 0;
  // ---- the lane's model constants: body (joint) and dof
  const double* bdp = FM.bd + (size_t)bl * F64_BD;
  const int* bip = FM.bi + (size_t)bl * F64_BI;
  const int parent = bip[0], jtype = isb ? bip[1] : -1, qadr = bip[2], dadr = bip[3];
  const int lastb = isb ? lane + bip[4] - 1 : lane;
  const int* dip = FM.di + (size_t)dl * F64_DI;
  const int d_body = dip[0], ddepth = isd ? dip[1] : 0, d_qadr = dip[2], act0 = dip[3], nact = isd ? dip[4] : 0, d_slot = dip[5];
  const bool d_scalar = isd && d_qadr >= 0;
  const double d_arm = FM.dd[2 * dl], d_damp = FM.dd[2 * dl + 1];
  const double h = FM.h;
  const double* lmp = LIMITS ? LM.lm + (size_t)dl * F64_LM : nullptr;
  const bool lim_on = LIMITS && d_scalar && lmp[0] != 0.0;
#if F64_STEP_CONTACTS
  // lane = geom: its tables; lane = dof: the depth-first range of its body (the contacts of that subtree act on the dof)
  const bool isg = lane < CM.ngeom;
  const int gl = isg ? lane : 0;
  const double* gdp = CM.gd + (size_t)gl * F64_GD;
  const int g_type = isg ? CM.gi[gl * F64_GI] : -1, g_body = CM.gi[gl * F64_GI + 1];
  const int d_b0 = isd ? d_body : 1, d_b1 = isd ? d_body + FM.bi[(size_t)d_body * F64_BI + 4] - 1 : 0;
#endif
#if F64_STEP_MESH
  const int g_v0 = MM.gv[2 * gl], g_nvert = isg ? MM.gv[2 * gl + 1] : 0;      // lane = geom: its vertices (none: no mesh)
#endif

  // ---- load the state: widened once
  int warn = 0;
  {
    const float* gq = A.qpos + (size_t)env * nq;
    const float* gv = A.qvel + (size_t)env * nv;
    for (int i = lane; i < nq; i += FMJ_F64_LANES) { const float v = gq[i]; QP[i] = (double)v; if (!(fabsf(v) <= 1e10f)) warn |= FMJ_WARN_BADQPOS; }   // mj_checkPos
    for (int i = lane; i < nv; i += FMJ_F64_LANES) { const float v = gv[i]; QV[i] = (double)v; XA[i] = 0.0; if (!(fabsf(v) <= 1e10f)) warn |= FMJ_WARN_BADQVEL; }   // mj_checkVel
  }
  double xf0 = 0.0, xf1 = 0.0, xf2 = 0.0, xf3 = 0.0, xf4 = 0.0, xf5 = 0.0;     // world-frame external force / torque on this body
  if (!(FUSED && A.do_drag) && A.xfrc_applied && isb) {      // (the fused drag writes the wrench itself)
    const float* x = A.xfrc_applied + (size_t)env * nb * 6 + bl * 6;
    xf0 = x[0]; xf1 = x[1]; xf2 = x[2]; xf3 = x[3]; xf4 = x[4]; xf5 = x[5];
  }
  // fused: what the previous launch left for this one - the motor torque of the joints row (physics.py:510-524)
  double cy_actsum = 0.0;
  const int link_row = FUSED ? bip[5] : -1, swim_slot = FUSED ? bip[6] : -1, joint_row = FUSED ? dip[6] : -1;
  if (FUSED && d_scalar) {
    const float* sa = A.sensordata + (size_t)env * FM.nsensordata + 6 * (nb - 1) + 3 * FM.njs;
    for (int a = 0; a < nact; a++) cy_actsum += (double)sa[FM.asrc[act0 + a]] * U.inv_torques;
  }
  double cy_limfrc = 0.0;      // fused: the carried joint-limit force of the joints row (physics.py:484-487)
  if (FUSED && LIMITS && lim_on) cy_limfrc = (double)A.sensordata[(size_t)env * FM.nsensordata + 6 * (nb - 1) + 3 * d_slot + 2] * U.inv_torques;
  double ws_qacc = 0.0;        // limits: the constrained qacc of the launch's last step (the next warm start, as mj_step saves it)
  // frozen (include/fmj.h): decided for the whole workgroup
  bool frozen = (A.status[env] & FMJ_WARN_FREEZE) != 0;
  frozen = wg_or(warn & FMJ_WARN_FREEZE, FLG + 0) != 0 || frozen;
  int steps_done = 0;
  if (FUSED && !frozen && A.n_steps > 0) {      // the links row and the drag of iteration0, from the poses and sensors fmj_data holds
    const int cl = lane < nb ? lane : 0;
    const float* p = A.xpos + (size_t)env * nb * 3 + cl * 3;
    const float* q = A.xquat + (size_t)env * nb * 4 + cl * 4;
    const float* ip = A.xipos + (size_t)env * nb * 3 + cl * 3;
    const float* sd = A.sensordata + (size_t)env * FM.nsensordata + 6 * (isb ? lane - 1 : 0);
    const dq cq = {(double)q[0], (double)q[1], (double)q[2], (double)q[3]};
    f64_emit_links_and_drag(U, A, env, A.iteration0, isb, link_row, swim_slot, dmk(p[0], p[1], p[2]), cq, dmk(ip[0], ip[1], ip[2]),
                            dmk(sd[0], sd[1], sd[2]), dmk(sd[3], sd[4], sd[5]), xf0, xf1, xf2, xf3, xf4, xf5);
  }
  __syncthreads();

  int sub = 0, itm = 0;      // fused: the sub-step inside the iteration, iterations completed in this launch
#pragma unroll 1
  for (int step = 0; step < A.n_steps; step++) {
    if (frozen) break;                          // uniform: every freeze decision is a workgroup OR
    const bool last = step == A.n_steps - 1;
    // fused: the counters of fmj_stage_step_head.inc: n_steps = iterations x substeps physics steps
    const int it = A.iteration0 + itm;
    const int S_sub = FUSED ? A.substeps : 1;
    const bool full = sub == 0;
    const int nsub = sub + 1 >= S_sub ? 0 : sub + 1;           // the next physics step: its sub index, whether it is a full step,
    const bool nfull = nsub == 0;                               // and task.iteration as its before_step will see it: the reference
    const int nit = (nfull ? it + 1 : it) + ((nsub >= 1 && nsub >= S_sub - 1) ? 1 : 0);   // advances it after sub-step S - 2 (task.py:352-355)
    // ---- before_step of a full step: the joints row (physics.py:500-524)
    if (FUSED && A.do_readout && full && d_scalar && joint_row >= 0) {
      float* row = A.joints + ((size_t)(it % A.buffer_size) * A.row_stride_joints + (size_t)env * U.n_joints * FMJ_JOINT_SIZE) + joint_row * FMJ_JOINT_SIZE;
      row[0] = (float)QP[d_qadr]; row[1] = (float)(QV[lane] * U.inv_angvel);
      row[2] = row[3] = row[4] = row[5] = row[6] = row[7] = 0.f;
      row[8] = (float)cy_actsum; row[9] = LIMITS ? (float)cy_limfrc : 0.f; row[10] = row[11] = 0.f;
    }
    // ---- RK4 (oracle rk4, the classical tableau): X[0] of the step and the sums of B F, one value per lane = dof, and what the step
    // leaves from its first pass (the joint's limit force, the link velocities), in the lane's column of RKL (F64_RK4_*: each lane reads
    // back only what it wrote, so no barrier orders them); the root's seven position values in the root body's lane's row.  They live
    // in LDS, not in registers, to keep the kernel's two waves at two workgroups per SIMD pair where the model's LDS allows it
    double* rk = RKS + 2 * nu + lane;
    double* rk_root = RKS + 2 * nu + F64_RK4_ROOT * FMJ_F64_LANES;
    int pass = 0;
    if (RK4) {
      rk[F64_RK4_Q0 * FMJ_F64_LANES] = d_scalar ? QP[d_qadr] : (FM.root_free && lane < 3) ? QP[lane] : 0.0;      // (a free root's three positions: for the checks)
      rk[F64_RK4_V0 * FMJ_F64_LANES] = isd ? QV[lane] : 0.0;
      rk[F64_RK4_SV * FMJ_F64_LANES] = 0.0; rk[F64_RK4_SA * FMJ_F64_LANES] = 0.0;
      if (jtype == FMJ_JNT_FREE) for (int k = 0; k < 7; k++) rk_root[k] = QP[qadr + k];
    }
#pragma unroll 1
    for (;;) {      // RK4: the forward pass at X[pass]; otherwise one pass (the stages below keep the indentation they had before this loop)
    // ---- K: local transforms, composed along the chains by pointer jumping through LDS (buffer r & 1)
    const d3 axis = dmk(bdp[20], bdp[21], bdp[22]);
    const d3 jpos = dmk(bdp[24], bdp[25], bdp[26]);
    d3 xp = dmk(bdp[0], bdp[1], bdp[2]);
    dq xq = {bdp[4], bdp[5], bdp[6], bdp[7]};
    if (jtype == FMJ_JNT_FREE) {
      xp = dmk(QP[qadr], QP[qadr + 1], QP[qadr + 2]);
      dq rq = {QP[qadr + 3], QP[qadr + 4], QP[qadr + 5], QP[qadr + 6]};
      xq = dqnormalize(rq);
    } else if (jtype == FMJ_JNT_HINGE) {
      const dq ql = daxisangle(axis, QP[qadr] - bdp[23]);
      xp = dadd(xp, dqrot(xq, dsub(jpos, dqrot(ql, jpos))));      // anchor - R(new) jnt_pos, in the parent's frame
      xq = dqmul(xq, ql);
    } else if (jtype == FMJ_JNT_SLIDE) {
      xp = dadd(xp, dqrot(xq, dscl(axis, QP[qadr] - bdp[23])));
    }
    if (!isb) { xp = dmk(0.0, 0.0, 0.0); xq.w = 1.0; xq.x = xq.y = xq.z = 0.0; }
    for (int r = 0; r < FM.jump_rounds; r++) {
      double* X = XCH + (r & 1) * (FMJ_F64_LANES * 8);
      X[lane * 8 + 0] = xp.x; X[lane * 8 + 1] = xp.y; X[lane * 8 + 2] = xp.z;
      X[lane * 8 + 4] = xq.w; X[lane * 8 + 5] = xq.x; X[lane * 8 + 6] = xq.y; X[lane * 8 + 7] = xq.z;
      __syncthreads();
      const int a = isb ? (int)FM.b_anc[lane * FM.anc_stride + r] : 0;
      const dq aq = {X[a * 8 + 4], X[a * 8 + 5], X[a * 8 + 6], X[a * 8 + 7]};
      xp = dadd(dmk(X[a * 8], X[a * 8 + 1], X[a * 8 + 2]), dqrot(aq, xp));
      xq = dqmul(aq, xq);
    }
    xq = dqnormalize(xq);
    const dm33 xmat = dq2m(xq);
    const d3 xi = dadd(xp, dmrot(xmat, dmk(bdp[8], bdp[9], bdp[10])));
    const double mass = isb ? bdp[3] : 0.0;
    // ---- C: the tree's centre of mass
    if (lane < nb) { MX[lane * 4] = mass * xi.x; MX[lane * 4 + 1] = mass * xi.y; MX[lane * 4 + 2] = mass * xi.z; }
    __syncthreads();                                                   // (also closes K's last reads of XCH)
    d3 com = dmk(0.0, 0.0, 0.0);
    for (int b = nb - 1; b >= 1; b--) com = dadd(com, dmk(MX[b * 4], MX[b * 4 + 1], MX[b * 4 + 2]));
    com = dmk(com.x / FM.mtot, com.y / FM.mtot, com.z / FM.mtot);
    // ---- cinert about the centre of mass (mj_comPos)
    di10 ci;
    {
      const dq iq = {bdp[12], bdp[13], bdp[14], bdp[15]};
      const dm33 R = dq2m(dqmul(xq, iq));
      const double n0 = bdp[16], n1 = bdp[17], n2 = bdp[18];
      const d3 dif = dsub(xi, com);
      ci.i0 = R.a0 * R.a0 * n0 + R.a1 * R.a1 * n1 + R.a2 * R.a2 * n2;
      ci.i1 = R.a3 * R.a3 * n0 + R.a4 * R.a4 * n1 + R.a5 * R.a5 * n2;
      ci.i2 = R.a6 * R.a6 * n0 + R.a7 * R.a7 * n1 + R.a8 * R.a8 * n2;
      ci.i3 = R.a0 * R.a3 * n0 + R.a1 * R.a4 * n1 + R.a2 * R.a5 * n2;
      ci.i4 = R.a0 * R.a6 * n0 + R.a1 * R.a7 * n1 + R.a2 * R.a8 * n2;
      ci.i5 = R.a3 * R.a6 * n0 + R.a4 * R.a7 * n1 + R.a5 * R.a8 * n2;
      ci.i0 += mass * (dif.y * dif.y + dif.z * dif.z);
      ci.i1 += mass * (dif.x * dif.x + dif.z * dif.z);
      ci.i2 += mass * (dif.x * dif.x + dif.y * dif.y);
      ci.i3 -= mass * dif.x * dif.y; ci.i4 -= mass * dif.x * dif.z; ci.i5 -= mass * dif.y * dif.z;
      ci.i6 = mass * dif.x; ci.i7 = mass * dif.y; ci.i8 = mass * dif.z; ci.i9 = mass;
      if (!isb) { di10 z = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0}; ci = z; }
      if (lane < nb) dput10(CI + lane * 10, ci);
    }
    // ---- V: cdof, vJ, cvel = chain sum of vJ, cacc = -g + chain sum of cdof_dot qvel (exchanges alternate between the two buffers)
    d6 cv, ca;
    {
      const d3 z3 = dmk(0.0, 0.0, 0.0);
      d6 vJ = {z3, z3}, vt = {z3, z3};
      if (jtype == FMJ_JNT_HINGE || jtype == FMJ_JNT_SLIDE) {
        const d3 axw = dmrot(xmat, axis);
        d6 cd;
        if (jtype == FMJ_JNT_HINGE) { const d3 anchor = dadd(xp, dmrot(xmat, jpos)); cd.r = axw; cd.l = dcross(axw, dsub(com, anchor)); }
        else { cd.r = z3; cd.l = axw; }
        dput6(CD + dadr * 6, cd);
        vJ = d6scl(cd, QV[dadr]);
      } else if (jtype == FMJ_JNT_FREE) {
        const d3 off = dsub(com, xp);
        vt.l = dmk(QV[dadr], QV[dadr + 1], QV[dadr + 2]);
        const d6 t0 = {z3, dmk(1.0, 0.0, 0.0)}, t1 = {z3, dmk(0.0, 1.0, 0.0)}, t2 = {z3, dmk(0.0, 0.0, 1.0)};
        dput6(CD + dadr * 6, t0); dput6(CD + (dadr + 1) * 6, t1); dput6(CD + (dadr + 2) * 6, t2);
        const d3 c0 = dmk(xmat.a0, xmat.a3, xmat.a6), c1 = dmk(xmat.a1, xmat.a4, xmat.a7), c2 = dmk(xmat.a2, xmat.a5, xmat.a8);
        const d6 r0 = {c0, dcross(c0, off)}, r1 = {c1, dcross(c1, off)}, r2 = {c2, dcross(c2, off)};
        dput6(CD + (dadr + 3) * 6, r0); dput6(CD + (dadr + 4) * 6, r1); dput6(CD + (dadr + 5) * 6, r2);
        vJ = d6add(d6add(d6scl(r0, QV[dadr + 3]), d6scl(r1, QV[dadr + 4])), d6scl(r2, QV[dadr + 5]));
      }
      int xb = 0;
#define XPULL6D(dst_, src_, v_) do { \
        double* X_ = XCH + xb * (FMJ_F64_LANES * 8); \
        dput6(X_ + lane * 8, v_); \
        __syncthreads(); \
        dst_ = dget6(X_ + (src_) * 8); \
        xb ^= 1; } while (0)
      cv = d6add(vt, vJ);
      for (int r = 0; r < FM.jump_rounds; r++) {
        d6 o; XPULL6D(o, isb ? (int)FM.b_anc[lane * FM.anc_stride + r] : 0, cv);
        cv = d6add(cv, o);
      }
      d6 cpar; XPULL6D(cpar, isb ? parent : 0, cv);
      cpar = d6add(cpar, vt);
      ca = dcross_motion(cpar, vJ);
      if (!isb) { ca.r = ca.l = z3; }
      for (int r = 0; r < FM.jump_rounds; r++) {
        d6 o; XPULL6D(o, isb ? (int)FM.b_anc[lane * FM.anc_stride + r] : 0, ca);
        ca = d6add(ca, o);
      }
#undef XPULL6D
      ca.l = dsub(ca.l, dmk(FM.gx, FM.gy, FM.gz));
      if (!isb) { cv.r = cv.l = z3; }
    }
    // ---- F: body force cinert cacc + cvel x* (cinert cvel) (mj_rne), minus the external wrench about the centre of mass
    {
      d6 f = d6add(dinert_mul(ci, ca), dcross_force(cv, dinert_mul(ci, cv)));
      const d3 fw = dmk(xf0, xf1, xf2), tw = dmk(xf3, xf4, xf5);
      f.r = dsub(f.r, dadd(tw, dcross(dsub(xi, com), fw)));
      f.l = dsub(f.l, fw);
      if (lane < nb) { if (!isb) { f.r = f.l = dmk(0.0, 0.0, 0.0); } dput6(CF + lane * 6, f); }
    }
    // ---- fused: the next before_step's links row and drag from this forward pass (this step's F consumed the wrench above); a
    // sub-step that writes no row (substep_links off, or task.iteration at the run's n_iterations) keeps the drag force it has
#define F64_EMIT_NEXT (FUSED && !last && (nfull || (A.sub_links && !(A.n_it_total > 0 && nit >= A.n_it_total))))
    if (!RK4 && F64_EMIT_NEXT) {
      const d3 linvel = dsub(cv.l, dcross(dsub(xi, com), cv.r));
      f64_emit_links_and_drag(U, A, env, nit, isb, link_row, swim_slot, xp, xq, xi, linvel, cv.r, xf0, xf1, xf2, xf3, xf4, xf5);
    }
    // RK4: the link velocities a step leaves are its first pass's (mj_forwardSkip skips the sensors of the later passes); they are stored,
    // and the next before_step's row is emitted, with the fourth pass's poses once that pass has passed its checks
    if (RK4 && pass == 0) {
      const d3 linvel = dsub(cv.l, dcross(dsub(xi, com), cv.r));
      rk[F64_RK4_LIN * FMJ_F64_LANES] = linvel.x; rk[(F64_RK4_LIN + 1) * FMJ_F64_LANES] = linvel.y; rk[(F64_RK4_LIN + 2) * FMJ_F64_LANES] = linvel.z;
      rk[F64_RK4_ANG * FMJ_F64_LANES] = cv.r.x; rk[(F64_RK4_ANG + 1) * FMJ_F64_LANES] = cv.r.y; rk[(F64_RK4_ANG + 2) * FMJ_F64_LANES] = cv.r.z;
    }
    // ---- sensors and poses of this (pre-integration) state
    if (!RK4 && last && lane < nb) {
      float* p = A.xpos + (size_t)env * nb * 3 + lane * 3; p[0] = (float)xp.x; p[1] = (float)xp.y; p[2] = (float)xp.z;
      float* q = A.xquat + (size_t)env * nb * 4 + lane * 4; q[0] = (float)xq.w; q[1] = (float)xq.x; q[2] = (float)xq.y; q[3] = (float)xq.z;
      float* ip = A.xipos + (size_t)env * nb * 3 + lane * 3; ip[0] = (float)xi.x; ip[1] = (float)xi.y; ip[2] = (float)xi.z;
      if (isb) {
        const d3 linvel = dsub(cv.l, dcross(dsub(xi, com), cv.r));
        float* sp = A.sensordata + (size_t)env * FM.nsensordata + 6 * (lane - 1);
        sp[0] = (float)linvel.x; sp[1] = (float)linvel.y; sp[2] = (float)linvel.z;
        sp[3] = (float)cv.r.x; sp[4] = (float)cv.r.y; sp[5] = (float)cv.r.z;
      }
    }
    __syncthreads();
#if F64_STEP_CONTACTS
    // ---- contacts: the narrow phase (lane = geom) into the oracle's order (ground geom, animat geom, slot), then the four rows of
    // each contact (lane = contact).  XCH is free between the V stage and the next pass's K: buffer 0 holds the poses, buffer 1 the list
    int ncon = 0;
    bool is_c = false;
    d3 c_pos = dmk(0.0, 0.0, 0.0);
    int c_geom = 0, c_plane = 0, c_ld = 0, c_dep = 0;
#if F64_STEP_ELLIPTIC
    // three rows per contact: normal, tangent 1, tangent 2.  c_mu: the friction of the tangents (fr), c_mi: fr / sqrt(impratio) (mu),
    // c_D: 1 / R of the normal row, c_zone: the cone zone at the iterate
    double c_mu = 0.0, c_mi = 0.0, c_D = 0.0, c_ar0 = 0.0, c_ar1 = 0.0, c_ar2 = 0.0;
    double c_ja0 = 0.0, c_ja1 = 0.0, c_ja2 = 0.0, c_jp0 = 0.0, c_jp1 = 0.0, c_jp2 = 0.0;      // J a - aref, J p
    double c_f0 = 0.0, c_f1 = 0.0, c_f2 = 0.0;
    int c_zone = 0;
#else
    double c_mu = 0.0, c_D = 0.0, c_ar0 = 0.0, c_ar1 = 0.0, c_ar2 = 0.0, c_ar3 = 0.0;
    double c_ja0 = 0.0, c_ja1 = 0.0, c_ja2 = 0.0, c_ja3 = 0.0, c_jp0 = 0.0, c_jp1 = 0.0, c_jp2 = 0.0, c_jp3 = 0.0;      // J a - aref, J p
    double c_f0 = 0.0, c_f1 = 0.0, c_f2 = 0.0, c_f3 = 0.0;
    bool c_a0 = false, c_a1 = false, c_a2 = false, c_a3 = false;
#endif
    d6 cbuf = {dmk(0.0, 0.0, 0.0), dmk(0.0, 0.0, 0.0)};      // lane = dof: the contact stiffness of its row
    {
      double* XP = XCH; double* XL = XCH + FMJ_F64_LANES * 8;
      if (lane < nb) {
        XP[lane * 8 + 0] = xp.x; XP[lane * 8 + 1] = xp.y; XP[lane * 8 + 2] = xp.z;
        XP[lane * 8 + 4] = xq.w; XP[lane * 8 + 5] = xq.x; XP[lane * 8 + 6] = xq.y; XP[lane * 8 + 7] = xq.z;
      }
      __syncthreads();
#if F64_STEP_MESH
      const bool animat = g_type == FMJ_GEOM_SPHERE || g_type == FMJ_GEOM_CAPSULE || g_type == FMJ_GEOM_BOX || g_type == FMJ_GEOM_CYLINDER || g_type == FMJ_GEOM_MESH;
#elif F64_STEP_TERRAIN
      const bool animat = g_type == FMJ_GEOM_SPHERE || g_type == FMJ_GEOM_CAPSULE || g_type == FMJ_GEOM_BOX || g_type == FMJ_GEOM_CYLINDER;
#else
      const bool animat = g_type == FMJ_GEOM_SPHERE || g_type == FMJ_GEOM_CAPSULE || g_type == FMJ_GEOM_BOX;
#endif
      const d3 gbp = dmk(XP[g_body * 8], XP[g_body * 8 + 1], XP[g_body * 8 + 2]);
      const dq gbq = {XP[g_body * 8 + 4], XP[g_body * 8 + 5], XP[g_body * 8 + 6], XP[g_body * 8 + 7]};
      int ntot = 0;
#pragma unroll 1
      for (int p = 0; p < CM.nplane; p++) {
#if F64_STEP_MESH
        const double* tgp = TM.tg + (size_t)p * F64_TG;
        const int cnt = animat ? f64_mesh_contacts(gdp, g_type, gbp, gbq, tgp, TM.hf, MM.mv, g_v0, g_nvert, lane, p, 0, 0, nullptr) : 0;
        int tot;
        const int base = ntot + wg_scan_excl(cnt, FLX + 4, tot);
        if (cnt > 0 && base < CM.max_contacts) f64_mesh_contacts(gdp, g_type, gbp, gbq, tgp, TM.hf, MM.mv, g_v0, g_nvert, lane, p, base, CM.max_contacts, XL);
#elif F64_STEP_TERRAIN
        const double* tgp = TM.tg + (size_t)p * F64_TG;
        const int cnt = animat ? f64_terrain_contacts(gdp, g_type, gbp, gbq, tgp, TM.hf, lane, p, 0, 0, nullptr) : 0;
        int tot;
        const int base = ntot + wg_scan_excl(cnt, FLX + 4, tot);
        if (cnt > 0 && base < CM.max_contacts) f64_terrain_contacts(gdp, g_type, gbp, gbq, tgp, TM.hf, lane, p, base, CM.max_contacts, XL);
#else
        const double* pdp = CM.pd + (size_t)p * F64_PD;
        const int cnt = animat ? f64_ground_contacts(gdp, g_type, gbp, gbq, pdp, lane, p, 0, 0, nullptr) : 0;
        int tot;
        const int base = ntot + wg_scan_excl(cnt, FLX + 4, tot);
        if (cnt > 0 && base < CM.max_contacts) f64_ground_contacts(gdp, g_type, gbp, gbq, pdp, lane, p, base, CM.max_contacts, XL);
#endif
        ntot += tot;
        __syncthreads();
      }
      ncon = ntot;
      if (ncon > CM.max_contacts) { ncon = CM.max_contacts; warn |= FMJ_WARN_CONTACTFULL; }
      is_c = lane < ncon;
      if (is_c) {
        const double* rec = XL + lane * 8;
        c_pos = dmk(rec[0], rec[1], rec[2]);
        const double dist = rec[3];
#if F64_STEP_TERRAIN
        { const int gp = (int)rec[7]; c_geom = gp >> 7; c_plane = gp & 127; }
        const double* cg = CM.gd + (size_t)c_geom * F64_GD;
        const double* cp = TM.tg + (size_t)c_plane * F64_TG;      // (friction and geom index where a plane's F64_PD row has them)
#else
        c_geom = (int)rec[4]; c_plane = (int)rec[5];
        const double* cg = CM.gd + (size_t)c_geom * F64_GD;
        const double* cp = CM.pd + (size_t)c_plane * F64_PD;
#endif
        const int cb = CM.gi[c_geom * F64_GI + 1];
        c_ld = CM.gi[c_geom * F64_GI + 2];
        c_dep = FM.di[(size_t)c_ld * F64_DI + 1];
        c_mu = fmax(fmax(cp[12], cg[10]), 1e-5);      // max over the two geoms (mj_contactParam), floor mjMINMU
#if F64_STEP_TERRAIN
        const d3 n = dmk(rec[4], rec[5], rec[6]);     // the contact's own normal; the frame by add_contact's rule (a plane's: its constants)
        d3 t1 = dmk(cp[15], cp[16], cp[17]), t2 = dmk(cp[18], cp[19], cp[20]);
        if (cp[14] != 0.0) f64_contact_frame(n, t1, t2);
        CN[lane * F64_TN] = n.x; CN[lane * F64_TN + 1] = n.y; CN[lane * F64_TN + 2] = n.z;      // (read back by this lane alone)
#else
        const d3 n = dmk(cp[0], cp[1], cp[2]), t1 = dmk(cp[6], cp[7], cp[8]), t2 = dmk(cp[9], cp[10], cp[11]);
#endif
        const d3 off = dsub(c_pos, com);
        const d6 V = f64_chain_sum(CD, QV, FM.danc, rs, c_ld, c_dep);
#if F64_STEP_ELLIPTIC
        // oracle make_constraints, elliptic branch: one row per axis of the contact frame, unscaled by the friction; diagApprox is the
        // bodies' invweight0 alone; only the normal row has a position (the tangents' aref has K = 0); the tangents' regulariser
        // R_t = R_n mu^2 / fr^2 with mu = fr / sqrt(impratio) enters the solve as D0 fr^2 / mu^2 (f64_cone_zone)
        const double diag = cg[11];
        double* ct = CT + lane * F64_CT;
        double imp, K, B;
        f64_row_impedance(cg + 12, h, dist, imp, K, B);      // (margin 0)
        const double R = fmax(F64_MINVAL, (1.0 - imp) * diag / imp);
#define F64_CONTACT_ROW(r_, u_, ar_, pos_) do { \
          const d6 W_ = {dcross(off, u_), u_}; \
          dput6(ct + 6 * (r_), W_); \
          ar_ = -B * d6dot(W_, V) - (pos_); } while (0)
        F64_CONTACT_ROW(0, n, c_ar0, K * imp * dist); F64_CONTACT_ROW(1, t1, c_ar1, 0.0); F64_CONTACT_ROW(2, t2, c_ar2, 0.0);
#undef F64_CONTACT_ROW
        c_mi = c_mu * (1.0 / CM.sqrt_impratio);
        c_D = 1.0 / R;
        ct[32] = (double)cb;
#else
        const double diag = cg[11] + c_mu * c_mu * cg[11];
        double* ct = CT + lane * F64_CT;
        double imp, K, B;
        f64_row_impedance(cg + 12, h, dist, imp, K, B);      // (margin 0)
        const double R = fmax(F64_MINVAL, (1.0 - imp) * diag / imp);
#define F64_CONTACT_ROW(r_, t_, sgn_, ar_) do { \
          const d3 u_ = dadd(n, dscl(t_, (sgn_) * c_mu)); \
          const d6 W_ = {dcross(off, u_), u_}; \
          dput6(ct + 6 * (r_), W_); \
          ar_ = -B * d6dot(W_, V) - K * imp * dist; } while (0)
        F64_CONTACT_ROW(0, t1, 1.0, c_ar0); F64_CONTACT_ROW(1, t1, -1.0, c_ar1); F64_CONTACT_ROW(2, t2, 1.0, c_ar2); F64_CONTACT_ROW(3, t2, -1.0, c_ar3);
#undef F64_CONTACT_ROW
        const double mi = c_mu / CM.sqrt_impratio;      // all rows of a contact share R = 2 mu^2 R_first, mu scaled by 1 / sqrt(impratio)
        c_D = 1.0 / fmax(F64_MINVAL, 2.0 * mi * mi * R);
        ct[32] = (double)cb;
#endif
      }
    }
#endif
    // ---- S: composite inertia and subtree force: the rows of the lane's own depth-first range, last body first
    if (isb) {
      di10 s = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
      d6 fs = {dmk(0.0, 0.0, 0.0), dmk(0.0, 0.0, 0.0)};
      for (int b = lastb; b >= lane; b--) {
        const di10 c = dget10(CI + b * 10);
        s.i0 += c.i0; s.i1 += c.i1; s.i2 += c.i2; s.i3 += c.i3; s.i4 += c.i4; s.i5 += c.i5; s.i6 += c.i6; s.i7 += c.i7; s.i8 += c.i8; s.i9 += c.i9;
        fs = d6add(fs, dget6(CF + b * 6));
      }
      dput10(CR + lane * 10, s);
      dput6(CS + lane * 6, fs);
    }
    __syncthreads();
    // ---- Q: qfrc_smooth = passive - bias + actuation (+ J' xfrc, inside the subtree force) (lane = dof)
    double qfrc = 0.0, bdamp = d_damp;
    d6 cd = {dmk(0.0, 0.0, 0.0), dmk(0.0, 0.0, 0.0)};
    if (isd) {
      cd = dget6(CD + lane * 6);
      const double qd = QV[lane];
      double passive = -d_damp * qd;
      double asum = 0.0;
      if (d_scalar) {
        const double qj = QP[d_qadr];
        if (FM.any_stiffness) {
          const double kst = FM.bd[(size_t)d_body * F64_BD + 27];
          if (kst != 0.0) passive += -kst * (qj - (double)A.qpos_spring[(size_t)env * nq + d_qadr]);
        }
        // fused: the wave controller (task.py:288-346), amp sin(2 pi frac(f t) + env_phase - lag) with t = iteration x the timestep of an
        // iteration (task.py:290); every step of an iteration evaluates it at the iteration's own time, so a sub-step holds the full step's ctrl
        const bool wave = FUSED && A.controller == 1;
        double cbase = 0.0;
        const float* w_amp = A.w_amp; const float* w_lag = A.w_lag;
        if (wave) {
          w_amp += (size_t)env * A.w_amp_stride; w_lag += (size_t)env * A.w_lag_stride;      // the env's rows (stride 0: the shared row)
          const double wfreq = A.w_freq_env ? (double)A.w_freq_env[env] : (double)A.w_freq;
          double cyc = wfreq * ((double)it * (h * (double)S_sub));
          cyc -= floor(cyc);
          cbase = 6.283185307179586 * cyc + (double)A.w_env[env];
        }
        for (int a = 0; a < nact; a++) {              // mj_fwdActuation, joint transmission
          const double* ap = FM.ad + (size_t)(act0 + a) * F64_AD;
          const int src = FM.asrc[act0 + a];
          double c;
          if (wave) {
            const double amp = (double)w_amp[src];
            c = amp != 0.0 ? amp * sin(cbase - (double)w_lag[src]) : 0.0;
            if (RK4) { if (pass == 0) RKS[nu + src] = c; }      // (stored with the step's commit)
            else if (last && A.ctrl_out) A.ctrl_out[(size_t)env * nu + src] = (float)c;      // what task.py:288-346 leaves in physics.data.ctrl
          } else c = A.ctrl ? (double)A.ctrl[(size_t)(FUSED ? itm : step) * A.ctrl_step_stride + (size_t)env * nu + src] : 0.0;   // fused: one ctrl row per iteration
          c = fmin(fmax(c, ap[4]), ap[5]);
          double f = ap[0] * c + ap[1] + ap[2] * qj + ap[3] * qd;
          f = fmin(fmax(f, ap[6]), ap[7]);
          if (FM.implicitfast && !A.disable_actuation && f > ap[6] && f < ap[7]) bdamp += -ap[3];
          if (A.disable_actuation) f = 0.0;
          if (RK4) { if (pass == 0) RKS[src] = f; }      // (stored with the step's commit)
          else if (last) A.sensordata[(size_t)env * FM.nsensordata + 6 * (nb - 1) + 3 * FM.njs + src] = (float)f;   // actuatorfrc
          asum += f;
        }
        if (FUSED && (!RK4 || pass == 0)) cy_actsum = asum * U.inv_torques;
      }
      qfrc = passive - d6dot(cd, dget6(CS + d_body * 6)) + asum;
    }
    // ---- limits: the candidate rows of the lane's joint (oracle make_constraints): lo is side -1 (J = +1), hi is side +1 (J = -1)
    bool c_lo = false, c_hi = false;
    double D_lo = 0.0, D_hi = 0.0, ar_lo = 0.0, ar_hi = 0.0;
    int lflags = 0;      // workgroup: 1 = some row is a candidate, 2 = some dof is damped
    if (CONS) {
      if (lim_on) {
        const double qj = QP[d_qadr], qd = QV[lane];
        const double dist_lo = qj - lmp[1], dist_hi = lmp[2] - qj;
        c_lo = dist_lo < lmp[3]; c_hi = dist_hi < lmp[3];
        if (c_lo) f64_limit_row(lmp, h, dist_lo, qd, D_lo, ar_lo);
        if (c_hi) f64_limit_row(lmp, h, dist_hi, -qd, D_hi, ar_hi);
      }
#if F64_STEP_CONTACTS
      lflags = wg_or(((c_lo || c_hi || ncon > 0) ? 1 : 0) | ((isd && bdamp != 0.0) ? 2 : 0), FLX + 0);
#else
      lflags = wg_or(((c_lo || c_hi) ? 1 : 0) | ((isd && bdamp != 0.0) ? 2 : 0), FLX + 0);
#endif
    }
    // The solve below runs once in a step without candidate rows (phase 2: M + h B, qfrc_smooth).  With candidate rows it runs for
    // a_s (phase 0: M), once per Newton iteration (phase 1: M + D_S, the gradient), and once more for the damped step (phase 2).
    int phase = 2, nt_iter = 0;
    double hb = RK4 ? 0.0 : bdamp, dadd = 0.0, rhs = isd ? qfrc : 0.0;      // RK4: no implicit damping, H = M in every pass
    double nt_a = 0.0, nt_as = 0.0, nt_r = 0.0, nt_g = 0.0, nt_qfc = 0.0, lim_f = 0.0;      // a, a_s, M (a - a_s), gradient, J' f, the joint's limit force
    bool act_lo = false, act_hi = false;
    if (CONS && (lflags & 1) != 0) { phase = 0; hb = 0.0; }
    const d6 buf = dinert_mul(dget10(CR + d_body * 10), cd);
    double x;
#pragma unroll 1
    for (;;) {      // (the stages below keep the indentation they had before the loop was put around them)
    // ---- M: row i of H (mj_crb, then mj_Euler's M + h B), H[i][j] at column depth(j)
    {
      if (isd) {
        double* row = HR + lane * rs;
        const uint8_t* an = FM.danc + (size_t)lane * rs;
#if F64_STEP_CONTACTS
        const d6 bufm = phase == 1 ? d6add(buf, cbuf) : buf;      // the Newton matrix: the composite contact stiffness beside the composite inertia
#else
        const d6& bufm = buf;
#endif
        for (int d = 0; d < ddepth; d++) row[d] = d6dot(dget6(CD + (int)an[d] * 6), bufm);
        row[ddepth] = (d_arm + d6dot(cd, bufm)) + h * hb;
        if (CONS) row[ddepth] += dadd;
        if (A.dbg_H && (!CONS || phase != 1) && (!RK4 || pass == 0)) {
          for (int d = 0; d < rs; d++) A.dbg_H[((size_t)env * nv + lane) * rs + d] = d <= ddepth ? (float)row[d] : 0.f;
          A.dbg_qfrc[(size_t)env * nv + lane] = (float)qfrc;
        }
      }
    }
    // ---- L: L'DL by rounds; the right-hand side is swept leaves-first in the same rounds
    x = rhs;
    {
      typedef const WideRoundW __attribute__((address_space(4)))* wround_p;
      const wround_p RND = (wround_p)FM.rounds;
      int prev_depth = -1;
#pragma unroll 1
      for (int rd = 0; rd < FM.nround; rd++) {
        const int dep = RND[rd].depth, np = RND[rd].np;
        if (isd && ddepth == dep && dep != prev_depth) XW[lane] = x;      // final: every round below this depth is done
        prev_depth = dep;
        __syncthreads();
#pragma unroll 1
        for (int c = 0; c < np; c++) {
          const int p = RND[rd].p[c];
          const unsigned long long am = RND[rd].anc[c][0], am1 = RND[rd].anc[c][1];
          if ((((wv ? am1 : am) >> (lane & 63)) & 1ull) != 0) {
            const double* rp = HR + p * rs;
            const double t = rp[ddepth] / rp[dep];
            double* row = HR + lane * rs;
            for (int d = 0; d <= ddepth; d++) row[d] -= t * rp[d];
            x -= t * XW[p];
          }
        }
      }
      __syncthreads();
    }
    // ---- X: divide by D, then the root-first sweep, one tree level at a time
    const double Dm = isd ? HR[lane * rs + ddepth] : 1.0;
    x *= 1.0 / Dm;
#pragma unroll 1
    for (int lvl = 0; lvl < FM.maxdep; lvl++) {
      if (isd && ddepth == lvl) XW[lane] = x;
      __syncthreads();
      if (isd && ddepth > lvl) x -= (HR[lane * rs + lvl] / Dm) * XW[FM.danc[(size_t)lane * rs + lvl]];
    }
    if (!CONS || phase == 2) break;
    // ---- limits: the Newton iteration on the primal problem (oracle solve_primal, unilateral rows); every branch below is uniform
    bool stop;
#if F64_STEP_ELLIPTIC
    bool small_gain = false;
#endif
    if (phase == 0) {                       // x = a_s: the first iterate, where M (a - a_s) = 0
      nt_as = nt_a = x; nt_r = 0.0;
      phase = 1;
      stop = LM.solver_iterations <= 0;     // (the forces of a_s, as primal_update leaves them)
#if F64_STEP_CONTACTS
      __syncthreads();                      // (the sweep's last reads of XW)
      XW[lane] = x;
      __syncthreads();
      if (is_c) {                           // J a_s - aref
        const d6 S = f64_chain_sum(CD, XW, FM.danc, rs, c_ld, c_dep);
        const double* ct = CT + lane * F64_CT;
#if F64_STEP_ELLIPTIC
        c_ja0 = d6dot(dget6(ct), S) - c_ar0; c_ja1 = d6dot(dget6(ct + 6), S) - c_ar1; c_ja2 = d6dot(dget6(ct + 12), S) - c_ar2;
#else
        c_ja0 = d6dot(dget6(ct), S) - c_ar0; c_ja1 = d6dot(dget6(ct + 6), S) - c_ar1;
        c_ja2 = d6dot(dget6(ct + 12), S) - c_ar2; c_ja3 = d6dot(dget6(ct + 18), S) - c_ar3;
#endif
      }
#endif
    } else {                                // x = (M + D_S)^-1 g: the search direction p = -x and M p = -g - D_S p
#if F64_STEP_CONTACTS
      const double sp = -x;
      double cMp = 0.0;                     // (J' D_S J p)_i = cdof_i . sum over the active rows of the subtree of D_e (J p)_e W_e
      __syncthreads();                      // (the sweep's last reads of XW)
      XW[lane] = sp;
      __syncthreads();
      if (is_c) {
        const d6 S = f64_chain_sum(CD, XW, FM.danc, rs, c_ld, c_dep);
        double* ct = CT + lane * F64_CT;
#if F64_STEP_ELLIPTIC
        c_jp0 = d6dot(dget6(ct), S); c_jp1 = d6dot(dget6(ct + 6), S); c_jp2 = d6dot(dget6(ct + 12), S);
        // the row scalars of J' Hc J p: (Hc J p)_a, with the Hc of the iterate the matrix was built from (the record's)
        const double r0 = ct[18] * c_jp0 + ct[19] * c_jp1 + ct[20] * c_jp2, r1 = ct[19] * c_jp0 + ct[21] * c_jp1 + ct[22] * c_jp2;
        const double r2 = ct[20] * c_jp0 + ct[22] * c_jp1 + ct[23] * c_jp2;
        ct[24] = r0; ct[25] = r1; ct[26] = r2;
#else
        c_jp0 = d6dot(dget6(ct), S); c_jp1 = d6dot(dget6(ct + 6), S); c_jp2 = d6dot(dget6(ct + 12), S); c_jp3 = d6dot(dget6(ct + 18), S);
        ct[28] = c_a0 ? c_D * c_jp0 : 0.0; ct[29] = c_a1 ? c_D * c_jp1 : 0.0; ct[30] = c_a2 ? c_D * c_jp2 : 0.0; ct[31] = c_a3 ? c_D * c_jp3 : 0.0;
#endif
      }
      __syncthreads();
#if F64_STEP_ELLIPTIC
      if (isd) { d6 fs, unused; f64_elliptic_subtree(CT, ncon, d_b0, d_b1, cd, false, fs, unused); cMp = d6dot(cd, fs); }
#else
      if (isd) { d6 fs, unused; f64_contact_subtree(CT, ncon, d_b0, d_b1, cd, false, fs, unused); cMp = d6dot(cd, fs); }
#endif
      const double Mp = -nt_g - dadd * sp - cMp;
#else
      const double sp = -x, Mp = -nt_g - dadd * sp;
#endif
      double s0 = sp * sp, s1 = sp * Mp, s2 = sp * nt_r, s3 = nt_r * (nt_a - nt_as);
      WG_SUM4(s0, s1, s2, s3);
      const double snorm = sqrt(s0), qg0 = 0.5 * s3, qg1 = s2, qg2 = 0.5 * s1;
      const double gtol = LM.tolerance * LM.ls_tolerance * snorm / LM.scale;
      const double j_lo = nt_a - ar_lo, j_hi = -nt_a - ar_hi;      // jar of the lane's rows at alpha = 0; Jv = +p, -p
      const auto ls_eval = [&](double alpha) {
        double c = 0.0, e0 = 0.0, e1 = 0.0, unused = 0.0;
        const double x_lo = j_lo + alpha * sp, x_hi = j_hi - alpha * sp;
        if (c_lo && x_lo < 0.0) { c += 0.5 * D_lo * x_lo * x_lo; e0 += D_lo * x_lo * sp; e1 += D_lo * sp * sp; }
        if (c_hi && x_hi < 0.0) { c += 0.5 * D_hi * x_hi * x_hi; e0 -= D_hi * x_hi * sp; e1 += D_hi * sp * sp; }
#if F64_STEP_ELLIPTIC
        if (is_c) {      // oracle ls_eval, the elliptic block: the cone at jar + alpha J p
          double cc, g0, g1, g2, h00, h01, h02, h11, h12, h22;
          f64_cone_zone(c_ja0 + alpha * c_jp0, c_ja1 + alpha * c_jp1, c_ja2 + alpha * c_jp2, c_D, c_mi, c_mu, cc, g0, g1, g2, h00, h01, h02, h11, h12, h22);
          c += cc;
          e0 -= g0 * c_jp0; e0 -= g1 * c_jp1; e0 -= g2 * c_jp2;
          e1 += h00 * c_jp0 * c_jp0 + h11 * c_jp1 * c_jp1 + h22 * c_jp2 * c_jp2 + 2.0 * (h01 * c_jp0 * c_jp1 + h02 * c_jp0 * c_jp2 + h12 * c_jp1 * c_jp2);
        }
#elif F64_STEP_CONTACTS
        if (is_c) {
#define F64_LS_ROW(ja_, jp_) do { const double x_ = (ja_) + alpha * (jp_); \
            if (x_ < 0.0) { c += 0.5 * c_D * x_ * x_; e0 += c_D * x_ * (jp_); e1 += c_D * (jp_) * (jp_); } } while (0)
          F64_LS_ROW(c_ja0, c_jp0); F64_LS_ROW(c_ja1, c_jp1); F64_LS_ROW(c_ja2, c_jp2); F64_LS_ROW(c_ja3, c_jp3);
#undef F64_LS_ROW
        }
#endif
        WG_SUM4(c, e0, e1, unused);
        F64LsPt pt;
        pt.alpha = alpha; pt.cost = qg0 + alpha * (qg1 + alpha * qg2) + c; pt.d0 = qg1 + 2.0 * alpha * qg2 + e0;
        pt.d1 = 2.0 * qg2 + e1; if (!(pt.d1 > F64_MINVAL)) pt.d1 = F64_MINVAL;
        return pt;
      };
      double alpha = 0.0;
#if F64_STEP_ELLIPTIC
      double ls_c0 = 0.0, ls_c = 0.0;       // the cost at alpha = 0 and at the step taken (the oracle's oldcost and cost)
#endif
      if (!(snorm < F64_MINVAL)) {          // primal_linesearch
        const F64LsPt p0 = ls_eval(0.0);
        F64LsPt p1 = ls_eval(-p0.d0 / p0.d1);
        if (p0.cost < p1.cost) p1 = p0;
        alpha = p1.alpha;
#if F64_STEP_ELLIPTIC
        ls_c0 = p0.cost; ls_c = p1.cost;
#endif
        if (!(fabs(p1.d0) < gtol)) {
          int it = 0;
          bool done = false;
          const double dir = p1.d0 < 0.0 ? 1.0 : -1.0;
          F64LsPt p2 = p1;
#pragma unroll 1
          while (p1.d0 * dir <= -gtol && it < LM.ls_iterations) {      // one-sided Newton until phi' changes sign
            p2 = p1; p1 = ls_eval(p1.alpha - p1.d0 / p1.d1); it++;
            if (fabs(p1.d0) < gtol) { done = true; break; }
          }
          alpha = p1.alpha;
#if F64_STEP_ELLIPTIC
          ls_c = p1.cost;
#endif
          if (!done && !(it >= LM.ls_iterations || p1.d0 * dir <= 0.0)) {
            F64LsPt lo = dir > 0.0 ? p2 : p1, hi = dir > 0.0 ? p1 : p2;      // phi'(lo) < 0 < phi'(hi): the minimiser is bracketed
            F64LsPt best = fabs(lo.d0) < fabs(hi.d0) ? lo : hi;
#pragma unroll 1
            while (it < LM.ls_iterations) {
              double an = best.alpha - best.d0 / best.d1;
              if (!(an > lo.alpha && an < hi.alpha)) an = 0.5 * (lo.alpha + hi.alpha);
              const F64LsPt pt = ls_eval(an); it++;
              best = pt;
              if (fabs(pt.d0) < gtol) { done = true; break; }
              if (pt.d0 < 0.0) lo = pt; else hi = pt;
              if (hi.alpha - lo.alpha <= 1e-16 * fabs(hi.alpha)) break;
            }
            alpha = (done || best.cost < p0.cost) ? best.alpha : 0.0;
#if F64_STEP_ELLIPTIC
            ls_c = (done || best.cost < p0.cost) ? best.cost : p0.cost;
#endif
          }
        }
      }
      nt_a += alpha * sp; nt_r += alpha * Mp;
#if F64_STEP_ELLIPTIC
      c_ja0 += alpha * c_jp0; c_ja1 += alpha * c_jp1; c_ja2 += alpha * c_jp2;
      small_gain = LM.scale * (ls_c0 - ls_c) < LM.tolerance;      // the oracle's improvement (solve_primal)
#elif F64_STEP_CONTACTS
      c_ja0 += alpha * c_jp0; c_ja1 += alpha * c_jp1; c_ja2 += alpha * c_jp2; c_ja3 += alpha * c_jp3;
#endif
      nt_iter++;
      stop = alpha == 0.0 || nt_iter >= LM.solver_iterations;
    }
    // the rows at the iterate (primal_update): active set, forces, J' f, gradient
    const double j_lo = nt_a - ar_lo, j_hi = -nt_a - ar_hi;
    const bool n_lo = c_lo && j_lo < 0.0, n_hi = c_hi && j_hi < 0.0;
#if F64_STEP_ELLIPTIC
    bool changed = n_lo != act_lo || n_hi != act_hi;
    bool middle = false;
    double qfc_con = 0.0;
    {      // oracle rows_update: the cone's zone, forces and Hessian at the iterate
      int nz = 0;
      double cc, h00 = 0.0, h01 = 0.0, h02 = 0.0, h11 = 0.0, h12 = 0.0, h22 = 0.0;
      if (is_c) nz = f64_cone_zone(c_ja0, c_ja1, c_ja2, c_D, c_mi, c_mu, cc, c_f0, c_f1, c_f2, h00, h01, h02, h11, h12, h22);
      changed = changed || nz != c_zone;
      c_zone = nz; middle = nz == 2;
      if (is_c) {      // (the last readers of these slots passed a workgroup sum since)
        double* ct = CT + lane * F64_CT;
        ct[18] = h00; ct[19] = h01; ct[20] = h02; ct[21] = h11; ct[22] = h12; ct[23] = h22;
        ct[24] = c_f0; ct[25] = c_f1; ct[26] = c_f2; ct[27] = (double)nz;
      }
      __syncthreads();
      if (isd) { d6 fs; f64_elliptic_subtree(CT, ncon, d_b0, d_b1, cd, true, fs, cbuf); qfc_con = d6dot(cd, fs); }      // J' f, and the next matrix
    }
#elif F64_STEP_CONTACTS
    bool changed = n_lo != act_lo || n_hi != act_hi;
    double qfc_con = 0.0;
    {
      const bool n0 = is_c && c_ja0 < 0.0, n1 = is_c && c_ja1 < 0.0, n2 = is_c && c_ja2 < 0.0, n3 = is_c && c_ja3 < 0.0;
      changed = changed || n0 != c_a0 || n1 != c_a1 || n2 != c_a2 || n3 != c_a3;
      c_a0 = n0; c_a1 = n1; c_a2 = n2; c_a3 = n3;
      c_f0 = n0 ? -c_D * c_ja0 : 0.0; c_f1 = n1 ? -c_D * c_ja1 : 0.0; c_f2 = n2 ? -c_D * c_ja2 : 0.0; c_f3 = n3 ? -c_D * c_ja3 : 0.0;
      if (is_c) {      // (the last readers of these slots passed a workgroup sum since)
        double* ct = CT + lane * F64_CT;
        ct[24] = n0 ? c_D : 0.0; ct[25] = n1 ? c_D : 0.0; ct[26] = n2 ? c_D : 0.0; ct[27] = n3 ? c_D : 0.0;
        ct[28] = c_f0; ct[29] = c_f1; ct[30] = c_f2; ct[31] = c_f3;
      }
      __syncthreads();
      if (isd) { d6 fs; f64_contact_subtree(CT, ncon, d_b0, d_b1, cd, true, fs, cbuf); qfc_con = d6dot(cd, fs); }      // J' f, and the next matrix
    }
#else
    const bool changed = n_lo != act_lo || n_hi != act_hi;
#endif
    act_lo = n_lo; act_hi = n_hi;
    const double f_lo = act_lo ? -D_lo * j_lo : 0.0, f_hi = act_hi ? -D_hi * j_hi : 0.0;
    nt_qfc = f_lo - f_hi; lim_f = f_lo + f_hi;
#if F64_STEP_CONTACTS
    nt_qfc += qfc_con;
#endif
    nt_g = nt_r - nt_qfc;
    {
      double g2 = nt_g * nt_g, u1 = 0.0, u2 = 0.0, u3 = 0.0;
      WG_SUM4(g2, u1, u2, u3);
#if F64_STEP_ELLIPTIC
      // unchanged zones end the solve only where the cost is piecewise quadratic: with no contact of the env in the middle zone, whose
      // cost is not quadratic.  Beside it the oracle's rule (solve_primal): the improvement or the gradient below the tolerance
      const int zf = wg_or((changed ? 1 : 0) | (middle ? 2 : 0), FLX + 2);
      if (zf == 0 || small_gain || LM.scale * sqrt(g2) < LM.tolerance) stop = true;
#else
      // an unchanged active set: the iterate minimises the quadratic of that set (after a_s: no row is active, a_s is the minimiser)
      if (wg_or(changed ? 1 : 0, FLX + 2) == 0 || LM.scale * sqrt(g2) < LM.tolerance) stop = true;
#endif
    }
    if (stop) {                             // dual_finish + euler(): M + h B with qfrc_smooth + qfrc_constraint, where anything is damped
      if (RK4 || (lflags & 2) == 0) { x = nt_a; break; }
      phase = 2; hb = bdamp; dadd = 0.0; rhs = isd ? qfrc + nt_qfc : 0.0;
    } else { dadd = (act_lo ? D_lo : 0.0) + (act_hi ? D_hi : 0.0); rhs = nt_g; }
    }
    const double my_qacc = x;
    if (RK4) {
      // ---- RK4: this pass's derivative F[pass] is (the velocity in QV, my_qacc).  Pass 0..2 advances to X[pass + 1] = X[0] (+) h A F[pass]
      // (A = 1/2, 1/2, 1); the last pass commits X[0] (+) h sum B F (B = 1/6, 1/3, 1/3, 1/6).  fmj_forward (integrate off) is the first
      // pass alone.  Every check of the Euler step is made in every pass, and decided for the workgroup before any lane stores.
      if (LIMITS && pass == 0) rk[F64_RK4_LIM * FMJ_F64_LANES] = lim_f;
      const double rk_q0 = rk[F64_RK4_Q0 * FMJ_F64_LANES], rk_v0 = rk[F64_RK4_V0 * FMJ_F64_LANES];
      const bool fin = !A.integrate || pass == 3;
      const double wB = (pass == 0 || pass == 3) ? 1.0 / 6.0 : 1.0 / 3.0;
      const double vs = isd ? QV[lane] : 0.0;
      const double rk_sv = rk[F64_RK4_SV * FMJ_F64_LANES] + wB * vs, rk_sa = rk[F64_RK4_SA * FMJ_F64_LANES] + wB * my_qacc;
      rk[F64_RK4_SV * FMJ_F64_LANES] = rk_sv; rk[F64_RK4_SA * FMJ_F64_LANES] = rk_sa;
      const d3 rk_p0 = dmk(rk_root[0], rk_root[1], rk_root[2]);      // (read by the root body's lane alone)
      const dq rk_r0 = {rk_root[3], rk_root[4], rk_root[5], rk_root[6]};
      const double hs = !A.integrate ? 0.0 : fin ? h : pass == 2 ? h : 0.5 * h;
      const double dvel = fin ? rk_sa : my_qacc, dpos = fin ? rk_sv : vs;
      const double nvel = rk_v0 + hs * dvel, npos = rk_q0 + hs * dpos;
      if (isd) {
        if (!(fabs(my_qacc) <= 1e10)) warn |= FMJ_WARN_BADQACC;
        if (!(fabs(nvel) <= 1e10)) warn |= FMJ_WARN_BADQVEL;
        if (FM.root_free && lane < 3 && A.integrate && !(fabs(npos) <= 1e10)) warn |= FMJ_WARN_BADQPOS;
      }
      XCH[lane] = dpos;      // for the root body's lane (XCH is free between the V stage and the next pass's K)
      if (wg_or(warn & FMJ_WARN_FREEZE, FLG + 2) != 0) {      // the step is undone: QP, QV back to X[0], nothing of it stored
        frozen = true;
        if (isd) QV[lane] = rk_v0;
        if (d_scalar) QP[d_qadr] = rk_q0;
        if (jtype == FMJ_JNT_FREE) {
          QP[qadr] = rk_p0.x; QP[qadr + 1] = rk_p0.y; QP[qadr + 2] = rk_p0.z;
          QP[qadr + 3] = rk_r0.w; QP[qadr + 4] = rk_r0.x; QP[qadr + 5] = rk_r0.y; QP[qadr + 6] = rk_r0.z;
        }
        __syncthreads();
        break;
      }
      if (A.integrate) {
        if (isd) QV[lane] = nvel;
        if (d_scalar) QP[d_qadr] = npos;
        if (jtype == FMJ_JNT_FREE) f64_integrate_free(QP + qadr, rk_p0, rk_r0, XCH + dadr, hs);
      }
      if (fin) {      // the step's commit: qacc and poses of this pass, sensors of the first
        const double rk_lim0 = LIMITS ? rk[F64_RK4_LIM * FMJ_F64_LANES] : 0.0;
        const d3 rk_lin = dmk(rk[F64_RK4_LIN * FMJ_F64_LANES], rk[(F64_RK4_LIN + 1) * FMJ_F64_LANES], rk[(F64_RK4_LIN + 2) * FMJ_F64_LANES]);
        const d3 rk_ang = dmk(rk[F64_RK4_ANG * FMJ_F64_LANES], rk[(F64_RK4_ANG + 1) * FMJ_F64_LANES], rk[(F64_RK4_ANG + 2) * FMJ_F64_LANES]);
        if (isd) {
          XA[lane] = my_qacc;
          if (CONS) { ws_qacc = my_qacc; if (FUSED) cy_limfrc = rk_lim0 * U.inv_torques; }
        }
        if (last && lane < nb) {
          float* p = A.xpos + (size_t)env * nb * 3 + lane * 3; p[0] = (float)xp.x; p[1] = (float)xp.y; p[2] = (float)xp.z;
          float* q = A.xquat + (size_t)env * nb * 4 + lane * 4; q[0] = (float)xq.w; q[1] = (float)xq.x; q[2] = (float)xq.y; q[3] = (float)xq.z;
          float* ip = A.xipos + (size_t)env * nb * 3 + lane * 3; ip[0] = (float)xi.x; ip[1] = (float)xi.y; ip[2] = (float)xi.z;
          if (isb) {
            float* sp = A.sensordata + (size_t)env * FM.nsensordata + 6 * (lane - 1);
            sp[0] = (float)rk_lin.x; sp[1] = (float)rk_lin.y; sp[2] = (float)rk_lin.z;
            sp[3] = (float)rk_ang.x; sp[4] = (float)rk_ang.y; sp[5] = (float)rk_ang.z;
          }
        }
        if (last && d_scalar) {
          float* s = A.sensordata + (size_t)env * FM.nsensordata + 6 * (nb - 1);
          s[3 * d_slot] = (float)rk_q0; s[3 * d_slot + 1] = (float)rk_v0; s[3 * d_slot + 2] = LIMITS ? (float)rk_lim0 : 0.f;   // jointpos, jointvel, jointlimitfrc
          for (int a = 0; a < nact; a++) {
            const int src = FM.asrc[act0 + a];
            s[3 * FM.njs + src] = (float)RKS[src];                                                           // actuatorfrc
            if (FUSED && A.controller == 1 && A.ctrl_out) A.ctrl_out[(size_t)env * nu + src] = (float)RKS[nu + src];
          }
        }
#if F64_STEP_CONTACTS
        if (last) {      // the contact list of the step's fourth pass (fmj_forward: of its only pass), past the freeze decision above
#include "fmj_f64_contact_store.inc"
        }
#endif
        // fused: the next before_step's links row and drag (fmj_before_step after an RK4 fmj_step reads the same out of fmj_data)
        if (F64_EMIT_NEXT) f64_emit_links_and_drag(U, A, env, nit, isb, link_row, swim_slot, xp, xq, xi, rk_lin, rk_ang, xf0, xf1, xf2, xf3, xf4, xf5);
        steps_done++;
      }
      __syncthreads();
      if (fin) break;
      pass++;
      continue;
    }
    // ---- semi-implicit Euler; the freeze is decided for the workgroup before any lane commits
    const double hstep = A.integrate ? h : 0.0;
    const double pre_qd = isd ? QV[lane] : 0.0;
    const double nvel = pre_qd + hstep * my_qacc;
    if (isd) {
      if (!(fabs(my_qacc) <= 1e10)) warn |= FMJ_WARN_BADQACC;
      if (!(fabs(nvel) <= 1e10)) warn |= FMJ_WARN_BADQVEL;
      if (FM.root_free && lane < 3 && A.integrate && !(fabs(QP[lane] + h * nvel) <= 1e10)) warn |= FMJ_WARN_BADQPOS;
    }
    if (wg_or(warn & FMJ_WARN_FREEZE, FLG + 2) != 0) frozen = true;
    if (isd && !frozen) {
      XA[lane] = my_qacc;
      if (CONS) { ws_qacc = (lflags & 1) != 0 ? nt_a : my_qacc; if (FUSED) cy_limfrc = lim_f * U.inv_torques; }
      QV[lane] = nvel;
      if (d_scalar) {
        const double pre_q = QP[d_qadr];
        QP[d_qadr] = pre_q + hstep * nvel;
        if (last) {
          float* s = A.sensordata + (size_t)env * FM.nsensordata + 6 * (nb - 1) + 3 * d_slot;   // jointpos, jointvel, jointlimitfrc
          s[0] = (float)pre_q; s[1] = (float)pre_qd; s[2] = LIMITS ? (float)lim_f : 0.f;
        }
      }
    }
#if F64_STEP_CONTACTS
    if (last && !frozen) {      // the contact list of the launch's last pass: pos, frame, force in the contact frame (mju_decodePyramid), geom1 << 16 | geom2
#include "fmj_f64_contact_store.inc"
    }
#endif
    if (!frozen) steps_done++;
    __syncthreads();
    if (jtype == FMJ_JNT_FREE && A.integrate && !frozen) {     // mj_integratePos of the free joint (lane = root body)
      const double nx = QP[qadr] + h * QV[dadr], ny = QP[qadr + 1] + h * QV[dadr + 1], nz = QP[qadr + 2] + h * QV[dadr + 2];
      if (!(fabs(nx) <= 1e10) || !(fabs(ny) <= 1e10) || !(fabs(nz) <= 1e10)) warn |= FMJ_WARN_BADQPOS;
      else {
        QP[qadr] = nx; QP[qadr + 1] = ny; QP[qadr + 2] = nz;
        d3 w = dmk(QV[dadr + 3], QV[dadr + 4], QV[dadr + 5]);
        double nrm = sqrt(ddot(w, w));
        if (nrm < 1e-15) { w = dmk(1.0, 0.0, 0.0); nrm = 0.0; } else w = dmk(w.x / nrm, w.y / nrm, w.z / nrm);
        dq qo = {QP[qadr + 3], QP[qadr + 4], QP[qadr + 5], QP[qadr + 6]};
        qo = dqmul(dqnormalize(qo), daxisangle(w, h * nrm));
        QP[qadr + 3] = qo.w; QP[qadr + 4] = qo.x; QP[qadr + 5] = qo.y; QP[qadr + 6] = qo.z;
      }
    }
    if (wg_or(warn & FMJ_WARN_BADQPOS, FLG + 4) != 0) frozen = true;   // (its barrier also orders the root update before the next step)
    break;
    }
    if (FUSED) { sub = nsub; itm += nfull ? 1 : 0; }
  }

  // ---- store the state: rounded once.  An env that completed no step keeps its buffers as they are.
  if (steps_done > 0) {
    float* oq = A.qpos + (size_t)env * nq;
    float* ov = A.qvel + (size_t)env * nv;
    if (A.integrate) {
      for (int i = lane; i < nq; i += FMJ_F64_LANES) oq[i] = (float)QP[i];
      for (int i = lane; i < nv; i += FMJ_F64_LANES) ov[i] = (float)QV[i];
    }
    if (A.qacc) for (int i = lane; i < nv; i += FMJ_F64_LANES) A.qacc[(size_t)env * nv + i] = (float)XA[i];
    if (CONS && A.qacc_warmstart && A.integrate && isd) A.qacc_warmstart[(size_t)env * nv + lane] = (float)ws_qacc;
    if (A.time && lane == 0 && A.integrate) A.time[env] = (float)((double)A.time[env] + h * steps_done);
  }
  const int w = wg_or(warn, FLG + 6);
  if (w != 0 && lane == 0) A.status[env] |= w;
}

#undef WG_SUM4
#undef F64_EMIT_NEXT
