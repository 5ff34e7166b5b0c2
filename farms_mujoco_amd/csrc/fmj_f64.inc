// fmj_f64.inc — the fp64 step kernel: an unconstrained step in double precision throughout, selected per context with
// fmj_create_ex(FMJ_PRECISION_F64) (included from fmj_hip.hip; the kernel itself is compiled in its own translation unit, -DFMJ_TU_F64).
//
// One workgroup of 128 threads (two wavefronts) per environment, whatever the model's size: lane t is body t and dof t, as in
// fmj_wide.inc.  The per-env buffers of fmj_data stay fp32: they are widened on load and rounded once on store (a launch of n steps
// keeps the state in LDS as doubles between its steps).  The model constants come from a second, fp64 set of tables (F64Model) that
// only fp64 contexts upload.  Every stage follows oracle/fmj_oracle.c's formulas (the 10-vector spatial inertias about the tree's centre
// of mass, mj_integratePos, true divisions and square roots); what differs is the order of some sums:
//   K / V   pointer jumping along the body chains through LDS, as in fmj_wide.inc (the oracle walks parent -> child)
//   C / S   the tree's centre of mass and the subtree sums (composite inertias, body forces): every lane adds the rows of its own
//           contiguous depth-first range [lane, lane + subtree size) from LDS, last body first: no prefix differences, no cancellation
//   M       lane = dof i writes row i of H = M + diag(armature + h (damping + implicitfast gains)) to LDS: H[i][j] at column depth(j)
//   L       L'DL on the rows in LDS by rounds of unrelated dofs of one depth (the WideRoundW rounds), one barrier per round: an
//           ancestor lane subtracts (H[p][i] / D_p) x row p for every pivot p of the round below it, and the same multiple of p's
//           right-hand side; a pivot's row and right-hand side are final before the first round of its depth
//   X       x_i /= D_i, then the root-first sweep a tree level at a time (one barrier per level)
//   freeze  decided for the workgroup (wg_or) before any lane commits a store; every barrier is reached by all 128 threads
// No private array is indexed at run time (nothing lives in scratch), no fast reciprocal / rsqrt, no fp32 intermediate.
//
// fmj_step_f64_kernel<true> is the fused loop of fmj_step_fused_f64 (include/fmj.h): what fmj_step_wide_kernel<true, ..> does around
// its steps (fmj_stage_carry_in / step_head / q / f .inc, emit_links_and_drag), in double.  Lane = dof writes the joints row of a full
// step and evaluates the controller (ctrl tape row of the iteration, or the wave controller with sin); after the forward pass of a
// step that is not the launch's last, lane = body writes the links row of the next before_step and computes its drag, whose
// world-frame wrench stays in registers as doubles for the next step's F.  Rows are rounded to fp32 at their store, the state where
// the launch ends.  Units and water come widened in F64Fused; the fused loop needs no LDS of its own.
//
// fmj_step_f64_kernel<.., true> (fmj_create_ex2 with FMJ_CREATE_F64_LIMITS) adds joint limits, solved exactly.  Lane = dof owns the
// up-to-two rows of its joint (oracle make_constraints, EFC_LIMIT: J = -side e_dof, so J M^-1 J' is never formed).  A step with no
// candidate row (dist < margin nowhere in the env: one wg_or) is the step above, bit for bit.  Otherwise the step minimises
//   0.5 (a - a_s)' M (a - a_s) + sum_e s_e(J_e a - aref_e),   s_e(x) = 0.5 x^2 / R_e for x < 0, else 0      (oracle solve_primal)
// by Newton's method from a_s = M^-1 qfrc_smooth.  The Newton matrix M + sum_active e_d e_d' / R_e is M with a larger diagonal, so each
// iteration refills the lane's row of HR from CR / CD (the M stage without h B, plus the lane's active 1 / R) and runs the L rounds and
// the X sweep again: no second copy of H.  With p = -(M + D_S)^-1 g one has M p = -g - D_S p, and r = M (a - a_s) is carried along the
// iterates: no product with M.  The line search is exact along the piecewise-quadratic cost (primal_linesearch: Newton on phi' from
// alpha = 0 until it changes sign, then Newton safeguarded by the bracket); each lane evaluates its own rows and the sums go through
// wg_sum4.  The loop ends when a step leaves the active set unchanged (the iterate is then the minimiser of the quadratic of that set),
// at the oracle's gradient tolerance, or after solver_iterations iterations.  Then, as dual_finish and euler() do: f_e = -x_e / R_e on
// the active rows, qfrc_constraint = J' f, and one more fill and factorisation of M + h B solved with qfrc_smooth + qfrc_constraint
// (the constrained qacc itself when nothing is damped).  Every new branch is decided from a workgroup reduction: it is uniform, and every
// barrier is reached by all 128 threads.

#define FMJ_F64_LANES 128
#define F64_BD 28      // doubles per body: pos(3) mass, quat(4), ipos(3) subtree mass, iquat(4), inertia(3) -, axis(3) qpos0, jnt_pos(3) stiffness
#define F64_BI 8       // ints per body: parent, joint type (-1 none), qpos address, dof address, subtree size, links row (-1 none), swimming slot (-1 none)
#define F64_DI 8       // ints per dof: body, depth, qpos address (-1: a free joint's dof), first actuator, actuator count, joint-sensor slot, joints row (-1 none)
#define F64_AD 8       // doubles per actuator (sorted by dof): gain, bias(3), ctrlrange(2), forcerange(2) (infinite where not limited)
#define F64_SW 10      // doubles per swimming slot: drag coefficients (3 force, 3 torque), mass, height, density, xfrc row
#define F64_LM 12      // doubles per dof of a limits context: limited (0 / 1), range(2), margin, solref(2), solimp(5), dof_invweight0

struct F64Model {
  int nbody, nv, nq, nu, rs, jump_rounds, anc_stride, root_free, any_stiffness, implicitfast, nsensordata, njs, maxdep, nround;
  double h, gx, gy, gz, mtot;
  const double* bd;             // [nbody][F64_BD]
  const int* bi;                // [nbody][F64_BI]
  const double* dd;             // [nv][2] armature, damping
  const int* di;                // [nv][F64_DI]
  const double* ad;             // [nact][F64_AD]
  const int* asrc;              // [nact] the model's actuator index (ctrl / actuatorfrc slot)
  const uint8_t* b_anc;         // [nbody][anc_stride] ancestor body at distance 2^r (DevModel's table)
  const uint8_t* danc;          // [nv][rs] ancestor dof at each depth below the dof's own
  const struct WideRoundW* rounds;   // [nround] elimination rounds, deepest level first
};

// What only the fused loop reads (a third kernel argument: F64Model and StepArgs keep their places in the kernarg segment).  Units and
// water arrive as fp32 in the C-ABI and are widened once, on the host; the reciprocals are double divisions.
struct F64Fused {
  double inv_meters, inv_velocity, inv_angvel, inv_torques, newtons, torques;
  double surface, viscosity, wvx, wvy, wvz, wgravity;
  const double* sw;             // [ns][F64_SW]
  int n_links, n_joints, n_xfrc;      // rows per env of the three ring tensors
};

// What only the LIMITS instantiations read (a fourth kernel argument, for the same reason).  The tolerances and the iteration budgets
// are the model's (solver_tolerance, ls_tolerance, solver_iterations, ls_iterations); scale = 1 / (meaninertia max(1, nv)).
struct F64Limits {
  int solver_iterations, ls_iterations;
  double tolerance, ls_tolerance, scale;
  const double* lm;             // [nv][F64_LM]
};

// LDS map, in doubles (ints at the end)
struct LdsLayoutD { int QP, QV, XA, XCH, CD, CI, CR, CF, CS, MX, HR, XW, FLG, total_bytes; };
__host__ __device__ inline LdsLayoutD ldsd_layout(int nb, int nv, int nq, int rs) {
  LdsLayoutD L; int o = 0;
  L.QP = o; o += (nq + 1) & ~1;
  L.QV = o; o += (nv + 1) & ~1;
  L.XA = o; o += (nv + 1) & ~1;
  L.XCH = o; o += 2 * FMJ_F64_LANES * 8;      // two exchange buffers of 8 doubles per lane (K / V)
  L.CD = o; o += nv * 6;                      // cdof
  L.CI = o; o += nb * 10;                     // cinert
  L.CR = o; o += nb * 10;                     // composite inertia
  L.CF = o; o += nb * 6;                      // body force
  L.CS = o; o += nb * 6;                      // subtree force
  L.MX = o; o += nb * 4;                      // mass * xipos, mass
  L.HR = o; o += nv * rs;                     // rows of H, then of L'DL
  L.XW = o; o += FMJ_F64_LANES;               // right-hand side / solution, published per lane
  L.FLG = o; o += 4;                          // wg_or slots (8 ints)
  L.total_bytes = o * 8;
  return L;
}

// What the LIMITS instantiations append to the map: two alternating buffers of 2 waves x 4 sums (wg_sum4) and 8 more wg_or ints
#define F64_LIMITS_LDS_DOUBLES 20
__host__ __device__ inline int ldsd_total_bytes(int nb, int nv, int nq, int rs, int limits) {
  return ldsd_layout(nb, nv, nq, rs).total_bytes + (limits ? F64_LIMITS_LDS_DOUBLES * 8 : 0);
}

#ifdef FMJ_TU_F64
struct d3 { double x, y, z; };
struct dq { double w, x, y, z; };
struct d6 { d3 r, l; };
__device__ __forceinline__ d3 dmk(double x, double y, double z) { d3 r = {x, y, z}; return r; }
__device__ __forceinline__ d3 dadd(d3 a, d3 b) { return dmk(a.x + b.x, a.y + b.y, a.z + b.z); }
__device__ __forceinline__ d3 dsub(d3 a, d3 b) { return dmk(a.x - b.x, a.y - b.y, a.z - b.z); }
__device__ __forceinline__ d3 dscl(d3 a, double s) { return dmk(a.x * s, a.y * s, a.z * s); }
__device__ __forceinline__ double ddot(d3 a, d3 b) { return a.x * b.x + a.y * b.y + a.z * b.z; }
__device__ __forceinline__ d3 dcross(d3 a, d3 b) { return dmk(a.y * b.z - a.z * b.y, a.z * b.x - a.x * b.z, a.x * b.y - a.y * b.x); }
__device__ __forceinline__ dq dqmul(dq a, dq b) {
  dq r;
  r.w = a.w * b.w - a.x * b.x - a.y * b.y - a.z * b.z;
  r.x = a.w * b.x + a.x * b.w + a.y * b.z - a.z * b.y;
  r.y = a.w * b.y - a.x * b.z + a.y * b.w + a.z * b.x;
  r.z = a.w * b.z + a.x * b.y - a.y * b.x + a.z * b.w;
  return r;
}
__device__ __forceinline__ dq dqnormalize(dq q) {      // mju_normalize4
  const double n = sqrt(q.w * q.w + q.x * q.x + q.y * q.y + q.z * q.z);
  if (n < 1e-15) { dq r = {1.0, 0.0, 0.0, 0.0}; return r; }
  dq r = {q.w / n, q.x / n, q.y / n, q.z / n};
  return r;
}
struct dm33 { double a0, a1, a2, a3, a4, a5, a6, a7, a8; };
__device__ __forceinline__ dm33 dq2m(dq q) {           // mju_quat2Mat
  dm33 m;
  const double q00 = q.w * q.w, q11 = q.x * q.x, q22 = q.y * q.y, q33 = q.z * q.z;
  m.a0 = q00 + q11 - q22 - q33; m.a4 = q00 - q11 + q22 - q33; m.a8 = q00 - q11 - q22 + q33;
  m.a1 = 2.0 * (q.x * q.y - q.w * q.z); m.a2 = 2.0 * (q.x * q.z + q.w * q.y);
  m.a3 = 2.0 * (q.x * q.y + q.w * q.z); m.a5 = 2.0 * (q.y * q.z - q.w * q.x);
  m.a6 = 2.0 * (q.x * q.z - q.w * q.y); m.a7 = 2.0 * (q.y * q.z + q.w * q.x);
  return m;
}
__device__ __forceinline__ d3 dmrot(const dm33& m, d3 v) {
  return dmk(m.a0 * v.x + m.a1 * v.y + m.a2 * v.z, m.a3 * v.x + m.a4 * v.y + m.a5 * v.z, m.a6 * v.x + m.a7 * v.y + m.a8 * v.z);
}
__device__ __forceinline__ d3 dqrot(dq q, d3 v) { return dmrot(dq2m(q), v); }      // mju_rotVecQuat
__device__ __forceinline__ dq daxisangle(d3 ax, double ang) {                     // mju_axisAngle2Quat
  if (ang == 0.0) { dq r = {1.0, 0.0, 0.0, 0.0}; return r; }
  double s, c;
  sincos(0.5 * ang, &s, &c);
  dq r = {c, ax.x * s, ax.y * s, ax.z * s};
  return r;
}
__device__ __forceinline__ d6 d6add(d6 a, d6 b) { d6 o = {dadd(a.r, b.r), dadd(a.l, b.l)}; return o; }
__device__ __forceinline__ d6 d6scl(d6 a, double s) { d6 o = {dscl(a.r, s), dscl(a.l, s)}; return o; }
__device__ __forceinline__ double d6dot(d6 a, d6 b) { return a.r.x * b.r.x + a.r.y * b.r.y + a.r.z * b.r.z + a.l.x * b.l.x + a.l.y * b.l.y + a.l.z * b.l.z; }
__device__ __forceinline__ d6 dcross_motion(d6 vel, d6 v) { d6 o = {dcross(vel.r, v.r), dadd(dcross(vel.r, v.l), dcross(vel.l, v.r))}; return o; }
__device__ __forceinline__ d6 dcross_force(d6 vel, d6 f) { d6 o = {dadd(dcross(vel.r, f.r), dcross(vel.l, f.l)), dcross(vel.r, f.l)}; return o; }
struct di10 { double i0, i1, i2, i3, i4, i5, i6, i7, i8, i9; };      // Ixx Iyy Izz Ixy Ixz Iyz m dx, m dy, m dz, m
__device__ __forceinline__ d6 dinert_mul(const di10& i, d6 v) {       // mju_mulInertVec
  d6 o;
  o.r.x = i.i0 * v.r.x + i.i3 * v.r.y + i.i4 * v.r.z - i.i8 * v.l.y + i.i7 * v.l.z;
  o.r.y = i.i3 * v.r.x + i.i1 * v.r.y + i.i5 * v.r.z + i.i8 * v.l.x - i.i6 * v.l.z;
  o.r.z = i.i4 * v.r.x + i.i5 * v.r.y + i.i2 * v.r.z - i.i7 * v.l.x + i.i6 * v.l.y;
  o.l.x = i.i8 * v.r.y - i.i7 * v.r.z + i.i9 * v.l.x;
  o.l.y = i.i6 * v.r.z - i.i8 * v.r.x + i.i9 * v.l.y;
  o.l.z = i.i7 * v.r.x - i.i6 * v.r.y + i.i9 * v.l.z;
  return o;
}
__device__ __forceinline__ void dput6(double* p, d6 v) { p[0] = v.r.x; p[1] = v.r.y; p[2] = v.r.z; p[3] = v.l.x; p[4] = v.l.y; p[5] = v.l.z; }
__device__ __forceinline__ d6 dget6(const double* p) { d6 v = {dmk(p[0], p[1], p[2]), dmk(p[3], p[4], p[5])}; return v; }
__device__ __forceinline__ void dput10(double* p, const di10& i) { p[0] = i.i0; p[1] = i.i1; p[2] = i.i2; p[3] = i.i3; p[4] = i.i4; p[5] = i.i5; p[6] = i.i6; p[7] = i.i7; p[8] = i.i8; p[9] = i.i9; }
__device__ __forceinline__ di10 dget10(const double* p) { di10 i = {p[0], p[1], p[2], p[3], p[4], p[5], p[6], p[7], p[8], p[9]}; return i; }

// emit_links_and_drag (fmj_hip.hip) in double, for lane = body: the links row of iteration `it` (reference physics.py:449-466,435-446)
// and the drag of a swimming link (drag.pyx:152-268 with com2urdf = identity: physics.py:455-466 fills both quaternions from xquat),
// its xfrc row and the body's world-frame wrench (xf0..2 force, xf3..5 torque).  The rows are rounded to fp32 at the store.
__device__ __forceinline__ void f64_emit_links_and_drag(const F64Fused& U, const StepArgs& A, int env, int it, bool isb, int link_row, int swim_slot,
                                                        d3 xpos, dq xquat, d3 xipos, d3 linvel, d3 angvel,
                                                        double& xf0, double& xf1, double& xf2, double& xf3, double& xf4, double& xf5) {
  const int index = it % A.buffer_size;
  const d3 r_com = dscl(xipos, U.inv_meters), r_urdf = dscl(xpos, U.inv_meters);
  const d3 r_lin = dscl(linvel, U.inv_velocity), r_ang = dscl(angvel, U.inv_angvel);
  if (A.do_readout && isb && link_row >= 0) {
    float* row = A.links + ((size_t)index * A.row_stride_links + (size_t)env * U.n_links * FMJ_LINK_SIZE) + link_row * FMJ_LINK_SIZE;
    const float qx = (float)xquat.x, qy = (float)xquat.y, qz = (float)xquat.z, qw = (float)xquat.w;      // wxyz -> xyzw (physics.py:458)
    row[0] = (float)r_com.x; row[1] = (float)r_com.y; row[2] = (float)r_com.z; row[3] = qx; row[4] = qy; row[5] = qz; row[6] = qw;
    row[7] = (float)r_urdf.x; row[8] = (float)r_urdf.y; row[9] = (float)r_urdf.z; row[10] = qx; row[11] = qy; row[12] = qz; row[13] = qw;
    row[14] = (float)r_lin.x; row[15] = (float)r_lin.y; row[16] = (float)r_lin.z;
    row[17] = (float)r_ang.x; row[18] = (float)r_ang.y; row[19] = (float)r_ang.z;
  }
  if (!A.do_drag) return;
  xf0 = xf1 = xf2 = xf3 = xf4 = xf5 = 0.0;
  if (!isb || swim_slot < 0) return;
  if (r_com.z > U.surface) return;                                    // drag.pyx:192-194: above the surface, no force and no row
  const double* sw = U.sw + (size_t)swim_slot * F64_SW;
  const dm33 R = dq2m(xquat);                                         // link -> world; world -> link is its transpose (drag.pyx:50-63, 235-244)
  d3 lin = dmk(R.a0 * r_lin.x + R.a3 * r_lin.y + R.a6 * r_lin.z, R.a1 * r_lin.x + R.a4 * r_lin.y + R.a7 * r_lin.z, R.a2 * r_lin.x + R.a5 * r_lin.y + R.a8 * r_lin.z);
  const d3 ang = dmk(R.a0 * r_ang.x + R.a3 * r_ang.y + R.a6 * r_ang.z, R.a1 * r_ang.x + R.a4 * r_ang.y + R.a7 * r_ang.z, R.a2 * r_ang.x + R.a5 * r_ang.y + R.a8 * r_ang.z);
  d3 buoy = dmk(0.0, 0.0, 0.0);
  const double mass = sw[6], height = sw[7], density = sw[8];
  if (A.use_buoyancy && mass > 0.0 && r_com.z < U.surface) {         // drag.pyx:139-146
    const double fz = -1000.0 * mass * U.wgravity / density * fmin(fmax(U.surface - r_com.z, 0.0) / height, 1.0);
    buoy = dmk(R.a6 * fz, R.a7 * fz, R.a8 * fz);
  }
  lin = dsub(lin, dmk(R.a0 * U.wvx + R.a3 * U.wvy + R.a6 * U.wvz, R.a1 * U.wvx + R.a4 * U.wvy + R.a7 * U.wvz, R.a2 * U.wvx + R.a5 * U.wvy + R.a8 * U.wvz));
  d3 f = dmk(fabs(lin.x) * lin.x * (U.viscosity * sw[0]) + buoy.x, fabs(lin.y) * lin.y * (U.viscosity * sw[1]) + buoy.y,
                   fabs(lin.z) * lin.z * (U.viscosity * sw[2]) + buoy.z);                                  // sign(v) v^2 c visc + buoyancy (drag.pyx:83-88)
  d3 t = dmk(fabs(ang.x) * ang.x * sw[3], fabs(ang.y) * ang.y * sw[4], fabs(ang.z) * ang.z * sw[5]);   // :104-108
  // drag.pyx:261-262 rotates both by urdf2com = conj(conj(q) q), a sandwich that multiplies by |q|^4: the identity for a unit quaternion.
  // Inside a launch |q| is 1 to the last bit of a double; the poses of fmj_data behind the iteration0 row are fp32, |q|^2 is 1 only to
  // 1e-7 there, and the reference's arithmetic carries that factor into the row (two ulps of the fp32 store)
  const double qq = xquat.w * xquat.w + xquat.x * xquat.x + xquat.y * xquat.y + xquat.z * xquat.z;
  f = dscl(f, qq * qq); t = dscl(t, qq * qq);
  float* xr = A.xfrc + ((size_t)index * A.row_stride_xfrc + (size_t)env * U.n_xfrc * FMJ_XFRC_SIZE) + (int)sw[9] * FMJ_XFRC_SIZE;
  xr[0] = (float)f.x; xr[1] = (float)f.y; xr[2] = (float)f.z; xr[3] = (float)t.x; xr[4] = (float)t.y; xr[5] = (float)t.z;
  const d3 fw = dmrot(R, f), tw = dmrot(R, t);
  xf0 = fw.x * U.newtons; xf1 = fw.y * U.newtons; xf2 = fw.z * U.newtons;
  xf3 = tw.x * U.torques; xf4 = tw.y * U.torques; xf5 = tw.z * U.torques;
}

// Sums of four doubles over the workgroup, on every lane and bitwise the same on every lane (a butterfly per wave, then wave 0 + wave 1).
// buf: 8 doubles; consecutive calls alternate between two buffers, so one barrier per call is enough: a lane still reading buffer A
// has not reached the barrier of the call that writes B, and A is rewritten only after that barrier.
__device__ __forceinline__ void wg_sum4(double& s0, double& s1, double& s2, double& s3, double* buf) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) { s0 += __shfl_xor(s0, o, 64); s1 += __shfl_xor(s1, o, 64); s2 += __shfl_xor(s2, o, 64); s3 += __shfl_xor(s3, o, 64); }
  if ((threadIdx.x & 63) == 0) { double* b = buf + (threadIdx.x >> 6) * 4; b[0] = s0; b[1] = s1; b[2] = s2; b[3] = s3; }
  __syncthreads();
  s0 = buf[0] + buf[4]; s1 = buf[1] + buf[5]; s2 = buf[2] + buf[6]; s3 = buf[3] + buf[7];
}

// One candidate limit row (oracle make_constraints: get_impedance, mj_makeImpedance, mj_referenceConstraint): D = 1 / R and aref from
// the row's pos = dist, vel = J qvel.  lm: the dof's F64_LM doubles.
#define F64_MINVAL 1e-15
#define F64_MINIMP 0.0001
#define F64_MAXIMP 0.9999
__device__ __forceinline__ void f64_limit_row(const double* lm, double h, double pos, double vel, double& D, double& aref) {
  const double margin = lm[3], sr0 = lm[4], sr1 = lm[5];
  const double dmin = fmin(fmax(lm[6], F64_MINIMP), F64_MAXIMP), dmax = fmin(fmax(lm[7], F64_MINIMP), F64_MAXIMP);
  const double width = fmax(0.0, lm[8]), mid = fmin(fmax(lm[9], F64_MINIMP), F64_MAXIMP), power = fmax(1.0, lm[10]);
  double imp;
  if (dmin == dmax || width <= F64_MINVAL) imp = 0.5 * (dmin + dmax);
  else {
    const double xx = fabs((pos - margin) / width);
    double y;
    if (xx >= 1.0) y = 1.0;
    else if (xx <= 0.0) y = 0.0;
    else if (power == 1.0) y = xx;
    else if (xx <= mid) y = pow(xx, power) / pow(mid, power - 1.0);
    else y = 1.0 - pow(1.0 - xx, power) / pow(1.0 - mid, power - 1.0);
    imp = dmin + y * (dmax - dmin);
  }
  double K, B;
  if (sr0 > 0.0) {
    const double tc = fmax(sr0, 2.0 * h);
    K = 1.0 / fmax(F64_MINVAL, dmax * dmax * tc * tc * sr1 * sr1);
    B = 2.0 / fmax(F64_MINVAL, dmax * tc);
  } else { K = -sr0 / fmax(F64_MINVAL, dmax * dmax); B = -sr1 / fmax(F64_MINVAL, dmax); }
  D = 1.0 / fmax(F64_MINVAL, (1.0 - imp) * lm[11] / imp);
  aref = -B * vel - K * imp * (pos - margin);
}

// A point of the line search (oracle ls_pt): the cost along the search line and its first two derivatives
struct F64LsPt { double alpha, cost, d0, d1; };

template <bool FUSED, bool LIMITS>
__global__ void __launch_bounds__(FMJ_F64_LANES) fmj_step_f64_kernel(const F64Model FM, const StepArgs A, const F64Fused U, const F64Limits LM) {
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
    if (FUSED && !last && (nfull || (A.sub_links && !(A.n_it_total > 0 && nit >= A.n_it_total)))) {
      const d3 linvel = dsub(cv.l, dcross(dsub(xi, com), cv.r));
      f64_emit_links_and_drag(U, A, env, nit, isb, link_row, swim_slot, xp, xq, xi, linvel, cv.r, xf0, xf1, xf2, xf3, xf4, xf5);
    }
    // ---- sensors and poses of this (pre-integration) state
    if (last && lane < nb) {
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
            if (last && A.ctrl_out) A.ctrl_out[(size_t)env * nu + src] = (float)c;      // what task.py:288-346 leaves in physics.data.ctrl
          } else c = A.ctrl ? (double)A.ctrl[(size_t)(FUSED ? itm : step) * A.ctrl_step_stride + (size_t)env * nu + src] : 0.0;   // fused: one ctrl row per iteration
          c = fmin(fmax(c, ap[4]), ap[5]);
          double f = ap[0] * c + ap[1] + ap[2] * qj + ap[3] * qd;
          f = fmin(fmax(f, ap[6]), ap[7]);
          if (FM.implicitfast && !A.disable_actuation && f > ap[6] && f < ap[7]) bdamp += -ap[3];
          if (A.disable_actuation) f = 0.0;
          if (last) A.sensordata[(size_t)env * FM.nsensordata + 6 * (nb - 1) + 3 * FM.njs + src] = (float)f;   // actuatorfrc
          asum += f;
        }
        if (FUSED) cy_actsum = asum * U.inv_torques;
      }
      qfrc = passive - d6dot(cd, dget6(CS + d_body * 6)) + asum;
    }
    // ---- limits: the candidate rows of the lane's joint (oracle make_constraints): lo is side -1 (J = +1), hi is side +1 (J = -1)
    bool c_lo = false, c_hi = false;
    double D_lo = 0.0, D_hi = 0.0, ar_lo = 0.0, ar_hi = 0.0;
    int lflags = 0;      // workgroup: 1 = some row is a candidate, 2 = some dof is damped
    if (LIMITS) {
      if (lim_on) {
        const double qj = QP[d_qadr], qd = QV[lane];
        const double dist_lo = qj - lmp[1], dist_hi = lmp[2] - qj;
        c_lo = dist_lo < lmp[3]; c_hi = dist_hi < lmp[3];
        if (c_lo) f64_limit_row(lmp, h, dist_lo, qd, D_lo, ar_lo);
        if (c_hi) f64_limit_row(lmp, h, dist_hi, -qd, D_hi, ar_hi);
      }
      lflags = wg_or(((c_lo || c_hi) ? 1 : 0) | ((isd && bdamp != 0.0) ? 2 : 0), FLX + 0);
    }
    // The solve below runs once in a step without candidate rows (phase 2: M + h B, qfrc_smooth).  With candidate rows it runs for
    // a_s (phase 0: M), once per Newton iteration (phase 1: M + D_S, the gradient), and once more for the damped step (phase 2).
    int phase = 2, nt_iter = 0;
    double hb = bdamp, dadd = 0.0, rhs = isd ? qfrc : 0.0;
    double nt_a = 0.0, nt_as = 0.0, nt_r = 0.0, nt_g = 0.0, nt_qfc = 0.0, lim_f = 0.0;      // a, a_s, M (a - a_s), gradient, J' f, the joint's limit force
    bool act_lo = false, act_hi = false;
    if (LIMITS && (lflags & 1) != 0) { phase = 0; hb = 0.0; }
    const d6 buf = dinert_mul(dget10(CR + d_body * 10), cd);
    double x;
#pragma unroll 1
    for (;;) {      // (the stages below keep the indentation they had before the loop was put around them)
    // ---- M: row i of H (mj_crb, then mj_Euler's M + h B), H[i][j] at column depth(j)
    {
      if (isd) {
        double* row = HR + lane * rs;
        const uint8_t* an = FM.danc + (size_t)lane * rs;
        for (int d = 0; d < ddepth; d++) row[d] = d6dot(dget6(CD + (int)an[d] * 6), buf);
        row[ddepth] = (d_arm + d6dot(cd, buf)) + h * hb;
        if (LIMITS) row[ddepth] += dadd;
        if (A.dbg_H && (!LIMITS || phase != 1)) {
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
    if (!LIMITS || phase == 2) break;
    // ---- limits: the Newton iteration on the primal problem (oracle solve_primal, unilateral rows); every branch below is uniform
    bool stop;
    if (phase == 0) {                       // x = a_s: the first iterate, where M (a - a_s) = 0
      nt_as = nt_a = x; nt_r = 0.0;
      phase = 1;
      stop = LM.solver_iterations <= 0;     // (the forces of a_s, as primal_update leaves them)
    } else {                                // x = (M + D_S)^-1 g: the search direction p = -x and M p = -g - D_S p
      const double sp = -x, Mp = -nt_g - dadd * sp;
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
        WG_SUM4(c, e0, e1, unused);
        F64LsPt pt;
        pt.alpha = alpha; pt.cost = qg0 + alpha * (qg1 + alpha * qg2) + c; pt.d0 = qg1 + 2.0 * alpha * qg2 + e0;
        pt.d1 = 2.0 * qg2 + e1; if (!(pt.d1 > F64_MINVAL)) pt.d1 = F64_MINVAL;
        return pt;
      };
      double alpha = 0.0;
      if (!(snorm < F64_MINVAL)) {          // primal_linesearch
        const F64LsPt p0 = ls_eval(0.0);
        F64LsPt p1 = ls_eval(-p0.d0 / p0.d1);
        if (p0.cost < p1.cost) p1 = p0;
        alpha = p1.alpha;
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
          }
        }
      }
      nt_a += alpha * sp; nt_r += alpha * Mp;
      nt_iter++;
      stop = alpha == 0.0 || nt_iter >= LM.solver_iterations;
    }
    // the rows at the iterate (primal_update): active set, forces, J' f, gradient
    const double j_lo = nt_a - ar_lo, j_hi = -nt_a - ar_hi;
    const bool n_lo = c_lo && j_lo < 0.0, n_hi = c_hi && j_hi < 0.0;
    const bool changed = n_lo != act_lo || n_hi != act_hi;
    act_lo = n_lo; act_hi = n_hi;
    const double f_lo = act_lo ? -D_lo * j_lo : 0.0, f_hi = act_hi ? -D_hi * j_hi : 0.0;
    nt_qfc = f_lo - f_hi; lim_f = f_lo + f_hi;
    nt_g = nt_r - nt_qfc;
    {
      double g2 = nt_g * nt_g, u1 = 0.0, u2 = 0.0, u3 = 0.0;
      WG_SUM4(g2, u1, u2, u3);
      // an unchanged active set: the iterate minimises the quadratic of that set (after a_s: no row is active, a_s is the minimiser)
      if (wg_or(changed ? 1 : 0, FLX + 2) == 0 || LM.scale * sqrt(g2) < LM.tolerance) stop = true;
    }
    if (stop) {                             // dual_finish + euler(): M + h B with qfrc_smooth + qfrc_constraint, where anything is damped
      if ((lflags & 2) == 0) { x = nt_a; break; }
      phase = 2; hb = bdamp; dadd = 0.0; rhs = isd ? qfrc + nt_qfc : 0.0;
    } else { dadd = (act_lo ? D_lo : 0.0) + (act_hi ? D_hi : 0.0); rhs = nt_g; }
    }
    const double my_qacc = x;
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
      if (LIMITS) { ws_qacc = (lflags & 1) != 0 ? nt_a : my_qacc; if (FUSED) cy_limfrc = lim_f * U.inv_torques; }
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
    if (LIMITS && A.qacc_warmstart && A.integrate && isd) A.qacc_warmstart[(size_t)env * nv + lane] = (float)ws_qacc;
    if (A.time && lane == 0 && A.integrate) A.time[env] = (float)((double)A.time[env] + h * steps_done);
  }
  const int w = wg_or(warn, FLG + 6);
  if (w != 0 && lane == 0) A.status[env] |= w;
}

#undef WG_SUM4
// -DFMJ_TU_F64: the two instantiations without limits; -DFMJ_TU_F64=2: the two LIMITS instantiations, a translation unit of their own
#if FMJ_TU_F64 == 2
extern "C" __attribute__((visibility("hidden"))) void* fmj_tu_f64_limits(int fused) {
  return fused ? (void*)fmj_step_f64_kernel<true, true> : (void*)fmj_step_f64_kernel<false, true>;
}
#else
extern "C" __attribute__((visibility("hidden"))) void* fmj_tu_f64(int fused) {
  return fused ? (void*)fmj_step_f64_kernel<true, false> : (void*)fmj_step_f64_kernel<false, false>;
}
#endif
#endif  // FMJ_TU_F64
