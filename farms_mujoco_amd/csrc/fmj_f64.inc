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
//
// fmj_step_f64_contacts_kernel<LIMITS> (fmj_create_ex2 with FMJ_CREATE_F64_CONTACTS; the step's text with F64_STEP_CONTACTS 1, helpers in
// fmj_f64_contacts.inc) adds ground contacts of sphere / capsule / box geoms under the pyramidal cone: four more unilateral rows per
// contact in the same Newton solve.  A row e of a contact at world point p with direction u = normal +- mu tangent is one spatial force
// about the centre of mass, W_e = {(p - com) x u, u}, and J_e[j] = cdof_j . W_e on the dof chain of the contact's body, zero elsewhere.
// J' D J therefore fills only entries (i, j) with j an ancestor of i - the pattern of M the rows in HR already have - and row i of the
// Newton matrix is the M stage's with buf_i + sum over active rows of the subtree of i of D_e (W_e . cdof_i) W_e in the place of buf_i.
// Lane = geom runs the narrow phase (oracle collide_plane) from the pass's poses, a workgroup prefix sum puts the contacts in the
// oracle's order, lane = contact owns the four rows of its contact (parameters, residuals and forces in registers; W, the active D
// and the forces in LDS for the dof lanes: F64_CT doubles per contact past the LIMITS block).  J a, J p and J qvel are W_e . the sum
// of cdof_j x_j over the chain of the contact's body.  A step in which no contact penetrates (and no limit row is a candidate) is the
// unconstrained step, bit for bit.
//
// fmj_step_f64_terrain_kernel<LIMITS> (fmj_create_ex2 with FMJ_CREATE_F64_CONTACTS | FMJ_CREATE_F64_TERRAIN; the step's text with
// F64_STEP_CONTACTS 1 and F64_STEP_TERRAIN 1, helpers in fmj_f64_terrain.inc) is that kernel with the ground's normal a per-contact
// quantity: the ground entries are the world's planes and its one heightfield (oracle ground_dist: the plane of the grid triangle under
// each candidate point; the samples are a double table in global memory), and the animat may carry cylinders (up to four rim points
// against the plane under the cylinder's centre).  The normal travels in the exchange record (pos, dist, normal, geom and ground entry
// in one double), the tangents come from it by add_contact's rule per contact (a plane's are its host-computed constants), and the
// normal stays in LDS (F64_TN doubles per contact past the records) for the record store of the launch's last step.
//
// fmj_step_f64_elliptic_kernel<LIMITS> (fmj_create_ex2 with FMJ_CREATE_F64_CONTACTS | FMJ_CREATE_F64_ELLIPTIC and a model whose cone is
// elliptic; the terrain kernels' text with F64_STEP_ELLIPTIC 1 on top, helpers in fmj_f64_elliptic.inc) solves the contacts under the
// elliptic cone: three rows per contact (normal, tangent 1, tangent 2: oracle make_constraints), whose share of the Newton matrix is
// J_c' Hc J_c with the 3 x 3 Hessian Hc of the cone's cost at the iterate (oracle cone_zone, newton_direction) - three rows on one
// ancestor chain, so the pattern of M holds as it does for the four pyramid rows.  The cost of a contact on the cone's surface (the
// middle zone) is not quadratic: an unchanged set of zones proves the minimiser only when no contact of the env is in that zone, and
// the solve otherwise ends by the oracle's rule (improvement or gradient below the tolerance).  The regulariser of the tangents does
// not depend on the friction (R_n / impratio), so a friction of 1e-5 is no stiffer than any other.  Arguments and LDS are the terrain
// kernels' (the record keeps its stride), and so is the narrow phase: one family for flat ground and terrain.
//
// fmj_step_f64_mesh_kernel<LIMITS> and fmj_step_f64_mesh_elliptic_kernel<LIMITS> (fmj_create_ex2 with FMJ_CREATE_F64_CONTACTS |
// FMJ_CREATE_F64_MESH and a model with a FMJ_GEOM_MESH geom; the terrain kernels' text, or the elliptic kernels', with F64_STEP_MESH 1
// on top, helper in fmj_f64_mesh.inc) add the convex mesh branch of collide_plane to the narrow phase: up to four contacts at the
// deepest penetrating vertices of the geom, each with the normal of the ground under its own vertex.  The vertices are a double table
// in global memory (a seventh argument, F64Mesh) that the geom's lane reads; LDS is the terrain kernels'.  Once a contact is in its
// slot of the exchange list nothing tells it from any other: the rest of the step is the terrain (elliptic) kernels' unchanged.
//
// fmj_step_f64_terrain_rk4_kernel<LIMITS> and fmj_step_f64_elliptic_rk4_kernel<LIMITS> (fmj_create_ex2 with FMJ_CREATE_F64_CONTACTS |
// FMJ_CREATE_F64_CONTACTS_RK4 and a model that integrates with RK4; the terrain kernels' text, or the elliptic kernels', with
// F64_STEP_RK4 1 on top) run the four passes of mj_RungeKutta with contacts (oracle rk4): every pass runs the narrow phase at its own
// poses and solves its own limit and contact rows with H = M; the step leaves the first pass's sensors and the fourth pass's poses,
// qacc (the next warm start) and contact list, FMJ_WARN_CONTACTFULL is the OR over the passes, and a check that fails in any pass
// undoes the step before any of it - the contact list included - is stored.  The stage state (F64_RK4_LDS_DOUBLES) lies past the
// contacts' normals: dynamic LDS is ldsd_terrain_bytes + F64_RK4_LDS_DOUBLES(nu) * 8.  Planes need no FMJ_CREATE_F64_TERRAIN.

#define FMJ_F64_LANES 128
#define F64_BD 28      // doubles per body: pos(3) mass, quat(4), ipos(3) subtree mass, iquat(4), inertia(3) -, axis(3) qpos0, jnt_pos(3) stiffness
#define F64_BI 8       // ints per body: parent, joint type (-1 none), qpos address, dof address, subtree size, links row (-1 none), swimming slot (-1 none)
#define F64_DI 8       // ints per dof: body, depth, qpos address (-1: a free joint's dof), first actuator, actuator count, joint-sensor slot, joints row (-1 none)
#define F64_AD 8       // doubles per actuator (sorted by dof): gain, bias(3), ctrlrange(2), forcerange(2) (infinite where not limited)
#define F64_SW 10      // doubles per swimming slot: drag coefficients (3 force, 3 torque), mass, height, density, xfrc row
#define F64_LM 12      // doubles per dof of a limits context: limited (0 / 1), range(2), margin, solref(2), solimp(5), dof_invweight0
#define F64_GD 24      // doubles per geom of a contacts context: size(3), pos(3), quat(4), friction, invweight0 of its body + the world's, then F64_LM doubles laid out as a limit row's (margin 0, the geom's solref / solimp)
#define F64_GI 4       // ints per geom: type, body, last dof of the body's chain (-1: none), -
#define F64_PD 16      // doubles per plane: normal(3), point(3), tangents(6) (oracle add_contact's frame), friction, geom index
#define F64_CT 33      // doubles of LDS per contact: W of the four rows (24), D of the active rows (4), a row scalar for J' (4), body (the elliptic kernels: fmj_f64_elliptic.inc)
#define F64_TG 24      // doubles per ground entry of a terrain context: frame (9, row-major), point(3), friction, geom index, kind (0 plane, 1 heightfield), then a plane's tangents (6) or a heightfield's ncol, nrow, x / y radius, z scale, cells per metre in x / y
#define F64_TN 3       // doubles of LDS per contact that the terrain kernels add past the F64_CT records: the contact's normal

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

// What only the contacts kernels read (a fifth argument of theirs).  The solver's settings come in F64Limits, whose lm is NULL
// when the model has no limited joint.
struct F64Contacts {
  int ngeom, nplane, max_contacts;
  double sqrt_impratio;         // sqrt(impratio), 1 where the model names none
  const double* gd;             // [ngeom][F64_GD]
  const int* gi;                // [ngeom][F64_GI]
  const double* pd;             // [nplane][F64_PD]
};

// What only the terrain kernels read (a sixth argument of theirs; they read no F64Contacts.pd)
struct F64Terrain {
  const double* tg;             // [F64Contacts.nplane][F64_TG] the ground entries in geom order
  const double* hf;             // [nrow][ncol] the heightfield's samples (NULL without one)
};

// What only the mesh kernels read (a seventh argument of theirs)
struct F64Mesh {
  const double* mv;             // [nmeshvert][3] the vertices of every mesh geom in its geom's frame, unrounded
  const int* gv;                // [F64Contacts.ngeom][2] a geom's first vertex and vertex count (0, 0: no mesh)
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
// What the contacts kernels append after the LIMITS block (which they always have): F64_CT doubles per contact
__host__ __device__ inline int ldsd_contacts_bytes(int nb, int nv, int nq, int rs, int max_contacts) {
  return ldsd_total_bytes(nb, nv, nq, rs, 1) + max_contacts * F64_CT * 8;
}
// The terrain kernels: the normals of the contacts (F64_TN doubles each) past the records
__host__ __device__ inline int ldsd_terrain_bytes(int nb, int nv, int nq, int rs, int max_contacts) {
  return ldsd_contacts_bytes(nb, nv, nq, rs, max_contacts) + max_contacts * F64_TN * 8;
}
// What the RK4 kernels append after that: the first pass's actuator forces [nu] and controls [nu], kept until the step's fourth pass
// has passed its checks (each slot is written and read back by the one lane that owns the actuator's dof), then F64_RK4_ROWS rows of
// one double per lane: q0, v0, sum B v, sum B a, the first pass's limit force, linear (3) and angular (3) link velocity, and a row
// whose first seven doubles are the free root's q0
enum { F64_RK4_Q0 = 0, F64_RK4_V0 = 1, F64_RK4_SV = 2, F64_RK4_SA = 3, F64_RK4_LIM = 4, F64_RK4_LIN = 5, F64_RK4_ANG = 8, F64_RK4_ROOT = 11, F64_RK4_ROWS = 12 };
#define F64_RK4_LDS_DOUBLES(nu) (2 * (nu) + F64_RK4_ROWS * FMJ_F64_LANES)

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

// One candidate row (oracle make_constraints: get_impedance, mj_makeImpedance, mj_referenceConstraint): the impedance and the
// spring / damper of aref from the row's pos = dist.  lm: F64_LM doubles (a dof's, or the tail of a geom's F64_GD).
#define F64_MINVAL 1e-15
#define F64_MINIMP 0.0001
#define F64_MAXIMP 0.9999
__device__ __forceinline__ void f64_row_impedance(const double* lm, double h, double pos, double& imp, double& K, double& B) {
  const double margin = lm[3], sr0 = lm[4], sr1 = lm[5];
  const double dmin = fmin(fmax(lm[6], F64_MINIMP), F64_MAXIMP), dmax = fmin(fmax(lm[7], F64_MINIMP), F64_MAXIMP);
  const double width = fmax(0.0, lm[8]), mid = fmin(fmax(lm[9], F64_MINIMP), F64_MAXIMP), power = fmax(1.0, lm[10]);
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
  if (sr0 > 0.0) {
    const double tc = fmax(sr0, 2.0 * h);
    K = 1.0 / fmax(F64_MINVAL, dmax * dmax * tc * tc * sr1 * sr1);
    B = 2.0 / fmax(F64_MINVAL, dmax * tc);
  } else { K = -sr0 / fmax(F64_MINVAL, dmax * dmax); B = -sr1 / fmax(F64_MINVAL, dmax); }
}
// a limit row: D = 1 / R with the dof's invweight0 (lm[11]) and aref from vel = J qvel
__device__ __forceinline__ void f64_limit_row(const double* lm, double h, double pos, double vel, double& D, double& aref) {
  double imp, K, B;
  f64_row_impedance(lm, h, pos, imp, K, B);
  D = 1.0 / fmax(F64_MINVAL, (1.0 - imp) * lm[11] / imp);
  aref = -B * vel - K * imp * (pos - lm[3]);
}

// A point of the line search (oracle ls_pt): the cost along the search line and its first two derivatives
struct F64LsPt { double alpha, cost, d0, d1; };

// mj_integratePos of a free joint from q0 (position, quaternion) by h vel (vel: three linear, three angular), written to qp[0..6]
__device__ __forceinline__ void f64_integrate_free(double* qp, d3 p0, dq q0, const double* vel, double h) {
  qp[0] = p0.x + h * vel[0]; qp[1] = p0.y + h * vel[1]; qp[2] = p0.z + h * vel[2];
  d3 w = dmk(vel[3], vel[4], vel[5]);
  double nrm = sqrt(ddot(w, w));
  if (nrm < 1e-15) { w = dmk(1.0, 0.0, 0.0); nrm = 0.0; } else w = dmk(w.x / nrm, w.y / nrm, w.z / nrm);
  const dq qo = dqmul(dqnormalize(q0), daxisangle(w, h * nrm));
  qp[3] = qo.w; qp[4] = qo.x; qp[5] = qo.y; qp[6] = qo.z;
}

// The step's text (fmj_f64_step.inc), once per integrator family, and once more with ground contacts (on planes, or on terrain)
#define F64_STEP_KERNEL fmj_step_f64_kernel
#define F64_STEP_RK4 0
#define F64_STEP_CONTACTS 0
#define F64_STEP_TERRAIN 0
#define F64_STEP_ELLIPTIC 0
#define F64_STEP_MESH 0
#include "fmj_f64_step.inc"
#undef F64_STEP_KERNEL
#undef F64_STEP_RK4
#if FMJ_TU_F64 == 3
#define F64_STEP_KERNEL fmj_step_f64_rk4_kernel
#define F64_STEP_RK4 1
#include "fmj_f64_step.inc"
#undef F64_STEP_KERNEL
#undef F64_STEP_RK4
#endif
#undef F64_STEP_CONTACTS
#if FMJ_TU_F64 == 4
#include "fmj_f64_contacts.inc"
#define F64_STEP_KERNEL fmj_step_f64_contacts_kernel
#define F64_STEP_RK4 0
#define F64_STEP_CONTACTS 1
#include "fmj_f64_step.inc"
#undef F64_STEP_KERNEL
#undef F64_STEP_RK4
#undef F64_STEP_CONTACTS
#endif
#undef F64_STEP_TERRAIN
#if FMJ_TU_F64 == 5
#include "fmj_f64_contacts.inc"
#include "fmj_f64_terrain.inc"
#define F64_STEP_KERNEL fmj_step_f64_terrain_kernel
#define F64_STEP_RK4 0
#define F64_STEP_CONTACTS 1
#define F64_STEP_TERRAIN 1
#include "fmj_f64_step.inc"
#undef F64_STEP_KERNEL
#undef F64_STEP_RK4
#undef F64_STEP_CONTACTS
#undef F64_STEP_TERRAIN
#endif
#undef F64_STEP_ELLIPTIC
#if FMJ_TU_F64 == 6
#include "fmj_f64_contacts.inc"
#include "fmj_f64_terrain.inc"
#include "fmj_f64_elliptic.inc"
#define F64_STEP_KERNEL fmj_step_f64_elliptic_kernel
#define F64_STEP_RK4 0
#define F64_STEP_CONTACTS 1
#define F64_STEP_TERRAIN 1
#define F64_STEP_ELLIPTIC 1
#include "fmj_f64_step.inc"
#undef F64_STEP_KERNEL
#undef F64_STEP_RK4
#undef F64_STEP_CONTACTS
#undef F64_STEP_TERRAIN
#undef F64_STEP_ELLIPTIC
#endif
#undef F64_STEP_MESH
#if FMJ_TU_F64 == 7 || FMJ_TU_F64 == 8
#include "fmj_f64_contacts.inc"
#include "fmj_f64_terrain.inc"
#if FMJ_TU_F64 == 8
#include "fmj_f64_elliptic.inc"
#define F64_STEP_KERNEL fmj_step_f64_mesh_elliptic_kernel
#define F64_STEP_ELLIPTIC 1
#else
#define F64_STEP_KERNEL fmj_step_f64_mesh_kernel
#define F64_STEP_ELLIPTIC 0
#endif
#include "fmj_f64_mesh.inc"
#define F64_STEP_RK4 0
#define F64_STEP_CONTACTS 1
#define F64_STEP_TERRAIN 1
#define F64_STEP_MESH 1
#include "fmj_f64_step.inc"
#undef F64_STEP_KERNEL
#undef F64_STEP_RK4
#undef F64_STEP_CONTACTS
#undef F64_STEP_TERRAIN
#undef F64_STEP_ELLIPTIC
#undef F64_STEP_MESH
#endif
#if FMJ_TU_F64 == 9 || FMJ_TU_F64 == 10
#include "fmj_f64_contacts.inc"
#include "fmj_f64_terrain.inc"
#if FMJ_TU_F64 == 10
#include "fmj_f64_elliptic.inc"
#define F64_STEP_KERNEL fmj_step_f64_elliptic_rk4_kernel
#define F64_STEP_ELLIPTIC 1
#else
#define F64_STEP_KERNEL fmj_step_f64_terrain_rk4_kernel
#define F64_STEP_ELLIPTIC 0
#endif
#define F64_STEP_RK4 1
#define F64_STEP_CONTACTS 1
#define F64_STEP_TERRAIN 1
#define F64_STEP_MESH 0
#include "fmj_f64_step.inc"
#undef F64_STEP_KERNEL
#undef F64_STEP_RK4
#undef F64_STEP_CONTACTS
#undef F64_STEP_TERRAIN
#undef F64_STEP_ELLIPTIC
#undef F64_STEP_MESH
#endif

// -DFMJ_TU_F64: the two instantiations without limits; -DFMJ_TU_F64=2: the two LIMITS instantiations, a translation unit of their own;
// -DFMJ_TU_F64=3: the four RK4 instantiations, one more; -DFMJ_TU_F64=4: the two contacts kernels, one more; -DFMJ_TU_F64=5: the two
// terrain kernels, one more; -DFMJ_TU_F64=6: the two elliptic kernels, one more; -DFMJ_TU_F64=7 and =8: the two mesh kernels and the
// two mesh-elliptic kernels, one more each; -DFMJ_TU_F64=9 and =10: the two terrain kernels with the RK4 pass loop and the two elliptic
// ones, one more each.  Every getter takes (fused, limits); a unit without fused builds, or with one setting of LIMITS, does not read that argument.
// (a getter names only its own unit's instantiations: naming another would instantiate it here)
#if FMJ_TU_F64 == 10
extern "C" __attribute__((visibility("hidden"))) void* fmj_tu_f64_elliptic_rk4(int /*fused: no fused builds*/, int limits) {
  return limits ? (void*)fmj_step_f64_elliptic_rk4_kernel<true> : (void*)fmj_step_f64_elliptic_rk4_kernel<false>;
}
#elif FMJ_TU_F64 == 9
extern "C" __attribute__((visibility("hidden"))) void* fmj_tu_f64_terrain_rk4(int /*fused: no fused builds*/, int limits) {
  return limits ? (void*)fmj_step_f64_terrain_rk4_kernel<true> : (void*)fmj_step_f64_terrain_rk4_kernel<false>;
}
#elif FMJ_TU_F64 == 8
extern "C" __attribute__((visibility("hidden"))) void* fmj_tu_f64_mesh_elliptic(int /*fused: no fused builds*/, int limits) {
  return limits ? (void*)fmj_step_f64_mesh_elliptic_kernel<true> : (void*)fmj_step_f64_mesh_elliptic_kernel<false>;
}
#elif FMJ_TU_F64 == 7
extern "C" __attribute__((visibility("hidden"))) void* fmj_tu_f64_mesh(int /*fused: no fused builds*/, int limits) {
  return limits ? (void*)fmj_step_f64_mesh_kernel<true> : (void*)fmj_step_f64_mesh_kernel<false>;
}
#elif FMJ_TU_F64 == 6
extern "C" __attribute__((visibility("hidden"))) void* fmj_tu_f64_elliptic(int /*fused: no fused builds*/, int limits) {
  return limits ? (void*)fmj_step_f64_elliptic_kernel<true> : (void*)fmj_step_f64_elliptic_kernel<false>;
}
#elif FMJ_TU_F64 == 5
extern "C" __attribute__((visibility("hidden"))) void* fmj_tu_f64_terrain(int /*fused: no fused builds*/, int limits) {
  return limits ? (void*)fmj_step_f64_terrain_kernel<true> : (void*)fmj_step_f64_terrain_kernel<false>;
}
#elif FMJ_TU_F64 == 4
extern "C" __attribute__((visibility("hidden"))) void* fmj_tu_f64_contacts(int /*fused: no fused builds*/, int limits) {
  return limits ? (void*)fmj_step_f64_contacts_kernel<true> : (void*)fmj_step_f64_contacts_kernel<false>;
}
#elif FMJ_TU_F64 == 3
extern "C" __attribute__((visibility("hidden"))) void* fmj_tu_f64_rk4(int fused, int limits) {
  if (limits) return fused ? (void*)fmj_step_f64_rk4_kernel<true, true> : (void*)fmj_step_f64_rk4_kernel<false, true>;
  return fused ? (void*)fmj_step_f64_rk4_kernel<true, false> : (void*)fmj_step_f64_rk4_kernel<false, false>;
}
#elif FMJ_TU_F64 == 2
extern "C" __attribute__((visibility("hidden"))) void* fmj_tu_f64_limits(int fused, int /*limits: always*/) {
  return fused ? (void*)fmj_step_f64_kernel<true, true> : (void*)fmj_step_f64_kernel<false, true>;
}
#else
extern "C" __attribute__((visibility("hidden"))) void* fmj_tu_f64(int fused, int /*limits: never*/) {
  return fused ? (void*)fmj_step_f64_kernel<true, false> : (void*)fmj_step_f64_kernel<false, false>;
}
#endif
#endif  // FMJ_TU_F64
