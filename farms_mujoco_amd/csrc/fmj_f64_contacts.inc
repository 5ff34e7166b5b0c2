// fmj_f64_contacts.inc - device helpers of fmj_step_f64_contacts_kernel (included by fmj_f64.inc in the -DFMJ_TU_F64=4 unit, ahead of
// the step's text; the description is in fmj_f64.inc): the ground narrow phase in double, the workgroup prefix sum that orders the
// contacts, the chain and subtree sums that stand for the products with J.  No private array is indexed at run time.

// Exclusive prefix sum of v over the workgroup's lanes and the total, on every lane.  buf: two ints of LDS; a barrier has to separate
// two calls.
__device__ __forceinline__ int wg_scan_excl(int v, int* buf, int& total) {
  const int l = threadIdx.x & 63;
  int s = v;
#pragma unroll
  for (int o = 1; o < 64; o <<= 1) { const int t = __shfl_up(s, o, 64); if (l >= o) s += t; }
  if (l == 63) buf[threadIdx.x >> 6] = s;
  __syncthreads();
  const int w0 = buf[0], w1 = buf[1];
  total = w0 + w1;
  return s - v + ((threadIdx.x >> 6) ? w0 : 0);
}

// One geom against one plane (oracle collide_plane with margin 0: sphere, capsule: its two end spheres, box: the first four penetrating
// corners in corner order).  bpos / bquat: the pose of the geom's body.  Returns the number of contacts; with out != NULL the contact
// k goes to slot base + k where that is below maxc: 8 doubles, pos(3), dist, geom, plane.
__device__ __forceinline__ int f64_ground_contacts(const double* gd, int type, d3 bpos, dq bquat, const double* pd, int g, int p,
                                                   int base, int maxc, double* out) {
  const dq lq = {gd[6], gd[7], gd[8], gd[9]};
  const dm33 gm = dq2m(dqmul(bquat, lq));
  const d3 gpos = dadd(bpos, dqrot(bquat, dmk(gd[3], gd[4], gd[5])));
  const d3 n = dmk(pd[0], pd[1], pd[2]), pp = dmk(pd[3], pd[4], pd[5]);
  int cnt = 0;
  const auto emit = [&](d3 c, double dist, double r) {
    if (dist < 0.0) {
      const int slot = base + cnt;
      if (out && slot < maxc) {
        const d3 pos = dsub(c, dscl(n, r + 0.5 * dist));
        double* o = out + slot * 8;
        o[0] = pos.x; o[1] = pos.y; o[2] = pos.z; o[3] = dist; o[4] = (double)g; o[5] = (double)p;
      }
      cnt++;
    }
  };
  if (type == FMJ_GEOM_SPHERE || type == FMJ_GEOM_CAPSULE) {
    const int nseg = type == FMJ_GEOM_CAPSULE ? 2 : 1;
    for (int s = 0; s < nseg; s++) {
      const double sgn = nseg == 2 ? (s == 0 ? 1.0 : -1.0) : 0.0;
      const d3 c = dadd(gpos, dmk(sgn * gd[1] * gm.a2, sgn * gd[1] * gm.a5, sgn * gd[1] * gm.a8));
      emit(c, ddot(dsub(c, pp), n) - gd[0], gd[0]);
    }
  } else if (type == FMJ_GEOM_BOX) {
#pragma unroll 1
    for (int corner = 0; corner < 8 && cnt < 4; corner++) {
      const d3 loc = dmk((corner & 1) ? gd[0] : -gd[0], (corner & 2) ? gd[1] : -gd[1], (corner & 4) ? gd[2] : -gd[2]);
      const d3 c = dadd(gpos, dmrot(gm, loc));
      emit(c, ddot(dsub(c, pp), n), 0.0);
    }
  }
  return cnt;
}

// sum of cdof_j x_j over the dof chain that ends in dof ld (x: nv doubles of LDS): the spatial velocity / acceleration whose product
// with W_e is J_e x
__device__ __forceinline__ d6 f64_chain_sum(const double* CD, const double* x, const uint8_t* danc, int rs, int ld, int depth) {
  d6 s = d6scl(dget6(CD + ld * 6), x[ld]);
  const uint8_t* an = danc + (size_t)ld * rs;
#pragma unroll 1
  for (int d = depth - 1; d >= 0; d--) { const int j = an[d]; s = d6add(s, d6scl(dget6(CD + j * 6), x[j])); }
  return s;
}

// The contacts whose body lies in the depth-first range [b0, b1] (the subtree of a dof's body), from their LDS records:
//   f:  sum_e F_e W_e              (F_e at record + 28: the force of row e, or D_e J_e p)       -> cdof_i . f = (J' F)_i
//   k:  sum_e D_e (W_e . cd) W_e   (D_e of the active rows at record + 24)                       -> the contact stiffness of row i
__device__ __forceinline__ void f64_contact_subtree(const double* CT, int ncon, int b0, int b1, d6 cd, bool want_k, d6& f, d6& k) {
  const d3 z3 = dmk(0.0, 0.0, 0.0);
  f.r = f.l = z3; k.r = k.l = z3;
#pragma unroll 1
  for (int c = 0; c < ncon; c++) {
    const double* ct = CT + c * F64_CT;
    const int cb = (int)ct[32];
    if (cb < b0 || cb > b1) continue;
#pragma unroll 1
    for (int r = 0; r < 4; r++) {
      const d6 W = dget6(ct + 6 * r);
      f = d6add(f, d6scl(W, ct[28 + r]));
      if (want_k) { const double D = ct[24 + r]; if (D != 0.0) k = d6add(k, d6scl(W, D * d6dot(W, cd))); }
    }
  }
}
