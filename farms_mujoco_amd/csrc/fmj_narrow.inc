// fmj_narrow.inc - collision helpers of the constraint kernels (fmj_step_kernel of fmj_hip.hip, fmj_step_cons2_kernel of
// fmj_cons2.inc), included once by fmj_hip.hip ahead of the kernels: device functions and one macro, no kernel locals.
// The narrow phase of one geom against one ground entry that both kernels run is fmj_narrow_ground.inc.

// ---- polytopes (box, cylinder, convex mesh) in explicit pairs: include/fmj.h (ABI 6), oracle poly_vertex / poly_signed / collide_pair
__device__ __forceinline__ bool geom_is_round(int t) { return t == FMJ_GEOM_SPHERE || t == FMJ_GEOM_CAPSULE; }
// vertex k of polytope (type, size row gs) in the geom frame
template <class MT>
__device__ __forceinline__ v3 poly_vertex(MT& M, int type, float4 gs, int k) {
  if (type == FMJ_GEOM_BOX) return mk3((k & 1) ? gs.x : -gs.x, (k & 2) ? gs.y : -gs.y, (k & 4) ? gs.z : -gs.z);
  if (type == FMJ_GEOM_CYLINDER) {          // 12 points on each rim in steps of 150 degrees, the first on +x; k < 12: the +z rim
    float sn, cs;
    sincospif((float)(((k % 12) * 5) % 12) * (1.0f / 6.0f), &sn, &cs);
    return mk3(gs.x * cs, gs.x * sn, k < 12 ? gs.y : -gs.y);
  }
  const float4 v = ldg4(M.mesh_vert, (unsigned)(__float_as_int(gs.x) + k));
  return mk3(v.x, v.y, v.z);
}
// signed distance of x (geom frame) to the polytope = max over its faces of (n . x - d), and that face's outward normal
template <class MT>
__device__ __forceinline__ float poly_signed(MT& M, int type, float4 gs, int face0, int nface, v3 x, v3* n) {
  if (type == FMJ_GEOM_BOX) {
    const float sx = fabsf(x.x) - gs.x, sy = fabsf(x.y) - gs.y, sz = fabsf(x.z) - gs.z;
    float s = sx; *n = mk3(x.x < 0.f ? -1.f : 1.f, 0.f, 0.f);
    if (sy > s) { s = sy; *n = mk3(0.f, x.y < 0.f ? -1.f : 1.f, 0.f); }
    if (sz > s) { s = sz; *n = mk3(0.f, 0.f, x.z < 0.f ? -1.f : 1.f); }
    return s;
  }
  if (type == FMJ_GEOM_CYLINDER) {
    const float r = sqrtf(x.x * x.x + x.y * x.y);
    float s = fabsf(x.z) - gs.y; *n = mk3(0.f, 0.f, x.z < 0.f ? -1.f : 1.f);
    if (r - gs.x > s) { s = r - gs.x; *n = r > 1e-15f ? mk3(x.x / r, x.y / r, 0.f) : mk3(1.f, 0.f, 0.f); }
    return s;
  }
  float s = -1e30f; *n = mk3(0.f, 0.f, 1.f);
  for (int f = 0; f < nface; f++) {
    const float4 pl = ldg4(M.mesh_face, (unsigned)(face0 + f));
    const float sf = pl.x * x.x + pl.y * x.y + pl.z * x.z - pl.w;
    if (sf > s) { s = sf; *n = mk3(pl.x, pl.y, pl.z); }
  }
  return s;
}
__device__ __forceinline__ float geom_rbound(int type, float4 gs) {
  return type == FMJ_GEOM_SPHERE ? gs.x : type == FMJ_GEOM_CAPSULE ? gs.x + gs.y : type == FMJ_GEOM_CYLINDER ? sqrtf(gs.x * gs.x + gs.y * gs.y)
       : type == FMJ_GEOM_BOX ? sqrtf(gs.x * gs.x + gs.y * gs.y + gs.z * gs.z) : gs.z;
}
// explicit pair (g1, g2) with at least one polytope: up to 4 contacts (position, normal from geom1 to geom2, distance), PO = body poses in LDS
template <class MT>
__device__ __forceinline__ int pair_polytope(MT& M, const float* PO, int g1, int g2, v3* cq, v3* nq, float* dq) {
  int type[2], face0[2], nface[2], nvert[2]; float4 gs[2]; v3 pos[2]; q4 wq[2], wqc[2];
#pragma unroll
  for (int k = 0; k < 2; k++) {
    const int g = k ? g2 : g1;
    const int4 gi = GTABI(g, 0);
    const float4 gp = GTAB(g, 2), gq = GTAB(g, 3);
    gs[k] = GTAB(g, 1);
    type[k] = gi.x; face0[k] = gi.w; nface[k] = __float_as_int(GTAB(g, 5).w);
    nvert[k] = gi.x == FMJ_GEOM_BOX ? 8 : gi.x == FMJ_GEOM_CYLINDER ? 24 : gi.x == FMJ_GEOM_MESH ? __float_as_int(gs[k].y) : 0;
    const float4 bp = *(const float4*)(PO + gi.y * 8), bq = *(const float4*)(PO + gi.y * 8 + 4);
    const q4 bqq = {bq.x, bq.y, bq.z, bq.w}, gqq = {gq.x, gq.y, gq.z, gq.w};
    wq[k] = qmul(bqq, gqq); wqc[k] = q4{wq[k].w, -wq[k].x, -wq[k].y, -wq[k].z};
    pos[k] = add3(mk3(bp.x, bp.y, bp.z), qrot(bqq, mk3(gp.x, gp.y, gp.z)));
  }
  const v3 dc = sub3(pos[1], pos[0]);
  if (sqrtf(dot3(dc, dc)) > geom_rbound(type[0], gs[0]) + geom_rbound(type[1], gs[1])) return 0;
  const bool r0 = geom_is_round(type[0]), r1 = geom_is_round(type[1]);
  int cnt = 0;
  if (r0 != r1) {                              // polytope against sphere / capsule: the round geom's centres against the faces
    const int rk = r0 ? 0 : 1, pk = 1 - rk;
    const float rad = gs[rk].x, half = gs[rk].y;
    const int ncen = type[rk] == FMJ_GEOM_CAPSULE ? 2 : 1;
    const v3 ax = qrot(wq[rk], mk3(0.f, 0.f, 1.f));
    for (int c = 0; c < ncen; c++) {
      const float sgn = ncen == 2 ? (c == 0 ? 1.f : -1.f) : 0.f;
      const v3 cw = add3(pos[rk], scl3(ax, sgn * half));
      v3 nl;
      const float dist = poly_signed(M, type[pk], gs[pk], face0[pk], nface[pk], qrot(wqc[pk], sub3(cw, pos[pk])), &nl) - rad;
      if (dist < 0.f) {
        const v3 nw = qrot(wq[pk], nl);
        const v3 cp = sub3(cw, scl3(nw, rad + 0.5f * dist)), n12 = pk == 0 ? nw : scl3(nw, -1.f);
#pragma unroll
        for (int q = 0; q < 2; q++) if (cnt == q) { cq[q] = cp; nq[q] = n12; dq[q] = dist; }
        cnt++;
      }
    }
    return cnt;
  }
  for (int side = 0; side < 2; side++) {       // side 0: geom1's vertices in geom2; side 1: geom2's vertices in geom1
    const int va = side, fb = 1 - side;
    for (int k = 0; k < nvert[va]; k++) {
      const v3 vw = add3(pos[va], qrot(wq[va], poly_vertex(M, type[va], gs[va], k)));
      v3 nl;
      float td = poly_signed(M, type[fb], gs[fb], face0[fb], nface[fb], qrot(wqc[fb], sub3(vw, pos[fb])), &nl);
      if (!(td < 0.f)) continue;
      const v3 nw = qrot(wq[fb], nl);
      v3 tc = sub3(vw, scl3(nw, 0.5f * td)), tn = fb == 0 ? nw : scl3(nw, -1.f);
      bool have = true;                          // insertion by depth, ties keep the earlier candidate (the rule of mesh against ground)
#pragma unroll
      for (int q = 0; q < 4; q++) {
        const bool empty = q >= cnt;
        if (have && (empty || td < dq[q])) {
          const float sd = dq[q]; const v3 sc = cq[q], sn = nq[q];
          dq[q] = td; cq[q] = tc; nq[q] = tn;
          td = sd; tc = sc; tn = sn;
          have = !empty;
        }
      }
      if (cnt < 4) cnt++;
    }
  }
  return cnt;
}

// Height of world point p above ground entry pl along the local surface normal, and that normal.  Plane: n . p - offset.
// Heightfield (MuJoCo hfield semantics: nrow x ncol samples over [-rx, rx] x [-ry, ry] of the geom frame, elevation = data *
// size z): the plane of the grid triangle under p (cells split along the diagonal (c, r) - (c + 1, r + 1)); nothing outside
// the grid.  PTAB(pl, 1).y != 0 marks a heightfield, PTAB(pl, 0) then holds its position, (pl, 2) its quaternion, (pl, 3)
// rx, ry, size z.
template <class MT>
__device__ __forceinline__ float ground_dist(MT& M, int pl, float4 pn, float4 pp, v3 p, v3* n) {
  if (pp.y == 0.f) { *n = mk3(pn.x, pn.y, pn.z); return dot3(p, *n) - pn.w; }
  const float4 hq = PTAB(pl, 2), hs = PTAB(pl, 3);
  const q4 q = {hq.x, hq.y, hq.z, hq.w}, qc = {hq.x, -hq.y, -hq.z, -hq.w};
  const v3 pl_ = qrot(qc, sub3(p, mk3(pn.x, pn.y, pn.z)));
  const int nc = M.hf_ncol, nr = M.hf_nrow;
  const float sx = (float)(nc - 1) / (2.f * hs.x), sy = (float)(nr - 1) / (2.f * hs.y);
  const float gx = (pl_.x + hs.x) * sx, gy = (pl_.y + hs.y) * sy;
  *n = qrot(q, mk3(0.f, 0.f, 1.f));
  if (!(gx >= 0.f && gx <= (float)(nc - 1) && gy >= 0.f && gy <= (float)(nr - 1))) return 1e30f;
  const int c = min((int)gx, nc - 2), r = min((int)gy, nr - 2);
  const float fx = gx - (float)c, fy = gy - (float)r;
  const float AS1* D = gptr(M.hf_data) + (size_t)r * nc + c;
  const float z00 = D[0] * hs.z, z10 = D[1] * hs.z, z01 = D[nc] * hs.z, z11 = D[nc + 1] * hs.z;
  float zs, gxs, gys;                                          // surface height under p and its slopes per cell
  if (fx >= fy) { gxs = z10 - z00; gys = z11 - z10; } else { gxs = z11 - z01; gys = z01 - z00; }
  zs = z00 + gxs * fx + gys * fy;
  const v3 nl = mk3(-gxs * sx, -gys * sy, 1.f);
  const float inv = 1.0f / sqrtf(dot3(nl, nl));
  *n = qrot(q, scl3(nl, inv));
  return (pl_.z - zs) * inv;                                   // n_z (p_z - z_surface)
}

// One contact record, 16 floats at CT + slot_ * 16: pos(3), frame(9): x = normal, t1 from (0,1,0) or (0,0,1) made orthogonal,
// t2 = n x t1 (mju_makeFrame), then dist, mu and two words of the site's own (z_, w_: packed integers or a float, as float values).
// pos_ may name nrm, the record's normal.  reads CT of the including kernel; the guard on the slot stays at the site.
#define CONTACT_RECORD(slot_, nrm_, pos_, dist_, mu_, z_, w_) do { \
    const v3 nrm = (nrm_); \
    v3 t1 = (nrm.y < -0.5f || nrm.y > 0.5f) ? mk3(0.f, 0.f, 1.f) : mk3(0.f, 1.f, 0.f); \
    t1 = sub3(t1, scl3(nrm, dot3(t1, nrm))); \
    t1 = scl3(t1, 1.0f / sqrtf(dot3(t1, t1))); \
    const v3 t2 = cross(nrm, t1); \
    const v3 pos = (pos_); \
    float* ct = CT + (slot_) * 16; \
    *(float4*)(ct) = make_float4(pos.x, pos.y, pos.z, nrm.x); \
    *(float4*)(ct + 4) = make_float4(nrm.y, nrm.z, t1.x, t1.y); \
    *(float4*)(ct + 8) = make_float4(t1.z, t2.x, t2.y, t2.z); \
    *(float4*)(ct + 12) = make_float4((dist_), (mu_), (z_), (w_)); } while (0)
