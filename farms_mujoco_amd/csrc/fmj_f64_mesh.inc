// fmj_f64_mesh.inc - device helpers of fmj_step_f64_mesh_kernel and fmj_step_f64_mesh_elliptic_kernel (included by fmj_f64.inc in the
// -DFMJ_TU_F64=7 and =8 units, after fmj_f64_terrain.inc and ahead of the step's text; the description is in fmj_f64.inc): the convex
// mesh branch of the ground narrow phase.  Every statement is the oracle's (collide_plane, FMJ_GEOM_MESH of oracle/fmj_oracle.c) but
// its insertion into dq[4] / cq[4][3] / nq[4][3], which would index private arrays at run time: the selection below gives the same
// list.  No private array is indexed at run time.

// One geom against one ground entry: a mesh geom here, every other type in f64_terrain_contacts.  mv: the vertices of all meshes,
// [nmeshvert][3] doubles in the geom's frame; v0, nvert: the geom's first vertex and count (fmj_create held the range inside the table).
// Up to four contacts at the deepest penetrating vertices, deepest first, equal depths in vertex order; nothing when the ground under
// the geom's origin is farther than the bounding radius gd[2].  Each contact has the normal of the ground under its own vertex.
// The counting pass (out == NULL) is one sweep over the vertices.  The emitting pass finds contact k as the vertex with the smallest key
// (depth, index) above contact k - 1's key: one candidate's state per sweep, up to four sweeps, and the oracle's order, ties included.
__device__ __forceinline__ int f64_mesh_contacts(const double* gd, int type, d3 bpos, dq bquat, const double* tg, const double* hf,
                                                 const double* mv, int v0, int nvert, int g, int p, int base, int maxc, double* out) {
  if (type != FMJ_GEOM_MESH) return f64_terrain_contacts(gd, type, bpos, bquat, tg, hf, g, p, base, maxc, out);
  const dq lq = {gd[6], gd[7], gd[8], gd[9]};
  const dm33 gm = dq2m(dqmul(bquat, lq));
  const d3 gpos = dadd(bpos, dqrot(bquat, dmk(gd[3], gd[4], gd[5])));
  d3 n;
  const double dc = f64_ground_dist(tg, hf, gpos, n);
  if (!(dc < gd[2])) return 0;
  const double* V = mv + 3 * (size_t)v0;
  int cnt = 0;
  if (!out) {
#pragma unroll 1
    for (int vtx = 0; vtx < nvert; vtx++) {
      const d3 c = dadd(gpos, dmrot(gm, dmk(V[3 * vtx], V[3 * vtx + 1], V[3 * vtx + 2])));
      if (f64_ground_dist(tg, hf, c, n) < 0.0) cnt++;
    }
    return cnt < 4 ? cnt : 4;
  }
  double ptd = 0.0;      // the key of the contact before this one (none: pidx < 0)
  int pidx = -1;
#pragma unroll 1
  for (int k = 0; k < 4; k++) {
    double btd = 0.0;
    int bidx = -1;
    d3 bc = gpos, bn = n;
#pragma unroll 1
    for (int vtx = 0; vtx < nvert; vtx++) {
      const d3 c = dadd(gpos, dmrot(gm, dmk(V[3 * vtx], V[3 * vtx + 1], V[3 * vtx + 2])));
      d3 nn;
      const double td = f64_ground_dist(tg, hf, c, nn);
      if (!(td < 0.0)) continue;
      if (pidx >= 0 && !(td > ptd || (td == ptd && vtx > pidx))) continue;      // at or before contact k - 1 in the order
      if (bidx >= 0 && !(td < btd)) continue;                                   // (the sweep runs in vertex order: the first of equals stays)
      btd = td; bidx = vtx; bc = c; bn = nn;
    }
    if (bidx < 0) break;
    const int slot = base + cnt;
    if (slot < maxc) {
      double* o = out + slot * 8;
      const d3 pos = dsub(bc, dscl(bn, 0.5 * btd));
      o[0] = pos.x; o[1] = pos.y; o[2] = pos.z; o[3] = btd; o[4] = bn.x; o[5] = bn.y; o[6] = bn.z; o[7] = (double)(g * 128 + p);
    }
    cnt++;
    ptd = btd; pidx = bidx;
  }
  return cnt;
}
