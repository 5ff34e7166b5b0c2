// fmj_f64_terrain.inc - device helpers of fmj_step_f64_terrain_kernel (included by fmj_f64.inc in the -DFMJ_TU_F64=5 unit, after
// fmj_f64_contacts.inc and ahead of the step's text; the description is in fmj_f64.inc): the ground narrow phase of the contacts
// kernels with the ground's normal a per-contact quantity - a heightfield beside the planes, cylinders beside sphere / capsule / box.
// Every statement is the oracle's (ground_dist, collide_plane, add_contact of oracle/fmj_oracle.c), in its order.  No private array
// is indexed at run time.

// Height of the world point pt above the ground entry tg (F64_TG doubles) along the local surface normal n (oracle ground_dist).
// Heightfield: the plane of the grid triangle under the point, cells split along the diagonal (c, r) - (c + 1, r + 1); 1e30 outside
// the grid.  hf: the samples, [nrow][ncol]; the cell indices are clamped to [0, ncol - 2] x [0, nrow - 2], so the four reads stay
// inside the table.
__device__ __forceinline__ double f64_ground_dist(const double* tg, const double* hf, d3 pt, d3& n) {
  const d3 dif = dsub(pt, dmk(tg[9], tg[10], tg[11]));
  n = dmk(tg[2], tg[5], tg[8]);
  if (tg[14] == 0.0) return ddot(dif, n);
  const double lx = tg[0] * dif.x + tg[3] * dif.y + tg[6] * dif.z, ly = tg[1] * dif.x + tg[4] * dif.y + tg[7] * dif.z,
               lz = tg[2] * dif.x + tg[5] * dif.y + tg[8] * dif.z;
  const int nc = (int)tg[15], nr = (int)tg[16];
  const double rx = tg[17], ry = tg[18], zt = tg[19], sx = tg[20], sy = tg[21];
  const double gx = (lx + rx) * sx, gy = (ly + ry) * sy;
  if (!(gx >= 0.0 && gx <= nc - 1 && gy >= 0.0 && gy <= nr - 1)) return 1e30;
  int c = (int)gx, r = (int)gy;
  if (c > nc - 2) c = nc - 2;
  if (r > nr - 2) r = nr - 2;
  const double fx = gx - c, fy = gy - r;
  const double* D = hf + (size_t)r * nc + c;
  const double z00 = D[0] * zt, z10 = D[1] * zt, z01 = D[nc] * zt, z11 = D[nc + 1] * zt;
  double gxs, gys;
  if (fx >= fy) { gxs = z10 - z00; gys = z11 - z10; } else { gxs = z11 - z01; gys = z01 - z00; }
  const double zs = z00 + gxs * fx + gys * fy;
  d3 nl = dmk(-gxs * sx, -gys * sy, 1.0);
  const double inv = 1.0 / sqrt(ddot(nl, nl));
  nl = dscl(nl, inv);
  n = dmk(tg[0] * nl.x + tg[1] * nl.y + tg[2] * nl.z, tg[3] * nl.x + tg[4] * nl.y + tg[5] * nl.z, tg[6] * nl.x + tg[7] * nl.y + tg[8] * nl.z);
  return (lz - zs) * inv;
}

// The tangents of a contact with normal n (oracle add_contact, mju_makeFrame)
__device__ __forceinline__ void f64_contact_frame(d3 n, d3& t1, d3& t2) {
  d3 t = (n.y < -0.5 || n.y > 0.5) ? dmk(0.0, 0.0, 1.0) : dmk(0.0, 1.0, 0.0);
  const double d = ddot(t, n);
  t = dsub(t, dscl(n, d));
  const double nn = sqrt(ddot(t, t));
  t1 = dmk(t.x / nn, t.y / nn, t.z / nn);
  t2 = dcross(n, t1);
}

// One geom against one ground entry (oracle collide_plane with margin 0: sphere, capsule: its two end spheres, cylinder: up to four rim
// points against the plane under its centre, box: the first four penetrating corners in corner order).  bpos / bquat: the pose of the
// geom's body.  Returns the number of contacts; with out != NULL the contact k goes to slot base + k where that is below maxc:
// 8 doubles, pos(3), dist, normal(3), geom * 128 + ground entry (both below 128).
__device__ __forceinline__ int f64_terrain_contacts(const double* gd, int type, d3 bpos, dq bquat, const double* tg, const double* hf,
                                                    int g, int p, int base, int maxc, double* out) {
  const dq lq = {gd[6], gd[7], gd[8], gd[9]};
  const dm33 gm = dq2m(dqmul(bquat, lq));
  const d3 gpos = dadd(bpos, dqrot(bquat, dmk(gd[3], gd[4], gd[5])));
  int cnt = 0;
  const auto emit = [&](d3 pos, d3 n, double dist) {
    const int slot = base + cnt;
    if (out && slot < maxc) {
      double* o = out + slot * 8;
      o[0] = pos.x; o[1] = pos.y; o[2] = pos.z; o[3] = dist; o[4] = n.x; o[5] = n.y; o[6] = n.z; o[7] = (double)(g * 128 + p);
    }
    cnt++;
  };
  d3 n;
  if (type == FMJ_GEOM_SPHERE || type == FMJ_GEOM_CAPSULE) {
    const int nseg = type == FMJ_GEOM_CAPSULE ? 2 : 1;
#pragma unroll 1
    for (int s = 0; s < nseg; s++) {
      const double sgn = nseg == 2 ? (s == 0 ? 1.0 : -1.0) : 0.0;
      const d3 c = dadd(gpos, dmk(sgn * gd[1] * gm.a2, sgn * gd[1] * gm.a5, sgn * gd[1] * gm.a8));
      const double dist = f64_ground_dist(tg, hf, c, n) - gd[0];
      if (dist < 0.0) emit(dsub(c, dscl(n, gd[0] + 0.5 * dist)), n, dist);
    }
  } else if (type == FMJ_GEOM_CYLINDER) {
    d3 axis = dmk(gm.a2, gm.a5, gm.a8);
    const double dist = f64_ground_dist(tg, hf, gpos, n);
    double prjaxis = ddot(n, axis);
    if (prjaxis > 0.0) { axis = dmk(-axis.x, -axis.y, -axis.z); prjaxis = -prjaxis; }
    d3 vec = dsub(dscl(axis, prjaxis), n);
    const double len2 = ddot(vec, vec);
    if (len2 >= 1e-30) vec = dscl(vec, gd[0] / sqrt(len2));
    else vec = dmk(gm.a0 * gd[0], gm.a3 * gd[0], gm.a6 * gd[0]);      // the axis along the normal: any rim direction, the geom's x
    const double prjvec = ddot(vec, n);
    axis = dscl(axis, gd[1]);
    prjaxis *= gd[1];
    const double d0 = dist + prjaxis + prjvec;
    if (d0 < 0.0) {
      emit(dsub(dadd(dadd(gpos, vec), axis), dscl(n, 0.5 * d0)), n, d0);
      const double d1 = dist - prjaxis + prjvec;
      if (d1 < 0.0) emit(dsub(dsub(dadd(gpos, vec), axis), dscl(n, 0.5 * d1)), n, d1);
      d3 vec1 = dcross(vec, axis);
      const double l1 = sqrt(ddot(vec1, vec1));
      if (l1 > 1e-15) vec1 = dscl(vec1, gd[0] * 0.8660254037844386 / l1);
      const double prjvec1 = ddot(vec1, n);
      const double d2 = dist + prjaxis - 0.5 * prjvec + prjvec1;
      if (d2 < 0.0) emit(dsub(dsub(dadd(dadd(gpos, vec1), axis), dscl(vec, 0.5)), dscl(n, 0.5 * d2)), n, d2);
      const double d3m = dist + prjaxis - 0.5 * prjvec - prjvec1;
      if (d3m < 0.0) emit(dsub(dsub(dadd(dsub(gpos, vec1), axis), dscl(vec, 0.5)), dscl(n, 0.5 * d3m)), n, d3m);
    }
  } else if (type == FMJ_GEOM_BOX) {
#pragma unroll 1
    for (int corner = 0; corner < 8 && cnt < 4; corner++) {
      const d3 loc = dmk((corner & 1) ? gd[0] : -gd[0], (corner & 2) ? gd[1] : -gd[1], (corner & 4) ? gd[2] : -gd[2]);
      const d3 c = dadd(gpos, dmrot(gm, loc));
      const double dist = f64_ground_dist(tg, hf, c, n);
      if (dist < 0.0) emit(dsub(c, dscl(n, 0.5 * dist)), n, dist);
    }
  }
  return cnt;
}
