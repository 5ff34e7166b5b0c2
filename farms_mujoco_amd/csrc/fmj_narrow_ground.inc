// fmj_narrow_ground.inc - narrow phase of one geom against one ground entry, shared by fmj_step_kernel (fmj_hip.hip, inside its
// loops over ground entries and geoms) and fmj_step_cons2_kernel (fmj_cons2.inc, its one ground entry): a block of statements on the
// including kernel's locals.
// Up to 4 contacts per geom: sphere 1, capsule 2 (segment ends), box the first 4 penetrating corners in corner order (what the
// oracle's collide_ground does), cylinder its rim points.  The convex-mesh block follows the include in the one-env kernel only.
// reads  M, PO, g (the lane's geom, may be >= M.ngeom), pn, pp (rows 0 and 1 of the ground entry);  updates cnt, rad, mu
// the includer supplies NP_PL (index of the ground entry) and NP_CQ / NP_NQ / NP_DQ (its arrays of 4 contact points, normals and
// distances, preset to (0, 0, 0), (0, 0, 1), 0): the first cnt entries are written
      if (g < M.ngeom) {
        const int4 gi = GTABI(g, 0);
        if (gi.x == FMJ_GEOM_SPHERE || gi.x == FMJ_GEOM_CAPSULE) {
          const float4 gs = GTAB(g, 1), gp = GTAB(g, 2), gq = GTAB(g, 3);
          const float4 bp = *(const float4*)(PO + gi.y * 8), bq = *(const float4*)(PO + gi.y * 8 + 4);
          const q4 bqq = {bq.x, bq.y, bq.z, bq.w};
          const v3 cen = add3(mk3(bp.x, bp.y, bp.z), qrot(bqq, mk3(gp.x, gp.y, gp.z)));
          rad = gs.x; mu = fmaxf(fmaxf(pp.x, gs.w), 1e-5f);
          v3 ax = mk3(0.f, 0.f, 0.f);
          if (gi.x == FMJ_GEOM_CAPSULE) { const q4 gqq = {gq.x, gq.y, gq.z, gq.w}; ax = scl3(qrot(qmul(bqq, gqq), mk3(0.f, 0.f, 1.f)), gs.y); }
          const v3 c0 = add3(cen, ax), c1 = sub3(cen, ax);
          v3 n0, n1;
          const float d0 = ground_dist(M, NP_PL, pn, pp, c0, &n0) - rad;
          const float d1 = ground_dist(M, NP_PL, pn, pp, c1, &n1) - rad;
          const bool a0 = d0 < 0.f, a1 = gi.x == FMJ_GEOM_CAPSULE && d1 < 0.f;
          if (a0) { NP_CQ[0] = c0; NP_DQ[0] = d0; NP_NQ[0] = n0; cnt = 1; }
          if (a1) { if (cnt == 0) { NP_CQ[0] = c1; NP_DQ[0] = d1; NP_NQ[0] = n1; } else { NP_CQ[1] = c1; NP_DQ[1] = d1; NP_NQ[1] = n1; } cnt++; }
        }
      }
      if (M.any_box) {
        const int4 gi = g < M.ngeom ? GTABI(g, 0) : make_int4(-1, 0, 0, 0);
        if (gi.x == FMJ_GEOM_BOX) {
          const float4 gs = GTAB(g, 1), gp = GTAB(g, 2), gq = GTAB(g, 3);
          const float4 bp = *(const float4*)(PO + gi.y * 8), bq = *(const float4*)(PO + gi.y * 8 + 4);
          const q4 bqq = {bq.x, bq.y, bq.z, bq.w}, gqq = {gq.x, gq.y, gq.z, gq.w};
          const q4 wq = qmul(bqq, gqq);
          const v3 cen = add3(mk3(bp.x, bp.y, bp.z), qrot(bqq, mk3(gp.x, gp.y, gp.z)));
          const v3 ex = scl3(qrot(wq, mk3(1.f, 0.f, 0.f)), gs.x), ey = scl3(qrot(wq, mk3(0.f, 1.f, 0.f)), gs.y), ez = scl3(qrot(wq, mk3(0.f, 0.f, 1.f)), gs.z);
          mu = fmaxf(fmaxf(pp.x, gs.w), 1e-5f);
#pragma unroll
          for (int corner = 0; corner < 8; corner++) {
            const v3 c = add3(add3(cen, (corner & 1) ? ex : scl3(ex, -1.f)), add3((corner & 2) ? ey : scl3(ey, -1.f), (corner & 4) ? ez : scl3(ez, -1.f)));
            v3 nc;
            const float d = ground_dist(M, NP_PL, pn, pp, c, &nc);
            const bool pen = d < 0.f && cnt < 4;
#pragma unroll
            for (int k = 0; k < 4; k++) if (pen && cnt == k) { NP_CQ[k] = c; NP_DQ[k] = d; NP_NQ[k] = nc; }
            cnt += pen ? 1 : 0;
          }
        }
        if (gi.x == FMJ_GEOM_CYLINDER) {      // rim points (the oracle's collide_ground, MuJoCo's mjc_PlaneCylinder construction)
          const float4 gs = GTAB(g, 1), gp = GTAB(g, 2), gq = GTAB(g, 3);
          const float4 bp = *(const float4*)(PO + gi.y * 8), bq = *(const float4*)(PO + gi.y * 8 + 4);
          const q4 bqq = {bq.x, bq.y, bq.z, bq.w}, gqq = {gq.x, gq.y, gq.z, gq.w};
          const q4 wq = qmul(bqq, gqq);
          const v3 cen = add3(mk3(bp.x, bp.y, bp.z), qrot(bqq, mk3(gp.x, gp.y, gp.z)));
          v3 nrm_;                                         // a heightfield is taken as the plane under the cylinder's centre
          const float dist = ground_dist(M, NP_PL, pn, pp, cen, &nrm_);
          v3 axis = qrot(wq, mk3(0.f, 0.f, 1.f));
          float prjaxis = dot3(nrm_, axis);
          if (prjaxis > 0.f) { axis = scl3(axis, -1.f); prjaxis = -prjaxis; }
          v3 vec = sub3(scl3(axis, prjaxis), nrm_);
          const float len2 = dot3(vec, vec);
          if (len2 >= 1e-30f) vec = scl3(vec, gs.x / sqrtf(len2)); else vec = scl3(qrot(wq, mk3(1.f, 0.f, 0.f)), gs.x);
          const float prjvec = dot3(vec, nrm_);
          axis = scl3(axis, gs.y); prjaxis *= gs.y;
          mu = fmaxf(fmaxf(pp.x, gs.w), 1e-5f);
          const float d0 = dist + prjaxis + prjvec;
          if (d0 < 0.f) {
            NP_CQ[0] = add3(cen, add3(vec, axis)); NP_DQ[0] = d0; cnt = 1;
            const float d1 = dist - prjaxis + prjvec;
            if (d1 < 0.f) { NP_CQ[1] = add3(cen, sub3(vec, axis)); NP_DQ[1] = d1; cnt = 2; }
            v3 vec1 = cross(vec, axis);
            const float l1 = sqrtf(dot3(vec1, vec1));
            if (l1 > 1e-15f) vec1 = scl3(vec1, gs.x * 0.8660254037844386f / l1);
            const float prjvec1 = dot3(vec1, nrm_);
#pragma unroll
            for (int sg = 0; sg < 2; sg++) {
              const float sgn = sg ? -1.f : 1.f;
              const float d2 = dist + prjaxis - 0.5f * prjvec + sgn * prjvec1;
              const v3 c2 = add3(cen, add3(scl3(vec1, sgn), sub3(axis, scl3(vec, 0.5f))));
              const bool pen = d2 < 0.f;
#pragma unroll
              for (int k = 1; k < 4; k++) if (pen && cnt == k) { NP_CQ[k] = c2; NP_DQ[k] = d2; }
              cnt += pen ? 1 : 0;
            }
          }
#pragma unroll
          for (int k = 0; k < 4; k++) NP_NQ[k] = nrm_;
        }
      }
