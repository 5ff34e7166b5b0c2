// fmj_stage_m.inc - step stage shared by fmj_step_kernel (fmj_hip.hip) and fmj_step_wide_kernel (fmj_wide.inc): a block of
// statements on the including kernel's locals.
// The including kernel defines, and undefines after the include, how a dof finds the lanes of its ancestors:
//   MROW_ANCL          the table: per dof and depth one byte that names the ancestor at that depth
//   MROW_LANE(byte_)   the ancestor's lane from that byte
// reads  cd, bf, sc, d_prm, dvel, isd, dlo, CD
// defines hrow, hdg_m, hdg_h (the two-wave kernel has no use for hdg_m: the compiler drops it)
    // ---- M: row i of M (lane = dof i), one entry per depth of the chain root -> i, born in registers:
    //      M[i][j] = w_j . (I_s w_i) + v_j(s) . (m v_i(s)), s = CoM of the subtree dof i moves, j = ancestor of i at that depth;
    //      v_j(s) = v_j + w_j x sc, so M[i][j] = w_j . (I_s w_i + sc x p_i) + v_j . p_i with p_i = m v_i(s): the bracket gi is
    //      the lane's own and an entry costs two dot products.  Slots at and past the lane's own depth hold finite values
    //      that are never read as matrix entries (beyond the chain the table names the lane itself); the diagonals live in
    //      hdg_m (+ armature) and hdg_h (+ armature + h damping).  Lanes without a dof have cd = 0: their rows are zero.
    f2_t hrow[MAXD / 2];
    float hdg_m, hdg_h;
    {
      const v3 gi = add3(bf.r, cross(sc, bf.l));
      const float mii = dot3(cd.r, gi) + dot3(cd.l, bf.l);
      hdg_m = isd ? mii + d_prm.x : 1.f;
      hdg_h = isd ? mii + (d_prm.x + M.hdamp * (d_prm.y + dvel)) : 1.f;
      const int maxdep = M.maxdep1;
#pragma unroll
      for (int g = 0; g < MAXD / 4; g++) {
        const uint32_t ab = gptr(MROW_ANCL)[(unsigned)dlo * (MAXD / 4) + g];
#pragma unroll
        for (int k = 0; k < 4; k++) {
          const int d = 4 * g + k;
          float mij = 0.f;
          if (d <= maxdep) {                        // uniform test, static register index
            const int al = MROW_LANE((ab >> (8 * k)) & 0xffu);      // lane = dof of the ancestor at depth d
            const s6 cdj = lds_get6(CD + al * 8);
            mij = dot3(cdj.r, gi) + dot3(cdj.l, bf.l);
          }
          if (k & 1) hrow[d / 2].y = mij; else hrow[d / 2].x = mij;
        }
      }
    }
