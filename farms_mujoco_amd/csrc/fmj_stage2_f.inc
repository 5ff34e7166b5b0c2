// fmj_stage2_f.inc - step stage shared by the two-env kernel (fmj_dual2.inc) and the two-env constraint kernel (fmj_cons2.inc): a block
// of statements on the including kernel's locals.
// F: the inertial part of the body force about the tree CoM, cinert * cacc + cvel x* (cinert * cvel) with cinert = {iw, dcom, mass}; the
// kernel subtracts the external force (its xf: carried across the steps in fmj_dual2.inc, re-read at that point in fmj_cons2.inc).
// reads  dcom, mass, iw, ca, cv
// defines f
      s6 ia, iv;
      ia.l = scl3(add3(ca.l, cross(ca.r, dcom)), mass);
      ia.r = add3(mk3(iw[0] * ca.r.x + iw[3] * ca.r.y + iw[4] * ca.r.z, iw[3] * ca.r.x + iw[1] * ca.r.y + iw[5] * ca.r.z,
                      iw[4] * ca.r.x + iw[5] * ca.r.y + iw[2] * ca.r.z), cross(dcom, ia.l));
      iv.l = scl3(add3(cv.l, cross(cv.r, dcom)), mass);
      iv.r = add3(mk3(iw[0] * cv.r.x + iw[3] * cv.r.y + iw[4] * cv.r.z, iw[3] * cv.r.x + iw[1] * cv.r.y + iw[5] * cv.r.z,
                      iw[4] * cv.r.x + iw[5] * cv.r.y + iw[2] * cv.r.z), cross(dcom, iv.l));
      s6 f = s6add(ia, cross_force(cv, iv));
