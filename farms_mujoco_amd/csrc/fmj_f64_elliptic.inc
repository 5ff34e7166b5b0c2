// fmj_f64_elliptic.inc - device helpers of fmj_step_f64_elliptic_kernel (included by fmj_f64.inc in the -DFMJ_TU_F64=6 unit, after
// fmj_f64_contacts.inc and fmj_f64_terrain.inc and ahead of the step's text; the description is in fmj_f64.inc): the three zones of the
// elliptic friction cone on the primal side and the subtree sums that stand for the products with J_c and J_c' Hc J_c.  Written from
// oracle/fmj_oracle.c's statements in their order.  No private array is indexed at run time.
//
// The LDS record of a contact keeps the stride of the pyramid kernels' (F64_CT doubles):
//    0..17  W of the three rows: normal, tangent 1, tangent 2 (unscaled by the friction)
//   18..23  Hc, the 3 x 3 Hessian of the cone's cost at the iterate, symmetric: 00 01 02 11 12 22
//   24..26  a row scalar for J': the force of the row, or (Hc J p) of the row
//   27      the zone (0 top, 1 bottom, 2 middle)
//   28..31  -
//   32      body

// oracle cone_zone: jar = (j0, j1, j2) the residuals of one contact's rows, D0 = 1 / R of the normal row, mu = friction / sqrt(impratio),
// fr = the friction coefficient of the tangents.  Gives the cost, the three forces and the six entries of Hc = d2 cost / d jar2;
// returns the zone (0 top: no force; 1 bottom: three quadratic rows; 2 middle: the cone's surface).
__device__ __forceinline__ int f64_cone_zone(double j0, double j1, double j2, double D0, double mu, double fr, double& cost,
                                             double& f0, double& f1, double& f2,
                                             double& h00, double& h01, double& h02, double& h11, double& h12, double& h22) {
  const double U1 = j1 * fr, U2 = j2 * fr;
  const double N = j0 * mu, T = sqrt(U1 * U1 + U2 * U2);
  f0 = f1 = f2 = 0.0;
  h00 = h01 = h02 = h11 = h12 = h22 = 0.0;
  cost = 0.0;
  if (N >= mu * T || (T <= 0.0 && N >= 0.0)) return 0;
  if (mu * N + T <= 0.0 || (T <= 0.0 && N < 0.0)) {
    const double Dt = D0 * fr * fr / (mu * mu);
    cost += 0.5 * D0 * j0 * j0; cost += 0.5 * Dt * j1 * j1; cost += 0.5 * Dt * j2 * j2;
    f0 = -D0 * j0; f1 = -Dt * j1; f2 = -Dt * j2;
    h00 = D0; h11 = Dt; h22 = Dt;
    return 1;
  }
  const double Dm = D0 / (mu * mu * (1.0 + mu * mu)), NmT = N - mu * T;
  cost = 0.5 * Dm * NmT * NmT;
  f0 = -Dm * NmT * mu; f1 = -f0 / T * U1 * fr; f2 = -f0 / T * U2 * fr;
  // a = d(N - mu T) / d jar; d2 T / d jar_a d jar_b = fr^2 delta_ab / T - fr^4 jar_a jar_b / T^3 on the tangents
  const double a0 = mu, a1 = -mu * fr * U1 / T, a2 = -mu * fr * U2 / T;
  h00 = Dm * a0 * a0; h01 = Dm * a0 * a1; h02 = Dm * a0 * a2; h11 = Dm * a1 * a1; h12 = Dm * a1 * a2; h22 = Dm * a2 * a2;
  const double k = -Dm * NmT * mu;      // > 0 in the middle zone
  h11 += k * (fr * fr / T - fr * fr * U1 * U1 / (T * T * T));
  h12 += k * (0.0 - fr * fr * U1 * U2 / (T * T * T));
  h22 += k * (fr * fr / T - fr * fr * U2 * U2 / (T * T * T));
  return 2;
}

// The elliptic twin of f64_contact_subtree: the contacts whose body lies in the depth-first range [b0, b1], from their LDS records:
//   f:  sum_a F_a W_a                        (F_a at record + 24: the force of row a, or (Hc J p)_a)   -> cdof_i . f = (J' F)_i
//   k:  sum_ab Hc[a][b] (W_a . cd) W_b       (Hc at record + 18; zero in the top zone)                  -> the contact stiffness of row i
__device__ __forceinline__ void f64_elliptic_subtree(const double* CT, int ncon, int b0, int b1, d6 cd, bool want_k, d6& f, d6& k) {
  const d3 z3 = dmk(0.0, 0.0, 0.0);
  f.r = f.l = z3; k.r = k.l = z3;
#pragma unroll 1
  for (int c = 0; c < ncon; c++) {
    const double* ct = CT + c * F64_CT;
    const int cb = (int)ct[32];
    if (cb < b0 || cb > b1) continue;
    double w0 = 0.0, w1 = 0.0, w2 = 0.0;      // W_a . cd
    const bool stiff = want_k && ct[27] != 0.0;
    { const d6 W = dget6(ct); f = d6add(f, d6scl(W, ct[24])); if (stiff) w0 = d6dot(W, cd); }
    { const d6 W = dget6(ct + 6); f = d6add(f, d6scl(W, ct[25])); if (stiff) w1 = d6dot(W, cd); }
    { const d6 W = dget6(ct + 12); f = d6add(f, d6scl(W, ct[26])); if (stiff) w2 = d6dot(W, cd); }
    if (stiff) {
      k = d6add(k, d6scl(dget6(ct), ct[18] * w0 + ct[19] * w1 + ct[20] * w2));
      k = d6add(k, d6scl(dget6(ct + 6), ct[19] * w0 + ct[21] * w1 + ct[22] * w2));
      k = d6add(k, d6scl(dget6(ct + 12), ct[20] * w0 + ct[22] * w1 + ct[23] * w2));
    }
  }
}
