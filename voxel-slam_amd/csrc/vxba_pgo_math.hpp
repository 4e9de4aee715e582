// Per-factor arithmetic of the pose-graph optimiser (include/vxba.h: vxba_pgo_*), host + device: the kernels of vxba_pgo.hip run it on
// the GPU, tests/hostmath/pgo_hostcheck.cpp compiles the same text with g++ for the CPU suite.
//
// Factors (GTSAM's BetweenFactor<Pose3> / PriorFactor<Pose3> with diagonal variances under the default Pose3 chart: rotation through
// the SO(3) logarithm, translation as is):
//   between (i, j, Z = (Zr, zt)):  e = [Log(Zr^T R_i^T R_j) ; Zr^T (R_i^T (p_j - p_i) - zt)]
//   prior   (i, Z):                e = [Log(Zr^T R_i)       ; Zr^T (p_i - zt)]
// Update (the library's): R <- R Exp(dphi), p <- p + dp; tangent order [dphi(3); dp(3)].  With it
//   de_R/dphi_j = Jr^-1(e_R)            de_R/dphi_i = -Jr^-1(e_R) R_j^T R_i
//   de_t/dphi_i = Zr^T hat(R_i^T (p_j - p_i))     de_t/dp_i = -Zr^T R_i^T     de_t/dp_j = Zr^T R_i^T
// (tests/test_pgo_cpu.py holds them against central differences).  Angles near pi are out of scope: no pose-graph residual is half a
// turn, and Log's th / sin(th) has its pole there.
//
// Layouts: a pose record is [R column-major 9 | p 3] as everywhere in the ABI; a measurement record is [Zr ROW-major 9 | zt 3] -- the
// first 12 doubles of the edge record vxba_hba_pass writes; 3 x 3 and 6 x 6 matrices in here are row-major.
#pragma once
#include <math.h>

#if defined(__HIPCC__)
#define VXP_HD __host__ __device__ __forceinline__
#define VXP_UNROLL _Pragma("unroll")
#else
#define VXP_HD inline
#define VXP_UNROLL
#endif

namespace vxpgo {

// rotation of a pose record as a row-major 3 x 3
VXP_HD void pose_R(const double* P, double R[9]) {
  VXP_UNROLL for (int r = 0; r < 3; r++) {
    VXP_UNROLL for (int c = 0; c < 3; c++) R[3 * r + c] = P[3 * c + r];
  }
}
// C = A^T B
VXP_HD void mul_tn(const double A[9], const double B[9], double C[9]) {
  VXP_UNROLL for (int r = 0; r < 3; r++) {
    VXP_UNROLL for (int c = 0; c < 3; c++) C[3 * r + c] = A[r] * B[c] + A[3 + r] * B[3 + c] + A[6 + r] * B[6 + c];
  }
}
// C = A B
VXP_HD void mul_nn(const double A[9], const double B[9], double C[9]) {
  VXP_UNROLL for (int r = 0; r < 3; r++) {
    VXP_UNROLL for (int c = 0; c < 3; c++) C[3 * r + c] = A[3 * r] * B[c] + A[3 * r + 1] * B[3 + c] + A[3 * r + 2] * B[6 + c];
  }
}
// y = A^T x
VXP_HD void mulv_t(const double A[9], const double x[3], double y[3]) {
  VXP_UNROLL for (int r = 0; r < 3; r++) y[r] = A[r] * x[0] + A[3 + r] * x[1] + A[6 + r] * x[2];
}

// Log of a rotation, accurate at the residual angles of a converged graph (1e-9 .. 1e-3 rad): the angle from atan2(|k|, (tr - 1) / 2)
// with k the vector of the skew part (= sin(th) axis), never from acos of the trace; th / sin(th) by its series below 1e-6 rad.
VXP_HD void so3_log(const double R[9], double w[3]) {
  const double kx = 0.5 * (R[7] - R[5]), ky = 0.5 * (R[2] - R[6]), kz = 0.5 * (R[3] - R[1]);
  const double s = sqrt(kx * kx + ky * ky + kz * kz);
  const double th = atan2(s, 0.5 * (R[0] + R[4] + R[8] - 1.0));
  const double f = th < 1e-6 ? 1.0 + th * th * (1.0 / 6.0) : th / s;
  w[0] = f * kx; w[1] = f * ky; w[2] = f * kz;
}

// Inverse right Jacobian of SO(3): I + hat(w) / 2 + c(a) hat(w)^2, c = 1 / a^2 - (1 + cos a) / (2 a sin a), a = |w|; below 1e-2 rad the
// closed form cancels (two terms of 1 / a^2 leaving 1 / 12), so the series 1/12 + a^2/720 + a^4/30240 takes over (next term 8e-7 a^6).
VXP_HD void so3_jr_inv(const double w[3], double J[9]) {
  const double a2 = w[0] * w[0] + w[1] * w[1] + w[2] * w[2];
  double c;
  if (a2 < 1e-4) c = 1.0 / 12.0 + a2 * (1.0 / 720.0 + a2 * (1.0 / 30240.0));
  else { const double a = sqrt(a2); c = 1.0 / a2 - (1.0 + cos(a)) / (2.0 * a * sin(a)); }
  const double x = w[0], y = w[1], z = w[2];
  // hat(w)^2 = w w^T - a2 I
  J[0] = 1.0 + c * (x * x - a2); J[1] = -0.5 * z + c * x * y;       J[2] = 0.5 * y + c * x * z;
  J[3] = 0.5 * z + c * x * y;    J[4] = 1.0 + c * (y * y - a2);     J[5] = -0.5 * x + c * y * z;
  J[6] = -0.5 * y + c * x * z;   J[7] = 0.5 * x + c * y * z;        J[8] = 1.0 + c * (z * z - a2);
}

// Exp of a rotation vector (Rodrigues); sin(a) / a and (1 - cos a) / a^2 by their series below 1e-2 rad.
VXP_HD void so3_exp(const double w[3], double E[9]) {
  const double a2 = w[0] * w[0] + w[1] * w[1] + w[2] * w[2];
  double A, B;
  if (a2 < 1e-4) { A = 1.0 - a2 * (1.0 / 6.0 - a2 * (1.0 / 120.0 - a2 * (1.0 / 5040.0))); B = 0.5 - a2 * (1.0 / 24.0 - a2 * (1.0 / 720.0 - a2 * (1.0 / 40320.0))); }
  else { const double a = sqrt(a2); A = sin(a) / a; B = (1.0 - cos(a)) / a2; }
  const double x = w[0], y = w[1], z = w[2];
  E[0] = 1.0 + B * (x * x - a2); E[1] = -A * z + B * x * y;       E[2] = A * y + B * x * z;
  E[3] = A * z + B * x * y;      E[4] = 1.0 + B * (y * y - a2);   E[5] = -A * x + B * y * z;
  E[6] = -A * y + B * x * z;     E[7] = A * x + B * y * z;        E[8] = 1.0 + B * (z * z - a2);
}

// pose record (+) [dphi; dp] -> pose record
VXP_HD void retract(const double* P, const double dx[6], double* out) {
  double R[9], E[9], N[9];
  pose_R(P, R);
  so3_exp(dx, E);
  mul_nn(R, E, N);
  VXP_UNROLL for (int r = 0; r < 3; r++) {
    VXP_UNROLL for (int c = 0; c < 3; c++) out[3 * c + r] = N[3 * r + c];
  }
  VXP_UNROLL for (int k = 0; k < 3; k++) out[9 + k] = P[9 + k] + dx[3 + k];
}

// ---- residuals -------------------------------------------------------------------------------------------------------------------
VXP_HD void between_residual(const double* Pi, const double* Pj, const double* Z, double e[6]) {
  double Ri[9], Rj[9], M[9], E[9];
  pose_R(Pi, Ri); pose_R(Pj, Rj);
  mul_tn(Ri, Rj, M);
  mul_tn(Z, M, E);
  so3_log(E, e);
  const double dp[3] = {Pj[9] - Pi[9], Pj[10] - Pi[10], Pj[11] - Pi[11]};
  double d[3];
  mulv_t(Ri, dp, d);
  const double dz[3] = {d[0] - Z[9], d[1] - Z[10], d[2] - Z[11]};
  mulv_t(Z, dz, e + 3);
}
VXP_HD void prior_residual(const double* Pi, const double* Z, double e[6]) {
  double Ri[9], E[9];
  pose_R(Pi, Ri);
  mul_tn(Z, Ri, E);
  so3_log(E, e);
  const double dz[3] = {Pi[9] - Z[9], Pi[10] - Z[10], Pi[11] - Z[11]};
  mulv_t(Z, dz, e + 3);
}

// ---- residual + Jacobians (6 x 6 row-major, columns [dphi; dp] of the node) -------------------------------------------------------
VXP_HD void between_lin(const double* Pi, const double* Pj, const double* Z, double e[6], double Ji[36], double Jj[36]) {
  double Ri[9], Rj[9], M[9], E[9], Jr[9], A[9];
  pose_R(Pi, Ri); pose_R(Pj, Rj);
  mul_tn(Ri, Rj, M);                          // R_i^T R_j
  mul_tn(Z, M, E);
  so3_log(E, e);
  const double dp[3] = {Pj[9] - Pi[9], Pj[10] - Pi[10], Pj[11] - Pi[11]};
  double d[3];
  mulv_t(Ri, dp, d);                          // R_i^T (p_j - p_i)
  const double dz[3] = {d[0] - Z[9], d[1] - Z[10], d[2] - Z[11]};
  mulv_t(Z, dz, e + 3);
  so3_jr_inv(e, Jr);
  // A = Jr^-1 M^T
  VXP_UNROLL for (int r = 0; r < 3; r++) {
    VXP_UNROLL for (int c = 0; c < 3; c++) A[3 * r + c] = Jr[3 * r] * M[3 * c] + Jr[3 * r + 1] * M[3 * c + 1] + Jr[3 * r + 2] * M[3 * c + 2];
  }
  const double H[9] = {0.0, -d[2], d[1], d[2], 0.0, -d[0], -d[1], d[0], 0.0};    // hat(d)
  double C[9], D[9];
  mul_tn(Z, H, C);                            // Zr^T hat(d)
  // D = Zr^T R_i^T
  VXP_UNROLL for (int r = 0; r < 3; r++) {
    VXP_UNROLL for (int c = 0; c < 3; c++) D[3 * r + c] = Z[r] * Ri[3 * c] + Z[3 + r] * Ri[3 * c + 1] + Z[6 + r] * Ri[3 * c + 2];
  }
  VXP_UNROLL for (int r = 0; r < 3; r++) {
    VXP_UNROLL for (int c = 0; c < 3; c++) {
      Ji[6 * r + c] = -A[3 * r + c];         Ji[6 * r + 3 + c] = 0.0;
      Ji[6 * (r + 3) + c] = C[3 * r + c];    Ji[6 * (r + 3) + 3 + c] = -D[3 * r + c];
      Jj[6 * r + c] = Jr[3 * r + c];         Jj[6 * r + 3 + c] = 0.0;
      Jj[6 * (r + 3) + c] = 0.0;             Jj[6 * (r + 3) + 3 + c] = D[3 * r + c];
    }
  }
}
VXP_HD void prior_lin(const double* Pi, const double* Z, double e[6], double J[36]) {
  double Jr[9];
  prior_residual(Pi, Z, e);
  so3_jr_inv(e, Jr);
  VXP_UNROLL for (int r = 0; r < 3; r++) {
    VXP_UNROLL for (int c = 0; c < 3; c++) {
      J[6 * r + c] = Jr[3 * r + c];          J[6 * r + 3 + c] = 0.0;
      J[6 * (r + 3) + c] = 0.0;              J[6 * (r + 3) + 3 + c] = Z[3 * c + r];      // Zr^T
    }
  }
}

// one entry of a weighted product: (Ja^T W Jb)(r, c), W = diag(w)
VXP_HD double jtwj(const double Ja[36], const double w[6], const double Jb[36], int r, int c) {
  double s = 0.0;
  VXP_UNROLL for (int k = 0; k < 6; k++) s += Ja[6 * k + r] * w[k] * Jb[6 * k + c];
  return s;
}
VXP_HD double jtwe(const double Ja[36], const double w[6], const double e[6], int r) {
  double s = 0.0;
  VXP_UNROLL for (int k = 0; k < 6; k++) s += Ja[6 * k + r] * w[k] * e[k];
  return s;
}
VXP_HD double half_wsq(const double e[6], const double w[6]) {
  double s = 0.0;
  VXP_UNROLL for (int k = 0; k < 6; k++) s += e[k] * e[k] * w[k];
  return 0.5 * s;
}

// Inverse of a symmetric positive definite 6 x 6 (a damped diagonal block: the block-Jacobi preconditioner) by in-place Gauss-Jordan
// without pivoting; every index is a compile-time constant once unrolled, so the 36 entries stay in registers.
VXP_HD void inv6_spd(double a[36]) {
  VXP_UNROLL for (int k = 0; k < 6; k++) {
    const double piv = 1.0 / a[7 * k];
    VXP_UNROLL for (int j = 0; j < 6; j++) if (j != k) a[6 * k + j] *= piv;
    VXP_UNROLL for (int i = 0; i < 6; i++) {
      if (i == k) continue;
      const double f = a[6 * i + k];
      VXP_UNROLL for (int j = 0; j < 6; j++) if (j != k) a[6 * i + j] -= f * a[6 * k + j];
      a[6 * i + k] = -f * piv;
    }
    a[7 * k] = piv;
  }
}

}  // namespace vxpgo
