// Per-point arithmetic of the initialisation's scan-to-cloud odometry (include/vxba.h: vxba_initodom_*), host + device: the kernels of
// vxba_init.hip run it on the GPU, tests/hostmath/init_hostcheck.cpp compiles the same text with g++ for the CPU suite.
//
// Reference: lio_state_estimation_kdtree (voxelslam.cpp:960-1098).  Per scan point: world point, five nearest cloud points, the plane
// direct . x = -1 through them by least squares, a residual gate of 0.1 on each of the five, then one row jac = [hat(p) R^T n ; n] with
// residual -(n . wld + d).
//
// Both translation units that include this file are compiled WITHOUT floating-point contraction, so every expression rounds as written.
// Everything is indexed statically (selects instead of stores through a computed index): nothing here may end up in scratch memory.
#pragma once
#include <math.h>

#if defined(__HIPCC__)
#define VXN_HD __host__ __device__ __forceinline__
#define VXN_UNROLL _Pragma("unroll")
#else
#define VXN_HD inline
#define VXN_UNROLL
#endif

namespace vxin {

constexpr int NMATCH = 5;
constexpr double GATE = 0.1;

// wld = R p + t, each component ((R0 x + R1 y) + R2 z) + t; R column-major
VXN_HD void world_point(const double* R, const double* t, const double p[3], double w[3]) {
  VXN_UNROLL for (int r = 0; r < 3; r++) w[r] = ((R[r] * p[0] + R[3 + r] * p[1]) + R[6 + r] * p[2]) + t[r];
}

// float32 squared distance ((dx dx + dy dy) + dz dz)
VXN_HD float sqdist(float ax, float ay, float az, float bx, float by, float bz) {
  const float dx = ax - bx, dy = ay - by, dz = az - bz;
  return (dx * dx + dy * dy) + dz * dz;
}

// candidate order of the search: (distance, index) ascending
VXN_HD bool closer(float d, int i, float e, int j) { return d < e || (d == e && i < j); }

// Least-squares solution of A x = -1 for the 5 x 3 matrix A (row-major, A[3 r + c]) by Householder QR with column pivoting: at every step
// the remaining column of largest squared norm comes first (of equal ones the leftmost), one reflection clears it below the diagonal.
// Rank rule: a pivot |R_kk| <= 3 * 2^-52 * |R_00| ends the factorisation; the components of x that belong to the remaining columns are
// zero (the basic solution), so five collinear or coincident points give a finite x that depends on nothing but A.  A == 0 gives x == 0.
VXN_HD void fit_plane5(const double* A, double x[3]) {
  double a[3][NMATCH], b[NMATCH], nrm[3];
  int perm[3] = {0, 1, 2};
  VXN_UNROLL for (int c = 0; c < 3; c++) {
    VXN_UNROLL for (int r = 0; r < NMATCH; r++) a[c][r] = A[3 * r + c];
  }
  VXN_UNROLL for (int r = 0; r < NMATCH; r++) b[r] = -1.0;
  bool live = true;
  int rank = 0;
  double piv0 = 0.0;
  VXN_UNROLL for (int k = 0; k < 3; k++) {
    VXN_UNROLL for (int c = k; c < 3; c++) {
      double s = 0.0;
      VXN_UNROLL for (int r = k; r < NMATCH; r++) s += a[c][r] * a[c][r];
      nrm[c] = s;
    }
    VXN_UNROLL for (int c = k + 1; c < 3; c++) {       // the largest to position k; strict >: of equal norms the leftmost stays
      const bool sw = nrm[c] > nrm[k];
      VXN_UNROLL for (int r = 0; r < NMATCH; r++) { const double u = a[k][r], v = a[c][r]; a[k][r] = sw ? v : u; a[c][r] = sw ? u : v; }
      { const double u = nrm[k], v = nrm[c]; nrm[k] = sw ? v : u; nrm[c] = sw ? u : v; }
      { const int u = perm[k], v = perm[c]; perm[k] = sw ? v : u; perm[c] = sw ? u : v; }
    }
    const double alpha = a[k][k];
    const double normx = sqrt(nrm[k]);
    const double beta = alpha > 0.0 ? -normx : normx;   // R_kk
    if (k == 0) piv0 = normx;
    live = live && normx > 3.0 * 2.220446049250313e-16 * piv0 && normx > 0.0;
    rank += live ? 1 : 0;
    // v = a_k - beta e_k; H = I - 2 v v^T / (v^T v)
    double v[NMATCH];
    double vtv = 0.0;
    VXN_UNROLL for (int r = k; r < NMATCH; r++) { v[r] = r == k ? alpha - beta : a[k][r]; vtv += v[r] * v[r]; }
    const double sc = (live && vtv > 0.0) ? 2.0 / vtv : 0.0;
    VXN_UNROLL for (int c = k + 1; c < 3; c++) {
      double d = 0.0;
      VXN_UNROLL for (int r = k; r < NMATCH; r++) d += v[r] * a[c][r];
      d *= sc;
      VXN_UNROLL for (int r = k; r < NMATCH; r++) a[c][r] -= d * v[r];
    }
    {
      double d = 0.0;
      VXN_UNROLL for (int r = k; r < NMATCH; r++) d += v[r] * b[r];
      d *= sc;
      VXN_UNROLL for (int r = k; r < NMATCH; r++) b[r] -= d * v[r];
    }
    a[k][k] = live ? beta : 1.0;    // 1.0: a divisor that is never used (rank <= k)
  }
  const double y2 = rank > 2 ? b[2] / a[2][2] : 0.0;
  const double y1 = rank > 1 ? (b[1] - a[2][1] * y2) / a[1][1] : 0.0;
  const double y0 = rank > 0 ? ((b[0] - a[1][0] * y1) - a[2][0] * y2) / a[0][0] : 0.0;
  VXN_UNROLL for (int j = 0; j < 3; j++) x[j] = perm[0] == j ? y0 : (perm[1] == j ? y1 : y2);
}

// the gate: false (rejected) if any |direct . A_i + 1| > 0.1; worst receives max_i |direct . A_i + 1|
VXN_HD bool gate5(const double* A, const double direct[3], double& worst) {
  bool ok = true;
  worst = 0.0;
  VXN_UNROLL for (int r = 0; r < NMATCH; r++) {
    const double e = fabs(((direct[0] * A[3 * r] + direct[1] * A[3 * r + 1]) + direct[2] * A[3 * r + 2]) + 1.0);
    worst = e > worst ? e : worst;
    ok = ok && e <= GATE;               // a value that is not finite fails too (upstream: its d is NaN, and `ds[i] >= 0` drops the point)
  }
  return ok;
}

// d = 1 / |direct|, n = direct d
VXN_HD void plane_of(const double direct[3], double n[3], double& d) {
  d = 1.0 / sqrt((direct[0] * direct[0] + direct[1] * direct[1]) + direct[2] * direct[2]);
  VXN_UNROLL for (int r = 0; r < 3; r++) n[r] = direct[r] * d;
}

// jac = [p x (R^T n) ; n], resid = -(n . wld + d)
VXN_HD void jac_row(const double* R, const double p[3], const double n[3], double d, const double w[3], double jac[6], double& resid) {
  double u[3];
  VXN_UNROLL for (int c = 0; c < 3; c++) u[c] = (R[3 * c] * n[0] + R[3 * c + 1] * n[1]) + R[3 * c + 2] * n[2];
  jac[0] = p[1] * u[2] - p[2] * u[1];
  jac[1] = p[2] * u[0] - p[0] * u[2];
  jac[2] = p[0] * u[1] - p[1] * u[0];
  jac[3] = n[0]; jac[4] = n[1]; jac[5] = n[2];
  resid = -(((n[0] * w[0] + n[1] * w[1]) + n[2] * w[2]) + d);
}

// ---- de-skew (Initialization::motion_blur, voxelslam.cpp:488-561) and push_imu (preintegration.hpp:50-73) ----------------------------
constexpr int POSE_LEN = 22;   // one IMU pose: [offt | R 9 column-major | p 3 | v 3 | rate 3 | acc_imu 3], the state AFTER the backward step to `head`

// Exp(ang_vel, dt) of tools.hpp:68-84: I + sin(|w| dt) K + (1 - cos(|w| dt)) K^2 with K = hat(w / |w|); the identity unless |w| > 1e-7.  Column-major.
VXN_HD void exp_rate(const double w[3], double dt, double E[9]) {
  const double a = sqrt((w[0] * w[0] + w[1] * w[1]) + w[2] * w[2]);
  E[0] = 1; E[1] = 0; E[2] = 0; E[3] = 0; E[4] = 1; E[5] = 0; E[6] = 0; E[7] = 0; E[8] = 1;
  if (!(a > 1e-7)) return;
  const double x = w[0] / a, y = w[1] / a, z = w[2] / a;
  const double ang = a * dt, s = sin(ang), c1 = 1.0 - cos(ang);
  // column-major E[3 c + r]; K^2 = k k^T - I for a unit k
  E[0] += c1 * (x * x - 1.0); E[3] += -s * z + c1 * x * y;   E[6] += s * y + c1 * x * z;
  E[1] += s * z + c1 * x * y;  E[4] += c1 * (y * y - 1.0);    E[7] += -s * x + c1 * y * z;
  E[2] += -s * y + c1 * x * z; E[5] += s * x + c1 * y * z;    E[8] += c1 * (z * z - 1.0);
}

// C = A B, 3 x 3 column-major
VXN_HD void mul33(const double* A, const double* B, double* C) {
  VXN_UNROLL for (int c = 0; c < 3; c++) {
    VXN_UNROLL for (int r = 0; r < 3; r++) C[3 * c + r] = (A[r] * B[3 * c] + A[3 + r] * B[3 * c + 1]) + A[6 + r] * B[3 * c + 2];
  }
}

// the mid-point sample of two IMU messages: rate = (g1 + g2) / 2 - bg, acc = (a1 + a2) / 2 * scale - ba   (motion_blur :500-508, push_imu :61-70)
VXN_HD void midpoint_sample(const double* g1, const double* g2, const double* a1, const double* a2, const double* bg, const double* ba, double scale, double rate[3],
                            double acc[3]) {
  VXN_UNROLL for (int k = 0; k < 3; k++) {
    rate[k] = 0.5 * (g1[k] + g2[k]) - bg[k];
    acc[k] = 0.5 * (a1[k] + a2[k]) * scale - ba[k];
  }
}

// one backward step of the pose table (motion_blur :510-520): from the running (R, p, v) at `tail` to `head`, dt = head - tail (negative)
VXN_HD void pose_step(double* R, double* p, double* v, const double rate[3], const double acc[3], const double g[3], double dt, double acc_imu[3]) {
  double E[9], Rn[9];
  exp_rate(rate, dt, E);
  VXN_UNROLL for (int r = 0; r < 3; r++) acc_imu[r] = ((R[r] * acc[0] + R[3 + r] * acc[1]) + R[6 + r] * acc[2]) + g[r];
  VXN_UNROLL for (int r = 0; r < 3; r++) {
    p[r] = (p[r] + v[r] * dt) + 0.5 * acc_imu[r] * dt * dt;
    v[r] = v[r] + acc_imu[r] * dt;
  }
  mul33(R, E, Rn);
  VXN_UNROLL for (int k = 0; k < 9; k++) R[k] = Rn[k];
}

// one point under one IMU pose (:548-555): R_i = R Exp(rate dt), T_ei = p + v dt + a dt^2 / 2 - xc.p, P = xc.R^T (R_i (ext.R P_i + ext.p) + T_ei)
VXN_HD void deskew_point(const double* e /* POSE_LEN */, const double* xc /* R 9 | p 3 */, const double* ext /* R 9 | p 3 */, const float* P, double curv, double out[3]) {
  const double dt = curv - e[0];
  const double *R = e + 1, *p = e + 10, *v = e + 13, *w = e + 16, *a = e + 19;
  double E[9], Ri[9], q[3], r[3];
  exp_rate(w, dt, E);
  mul33(R, E, Ri);
  const double pi[3] = {(double)P[0], (double)P[1], (double)P[2]};
  world_point(ext, ext + 9, pi, q);
  VXN_UNROLL for (int k = 0; k < 3; k++) {
    const double T = ((p[k] + v[k] * dt) + 0.5 * a[k] * dt * dt) - xc[9 + k];
    r[k] = ((Ri[k] * q[0] + Ri[3 + k] * q[1]) + Ri[6 + k] * q[2]) + T;
  }
  VXN_UNROLL for (int c = 0; c < 3; c++) out[c] = (xc[3 * c] * r[0] + xc[3 * c + 1] * r[1]) + xc[3 * c + 2] * r[2];
}

// point_notime: the extrinsic only
VXN_HD void extrinsic_point(const double* ext, const float* P, double out[3]) {
  const double pi[3] = {(double)P[0], (double)P[1], (double)P[2]};
  world_point(ext, ext + 9, pi, out);
}

// ---- the per-point variances of motion_init's converged rounds --------------------------------------------------------------------------
// calcBodyVar (voxelslam.hpp:164-185): range and range_inc^2 are float there; a zero z becomes 0.0001 IN the point.  V 3 x 3 column-major.
VXN_HD void body_var(double pb[3], float range_inc, double dir_var, double V[9]) {
  if (pb[2] == 0) pb[2] = 0.0001;
  const double nn = sqrt((pb[0] * pb[0] + pb[1] * pb[1]) + pb[2] * pb[2]);
  const double r = (double)(float)nn, range_var = (double)(range_inc * range_inc);
  const double d[3] = {pb[0] / nn, pb[1] / nn, pb[2] / nn};
  double b1[3] = {1.0, 1.0, -(d[0] + d[1]) / d[2]};
  const double n1 = sqrt((b1[0] * b1[0] + b1[1] * b1[1]) + b1[2] * b1[2]);
  b1[0] /= n1; b1[1] /= n1; b1[2] /= n1;
  double b2[3] = {b1[1] * d[2] - b1[2] * d[1], b1[2] * d[0] - b1[0] * d[2], b1[0] * d[1] - b1[1] * d[0]};
  const double n2 = sqrt((b2[0] * b2[0] + b2[1] * b2[1]) + b2[2] * b2[2]);
  b2[0] /= n2; b2[1] /= n2; b2[2] /= n2;
  // A = range hat(d) [b1 b2]
  const double a1[3] = {r * (d[1] * b1[2] - d[2] * b1[1]), r * (d[2] * b1[0] - d[0] * b1[2]), r * (d[0] * b1[1] - d[1] * b1[0])};
  const double a2[3] = {r * (d[1] * b2[2] - d[2] * b2[1]), r * (d[2] * b2[0] - d[0] * b2[2]), r * (d[0] * b2[1] - d[1] * b2[0])};
  VXN_UNROLL for (int c = 0; c < 3; c++) {
    VXN_UNROLL for (int rr = 0; rr < 3; rr++) V[3 * c + rr] = (d[rr] * range_var * d[c] + a1[rr] * dir_var * a1[c]) + a2[rr] * dir_var * a2[c];
  }
}

// pvec_update (voxelslam.hpp:203-215): O = R V R^T + hat(p) rot_var hat(p)^T + tsl_var, all 3 x 3 column-major
VXN_HD void world_var(const double* R, const double p[3], const double V[9], const double* rot_var, const double* tsl_var, double O[9]) {
  const double H[9] = {0, p[2], -p[1], -p[2], 0, p[0], p[1], -p[0], 0};
  double T[9], Ht[9], Rt[9], A[9], B[9];
  VXN_UNROLL for (int c = 0; c < 3; c++) {
    VXN_UNROLL for (int r = 0; r < 3; r++) { Ht[3 * c + r] = H[3 * r + c]; Rt[3 * c + r] = R[3 * r + c]; }
  }
  mul33(R, V, T); mul33(T, Rt, A);
  mul33(H, rot_var, T); mul33(T, Ht, B);
  VXN_UNROLL for (int k = 0; k < 9; k++) O[k] = (A[k] + B[k]) + tsl_var[k];
}

// align_gravity (voxelslam.cpp:461-486) on W states of 24: g of state 0 turned onto +-z by the rotation about n0 x n1 through asin(|n0 x n1|); every
// pose rotated about p of state 0, every velocity rotated, every g replaced.
VXN_HD void align_gravity(double* xs, int W) {
  const double* g = xs + 21;
  const double gn = sqrt((g[0] * g[0] + g[1] * g[1]) + g[2] * g[2]);
  const double n0[3] = {g[0] / gn, g[1] / gn, g[2] / gn};
  const double n1[3] = {0.0, 0.0, n0[2] < 0 ? -1.0 : 1.0};
  double k[3] = {n0[1] * n1[2] - n0[2] * n1[1], n0[2] * n1[0] - n0[0] * n1[2], n0[0] * n1[1] - n0[1] * n1[0]};
  const double rn = sqrt((k[0] * k[0] + k[1] * k[1]) + k[2] * k[2]);
  k[0] /= rn; k[1] /= rn; k[2] /= rn;
  const double ang = asin(rn), s = sin(ang), c1 = 1.0 - cos(ang);
  const double x = k[0], y = k[1], z = k[2];
  double E[9] = {1, 0, 0, 0, 1, 0, 0, 0, 1};      // column-major, as exp_rate
  E[0] += c1 * (x * x - 1.0); E[3] += -s * z + c1 * x * y;   E[6] += s * y + c1 * x * z;
  E[1] += s * z + c1 * x * y;  E[4] += c1 * (y * y - 1.0);    E[7] += -s * x + c1 * y * z;
  E[2] += -s * y + c1 * x * z; E[5] += s * x + c1 * y * z;    E[8] += c1 * (z * z - 1.0);
  const double zero[3] = {0, 0, 0};
  double g0[3], p0[3] = {xs[9], xs[10], xs[11]};
  world_point(E, zero, g, g0);
  for (int i = 0; i < W; i++) {
    double* s_ = xs + 24 * i;
    const double dp[3] = {s_[9] - p0[0], s_[10] - p0[1], s_[11] - p0[2]};
    double q[3], Rn[9], v[3] = {s_[12], s_[13], s_[14]}, vn[3];
    world_point(E, p0, dp, q);
    mul33(E, s_, Rn);
    world_point(E, zero, v, vn);
    for (int t = 0; t < 9; t++) s_[t] = Rn[t];
    for (int t = 0; t < 3; t++) { s_[9 + t] = q[t]; s_[12 + t] = vn[t]; s_[21 + t] = g0[t]; }
  }
}

}  // namespace vxin
