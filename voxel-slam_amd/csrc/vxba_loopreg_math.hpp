// Per-point and per-pair arithmetic of the loop-edge registration (include/vxba.h: vxba_loopreg_*), host + device: the kernels of
// vxba_loopreg.hip run it on the GPU, tests/hostmath/loopreg_hostcheck.cpp compiles the same text with g++ for the CPU suite.
//
// Reference: icp_normal (loop_refine.hpp:47-145) and STDescManager::plane_geometric_verify (BTC.cpp:1422-1479).  Both transform a source
// plane (centre, normal) by a pose hypothesis, look up the nearest target centre and gate the pair:
//   (|n - n_t| < a or |n + n_t| < b) and |n_t . (p - p_t)| < c and |p - p_t| < d
// The ICP adds one row per gated pair:  rr = n_t . (p - p_t),  jac = [hat(p_local) R^T n_t ; n_t],  update R <- R Exp(dphi), t <- t + dt.
//
// Both translation units that include this file are compiled WITHOUT floating-point contraction (csrc/Makefile, the host check's g++
// line), so that every expression below rounds as it is written -- tests/_loopreg_ref.py writes the same expressions in numpy.
//
// Layouts: a pose record is [R column-major 9 | t 3] as everywhere in the ABI; a plane record is six float32 (x, y, z, nx, ny, nz).
#pragma once
#include <math.h>

#if defined(__HIPCC__)
#define VXL_HD __host__ __device__ __forceinline__
#define VXL_UNROLL _Pragma("unroll")
#else
#define VXL_HD inline
#define VXL_UNROLL
#endif

namespace vxlr {

constexpr int ACC_LEN = 35;     // Hess upper triangle 21 | JacT 6 | resi 1 | sum n_t n_t^T upper triangle 6 | match count 1
constexpr int ACC_JACT = 21, ACC_RESI = 27, ACC_NORM = 28, ACC_COUNT = 34;

// p = R p_local + t, n = R n_local in float64 from the float32 fields; each component ((R0 x + R1 y) + R2 z) + t
VXL_HD void transform_plane(const double* P, const float* s, double p[3], double n[3]) {
  const double x = (double)s[0], y = (double)s[1], z = (double)s[2], nx = (double)s[3], ny = (double)s[4], nz = (double)s[5];
  VXL_UNROLL for (int r = 0; r < 3; r++) {
    p[r] = ((P[r] * x + P[3 + r] * y) + P[6 + r] * z) + P[9 + r];
    n[r] = (P[r] * nx + P[3 + r] * ny) + P[6 + r] * nz;
  }
}

// the gate of one (source, target) pair; rr receives n_t . (p - p_t)
VXL_HD bool gate(const double p[3], const double n[3], const float* t, const double g[4], double& rr) {
  const double tp[3] = {(double)t[0], (double)t[1], (double)t[2]}, tn[3] = {(double)t[3], (double)t[4], (double)t[5]};
  const double d[3] = {p[0] - tp[0], p[1] - tp[1], p[2] - tp[2]};
  const double i0 = n[0] - tn[0], i1 = n[1] - tn[1], i2 = n[2] - tn[2];
  const double a0 = n[0] + tn[0], a1 = n[1] + tn[1], a2 = n[2] + tn[2];
  const double inc = sqrt((i0 * i0 + i1 * i1) + i2 * i2), add = sqrt((a0 * a0 + a1 * a1) + a2 * a2);
  rr = (tn[0] * d[0] + tn[1] * d[1]) + tn[2] * d[2];
  const double pp = sqrt((d[0] * d[0] + d[1] * d[1]) + d[2] * d[2]);
  return (inc < g[0] || add < g[1]) && fabs(rr) < g[2] && pp < g[3];
}

// jac = [p_local x (R^T n_t) ; n_t]
VXL_HD void jac_row(const double* P, const float* s, const float* t, double jac[6]) {
  const double tn[3] = {(double)t[3], (double)t[4], (double)t[5]};
  const double pl[3] = {(double)s[0], (double)s[1], (double)s[2]};
  double u[3];
  VXL_UNROLL for (int c = 0; c < 3; c++) u[c] = (P[3 * c] * tn[0] + P[3 * c + 1] * tn[1]) + P[3 * c + 2] * tn[2];
  jac[0] = pl[1] * u[2] - pl[2] * u[1];
  jac[1] = pl[2] * u[0] - pl[0] * u[2];
  jac[2] = pl[0] * u[1] - pl[1] * u[0];
  jac[3] = tn[0]; jac[4] = tn[1]; jac[5] = tn[2];
}

// one gated pair into the 35 sums
VXL_HD void accumulate(const double jac[6], const float* t, double rr, double acc[ACC_LEN]) {
  int k = 0;
  VXL_UNROLL for (int r = 0; r < 6; r++) {
    VXL_UNROLL for (int c = r; c < 6; c++) acc[k++] += jac[r] * jac[c];
  }
  VXL_UNROLL for (int r = 0; r < 6; r++) acc[ACC_JACT + r] += jac[r] * rr;
  acc[ACC_RESI] += 0.5 * rr * rr;
  const double tn[3] = {(double)t[3], (double)t[4], (double)t[5]};
  k = ACC_NORM;
  VXL_UNROLL for (int r = 0; r < 3; r++) {
    VXL_UNROLL for (int c = r; c < 3; c++) acc[k++] += tn[r] * tn[c];
  }
  acc[ACC_COUNT] += 1.0;
}

// Hess dx = -JacT by an unpivoted LDL^T of the symmetric 6 x 6 given by its upper triangle (row by row, 21 values).  A pivot that is zero
// or not finite leaves values that are not finite in dx: the caller's finite test is the failure test.
VXL_HD void solve6(const double hu[21], const double jt[6], double dx[6]) {
  double A[36];
  int k = 0;
  VXL_UNROLL for (int r = 0; r < 6; r++) {
    VXL_UNROLL for (int c = r; c < 6; c++) { A[6 * r + c] = hu[k]; A[6 * c + r] = hu[k]; k++; }
  }
  double L[36], D[6];
  VXL_UNROLL for (int j = 0; j < 6; j++) {
    double d = A[7 * j];
    VXL_UNROLL for (int q = 0; q < j; q++) d -= L[6 * j + q] * L[6 * j + q] * D[q];
    D[j] = d;
    VXL_UNROLL for (int i = j + 1; i < 6; i++) {
      double v = A[6 * i + j];
      VXL_UNROLL for (int q = 0; q < j; q++) v -= L[6 * i + q] * L[6 * j + q] * D[q];
      L[6 * i + j] = v / d;
    }
  }
  double y[6];
  VXL_UNROLL for (int i = 0; i < 6; i++) {
    double v = -jt[i];
    VXL_UNROLL for (int q = 0; q < i; q++) v -= L[6 * i + q] * y[q];
    y[i] = v;
  }
  VXL_UNROLL for (int i = 5; i >= 0; i--) {
    double v = y[i] / D[i];
    VXL_UNROLL for (int q = i + 1; q < 6; q++) v -= L[6 * q + i] * dx[q];
    dx[i] = v;
  }
}

// Exp as the reference writes it (tools.hpp:51-66): I + sin(a) K + (1 - cos a) K^2 with K = hat(w / a); the identity below 1e-11.  Row-major.
VXL_HD void so3_exp(const double w[3], double E[9]) {
  const double a = sqrt((w[0] * w[0] + w[1] * w[1]) + w[2] * w[2]);
  E[0] = 1; E[1] = 0; E[2] = 0; E[3] = 0; E[4] = 1; E[5] = 0; E[6] = 0; E[7] = 0; E[8] = 1;
  if (!(a >= 1e-11)) return;
  const double x = w[0] / a, y = w[1] / a, z = w[2] / a;
  const double s = sin(a), c1 = 1.0 - cos(a);
  // K^2 = k k^T - I for a unit k
  E[0] += c1 * (x * x - 1.0); E[1] += -s * z + c1 * x * y;   E[2] += s * y + c1 * x * z;
  E[3] += s * z + c1 * x * y;  E[4] += c1 * (y * y - 1.0);    E[5] += -s * x + c1 * y * z;
  E[6] += -s * y + c1 * x * z; E[7] += s * x + c1 * y * z;    E[8] += c1 * (z * z - 1.0);
}

// pose record (+) [dphi; dt]: R <- R Exp(dphi), t <- t + dt
VXL_HD void retract(const double* P, const double dx[6], double* out) {
  double E[9];
  so3_exp(dx, E);
  double N[9];
  VXL_UNROLL for (int r = 0; r < 3; r++) {
    VXL_UNROLL for (int c = 0; c < 3; c++) N[3 * c + r] = (P[r] * E[c] + P[3 + r] * E[3 + c]) + P[6 + r] * E[6 + c];
  }
  VXL_UNROLL for (int q = 0; q < 9; q++) out[q] = N[q];
  VXL_UNROLL for (int q = 0; q < 3; q++) out[9 + q] = P[9 + q] + dx[3 + q];
}

// The state of one pair between iterations (loop_refine.hpp:62-63, 121-130)
struct IcpState {
  int iter;          // iterations run
  int done;          // nothing more to do
  int is_converge;   // the step norms were below step_tol once: the tight gates are in force
  int failed;        // fewer than 6 matches or a step that is not finite: stopped, never accepted
};

// after the sums of one iteration: decide about the step dx.  Returns true when the step is to be applied.
VXL_HD bool icp_advance(IcpState& st, double match_num, const double dx[6], double step_tol, int max_iter) {
  st.iter += 1;
  bool fin = match_num >= 6.0;
  VXL_UNROLL for (int q = 0; q < 6; q++) fin = fin && (fabs(dx[q]) <= 1.79e308);     // false for NaN and infinities
  if (!fin) { st.done = 1; st.failed = 1; st.is_converge = 0; return false; }
  const double nr = sqrt((dx[0] * dx[0] + dx[1] * dx[1]) + dx[2] * dx[2]), nt = sqrt((dx[3] * dx[3] + dx[4] * dx[4]) + dx[5] * dx[5]);
  // written as selects of values: `if (is_converge) done = 1; else is_converge = 1;` compiles to a store through a selected address on the
  // GPU, which puts the state into scratch memory
  const bool small = nr < step_tol && nt < step_tol;
  const int was = st.is_converge;
  st.done = ((small && was) || st.iter >= max_iter) ? 1 : st.done;
  st.is_converge = small ? 1 : was;
  return true;
}

// voxel coordinate of BTC.cpp:287-295: divide, subtract 1.0 where negative, truncate
VXL_HD long long voxel_coord(double v, double voxel_size) {
  double l = v / voxel_size;
  if (l < 0) l -= 1.0;
  return (long long)l;
}

}  // namespace vxlr
