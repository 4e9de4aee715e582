// Arithmetic of IMUEKF (VoxelSLAM/src/ekf_imu.hpp:41-214; include/vxba.h: vxba_imuekf_*), host + device: vxba_imuekf.hip runs the propagation on the
// host and the de-skew in its kernel, tests/hostmath/imuekf_hostcheck.cpp compiles the same text with g++ for the CPU suite.  The 3 x 3 pieces
// (exp_rate, mul33, midpoint_sample, world_point) are those of the initialisation's motion_blur in vxba_init_math.hpp.
//
// Both translation units that include this file are compiled WITHOUT floating-point contraction, so every expression rounds as written.
//
// Reference semantics that are kept as they are, not repaired:
//   * IMU_init (:167-195): the first message sets the means and init_num = 1; EVERY message (the first too) then does init_num++, so message k >= 2 of
//     a fresh filter is folded in with the divisor k and init_num ends at count + 1.  The recurrence mean += (x - mean) / init_num is evaluated in
//     upstream's order, not as a sum divided once.  init_num persists over calls.
//   * the working list is last_imu followed by the K messages; a pair is skipped when tail.stamp < last_pcl_end_time; cur_time = max(head.stamp,
//     last_pcl_end_time), dt = tail.stamp - cur_time, offt = cur_time - beg_time (:59-87).
//   * acc_imu = R acc + g with the OLD R; the pose entry is stored BEFORE the step; cov = F cov F^T + cov_w, then p, v, then R = R Exp(rate, dt).
//   * the tail (:117-123): note = +-1, dt = note (end_time - last stamp), with the LAST surviving pair's rate and acc_imu.
//   * the de-skew (:138-163): point j > 0 belongs to the latest head with t_i < (double)toff_j, strictly; points with toff <= t_0 stay as they are;
//     the compensated point is rounded to float; point 0 is compensated once under EVERY head earlier than it, latest first, each application on the
//     float result of the one before (the inner loop breaks at begin() without leaving the outer one).
#pragma once
#include "vxba_init_math.hpp"

namespace vxek {

constexpr int STATE_LEN = 24;                  // [R 9 col-major | p | v | bg | ba | g]
constexpr int DIM = 15;                        // rot, p, v, bg, ba
constexpr int POSE_LEN = vxin::POSE_LEN;       // [offt | R 9 | p 3 | v 3 | rate 3 | acc_imu 3], the state BEFORE the step from `head`
constexpr int DEV_POSE_LEN = 24;               // [offt | R 9 | p 3 | v 3 | unit axis 3 | acc_imu 3 | |rate| | 0]: what the kernel keeps in LDS
constexpr int MAX_HEADS = 64;
constexpr int MIN_INIT_NUM = 30;
constexpr double G_M_S2 = 9.8;                 // tools.hpp:15

// the filter's own state, everything but the device buffers
struct Filter {
  int init_flag = 0, init_num = 0;
  double mean_acc[3] = {0, 0, 0}, mean_gyr[3] = {0, 0, 0};
  double scale_gravity = 1.0, last_pcl_end_time = 0.0;
  double last_imu[7] = {0, 0, 0, 0, 0, 0, 0};  // stamp | gyr | acc
};
struct Noise { double cov_acc[3], cov_gyr[3], cov_bias_gyr[3], cov_bias_acc[3]; };

// IMU_init (:167-195)
VXN_HD void imu_init(Filter& f, int K, const double* stamps, const double* gyr, const double* acc) {
  for (int k = 0; k < K; k++) {
    if (f.init_num != 0) {
      for (int r = 0; r < 3; r++) {
        f.mean_acc[r] += (acc[3 * k + r] - f.mean_acc[r]) / f.init_num;
        f.mean_gyr[r] += (gyr[3 * k + r] - f.mean_gyr[r]) / f.init_num;
      }
    } else {
      for (int r = 0; r < 3; r++) { f.mean_acc[r] = acc[3 * k + r]; f.mean_gyr[r] = gyr[3 * k + r]; }
      f.init_num = 1;
    }
    f.init_num++;
  }
  if (K > 0) {
    f.last_imu[0] = stamps[K - 1];
    for (int r = 0; r < 3; r++) { f.last_imu[1 + r] = gyr[3 * (K - 1) + r]; f.last_imu[4 + r] = acc[3 * (K - 1) + r]; }
  }
}

// process() of a filter that is not initialised (:199-210): g is state + 21
VXN_HD void process_init(Filter& f, int acc_in_g, int K, const double* stamps, const double* gyr, const double* acc, double end_time, double* g) {
  imu_init(f, K, stamps, gyr, acc);
  const double nrm = sqrt((f.mean_acc[0] * f.mean_acc[0] + f.mean_acc[1] * f.mean_acc[1]) + f.mean_acc[2] * f.mean_acc[2]);
  if (nrm < 2 && acc_in_g) f.scale_gravity = G_M_S2;
  for (int r = 0; r < 3; r++) g[r] = -f.mean_acc[r] * f.scale_gravity;
  if (f.init_num > MIN_INIT_NUM) f.init_flag = 1;
  f.last_pcl_end_time = end_time;
}

// F_x and cov_w of one step (:89-103), 15 x 15 column-major; R is the rotation BEFORE the step, rate / acc the bias-free mid-point sample
VXN_HD void step_matrices(const double* R, const double rate[3], const double acc[3], double dt, const Noise& nz, double* F, double* W) {
  for (int k = 0; k < DIM * DIM; k++) { F[k] = 0.0; W[k] = 0.0; }
  for (int k = 0; k < DIM; k++) F[DIM * k + k] = 1.0;
  double E[9], RS[9], A[9], Rt[9], B[9];
  vxin::exp_rate(rate, -dt, E);
  const double S[9] = {0, acc[2], -acc[1], -acc[2], 0, acc[0], acc[1], -acc[0], 0};   // hat(acc), column-major
  vxin::mul33(R, S, RS);
  for (int c = 0; c < 3; c++) {
    for (int r = 0; r < 3; r++) {
      F[DIM * c + r] = E[3 * c + r];
      F[DIM * (6 + c) + 3 + r] = r == c ? dt : 0.0;
      F[DIM * (9 + c) + r] = r == c ? -dt : 0.0;
      F[DIM * c + 6 + r] = -RS[3 * c + r] * dt;
      F[DIM * (12 + c) + 6 + r] = -R[3 * c + r] * dt;
      A[3 * c + r] = R[3 * c + r] * nz.cov_acc[c];
      Rt[3 * c + r] = R[3 * r + c];
    }
  }
  vxin::mul33(A, Rt, B);
  for (int c = 0; c < 3; c++) {
    W[DIM * c + c] = nz.cov_gyr[c] * dt * dt;
    W[DIM * (9 + c) + 9 + c] = nz.cov_bias_gyr[c] * dt * dt;
    W[DIM * (12 + c) + 12 + c] = nz.cov_bias_acc[c] * dt * dt;
    for (int r = 0; r < 3; r++) W[DIM * (6 + c) + 6 + r] = B[3 * c + r] * dt * dt;
  }
}

// cov = F cov F^T + W, every sum over k ascending
VXN_HD void cov_step(const double* F, const double* W, double* cov) {
  double T[DIM * DIM];
  for (int c = 0; c < DIM; c++) {
    for (int r = 0; r < DIM; r++) {
      double s = 0.0;
      for (int k = 0; k < DIM; k++) s += F[DIM * k + r] * cov[DIM * c + k];
      T[DIM * c + r] = s;
    }
  }
  for (int c = 0; c < DIM; c++) {
    for (int r = 0; r < DIM; r++) {
      double s = 0.0;
      for (int k = 0; k < DIM; k++) s += T[DIM * k + r] * F[DIM * k + c];
      cov[DIM * c + r] = s + W[DIM * c + r];
    }
  }
}

enum { PROP_OK = 0, PROP_NO_PAIR = 1, PROP_TOO_MANY = 2 };

// motion_blur's forward half (:43-133) on a filter that is initialised.  state / cov are updated and the filter's last_imu / last_pcl_end_time moved
// on only with PROP_OK.  table: room for min(K, MAX_HEADS) rows of POSE_LEN; imus_out: (K + 1) x 7, the list as upstream leaves it for push_imu.
VXN_HD int propagate(Filter& f, const Noise& nz, int K, const double* stamps, const double* gyr, const double* acc, double beg_time, double end_time, double* state,
                     double* cov, double* table, int* M_out, double* imus_out) {
  double R[9], p[3], v[3], rate[3] = {0, 0, 0}, a[3], acc_imu[3] = {0, 0, 0}, C[DIM * DIM], F[DIM * DIM], W[DIM * DIM];
  for (int k = 0; k < 9; k++) R[k] = state[k];
  for (int k = 0; k < 3; k++) { p[k] = state[9 + k]; v[k] = state[12 + k]; }
  for (int k = 0; k < DIM * DIM; k++) C[k] = cov[k];
  const double *bg = state + 15, *ba = state + 18, *g = state + 21;
  int M = 0, pairs = 0;
  for (int t = 0; t < K; t++) {                        // head = working message t, tail = t + 1; working message 0 is last_imu
    const double* hg = t == 0 ? f.last_imu + 1 : gyr + 3 * (t - 1);
    const double* ha = t == 0 ? f.last_imu + 4 : acc + 3 * (t - 1);
    const double hs = t == 0 ? f.last_imu[0] : stamps[t - 1], ts = stamps[t];
    if (ts < f.last_pcl_end_time) continue;
    pairs++;
    if (M >= MAX_HEADS) continue;                      // counted, refused below
    vxin::midpoint_sample(hg, gyr + 3 * t, ha, acc + 3 * t, bg, ba, f.scale_gravity, rate, a);
    for (int r = 0; r < 3; r++) acc_imu[r] = ((R[r] * a[0] + R[3 + r] * a[1]) + R[6 + r] * a[2]) + g[r];
    const double cur = hs < f.last_pcl_end_time ? f.last_pcl_end_time : hs;
    const double dt = ts - cur;
    double* o = table + (size_t)POSE_LEN * M;
    o[0] = cur - beg_time;
    for (int k = 0; k < 9; k++) o[1 + k] = R[k];
    for (int k = 0; k < 3; k++) { o[10 + k] = p[k]; o[13 + k] = v[k]; o[16 + k] = rate[k]; o[19 + k] = acc_imu[k]; }
    M++;
    step_matrices(R, rate, a, dt, nz, F, W);
    cov_step(F, W, C);
    double E[9], Rn[9];
    vxin::exp_rate(rate, dt, E);
    for (int r = 0; r < 3; r++) {
      p[r] = (p[r] + v[r] * dt) + 0.5 * acc_imu[r] * dt * dt;
      v[r] = v[r] + acc_imu[r] * dt;
    }
    vxin::mul33(R, E, Rn);
    for (int k = 0; k < 9; k++) R[k] = Rn[k];
  }
  *M_out = M;
  if (pairs == 0) return PROP_NO_PAIR;
  if (pairs > MAX_HEADS) { *M_out = pairs; return PROP_TOO_MANY; }
  {
    const double imu_end = stamps[K - 1];
    const double note = end_time > imu_end ? 1.0 : -1.0;
    const double dt = note * (end_time - imu_end);
    const double nr[3] = {note * rate[0], note * rate[1], note * rate[2]};
    double E[9], Rn[9];
    vxin::exp_rate(nr, dt, E);
    vxin::mul33(R, E, Rn);
    for (int k = 0; k < 9; k++) state[k] = Rn[k];
    for (int r = 0; r < 3; r++) {
      state[12 + r] = v[r] + note * acc_imu[r] * dt;
      state[9 + r] = (p[r] + note * v[r] * dt) + note * 0.5 * acc_imu[r] * dt * dt;
    }
  }
  for (int k = 0; k < DIM * DIM; k++) cov[k] = C[k];
  if (imus_out) {
    for (int k = 0; k < 7; k++) imus_out[k] = f.last_imu[k];
    imus_out[0] = f.last_pcl_end_time;
    for (int t = 0; t < K; t++) {
      double* o = imus_out + 7 * (t + 1);
      o[0] = stamps[t];
      for (int r = 0; r < 3; r++) { o[1 + r] = gyr[3 * t + r]; o[4 + r] = acc[3 * t + r]; }
    }
    imus_out[7 * K] = end_time;
  }
  f.last_imu[0] = stamps[K - 1];                       // the ORIGINAL stamp: upstream re-stamps a copy
  for (int r = 0; r < 3; r++) { f.last_imu[1 + r] = gyr[3 * (K - 1) + r]; f.last_imu[4 + r] = acc[3 * (K - 1) + r]; }
  f.last_pcl_end_time = end_time;
  return PROP_OK;
}

// what the kernel keeps per head: the unit axis and |rate| instead of the rate (Exp's sqrt and divisions leave the per-point work); a rate that Exp
// treats as zero (not > 1e-7) has |rate| = 0 and a zero axis
VXN_HD void hoist_row(const double* e, double* d) {
  for (int k = 0; k < 16; k++) d[k] = e[k];
  const double* w = e + 16;
  const double a = sqrt((w[0] * w[0] + w[1] * w[1]) + w[2] * w[2]);
  const bool live = a > 1e-7;
  for (int k = 0; k < 3; k++) { d[16 + k] = live ? w[k] / a : 0.0; d[19 + k] = e[19 + k]; }
  d[22] = live ? a : 0.0;
  d[23] = 0.0;
}

// the latest head with t_i < t (strict), -1 if none; tab rows of `stride` doubles with t first, t non-decreasing
VXN_HD int find_head(const double* tab, int stride, int M, double t) {
  int lo = 0, hi = M;
  while (lo < hi) {
    const int mid = (lo + hi) >> 1;
    if (tab[(size_t)stride * mid] < t) lo = mid + 1; else hi = mid;
  }
  return lo - 1;
}

// one point under one head (:150-160): P = L^T (xc.R^T (R_i (L P_i + l) + T_ei) - l), rounded to float.  d: a DEV_POSE_LEN row, xc = [R 9 | p 3] of the
// PROPAGATED state, ext = [L 9 | l 3].  One sin / cos pair.
VXN_HD void deskew_point(const double* d, const double* xc, const double* ext, const float* P, double t, float* out) {
  const double dt = t - d[0];
  const double *R = d + 1, *p = d + 10, *v = d + 13, *a = d + 19;
  const double x = d[16], y = d[17], z = d[18];
  double E[9] = {1, 0, 0, 0, 1, 0, 0, 0, 1}, Ri[9], q[3], r[3], u[3];
  if (d[22] > 0.0) {                                   // Exp(rate, dt) as vxin::exp_rate builds it
    const double ang = d[22] * dt, s = sin(ang), c1 = 1.0 - cos(ang);
    E[0] += c1 * (x * x - 1.0); E[3] += -s * z + c1 * x * y;   E[6] += s * y + c1 * x * z;
    E[1] += s * z + c1 * x * y;  E[4] += c1 * (y * y - 1.0);    E[7] += -s * x + c1 * y * z;
    E[2] += -s * y + c1 * x * z; E[5] += s * x + c1 * y * z;    E[8] += c1 * (z * z - 1.0);
  }
  vxin::mul33(R, E, Ri);
  const double pi[3] = {(double)P[0], (double)P[1], (double)P[2]};
  vxin::world_point(ext, ext + 9, pi, q);
  VXN_UNROLL for (int k = 0; k < 3; k++) {
    const double T = ((p[k] + v[k] * dt) + 0.5 * a[k] * dt * dt) - xc[9 + k];
    r[k] = ((Ri[k] * q[0] + Ri[3 + k] * q[1]) + Ri[6 + k] * q[2]) + T;
  }
  VXN_UNROLL for (int c = 0; c < 3; c++) u[c] = ((xc[3 * c] * r[0] + xc[3 * c + 1] * r[1]) + xc[3 * c + 2] * r[2]) - ext[9 + c];
  VXN_UNROLL for (int c = 0; c < 3; c++) out[c] = (float)((ext[3 * c] * u[0] + ext[3 * c + 1] * u[1]) + ext[3 * c + 2] * u[2]);
}

// point q of the scan under the whole table: what the kernel's lane q does, and the host check
VXN_HD void deskew_scan_point(const double* tab, int M, const double* xc, const double* ext, const float* xyz, const float* toff, long long q, float* out) {
  float P[3] = {xyz[3 * q], xyz[3 * q + 1], xyz[3 * q + 2]};
  const double t = (double)toff[q];
  const int h = find_head(tab, DEV_POSE_LEN, M, t);
  const int last = q == 0 ? 0 : h;                     // point 0: every head from h down to 0; any other point: head h alone
  for (int i = h; i >= last && i >= 0; i--) {
    float o[3];
    deskew_point(tab + (size_t)DEV_POSE_LEN * i, xc, ext, P, t, o);
    P[0] = o[0]; P[1] = o[1]; P[2] = o[2];
  }
  out[0] = P[0]; out[1] = P[1]; out[2] = P[2];        // untouched points: the same bits
}

}  // namespace vxek
