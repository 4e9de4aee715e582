// Per-triangle and per-pair arithmetic of the loop search (include/vxba.h: vxba_loopsearch_*), host + device: the kernels of
// vxba_loopsearch.hip run it on the GPU, tests/hostmath/loopsearch_hostcheck.cpp compiles the same text with g++ for the CPU suite.
//
// Reference: STDescManager::generate_std (BTC.cpp:979-1126), AddSTDescs (:258-277), candidate_selector (:1128-1279), candidate_verify and
// triangle_solver (:1281-1420), binary_similarity (:70-80).
//
// Both translation units that include this file are compiled WITHOUT floating-point contraction (csrc/Makefile, the host check's g++
// line), so that every expression below rounds as it is written -- tests/_loopsearch_ref.py writes the same expressions in numpy.
#pragma once
#include <math.h>
#include <stdint.h>

#if defined(__HIPCC__)
#define VXS_HD __host__ __device__ __forceinline__
#else
#define VXS_HD inline
#endif

namespace vxls {

constexpr int KEY_BITS = 21;                       // a side key (int64)(float)(1000 side) and a cell coordinate each fit 21 bits (checked on the host)
constexpr unsigned long long KEY_NONE = ~0ull;     // a rejected triangle; an empty slot of the cell table

VXS_HD int popcount64(unsigned long long v) {
#if defined(__HIP_DEVICE_COMPILE__)
  return __popcll(v);
#else
  return __builtin_popcountll(v);
#endif
}

// |p - q| of two float32 corners as the reference forms it (BTC.cpp:1011-1016): the difference in float32, its square (exact) and the sum in float64
VXS_HD double side(const float* p, const float* q) {
  const float dx = p[0] - q[0], dy = p[1] - q[1], dz = p[2] - q[2];
  const double x = (double)dx, y = (double)dy, z = (double)dz;
  return sqrt((x * x + y * y) + z * z);
}

VXS_HD double norm3(double x, double y, double z) { return sqrt((x * x + y * y) + z * z); }

// The three conditional swaps of BTC.cpp:1032-1055 on the sides a = |p1 p2|, b = |p1 p3|, c = |p2 p3|.  m* are the vertex sets of the sides as
// bit masks (bit 0 = the corner itself, bit 1 = neighbour m, bit 2 = neighbour n) and travel with them; on return a <= b <= c and
// v[0] = A (shared by a and b), v[1] = B (a and c), v[2] = C (b and c), each 0, 1 or 2.
VXS_HD void sort_sides(double& a, double& b, double& c, int v[3]) {
  int ma = 3, mb = 5, mc = 6;
  double t; int mt;
  if (a > b) { t = a; a = b; b = t; mt = ma; ma = mb; mb = mt; }
  if (b > c) { t = b; b = c; c = t; mt = mb; mb = mc; mc = mt; }
  if (a > b) { t = a; a = b; b = t; mt = ma; ma = mb; mb = mt; }
  const int A = ma & mb, B = ma & mc, C = mb & mc;
  v[0] = A >> 1; v[1] = B >> 1; v[2] = C >> 1;          // 1, 2, 4 -> 0, 1, 2
}

// a triangle passes when every side lies in [min_len, max_len] (tested before the sort) ...
VXS_HD bool sides_in_range(double a, double b, double c, double min_len, double max_len) {
  return !(a > max_len || b > max_len || c > max_len || a < min_len || b < min_len || c < min_len);
}
// ... and, after the sort, is not near-collinear (BTC.cpp:1056)
VXS_HD bool not_collinear(double a, double b, double c) { return !(fabs(c - (a + b)) < 0.2); }

// the dedupe key of a side: the product in float64, rounded to float32 (pcl::PointXYZ), truncated (BTC.cpp:1060-1064)
VXS_HD long long side_key(double s) { return (long long)(float)(s * 1000.0); }
VXS_HD unsigned long long pack3(long long x, long long y, long long z) {
  return ((unsigned long long)x << (2 * KEY_BITS)) | ((unsigned long long)y << KEY_BITS) | (unsigned long long)z;
}

// the cell a descriptor is filed under (AddSTDescs) and the cell a query visits under one neighbour offset (candidate_selector)
VXS_HD int cell_add(double t) { return (int)(t + 0.5); }
VXS_HD int cell_query(double t, int inc) { return (int)(t + (double)inc); }
// |triangle - (cell + 0.5)| of BTC.cpp:1173-1176
VXS_HD double cell_distance(const double t[3], const int c[3]) { return norm3(t[0] - ((double)c[0] + 0.5), t[1] - ((double)c[1] + 0.5), t[2] - ((double)c[2] + 0.5)); }

// binary_similarity over three corners: each 2 |b1 & b2| / (|b1| + |b2|), summed (A + B) + C, divided by 3.  0 / 0 is NaN and compares false.
VXS_HD double similarity1(unsigned long long p, unsigned long long q) { return 2.0 * (double)popcount64(p & q) / (double)(popcount64(p) + popcount64(q)); }
VXS_HD double similarity(const unsigned long long p[3], const unsigned long long q[3]) { return ((similarity1(p[0], q[0]) + similarity1(p[1], q[1])) + similarity1(p[2], q[2])) / 3.0; }

VXS_HD void cross3(const double* a, const double* b, double* c) {
  c[0] = a[1] * b[2] - a[2] * b[1]; c[1] = a[2] * b[0] - a[0] * b[2]; c[2] = a[0] * b[1] - a[1] * b[0];
}

// triangle_solver (BTC.cpp:1398-1420): the proper rotation R maximising tr(R S Q^T), S and Q the vertex-minus-centre columns of the source and of
// the reference triangle, and t = c_ref - R c_src -- V U^T of the SVD of S Q^T with the sign fixed on the smallest singular direction.  Two steps,
// no eigen-solver:
//   1. a start from the geometry.  Both column sets are planar up to the difference between the centre (mean of the float32-rounded corners) and
//      the mean of the float64 locations, so S Q^T has rank 2 up to ~1e-6 of its size and the maximiser takes the source plane onto the reference
//      plane: normal onto normal or onto minus normal, each with its best in-plane angle in closed form; the better of the two.
//   2. Newton on SO(3) for the full 3 x 3 problem: with M = R S Q^T and R <- Exp(w) R, tr(Exp(w) M) = tr M + g . w - w^T K w / 2 + ...,
//      g = (M12 - M21, M20 - M02, M01 - M10), K = tr(M) I - (M + M^T) / 2; w = K^-1 g.  K has the eigenvalues s_i + s_j of the singular values, so
//      it is positive definite wherever the triangle test leaves a triangle; from a start ~1e-5 away three steps are two more than rounding needs.
// loc: the three corner locations (A, B, C) x 3.  P: [R column-major 9 | t 3].  Degenerate triangles give a P that is not finite.
VXS_HD void triangle_pose(const double* sl, const double* sc, const double* rl, const double* rc, double* P) {
  double s[9], q[9];
  for (int k = 0; k < 9; k++) { s[k] = sl[k] - sc[k % 3]; q[k] = rl[k] - rc[k % 3]; }
  double e1[3], e2[3], ns[3], f1[3], f2[3], nr[3];
  cross3(s, s + 3, ns); cross3(q, q + 3, nr);
  const double lns = norm3(ns[0], ns[1], ns[2]), lnr = norm3(nr[0], nr[1], nr[2]), le = norm3(s[0], s[1], s[2]), lf = norm3(q[0], q[1], q[2]);
  for (int k = 0; k < 3; k++) { ns[k] /= lns; nr[k] /= lnr; e1[k] = s[k] / le; f1[k] = q[k] / lf; }
  cross3(ns, e1, e2); cross3(nr, f1, f2);
  // in-plane coordinates and the four sums of the two 2-D problems
  double sxx = 0, sxy = 0, syx = 0, syy = 0;
  for (int v = 0; v < 3; v++) {
    const double* a = s + 3 * v; const double* b = q + 3 * v;
    const double xs = (a[0] * e1[0] + a[1] * e1[1]) + a[2] * e1[2], ys = (a[0] * e2[0] + a[1] * e2[1]) + a[2] * e2[2];
    const double xr = (b[0] * f1[0] + b[1] * f1[1]) + b[2] * f1[2], yr = (b[0] * f2[0] + b[1] * f2[1]) + b[2] * f2[2];
    sxx += xs * xr; sxy += xs * yr; syx += ys * xr; syy += ys * yr;
  }
  const double A0 = sxx + syy, B0 = sxy - syx;         // normal onto normal
  const double A1 = sxx - syy, B1 = -sxy - syx;        // normal onto minus normal: the reference basis (f1, -f2, -n_r)
  const double h0 = sqrt(A0 * A0 + B0 * B0), h1 = sqrt(A1 * A1 + B1 * B1);
  const bool flip = h1 > h0;
  const double sg = flip ? -1.0 : 1.0;
  const double co = (flip ? A1 : A0) / (flip ? h1 : h0), si = (flip ? B1 : B0) / (flip ? h1 : h0);
  // R = [g1 g2 g3] [e1 e2 n_s]^T with g1 = co f1 + si f2', g2 = -si f1 + co f2', g3 = n_r', (f2', n_r') = sg (f2, n_r); row-major here
  double R[9];
  for (int r = 0; r < 3; r++) {
    const double f2r = sg * f2[r];
    const double g1 = co * f1[r] + si * f2r, g2 = co * f2r - si * f1[r], g3 = sg * nr[r];
    for (int c = 0; c < 3; c++) R[3 * r + c] = (g1 * e1[c] + g2 * e2[c]) + g3 * ns[c];
  }
  double H[9];                                          // S Q^T
  for (int i = 0; i < 3; i++)
    for (int j = 0; j < 3; j++) H[3 * i + j] = (s[i] * q[j] + s[3 + i] * q[3 + j]) + s[6 + i] * q[6 + j];
  for (int it = 0; it < 3; it++) {
    double M[9];
    for (int i = 0; i < 3; i++)
      for (int j = 0; j < 3; j++) M[3 * i + j] = (R[3 * i] * H[j] + R[3 * i + 1] * H[3 + j]) + R[3 * i + 2] * H[6 + j];
    const double g[3] = {M[5] - M[7], M[6] - M[2], M[1] - M[3]};
    const double tr = (M[0] + M[4]) + M[8];
    const double k00 = tr - M[0], k11 = tr - M[4], k22 = tr - M[8], k01 = -0.5 * (M[1] + M[3]), k02 = -0.5 * (M[2] + M[6]), k12 = -0.5 * (M[5] + M[7]);
    // w = K^-1 g through the adjugate
    const double c00 = k11 * k22 - k12 * k12, c01 = k02 * k12 - k01 * k22, c02 = k01 * k12 - k02 * k11, c11 = k00 * k22 - k02 * k02, c12 = k01 * k02 - k00 * k12,
                 c22 = k00 * k11 - k01 * k01;
    const double det = (k00 * c00 + k01 * c01) + k02 * c02;
    const double w[3] = {((c00 * g[0] + c01 * g[1]) + c02 * g[2]) / det, ((c01 * g[0] + c11 * g[1]) + c12 * g[2]) / det, ((c02 * g[0] + c12 * g[1]) + c22 * g[2]) / det};
    const double t2 = (w[0] * w[0] + w[1] * w[1]) + w[2] * w[2], th = sqrt(t2);
    const double a = th < 1e-4 ? 1.0 - t2 / 6.0 : sin(th) / th, b = th < 1e-4 ? 0.5 - t2 / 24.0 : (1.0 - cos(th)) / t2;
    // E = I + a [w]x + b [w]x^2
    const double E[9] = {1.0 - b * (w[1] * w[1] + w[2] * w[2]), b * w[0] * w[1] - a * w[2],             b * w[0] * w[2] + a * w[1],
                         b * w[0] * w[1] + a * w[2],             1.0 - b * (w[0] * w[0] + w[2] * w[2]), b * w[1] * w[2] - a * w[0],
                         b * w[0] * w[2] - a * w[1],             b * w[1] * w[2] + a * w[0],             1.0 - b * (w[0] * w[0] + w[1] * w[1])};
    double N[9];
    for (int i = 0; i < 3; i++)
      for (int j = 0; j < 3; j++) N[3 * i + j] = (E[3 * i] * R[j] + E[3 * i + 1] * R[3 + j]) + E[3 * i + 2] * R[6 + j];
    for (int k = 0; k < 9; k++) R[k] = N[k];
  }
  for (int c = 0; c < 3; c++)
    for (int r = 0; r < 3; r++) P[3 * c + r] = R[3 * r + c];
  for (int r = 0; r < 3; r++) P[9 + r] = rc[r] - ((P[r] * sc[0] + P[3 + r] * sc[1]) + P[6 + r] * sc[2]);
}

// |R x + t - y| < thr for the three corners, tested A, B, C (BTC.cpp:1314-1328)
VXS_HD bool pair_votes(const double* P, const double* sl, const double* rl, double thr) {
  for (int v = 0; v < 3; v++) {
    const double* x = sl + 3 * v; const double* y = rl + 3 * v;
    double d[3];
    for (int r = 0; r < 3; r++) d[r] = (((P[r] * x[0] + P[3 + r] * x[1]) + P[6 + r] * x[2]) + P[9 + r]) - y[r];
    if (!(norm3(d[0], d[1], d[2]) < thr)) return false;
  }
  return true;
}

VXS_HD bool finite12(const double* P) {
  bool ok = true;
  for (int k = 0; k < 12; k++) ok = ok && (fabs(P[k]) <= 1.79e308);
  return ok;
}

}  // namespace vxls
