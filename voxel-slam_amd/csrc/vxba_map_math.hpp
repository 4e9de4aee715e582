// Pure arithmetic of the incremental local map (vxba_map.hip), host + device: the kernels run it on the GPU, tests/hostmath/map_hostcheck.cpp
// compiles the same text with g++ -ffp-contract=off for the CPU suite (tests/test_map_cpu.py).
//
// Reference: PointCluster::push / transform tools.hpp:326-331, 357-363; Bf_var voxel_map.hpp:91-106; the octant test of OctoTree::allocate :1029-1032;
// xx.R * pv.pnt + xx.p :1100, 1264; OctoTree::plane_update :1118-1146.  The float-typed voxel index is the odometry's (vxba_lio_math.hpp): one text
// for cut_voxel (voxel_map.hpp:1553-1560) and match (:1678-1685).
// Arithmetic that decides tree structure or feeds running sums (world point, octant test, cluster push, covariance sum) is written unfused, as the
// reference's x86-64 build computes it; cl_transform and plane_update_math follow the compiler's contraction on the device.
#pragma once
#include "vxba_lio_math.hpp"

#if defined(__HIPCC__)
#define VXM_FI __device__ __forceinline__
#define VXM_FN __device__
#else
#define VXM_FI inline
#define VXM_FN inline
#endif

namespace vxmap {

using vxl::voxel_index;

// ---- unfused helpers --------------------------------------------------------------------------------------------------------
VXM_FI double madd_u(double acc, double a, double b) {
#pragma clang fp contract(off)
  const double p = a * b;
  return acc + p;
}
VXM_FI double mul_u(double a, double b) {
#pragma clang fp contract(off)
  const double p = a * b;
  return p;
}
// xx.R * pv.pnt + xx.p (voxel_map.hpp:1100, 1264): (R(r,0) x + R(r,1) y) + R(r,2) z, then + p
VXM_FI void to_world(const double* Rp, const double* x, double* w) {
#pragma unroll
  for (int r = 0; r < 3; r++) {
    double s = mul_u(Rp[r], x[0]);
    s = madd_u(s, Rp[3 + r], x[1]);
    s = madd_u(s, Rp[6 + r], x[2]);
    w[r] = s + Rp[9 + r];
  }
}
// PointCluster::push (tools.hpp:326-331) on the packed cluster [Pxx Pxy Pxz Pyy Pyz Pzz vx vy vz N]
VXM_FI void cl_push(double* c, const double* x) {
  c[9] += 1.0;
  c[0] = madd_u(c[0], x[0], x[0]); c[1] = madd_u(c[1], x[0], x[1]); c[2] = madd_u(c[2], x[0], x[2]);
  c[3] = madd_u(c[3], x[1], x[1]); c[4] = madd_u(c[4], x[1], x[2]); c[5] = madd_u(c[5], x[2], x[2]);
  c[6] += x[0]; c[7] += x[1]; c[8] += x[2];
}
// cov_add += Bf_var(pv, vec) (voxel_map.hpp:91-106), column-major 9x9; Biup = Bi * var evaluated as the text does
VXM_FI void cov_add_point(double* acc, const double* x, const double* V /* column-major 3x3 */) {
  const double Bi[6][3] = {{2 * x[0], 0, 0}, {x[1], x[0], 0}, {x[2], 0, x[0]}, {0, 2 * x[1], 0}, {0, x[2], x[1]}, {0, 0, 2 * x[2]}};
  double Biup[6][3];
#pragma unroll
  for (int r = 0; r < 6; r++)
#pragma unroll
    for (int k = 0; k < 3; k++) Biup[r][k] = madd_u(madd_u(mul_u(Bi[r][0], V[3 * k]), Bi[r][1], V[3 * k + 1]), Bi[r][2], V[3 * k + 2]);
#pragma unroll
  for (int r = 0; r < 6; r++)
#pragma unroll
    for (int k = 0; k < 6; k++) acc[9 * k + r] += madd_u(madd_u(mul_u(Biup[r][0], Bi[k][0]), Biup[r][1], Bi[k][1]), Biup[r][2], Bi[k][2]);
#pragma unroll
  for (int r = 0; r < 6; r++)
#pragma unroll
    for (int k = 0; k < 3; k++) { acc[9 * (6 + k) + r] += Biup[r][k]; acc[9 * r + 6 + k] += Biup[r][k]; }
#pragma unroll
  for (int r = 0; r < 3; r++)
#pragma unroll
    for (int k = 0; k < 3; k++) acc[9 * (6 + k) + 6 + r] += V[3 * k + r];
}
VXM_FI int octant_of(const double* w, const double* c) {
  return 4 * (w[0] > c[0] ? 1 : 0) + 2 * (w[1] > c[1] ? 1 : 0) + (w[2] > c[2] ? 1 : 0);
}

// PointCluster::transform (tools.hpp:357-363) on packed clusters, pose R column-major | p
VXM_FI void cl_transform(const double* s, const double* Rp, double* o) {
  const double N = s[9];
  const double P[9] = {s[0], s[1], s[2], s[1], s[3], s[4], s[2], s[4], s[5]};   // symmetric, row r col c = P[3r+c]
  double Rv[3], RP[9], out[9];
#pragma unroll
  for (int r = 0; r < 3; r++) Rv[r] = Rp[r] * s[6] + Rp[3 + r] * s[7] + Rp[6 + r] * s[8];
#pragma unroll
  for (int r = 0; r < 3; r++)
#pragma unroll
    for (int c = 0; c < 3; c++) RP[3 * r + c] = Rp[r] * P[c] + Rp[3 + r] * P[3 + c] + Rp[6 + r] * P[6 + c];
#pragma unroll
  for (int r = 0; r < 3; r++)
#pragma unroll
    for (int c = 0; c < 3; c++) {
      const double rprt = RP[3 * r] * Rp[c] + RP[3 * r + 1] * Rp[3 + c] + RP[3 * r + 2] * Rp[6 + c];
      out[3 * r + c] = ((rprt + Rv[r] * Rp[9 + c]) + Rv[c] * Rp[9 + r]) + (N * Rp[9 + r]) * Rp[9 + c];
    }
  o[0] = out[0]; o[1] = out[1]; o[2] = out[2]; o[3] = out[4]; o[4] = out[5]; o[5] = out[8];
#pragma unroll
  for (int r = 0; r < 3; r++) o[6 + r] = Rv[r] + N * Rp[9 + r];
  o[9] = N;
}

// The arithmetic of OctoTree::plane_update (voxel_map.hpp:1118-1146): clv the merged cluster, U / lam its eigenvectors (3 * column + row) / eigenvalues,
// CA the node's cov_add (column-major 9x9), ca9 its 3x3 variance block as the caller has already fetched it.  Out: the centre c and plane_var Pv
// (column-major 6x6, normal | centre).
VXM_FN void plane_update_math(const double* CA, const double* ca9, const double* clv, const double* U, const double* lam, double* c, double* Pv) {
  const double N = clv[9];
  const double nv = 1.0 / N;
  c[0] = clv[6] / N; c[1] = clv[7] / N; c[2] = clv[8] / N;
  double u_c[3][9];
  for (int r = 0; r < 3; r++)
    for (int q = 0; q < 9; q++) u_c[r][q] = 0.0;
  const double* ul = U;
  for (int k = 1; k < 3; k++) {
    const double* uk = U + 3 * k;
    const double kc = uk[0] * c[0] + uk[1] * c[1] + uk[2] * c[2], lc = ul[0] * c[0] + ul[1] * c[1] + ul[2] * c[2];
    const double fkl[9] = {uk[0] * ul[0], uk[1] * ul[0] + uk[0] * ul[1], uk[2] * ul[0] + uk[0] * ul[2], uk[1] * ul[1], uk[1] * ul[2] + uk[2] * ul[1], uk[2] * ul[2],
                           -(kc * ul[0] + lc * uk[0]), -(kc * ul[1] + lc * uk[1]), -(kc * ul[2] + lc * uk[2])};
    const double sc = nv / (lam[0] - lam[k]);
    for (int r = 0; r < 3; r++)
      for (int q = 0; q < 9; q++) u_c[r][q] += sc * uk[r] * fkl[q];
  }
  double Jc[3][9];
  for (int r = 0; r < 3; r++)
    for (int q = 0; q < 9; q++) {
      double t = 0.0;
      for (int k = 0; k < 9; k++) t += u_c[r][k] * CA[9 * q + k];
      Jc[r][q] = t;
    }
  for (int r = 0; r < 3; r++)
    for (int q = 0; q < 3; q++) {
      double t = 0.0;
      for (int k = 0; k < 9; k++) t += Jc[r][k] * u_c[q][k];
      Pv[6 * q + r] = t;
      const double jn = nv * Jc[r][6 + q];
      Pv[6 * (3 + q) + r] = jn;
      Pv[6 * r + 3 + q] = jn;
      Pv[6 * (3 + q) + 3 + r] = nv * nv * ca9[3 * q + r];
    }
}

}  // namespace vxmap
