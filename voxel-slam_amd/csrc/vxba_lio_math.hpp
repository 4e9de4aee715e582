// Per-point arithmetic of the odometry's point-to-plane sweep (vxba_lio.hip: lio_sweep_kernel), host + device: the kernel runs it on the
// GPU, tests/hostmath/lio_hostcheck.cpp compiles the same text with g++ -ffp-contract=off for the CPU suite (tests/test_lio_cpu.py).
//
// Reference: lio_state_estimation voxelslam.cpp:873-919 with `match` voxel_map.hpp:1335-1392, 1674-1698.  Here: the key of a root voxel, the
// float-typed voxel index, the leaf test with both gates and sigma, and the column bookkeeping of the wave's reduce-scatter.  The descent to
// the finest cell and what a matched point adds to the 34 sums stay in vxba_lio.hip next to the table probe, the loads and the cross-lane
// exchange: as functions of this header they compile to another gfx950 instruction stream of lio_sweep_kernel (a branch's polarity; three
// instructions fewer), while everything here compiles to the stream the kernel had with the text in place.
#pragma once
#include <math.h>
#include <stddef.h>

#include "vxba_lio_ctl.hpp"

#if defined(__HIPCC__)
#define VXL_HD __host__ __device__ inline
#define VXL_FN __device__ inline
#define VXL_FI __device__ __forceinline__
#else
#define VXL_HD inline
#define VXL_FN inline
#define VXL_FI inline
// the host build is compiled without contraction: the rounded single operations are the plain operators
inline float __fsub_rn(float a, float b) { return a - b; }
inline float __fmul_rn(float a, float b) { return a * b; }
#endif

namespace vxl {

constexpr int PLANE_LEN = 32;    // f64 per plane record: center 3 | normal 3 | radius | hl | box centre 3 | plane_var upper triangle 21
constexpr unsigned long long EMPTY_KEY = ~0ull;
constexpr long long LOC_OFF = 1ll << 20;   // root voxel indices in [-2^20, 2^20)

struct MapView {
  const unsigned long long* keys;
  const int* cells;
  const double* planes;
  unsigned long long cap_mask;
  int cells_per_root;
  int max_layer;
  double voxel_size;
};

struct SweepArg {
  double R[9];        // column-major
  double p[3];
  double rot_var[9];  // cov.block<3,3>(0,0), column-major
  double tsl_var[9];  // cov.block<3,3>(3,3)
};

VXL_HD unsigned long long mix64(unsigned long long x) {
  x ^= x >> 33; x *= 0xff51afd7ed558ccdull; x ^= x >> 33; x *= 0xc4ceb9fe1a85ec53ull; x ^= x >> 33;
  return x;
}
VXL_HD bool pack_key(long long x, long long y, long long z, unsigned long long& key) {
  const long long a = x + LOC_OFF, b = y + LOC_OFF, c = z + LOC_OFF;
  if ((a | b | c) < 0 || a >= 2 * LOC_OFF || b >= 2 * LOC_OFF || c >= 2 * LOC_OFF) return false;
  key = ((unsigned long long)a << 42) | ((unsigned long long)b << 21) | (unsigned long long)c;
  return true;
}

// a*b rounded, then added / subtracted: what the reference's host build (x86-64 without FMA) computes.  The __fmul_rn / __dmul_rn
// intrinsics are plain operators in this toolchain and get contracted into v_fma after inlining; the pragma clears the contract
// flag on exactly these two instructions and survives inlining (checked in the ISA).
VXL_FI float mul_sub_unfused(float c, float a, float b) {
#pragma clang fp contract(off)
  const float p = a * b;
  return c - p;
}
VXL_FI double mul_add_unfused(double acc, double a, double b) {
#pragma clang fp contract(off)
  const double p = a * b;
  return acc + p;
}

// the float-typed voxel index of match() (voxel_map.hpp:1678-1685): double division, rounded to float, `-= 1` in float below zero,
// truncated to int64
VXL_FN long long voxel_index(double w, double voxel_size) {
  float loc = (float)(w / voxel_size);
  if (loc < 0.0f) loc = __fsub_rn(loc, 1.0f);
  return (long long)loc;
}

// the leaf test of OctoTree::match (voxel_map.hpp:1340-1365); float-typed quantities kept in float, unfused
VXL_FN bool plane_test(const double* __restrict__ pl, const double w[3], const SweepArg& a, const double pnt[3], const double var[6], double& sigma_d,
                                  double nrm[3], double& resi) {
  const double d0 = w[0] - pl[0], d1 = w[1] - pl[1], d2 = w[2] - pl[2];
  nrm[0] = pl[3]; nrm[1] = pl[4]; nrm[2] = pl[5];
  resi = nrm[0] * d0 + nrm[1] * d1 + nrm[2] * d2;
  const float dis_to_plane = (float)fabs(resi);
  const float dis_to_center = (float)(d0 * d0 + d1 * d1 + d2 * d2);
  const float range_dis = mul_sub_unfused(dis_to_center, dis_to_plane, dis_to_plane);
  const float radius = (float)pl[6];
  if (!(range_dis <= __fmul_rn(9.0f, radius))) return false;
  // J plane_var J^T with J = [d, -n]; the record holds the symmetrised upper triangle
  const double J[6] = {d0, d1, d2, -nrm[0], -nrm[1], -nrm[2]};
  const double* S = pl + 11;
  double sigma_l = 0.0;
  int k = 0;
#pragma unroll
  for (int r = 0; r < 6; r++) {
    double t = 0.0;
#pragma unroll
    for (int c = r; c < 6; c++, k++) t += S[k] * J[c] * (c == r ? 1.0 : 2.0);
    sigma_l += J[r] * t;
  }
  // n^T (R var R^T + phat rot_var phat^T + tsl_var) n  with  q = R^T n,  b = phat^T n = n x pnt
  const double q0 = a.R[0] * nrm[0] + a.R[1] * nrm[1] + a.R[2] * nrm[2];
  const double q1 = a.R[3] * nrm[0] + a.R[4] * nrm[1] + a.R[5] * nrm[2];
  const double q2 = a.R[6] * nrm[0] + a.R[7] * nrm[1] + a.R[8] * nrm[2];
  const double b0 = nrm[1] * pnt[2] - nrm[2] * pnt[1], b1 = nrm[2] * pnt[0] - nrm[0] * pnt[2], b2 = nrm[0] * pnt[1] - nrm[1] * pnt[0];
  sigma_l += q0 * (var[0] * q0 + 2.0 * (var[1] * q1 + var[2] * q2)) + q1 * (var[3] * q1 + 2.0 * var[4] * q2) + q2 * var[5] * q2;
  sigma_l += b0 * (a.rot_var[0] * b0 + a.rot_var[3] * b1 + a.rot_var[6] * b2) + b1 * (a.rot_var[1] * b0 + a.rot_var[4] * b1 + a.rot_var[7] * b2) +
             b2 * (a.rot_var[2] * b0 + a.rot_var[5] * b1 + a.rot_var[8] * b2);
  sigma_l += nrm[0] * (a.tsl_var[0] * nrm[0] + a.tsl_var[3] * nrm[1] + a.tsl_var[6] * nrm[2]) + nrm[1] * (a.tsl_var[1] * nrm[0] + a.tsl_var[4] * nrm[1] + a.tsl_var[7] * nrm[2]) +
             nrm[2] * (a.tsl_var[2] * nrm[0] + a.tsl_var[5] * nrm[1] + a.tsl_var[8] * nrm[2]);
  if (!((double)dis_to_plane < 3.0 * sqrt(sigma_l))) return false;
  sigma_d = sigma_l;
  return true;
}

// one butterfly step of the reduce-scatter, seen from one lane: it keeps M of its sums, the upper or the lower half
VXL_FI void scatter_step(bool up, int M, int& col, int& real) {
  if (up) { col += M; real -= M; } else { real = real < M ? real : M; }
}

}  // namespace vxl
