// Per-scan and per-point arithmetic of the keyframe builder (include/vxba.h: vxba_keyframe_*), host + device: vxba_keyframe.hip runs it on the
// GPU and in its host shell, tests/hostmath/keyframe_hostcheck.cpp compiles the same text with g++ for the CPU suite.
//
// Reference: the front half of thd_loop_closure (voxelslam.cpp:1898-1977) and down_sampling_pvec (voxel_map.hpp:24-65).
//   rule       ang = |Log(x_key.R^T xc.R)| * 57.3, len = |xc.p - x_key.p|                                   (:1932-1933, Log: tools.hpp:86-91)
//   assembly   delta_p = xc.R^T (bl.p - xc.p), delta_R = xc.R^T bl.R, q = delta_R pnt + delta_p             (:1948-1952)
//   voxel      float l = q / vs; if (l < 0) l -= 1.0; (int64_t)l                                            (voxel_map.hpp:32-37)
//   mean       m = (m * c + v) / (c + 1), per element, c the int count so far                               (voxel_map.hpp:46-47)
// Association (pinned by tests/golden/keyframe/keyframe.npz, the reference's own down_sampling_pvec over the assembly loop restated on the
// shim's Eigen): every 3-term inner product is (a0 b0 + a1 b1) + a2 b2, the translation is added last, the mean divides -- a true division --
// after the multiply-add, nothing is fused.  Both translation units that include this file are compiled WITHOUT floating-point contraction.
//
// Layout: a pose record is [R column-major 9 | t 3] as everywhere in the ABI.
#pragma once
#include <math.h>
#include <stdint.h>

#if defined(__HIPCC__)
#define VXK_HD __host__ __device__ __forceinline__
#define VXK_UNROLL _Pragma("unroll")
#else
#define VXK_HD inline
#define VXK_UNROLL
#endif

namespace vxkf {

constexpr long long KEY_OFF = 1ll << 20;   // voxel indices in (-2^20, 2^20), like vxba_down_sampling_voxel
constexpr int KEY_BITS = 21;

// A^T B for two column-major 3 x 3: out(i, j) = (A(0,i) B(0,j) + A(1,i) B(1,j)) + A(2,i) B(2,j)
VXK_HD void mat_tmul(const double* A, const double* B, double* out) {
  VXK_UNROLL for (int j = 0; j < 3; j++)
    VXK_UNROLL for (int i = 0; i < 3; i++) out[3 * j + i] = (A[3 * i] * B[3 * j] + A[3 * i + 1] * B[3 * j + 1]) + A[3 * i + 2] * B[3 * j + 2];
}

// delta_R = xc.R^T bl.R (column-major), delta_p = xc.R^T (bl.p - xc.p): the pose of a buffered scan in the newest scan's frame
VXK_HD void delta_pose(const double* xc, const double* bl, double* dR, double* dp) {
  mat_tmul(xc, bl, dR);
  const double d0 = bl[9] - xc[9], d1 = bl[10] - xc[10], d2 = bl[11] - xc[11];
  VXK_UNROLL for (int i = 0; i < 3; i++) dp[i] = (xc[3 * i] * d0 + xc[3 * i + 1] * d1) + xc[3 * i + 2] * d2;
}

// q = delta_R pnt + delta_p
VXK_HD void transform_point(const double* dR, const double* dp, const double* p, double* q) {
  VXK_UNROLL for (int i = 0; i < 3; i++) q[i] = ((dR[i] * p[0] + dR[3 + i] * p[1]) + dR[6 + i] * p[2]) + dp[i];
}

// upstream's float-typed voxel index of one coordinate; the caller tests the range
VXK_HD long long voxel_index(double q, double vs) {
  float l = (float)(q / vs);
  if (l < 0) l = (float)((double)l - 1.0);
  return (long long)l;
}

// the 63-bit key of a point (x most significant: ascending keys = ascending (x, y, z) voxel index); false where a coordinate is not finite
// or an index lies outside (-2^20, 2^20) -- the key is then 0
VXK_HD bool voxel_key(const double* q, double vs, unsigned long long* key) {
  unsigned long long k = 0;
  bool ok = true;
  VXK_UNROLL for (int j = 0; j < 3; j++) {
    const float l0 = (float)(q[j] / vs);
    // a quotient beyond 2^20 in magnitude, an infinity or a NaN fails this test before any conversion to an integer
    if (!(l0 > -1048576.0f && l0 < 1048576.0f)) { ok = false; continue; }
    const long long pos = voxel_index(q[j], vs);
    if (pos <= -KEY_OFF || pos >= KEY_OFF) { ok = false; continue; }
    k = (k << KEY_BITS) | (unsigned long long)(pos + KEY_OFF);
  }
  *key = ok ? k : 0ull;
  return ok;
}

// one step of the running mean: c points are in m already
VXK_HD double mean_step(double m, int c, double v) { return (m * (double)c + v) / (double)(c + 1); }

// ang [deg, upstream's 57.3] and len of the keyframe rule
VXK_HD void rule_metrics(const double* x_key, const double* xc, double* ang, double* len) {
  double M[9];
  mat_tmul(x_key, xc, M);
  const double tr = (M[0] + M[4]) + M[8];
  const double theta = tr > 3.0 - 1e-6 ? 0.0 : acos(0.5 * (tr - 1));
  const double K[3] = {M[5] - M[7], M[6] - M[2], M[1] - M[3]};      // R(2,1) - R(1,2), R(0,2) - R(2,0), R(1,0) - R(0,1)
  const double s = fabs(theta) < 0.001 ? 0.5 : 0.5 * theta / sin(theta);
  const double w0 = s * K[0], w1 = s * K[1], w2 = s * K[2];
  *ang = sqrt((w0 * w0 + w1 * w1) + w2 * w2) * 57.3;
  const double d0 = xc[9] - x_key[9], d1 = xc[10] - x_key[10], d2 = xc[11] - x_key[11];
  *len = sqrt((d0 * d0 + d1 * d1) + d2 * d2);
}

}  // namespace vxkf
