// Per-point arithmetic of the saved-session unit (include/vxba.h: vxba_session_*, vxba_globalmap), host + device: vxba_session.hip runs it on the GPU,
// tests/hostmath/session_hostcheck.cpp compiles the same text with g++ for the CPU suite.
//
// Reference: previous_map_read (voxelslam.cpp:307-448), pub_globalmap (:108-150), down_sampling_voxel (tools.hpp:201-238).
//   merge      delta_p = xc.R^T (xj.p - xc.p), delta_R = xc.R^T xj.R, pt = float(delta_R double(pp) + delta_p)          (:350-358, :385-393)
//   map        pp = float(xx.R double(ap) + xx.p)                                                                        (:135-137)
//   voxel      float loc = p / voxel_size; if (loc < 0) loc -= 1.0; (int64_t)loc -- on the FLOAT point, as down_sampling_voxel does  (tools.hpp:211-214)
//   mean       pp = (pp * curvature + p) / (curvature + 1) in float, curvature a float count                             (tools.hpp:227-230)
// The pose algebra and its association are vxba_keyframe_math.hpp's (vxkf::delta_pose, vxkf::transform_point); what is added here is the
// rounding to float32 that PointXYZI / PointType force between the stages, and the float filter of vxba_downsample.hip restated (that unit keeps
// its own text: its kernels are not touched).  Both translation units that include this file are compiled WITHOUT floating-point contraction.
#pragma once
#include "vxba_keyframe_math.hpp"

namespace vxss {

constexpr long long KEY_OFF = 1ll << 20;   // voxel indices in [-2^20, 2^20), like vxba_down_sampling_voxel

// a float32 point moved by (dR, dp) and rounded back to float32
VXK_HD void move_point(const double* dR, const double* dp, const float* v, float* out) {
  const double p[3] = {(double)v[0], (double)v[1], (double)v[2]};
  double q[3];
  vxkf::transform_point(dR, dp, p, q);
  out[0] = (float)q[0]; out[1] = (float)q[1]; out[2] = (float)q[2];
}

// the 63-bit voxel key of a float32 point (x most significant); false where a coordinate is not finite or its index lies outside [-2^20, 2^20):
// the range vxba_down_sampling_voxel accepts.  The comparison on the float comes first: nothing out of range is ever converted to an integer.
VXK_HD bool voxel_key(const float* v, double vs, unsigned long long* key) {
  unsigned long long k = 0;
  bool ok = true;
  VXK_UNROLL for (int j = 0; j < 3; j++) {
    float loc = (float)((double)v[j] / vs);
    if (loc < 0) loc = (float)((double)loc - 1.0);
    if (!(loc > -1048577.0f && loc < 1048576.0f)) { ok = false; continue; }
    const long long pos = (long long)loc;
    if (pos < -KEY_OFF || pos >= KEY_OFF) { ok = false; continue; }
    k = (k << 21) | (unsigned long long)(pos + KEY_OFF);
  }
  *key = ok ? k : 0ull;
  return ok;
}

// one step of down_sampling_voxel's running mean: `cur` points are in m already
VXK_HD float mean_step(float m, float cur, float v) { return (m * cur + v) / (cur + 1.0f); }

// the largest s in [0, n) with ptr[s] <= g, for a non-decreasing ptr[0 .. n] with ptr[0] <= g < ptr[n]: the owner of row g (empty owners are skipped)
template <class T>
VXK_HD long long owner_of(const T* ptr, long long n, long long g) {
  long long lo = 0, hi = n;      // invariant: ptr[lo] <= g < ptr[hi]
  while (hi - lo > 1) {
    const long long mid = (lo + hi) >> 1;
    if ((long long)ptr[mid] <= g) lo = mid; else hi = mid;
  }
  return lo;
}

// pub_globalmap's stride: psize / (10 * interval_size) + 1 in 64-bit arithmetic (upstream: uint, which wraps beyond 4.29e9 points)
VXK_HD long long map_jump(long long psize, long long interval_size) { return psize / (10 * interval_size) + 1; }
// points 0, jump, 2 jump, ... of a cloud of n
VXK_HD long long map_count(long long n, long long jump) { return n > 0 ? (n + jump - 1) / jump : 0; }

}  // namespace vxss
