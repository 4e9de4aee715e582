// Per-point and per-keyframe arithmetic of the loop hand-back (include/vxba.h: vxba_kfarchive_*), host + device: vxba_handback.hip runs it on the
// GPU and in its host shell, tests/hostmath/handback_hostcheck.cpp compiles the same text with g++ for the CPU suite.
//
// Reference: keyframe_loading (voxelslam.cpp:1189-1228), the tail of thd_loop_closure's optimisation branch (:2131-2167), loop_update (:1161-1168).
//   world      q = x0.R double(ap) + x0.p per keyframe point (:1216-1217, :2143-2144); q = xx.R pnt + xx.p per buffered scan point (:1166)
//   var        diag(double(normal[0..2])) for map_loop (:2145-2146), zero for keyframe_loading (:1210), the scan's own 3 x 3 for a buffered
//              scan (:1164); NEVER rotated, although the frame changes
//   search     pl_kdmap holds float32 positions (:2159-2162); the query is float32 (:1193-1196); squared distances are float32
// The pose algebra and its association are vxba_keyframe_math.hpp's (vxkf::transform_point: every inner product (a0 b0 + a1 b1) + a2 b2, the
// translation added last); the owner of an output row in the offset table is vxba_session_math.hpp's vxss::owner_of.  Both translation units
// that include this file are compiled WITHOUT floating-point contraction.
#pragma once
#include "vxba_session_math.hpp"

namespace vxhb {

// a float32 keyframe point under the pose [R column-major 9 | p 3], in float64
VXK_HD void world_point(const double* pose, const float* v, double* q) {
  const double p[3] = {(double)v[0], (double)v[1], (double)v[2]};
  vxkf::transform_point(pose, pose + 9, p, q);
}

// a float64 body point of a buffered scan under its pose
VXK_HD void world_point(const double* pose, const double* v, double* q) { vxkf::transform_point(pose, pose + 9, v, q); }

// entry c (0..8, column-major or row-major alike) of diag(double(v3), double(v4), double(v5))
VXK_HD double diag_entry(float v3, float v4, float v5, int c) { return c == 0 ? (double)v3 : c == 4 ? (double)v4 : c == 8 ? (double)v5 : 0.0; }

// the float32 squared distance the radius search compares: (dx dx + dy dy) + dz dz
VXK_HD float dist2(const float* a, const float* b) {
  const float dx = a[0] - b[0], dy = a[1] - b[1], dz = a[2] - b[2];
  return (dx * dx + dy * dy) + dz * dz;
}

// keyframe_loading's walk over a snapshot of n_hist float32 positions: among those with d2 < r2 (strict), ascending d2 and then ascending index,
// the first whose exist flag is set; -1 when there is none.  Candidates without the flag are skipped and do not end the walk.
inline long long nearest_existing(const float* snap, long long n_hist, const unsigned char* exist, const float* pc, float r2) {
  long long best = -1;
  float best_d2 = 0.0f;
  for (long long k = 0; k < n_hist; k++) {
    if (!exist[k]) continue;
    const float d2 = dist2(snap + 3 * k, pc);
    if (!(d2 < r2)) continue;
    if (best < 0 || d2 < best_d2) { best = k; best_d2 = d2; }      // an equal d2 keeps the lower index
  }
  return best;
}

}  // namespace vxhb
