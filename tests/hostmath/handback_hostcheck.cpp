// Host build of the loop hand-back's arithmetic (voxel-slam_amd/csrc/vxba_handback_math.hpp), checked against tests/_handback_ref.py by
// tests/test_handback_cpu.py.  Built by the test with: g++ -O2 -std=c++17 -fPIC -shared -ffp-contract=off
#include <cstdint>

#include "../../voxel-slam_amd/csrc/vxba_handback_math.hpp"

extern "C" {

// n keyframe rows (x, y, z, var00, var11, var22 float32) under a pose: world points n x 3 and variances n x 9, as the kernel writes them
void hbh_keyframe(int n, const double* pose, const float* xyzv, double* pnt, double* var) {
  for (int k = 0; k < n; k++) {
    const float* r = xyzv + 6 * k;
    vxhb::world_point(pose, r, pnt + 3 * k);
    for (int c = 0; c < 9; c++) var[9 * k + c] = vxhb::diag_entry(r[3], r[4], r[5], c);
  }
}
// n float64 body points of a buffered scan under its pose
void hbh_scan(int n, const double* pose, const double* body, double* pnt) {
  for (int k = 0; k < n; k++) vxhb::world_point(pose, body + 3 * k, pnt + 3 * k);
}
void hbh_dist2(int n, const float* snap, const float* pc, float* out) {
  for (int k = 0; k < n; k++) out[k] = vxhb::dist2(snap + 3 * k, pc);
}
long long hbh_nearest(const float* snap, long long n, const unsigned char* exist, const float* pc, float r2) { return vxhb::nearest_existing(snap, n, exist, pc, r2); }
long long hbh_owner(const long long* ptr, long long n, long long g) { return vxss::owner_of(ptr, n, g); }
}
