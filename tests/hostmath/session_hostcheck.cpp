// Host build of the saved-session unit's arithmetic (voxel-slam_amd/csrc/vxba_session_math.hpp), checked against tests/_session_ref.py by
// tests/test_session_cpu.py.  Built by the test with: g++ -O2 -std=c++17 -fPIC -shared -ffp-contract=off
#include <cstdint>

#include "../../voxel-slam_amd/csrc/vxba_session_math.hpp"

extern "C" {

// n float32 points of frame xj in frame xc, float32
void ssh_move(int n, const double* xc, const double* xj, const float* p, float* out) {
  double dR[9], dp[3];
  vxkf::delta_pose(xc, xj, dR, dp);
  for (int k = 0; k < n; k++) vxss::move_point(dR, dp, p + 3 * k, out + 3 * k);
}
// n float32 points under the pose [R column-major | p] itself: the global map's expression
void ssh_pose(int n, const double* pose, const float* p, float* out) {
  for (int k = 0; k < n; k++) vxss::move_point(pose, pose + 9, p + 3 * k, out + 3 * k);
}
void ssh_keys(int n, const float* p, double vs, uint64_t* key, uint8_t* ok) {
  for (int k = 0; k < n; k++) {
    unsigned long long kk = 0;
    ok[k] = vxss::voxel_key(p + 3 * k, vs, &kk) ? 1 : 0;
    key[k] = kk;
  }
}
// the float running mean of n rows of three in order
void ssh_mean(int n, const float* rows, float* out) {
  for (int j = 0; j < 3; j++) out[j] = rows[j];
  float cur = 1.0f;
  for (int k = 1; k < n; k++, cur += 1.0f)
    for (int j = 0; j < 3; j++) out[j] = vxss::mean_step(out[j], cur, rows[3 * k + j]);
}
long long ssh_owner(const long long* ptr, long long n, long long g) { return vxss::owner_of(ptr, n, g); }
long long ssh_jump(long long psize, long long interval) { return vxss::map_jump(psize, interval); }
long long ssh_count(long long n, long long jump) { return vxss::map_count(n, jump); }
}
