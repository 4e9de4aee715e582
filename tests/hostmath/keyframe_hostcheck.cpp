// Host build of the keyframe builder's arithmetic (voxel-slam_amd/csrc/vxba_keyframe_math.hpp), checked against tests/_keyframe_ref.py by
// tests/test_keyframe_cpu.py.  Built by the test with: g++ -O2 -std=c++17 -fPIC -shared -ffp-contract=off
#include <cstdint>

#include "../../voxel-slam_amd/csrc/vxba_keyframe_math.hpp"

using namespace vxkf;

extern "C" {

void kfh_delta(int n, const double* xc, const double* bl, double* dR, double* dp) {
  for (int k = 0; k < n; k++) delta_pose(xc + 12 * k, bl + 12 * k, dR + 9 * k, dp + 3 * k);
}
// n points under ONE (delta_R, delta_p)
void kfh_transform(int n, const double* dR, const double* dp, const double* p, double* q) {
  for (int k = 0; k < n; k++) transform_point(dR, dp, p + 3 * k, q + 3 * k);
}
void kfh_keys(int n, const double* q, double vs, uint64_t* key, uint8_t* ok) {
  for (int k = 0; k < n; k++) {
    unsigned long long kk = 0;
    ok[k] = voxel_key(q + 3 * k, vs, &kk) ? 1 : 0;
    key[k] = kk;
  }
}
// the running mean of n rows of six in order, starting from the first row with a count of one
void kfh_mean(int n, const double* rows, double* out) {
  for (int j = 0; j < 6; j++) out[j] = rows[j];
  for (int k = 1; k < n; k++)
    for (int j = 0; j < 6; j++) out[j] = mean_step(out[j], k, rows[6 * k + j]);
}
void kfh_rule(const double* x_key, const double* xc, double* ang_len) { rule_metrics(x_key, xc, ang_len, ang_len + 1); }
}
