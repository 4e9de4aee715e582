// Host build of the loop-edge registration's per-point and per-pair arithmetic (voxel-slam_amd/csrc/vxba_loopreg_math.hpp), checked against
// tests/_loopreg_ref.py by tests/test_loopreg_cpu.py.  Built by the test with: g++ -O2 -std=c++17 -fPIC -shared -ffp-contract=off
#include <cstdint>

#include "../../voxel-slam_amd/csrc/vxba_loopreg_math.hpp"

using namespace vxlr;

extern "C" {

// n (pose, source row, target row) triples: transformed centre and normal, the gate's verdict and n_t . (p - p_t)
void lrh_gate(int n, const double* poses, const float* src, const float* tar, const double* gates, double* p, double* nrm, uint8_t* ok, double* rr) {
  for (int k = 0; k < n; k++) {
    transform_plane(poses + 12 * k, src + 6 * k, p + 3 * k, nrm + 3 * k);
    ok[k] = gate(p + 3 * k, nrm + 3 * k, tar + 6 * k, gates, rr[k]) ? 1 : 0;
  }
}
void lrh_jac(int n, const double* poses, const float* src, const float* tar, double* jac) {
  for (int k = 0; k < n; k++) jac_row(poses + 12 * k, src + 6 * k, tar + 6 * k, jac + 6 * k);
}
// the 35 sums of n gated rows under ONE pose
void lrh_accumulate(int n, const double* pose, const float* src, const float* tar, const double* rr, double* acc) {
  for (int k = 0; k < ACC_LEN; k++) acc[k] = 0.0;
  for (int k = 0; k < n; k++) {
    double jac[6];
    jac_row(pose, src + 6 * k, tar + 6 * k, jac);
    accumulate(jac, tar + 6 * k, rr[k], acc);
  }
}
void lrh_solve(int n, const double* hu, const double* jt, double* dx) {
  for (int k = 0; k < n; k++) solve6(hu + 21 * k, jt + 6 * k, dx + 6 * k);
}
void lrh_exp(int n, const double* w, double* E) {
  for (int k = 0; k < n; k++) so3_exp(w + 3 * k, E + 9 * k);
}
void lrh_retract(int n, const double* P, const double* dx, double* out) {
  for (int k = 0; k < n; k++) retract(P + 12 * k, dx + 6 * k, out + 12 * k);
}
// a scripted run of the state machine: step k has match[k] gated rows and the step dx[k]; stops where the machine does.  states K x 5:
// [iter, done, is_converge, failed, step applied] after each step taken; returns the number of steps taken.
int lrh_state_machine(int K, const double* match, const double* dx, double step_tol, int max_iter, int* states) {
  IcpState st{0, 0, 0, 0};
  int k = 0;
  for (; k < K && !st.done; k++) {
    const bool apply = icp_advance(st, match[k], dx + 6 * k, step_tol, max_iter);
    states[5 * k] = st.iter; states[5 * k + 1] = st.done; states[5 * k + 2] = st.is_converge; states[5 * k + 3] = st.failed; states[5 * k + 4] = apply ? 1 : 0;
  }
  return k;
}
void lrh_voxel_coord(int n, const double* v, double voxel_size, int64_t* out) {
  for (int k = 0; k < n; k++) out[k] = (int64_t)voxel_coord(v[k], voxel_size);
}
}
