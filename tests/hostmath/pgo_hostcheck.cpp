// Host build of the pose-graph optimiser's per-factor arithmetic (voxel-slam_amd/csrc/vxba_pgo_math.hpp), checked against
// tests/_pgo_ref.py by tests/test_pgo_cpu.py.  Built by the test with: g++ -O2 -std=c++17 -fPIC -shared -ffp-contract=off
#include "../../voxel-slam_amd/csrc/vxba_pgo_math.hpp"

using namespace vxpgo;

extern "C" {

// n between factors: Pi, Pj n x 12 pose records, Z n x 12 measurement records, w n x 6 -> e n x 6, Ji, Jj, B = Ji^T W Jj n x 36 (row-major)
void pgoh_between(int n, const double* Pi, const double* Pj, const double* Z, const double* w, double* e, double* Ji, double* Jj, double* B) {
  for (int f = 0; f < n; f++) {
    between_lin(Pi + 12 * f, Pj + 12 * f, Z + 12 * f, e + 6 * f, Ji + 36 * f, Jj + 36 * f);
    for (int r = 0; r < 6; r++)
      for (int c = 0; c < 6; c++) B[36 * f + 6 * r + c] = jtwj(Ji + 36 * f, w + 6 * f, Jj + 36 * f, r, c);
  }
}
void pgoh_between_residual(int n, const double* Pi, const double* Pj, const double* Z, double* e) {
  for (int f = 0; f < n; f++) between_residual(Pi + 12 * f, Pj + 12 * f, Z + 12 * f, e + 6 * f);
}
void pgoh_prior(int n, const double* Pi, const double* Z, double* e, double* J) {
  for (int f = 0; f < n; f++) prior_lin(Pi + 12 * f, Z + 12 * f, e + 6 * f, J + 36 * f);
}
void pgoh_retract(int n, const double* P, const double* dx, double* out) {
  for (int k = 0; k < n; k++) retract(P + 12 * k, dx + 6 * k, out + 12 * k);
}
void pgoh_inv6(int n, double* A) {
  for (int k = 0; k < n; k++) inv6_spd(A + 36 * k);
}
}
