// The control block of a device-resident iterated-EKF estimation, shared by the two odometries that run it: the scan-to-map one
// (vxba_lio.hip, lio_state_estimation) and the scan-to-cloud one of the initialisation (vxba_init.hip, lio_state_estimation_kdtree).
// Both enqueue VXBA_LIO_MAX_ITER rounds of (sweep, lio_ekf_kernel) and copy this block back once.
#pragma once

namespace vxl {

constexpr int NSUM = 34;         // HTH 21 | HTz 6 | nnt 6 | count
constexpr int SWEEP_OUT = 52;    // HTH 36 col-major | HTz 6 | nnt 9 col-major | match_num

struct LioCtl {
  double state[24], x_prop[24];   // x_curr (in/out) and the propagated state the call started from
  double cov[225], cov_inv[225];  // x_curr.cov (in/out), its inverse at entry (the initialisation passes cov^-1 / 1000)
  double G[90];                   // G.block<15,6>(0,0) of the last iteration
  double sweeps[4 * SWEEP_OUT];
  double info[4];                 // ok, iterations, match_num, smallest eigenvalue of nnt
  int rematch_num, iter, done, pad;
  // the initialisation's schedule (voxelslam.cpp:1065-1076): whether the next sweep searches again, whether any step has converged, which
  // iteration's per-point planes are the current ones, and the refind flag every sweep ran under
  int refind, converged, slot, pad2;
  int refind_trace[4];
};

}  // namespace vxl
