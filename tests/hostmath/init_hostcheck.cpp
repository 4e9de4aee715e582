// Host build of the initialisation odometry's per-point arithmetic (voxel-slam_amd/csrc/vxba_init_math.hpp), checked against
// tests/_init_ref.py by tests/test_init_cpu.py.  Built by the test with: g++ -O2 -std=c++17 -fPIC -shared -ffp-contract=off
#include <cstdint>

#include "../../voxel-slam_amd/csrc/vxba_init_math.hpp"

using namespace vxin;

extern "C" {

// n neighbourhoods (5 x 3 row-major each): direct, the gate's verdict, its worst residual, and (n, d)
void inh_fit(int n, const double* A, double* direct, uint8_t* ok, double* worst, double* plane) {
  for (int k = 0; k < n; k++) {
    fit_plane5(A + 15 * k, direct + 3 * k);
    ok[k] = gate5(A + 15 * k, direct + 3 * k, worst[k]) ? 1 : 0;
    plane_of(direct + 3 * k, plane + 4 * k, plane[4 * k + 3]);
  }
}
// n points under ONE state [R col-major 9 | p 3]: world point, Jacobian row and residual for the planes (n, d) given
void inh_rows(int n, const double* state, const double* pnt, const double* plane, double* wld, double* jac, double* resid) {
  for (int k = 0; k < n; k++) {
    world_point(state, state + 9, pnt + 3 * k, wld + 3 * k);
    jac_row(state, pnt + 3 * k, plane + 4 * k, plane[4 * k + 3], wld + 3 * k, jac + 6 * k, resid[k]);
  }
}
// brute-force five nearest of every query by the product's distance and order (a plain insertion over the whole cloud)
void inh_knn(int M, const float* cloud, int n, const float* q, int32_t* idx, float* sqd) {
  for (int i = 0; i < n; i++) {
    float bd[NMATCH];
    int bi[NMATCH];
    for (int k = 0; k < NMATCH; k++) { bd[k] = INFINITY; bi[k] = 0x7fffffff; }
    for (int c = 0; c < M; c++) {
      float d = sqdist(cloud[3 * c], cloud[3 * c + 1], cloud[3 * c + 2], q[3 * i], q[3 * i + 1], q[3 * i + 2]);
      int j = c;
      for (int k = 0; k < NMATCH; k++)
        if (closer(d, j, bd[k], bi[k])) { const float td = bd[k]; const int ti = bi[k]; bd[k] = d; bi[k] = j; d = td; j = ti; }
    }
    for (int k = 0; k < NMATCH; k++) { idx[NMATCH * i + k] = bi[k] == 0x7fffffff ? -1 : bi[k]; sqd[NMATCH * i + k] = bd[k]; }
  }
}
// m points, each under its own IMU pose row (POSE_LEN doubles): the de-skew arithmetic; head < 0 rows use the extrinsic only
void inh_deskew(int m, const double* rows, const int32_t* has_pose, const double* xc, const double* ext, const float* P, const double* curv, double* out) {
  for (int k = 0; k < m; k++) {
    if (has_pose[k]) deskew_point(rows + POSE_LEN * k, xc, ext, P + 3 * k, curv[k], out + 3 * k);
    else extrinsic_point(ext, P + 3 * k, out + 3 * k);
  }
}
// K messages -> K - 1 mid-point samples under (bg, ba, scale)
void inh_midpoint(int K, const double* gyr, const double* acc, const double* bg, const double* ba, double scale, double* rate, double* a) {
  for (int t = 1; t < K; t++) midpoint_sample(gyr + 3 * (t - 1), gyr + 3 * t, acc + 3 * (t - 1), acc + 3 * t, bg, ba, scale, rate + 3 * (t - 1), a + 3 * (t - 1));
}
// n body points -> calcBodyVar's variance (and the point as it rewrites it), then pvec_update's world variance under (R, rot_var, tsl_var)
void inh_pointvar(int n, double* pnt, float range_inc, double dir_var, const double* R, const double* rot_var, const double* tsl_var, double* body_v, double* world_v) {
  for (int k = 0; k < n; k++) {
    body_var(pnt + 3 * k, range_inc, dir_var, body_v + 9 * k);
    world_var(R, pnt + 3 * k, body_v + 9 * k, rot_var, tsl_var, world_v + 9 * k);
  }
}
void inh_align_gravity(double* xs, int W) { align_gravity(xs, W); }
}
