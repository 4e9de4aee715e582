// Host build of IMUEKF's arithmetic (voxel-slam_amd/csrc/vxba_imuekf_math.hpp), checked against tests/_imuekf_ref.py by tests/test_imuekf_cpu.py.
// Built by the test with: g++ -O2 -std=c++17 -fPIC -shared -ffp-contract=off
#include <cstdint>
#include <vector>

#include "../../voxel-slam_amd/csrc/vxba_imuekf_math.hpp"

using namespace vxek;

namespace {
// the filter as 17 doubles: [init_flag | init_num | mean_acc 3 | mean_gyr 3 | scale_gravity | last_pcl_end_time | last_imu 7]
Filter load(const double* a) {
  Filter f;
  f.init_flag = (int)a[0]; f.init_num = (int)a[1];
  for (int k = 0; k < 3; k++) { f.mean_acc[k] = a[2 + k]; f.mean_gyr[k] = a[5 + k]; }
  f.scale_gravity = a[8]; f.last_pcl_end_time = a[9];
  for (int k = 0; k < 7; k++) f.last_imu[k] = a[10 + k];
  return f;
}
void store(const Filter& f, double* a) {
  a[0] = f.init_flag; a[1] = f.init_num;
  for (int k = 0; k < 3; k++) { a[2 + k] = f.mean_acc[k]; a[5 + k] = f.mean_gyr[k]; }
  a[8] = f.scale_gravity; a[9] = f.last_pcl_end_time;
  for (int k = 0; k < 7; k++) a[10 + k] = f.last_imu[k];
}
}  // namespace

extern "C" {

void ekh_imu_init(double* filt, int K, const double* stamps, const double* gyr, const double* acc) {
  Filter f = load(filt);
  imu_init(f, K, stamps, gyr, acc);
  store(f, filt);
}

void ekh_process_init(double* filt, int acc_in_g, int K, const double* stamps, const double* gyr, const double* acc, double end_time, double* state) {
  Filter f = load(filt);
  process_init(f, acc_in_g, K, stamps, gyr, acc, end_time, state + 21);
  store(f, filt);
}

// F_x and cov_w of one step, 15 x 15 column-major; noise = [cov_acc | cov_gyr | cov_bias_gyr | cov_bias_acc]
void ekh_step_matrices(const double* R, const double* rate, const double* acc, double dt, const double* noise, double* F, double* W) {
  Noise nz;
  for (int k = 0; k < 3; k++) { nz.cov_acc[k] = noise[k]; nz.cov_gyr[k] = noise[3 + k]; nz.cov_bias_gyr[k] = noise[6 + k]; nz.cov_bias_acc[k] = noise[9 + k]; }
  step_matrices(R, rate, acc, dt, nz, F, W);
}

// motion_blur: the forward half, then every point as the kernel's lanes treat it.  Returns propagate()'s code; *M heads, table M x 22, out n x 3.
int ekh_motion_blur(double* filt, const double* noise, int K, const double* stamps, const double* gyr, const double* acc, double beg_time, double end_time, double* state,
                    double* cov, double* table, int* M, double* imus_out, const double* ext, int64_t n, const float* xyz, const float* toff, float* out) {
  Filter f = load(filt);
  Noise nz;
  for (int k = 0; k < 3; k++) { nz.cov_acc[k] = noise[k]; nz.cov_gyr[k] = noise[3 + k]; nz.cov_bias_gyr[k] = noise[6 + k]; nz.cov_bias_acc[k] = noise[9 + k]; }
  const int rc = propagate(f, nz, K, stamps, gyr, acc, beg_time, end_time, state, cov, table, M, imus_out);
  if (rc != PROP_OK) return rc;
  store(f, filt);
  std::vector<double> dev((size_t)DEV_POSE_LEN * (*M > 0 ? *M : 1));
  for (int i = 0; i < *M; i++) hoist_row(table + (size_t)POSE_LEN * i, dev.data() + (size_t)DEV_POSE_LEN * i);
  for (int64_t q = 0; q < n; q++) deskew_scan_point(dev.data(), *M, state, ext, xyz, toff, q, out + 3 * q);
  return rc;
}

}  // extern "C"
