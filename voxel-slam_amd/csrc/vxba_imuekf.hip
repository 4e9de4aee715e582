// IMUEKF on the GPU -- self-contained translation unit: the `vxba_imuekf_*` entry points of include/vxba.h.
//
// What it replaces (VoxelSLAM/src): `IMUEKF::process` (ekf_imu.hpp:41-214), the first link of both `initialization()` (voxelslam.cpp:1237) and the
// steady-state odometry (:1571), and the voxel filter with its < 500 fallback behind it (:1574-1581).
//
// The filter's state machine, IMU_init and the forward propagation with its 15 x 15 covariance run on the host in f64 (vxba_imuekf_math.hpp: at most
// 64 steps of 15 x 15 products -- microseconds).  The scan is de-skewed by one launch:
//
//   imuekf_deskew_kernel   one lane per point, 256-lane workgroups.  The pose table (M <= 64 heads x 24 doubles: 12 KB) goes to LDS once per
//                          workgroup, with the unit axis and |rate| of every head hoisted by the host.  A lane finds its head by binary search on
//                          the heads' times, evaluates one sin / cos pair in f64 and writes the float result to a SECOND buffer; a point at or
//                          before the first head is copied bit for bit.  Lane 0 of the scan walks every head earlier than point 0, latest first.
//
// Table, xyz and toff go up in ONE copy from one pinned staging block.  vxba_imuekf_process does not wait for the device: the staging block's
// reuse is guarded by an event that the next call finds complete.  vxba_imuekf_filter waits once per filter pass, inside the filter, for the voxel
// count.  Launches and waits do not depend on n.  The filtered cloud is handed on in device memory (vxba_lio_scan_raw_device); its consumers wait
// on this handle's stream through the event recorded behind the filter.
//
// vxba_imuekf_process_device is the same call with the scan taken from a scan intake's resident cloud (vxba_intake.hip): only the table goes up, the
// kernel reads the intake's buffers behind the intake's event, and the host walks over the scan are replaced by what the intake guarantees.
#include "vxba_wait.hpp"
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <cstdint>
#include <cstring>
#include <mutex>
#include <string>
#include <vector>

#include "../../include/vxba.h"
#include "vxba_dev.hpp"
#include "vxba_downsample.h"
#include "vxba_imuekf_math.hpp"
#include "vxba_internal.h"

namespace vxek {

struct DeskewArg { double xc[12]; double ext[12]; };

__global__ __launch_bounds__(256) void imuekf_deskew_kernel(const double* __restrict__ table, int M, const float* __restrict__ xyz, const float* __restrict__ toff, long long n,
                                                            DeskewArg a, float* __restrict__ out) {
  __shared__ double tab[MAX_HEADS * DEV_POSE_LEN];
  const int len = (M < MAX_HEADS ? M : MAX_HEADS) * DEV_POSE_LEN;
  for (int i = threadIdx.x; i < len; i += 256) tab[i] = table[i];
  __syncthreads();
  const long long q = (long long)blockIdx.x * 256 + threadIdx.x;
  if (q >= n) return;
  float o[3];
  deskew_scan_point(tab, M < MAX_HEADS ? M : MAX_HEADS, a.xc, a.ext, xyz, toff, q, o);
  out[3 * q] = o[0]; out[3 * q + 1] = o[1]; out[3 * q + 2] = o[2];
}

constexpr size_t TABLE_BYTES = (size_t)MAX_HEADS * DEV_POSE_LEN * sizeof(double);

}  // namespace vxek

struct vxba_imuekf {
  int device = 0;
  vxu::Stream s;
  vxu::Event ev_staged, ev_filtered;
  bool staged_pending = false;
  vxu::Event ev_prof[4];   // vxba_imuekf_set_profiling: around the de-skew (upload + kernel) and around the filter
  bool profiling = false, prof_deskew = false, prof_filter = false;
  vxba_imuekf_params prm;
  vxek::Filter f;
  vxu::Pin<char> h_stage;        // pinned: [table | xyz 12 n | toff 4 n]
  vxu::Dev<char> d_in;           // the same layout on the device
  vxu::Dev<float> d_desk;        // the de-skewed cloud, n x 3
  vxu::Dev<float> d_filt;        // the filtered cloud, up to n x 3
  int64_t cap() const { return (int64_t)d_filt.capacity() / 3; }      // points; the four grow together, d_filt last
  int64_t n = 0, n_filt = 0;
  int M = 0, passes = 0;
  double table[vxek::MAX_HEADS * vxek::POSE_LEN];
  vxd::Scratch ds;
  int64_t launches = 0, waits = 0;
  std::string err;
  std::recursive_mutex mtx;
};

namespace {

#define EK_LOCK(h) std::lock_guard<std::recursive_mutex> lk__((h)->mtx)

// the filtered clouds that are handed on in device memory, and the event behind each one's last filter
std::mutex g_reg_mtx;
struct Produced { const void* ptr; hipEvent_t ev; };
std::vector<Produced> g_reg;

void reg_remove(const void* p) {
  std::lock_guard<std::mutex> lk(g_reg_mtx);
  g_reg.erase(std::remove_if(g_reg.begin(), g_reg.end(), [&](const Produced& x) { return x.ptr == p; }), g_reg.end());
}
void reg_add(const void* p, hipEvent_t ev) {
  std::lock_guard<std::mutex> lk(g_reg_mtx);
  g_reg.push_back({p, ev});
}

bool finite_all(const double* a, size_t n) { for (size_t i = 0; i < n; i++) if (!std::isfinite(a[i])) return false; return true; }
bool finite_all(const float* a, size_t n) { for (size_t i = 0; i < n; i++) if (!std::isfinite(a[i])) return false; return true; }

vxek::Noise noise_of(const vxba_imuekf_params& p) {
  vxek::Noise z;
  std::memcpy(z.cov_acc, p.cov_acc, sizeof z.cov_acc); std::memcpy(z.cov_gyr, p.cov_gyr, sizeof z.cov_gyr);
  std::memcpy(z.cov_bias_gyr, p.cov_bias_gyr, sizeof z.cov_bias_gyr); std::memcpy(z.cov_bias_acc, p.cov_bias_acc, sizeof z.cov_bias_acc);
  return z;
}

// room for n points everywhere; what the buffers hold is not kept
int ek_reserve(vxba_imuekf* h, int64_t n) {
  if (n <= h->cap()) return VXBA_OK;
  VX_HIP(h, hipStreamSynchronize(h->s));
  h->waits += 1;
  h->staged_pending = false;
  const int64_t cap = (std::max<int64_t>(n, 2 * h->cap()) + 255) / 256 * 256;
  if (h->d_filt) reg_remove(h->d_filt);      // the registry of produced clouds is keyed on the pointer: out before the block goes, in again below
  h->h_stage.release(); h->d_in.release(); h->d_desk.release(); h->d_filt.release();
  h->n = 0; h->n_filt = 0;
  const size_t bytes = vxek::TABLE_BYTES + (size_t)cap * 16;
  VX_HIP(h, h->h_stage.reserve(bytes));
  VX_HIP(h, h->d_in.reserve(bytes));
  VX_HIP(h, h->d_desk.reserve((size_t)cap * 3));
  VX_HIP(h, h->d_filt.reserve((size_t)cap * 3));
  reg_add(h->d_filt, h->ev_filtered);
  return VXBA_OK;
}

void ek_reset(vxba_imuekf* h) {
  h->f = vxek::Filter();
  h->n = 0; h->n_filt = 0; h->M = 0; h->passes = 0; h->launches = 0; h->waits = 0;
}

}  // namespace

// the consumer's half of the device route: `consumer_stream` waits for the filter that produced d_ptr.  1: enqueued; 0: not a cloud of this unit
extern "C" int vxba_internal_wait_for_producer(const void* d_ptr, void* consumer_stream) {
  std::lock_guard<std::mutex> lk(g_reg_mtx);
  for (const Produced& x : g_reg) {
    if (x.ptr != d_ptr) continue;
    return hipStreamWaitEvent((hipStream_t)consumer_stream, x.ev, 0) == hipSuccess ? 1 : -1;
  }
  return 0;
}

extern "C" {

void vxba_imuekf_default_params(vxba_imuekf_params* p) {
  if (!p) return;
  std::memset(p, 0, sizeof *p);
  for (int k = 0; k < 3; k++) { p->cov_acc[k] = 0.1; p->cov_gyr[k] = 0.1; p->cov_bias_gyr[k] = 1e-4; p->cov_bias_acc[k] = 1e-4; }
  p->ext[0] = p->ext[4] = p->ext[8] = 1.0;
  p->acc_in_g = 1;
  p->point_notime = 0;
}

int vxba_imuekf_create(int device, const vxba_imuekf_params* params, vxba_imuekf** out) {
  if (!out) return VXBA_ERR_ARG;
  *out = nullptr;
  vxba_imuekf_params prm;
  if (params) prm = *params; else vxba_imuekf_default_params(&prm);
  if (!finite_all(prm.cov_acc, 12) || !finite_all(prm.ext, 12)) return VXBA_ERR_ARG;
  if (const int rc = vxu::select_device(device)) return rc;
  vxba_imuekf* h = new vxba_imuekf();
  h->device = device;
  h->prm = prm;
  if (h->s.create() != hipSuccess || h->ev_staged.create(hipEventDisableTiming) != hipSuccess || h->ev_filtered.create(hipEventDisableTiming) != hipSuccess) {
    delete h;
    return VXBA_ERR_HIP;
  }
  *out = h;
  return VXBA_OK;
}

int vxba_imuekf_destroy(vxba_imuekf* h) {
  if (!h) return VXBA_ERR_ARG;
  hipSetDevice(h->device);
  if (h->s) hipStreamSynchronize(h->s);
  if (h->d_filt) reg_remove(h->d_filt);
  h->ds.release();
  delete h;
  return VXBA_OK;
}

const char* vxba_imuekf_last_error(const vxba_imuekf* h) { return h ? h->err.c_str() : "null handle"; }

int vxba_imuekf_clear(vxba_imuekf* h) {
  if (!h) return VXBA_ERR_ARG;
  EK_LOCK(h);
  ek_reset(h);
  return VXBA_OK;
}

int vxba_imuekf_reinit(vxba_imuekf* h, int K, const double* stamps, const double* gyr, const double* acc, double scale, double* g_out) {
  if (!h || K < 1 || !stamps || !gyr || !acc || !g_out) return VXBA_ERR_ARG;
  EK_LOCK(h);
  if (!finite_all(stamps, (size_t)K) || !finite_all(gyr, (size_t)3 * K) || !finite_all(acc, (size_t)3 * K) || !std::isfinite(scale))
    return vxu::fail(h, VXBA_ERR_ARG, "vxba_imuekf_reinit: an input is not finite");
  for (int r = 0; r < 3; r++) h->f.mean_acc[r] = 0.0;          // voxelslam.cpp:1302-1305; mean_gyr is overwritten by the first message
  h->f.init_num = 0;
  vxek::imu_init(h->f, K, stamps, gyr, acc);
  for (int r = 0; r < 3; r++) g_out[r] = -h->f.mean_acc[r] * scale;
  return VXBA_OK;
}

// process() on either route.  dev == NULL: xyz / toff are host arrays, checked here and uploaded behind the pose table; otherwise the scan is the
// resident cloud of a scan intake, which guarantees what the host checks look for (finite, non-decreasing, n >= 1), and only the table goes up.
struct DevScan { const float* d_xyz; const float* d_toff; float toff_first; hipEvent_t ev; };

static int ek_process(vxba_imuekf* h, int64_t n, const float* xyz, const float* toff, const DevScan* dev, int K, const double* stamps, const double* gyr, const double* acc,
                      double beg_time, double end_time, double* state, double* cov, double* imus_out, int* K_out, double* info) {
  if (!h || !state || !cov || K < 1 || !stamps || !gyr || !acc || n < 0 || n >= ((int64_t)1 << 31)) return h ? vxu::fail(h, VXBA_ERR_ARG, "vxba_imuekf_process: bad argument") : VXBA_ERR_ARG;
  EK_LOCK(h);
  if (!finite_all(stamps, (size_t)K) || !finite_all(gyr, (size_t)3 * K) || !finite_all(acc, (size_t)3 * K) || !std::isfinite(beg_time) || !std::isfinite(end_time) ||
      !finite_all(state, vxek::STATE_LEN) || !finite_all(cov, vxek::DIM * vxek::DIM))
    return vxu::fail(h, VXBA_ERR_ARG, "vxba_imuekf_process: an input is not finite");
  if (K_out) *K_out = 0;
  if (!h->f.init_flag) {
    vxek::process_init(h->f, h->prm.acc_in_g, K, stamps, gyr, acc, end_time, state + 21);
    if (info) { std::memset(info, 0, 8 * sizeof(double)); info[5] = h->f.scale_gravity; info[6] = (double)h->f.init_num; }
    return VXBA_OK;
  }
  const bool notime = h->prm.point_notime != 0;
  if (n == 0 || (!dev && (!xyz || (!notime && !toff)))) return vxu::fail(h, VXBA_ERR_ARG, "vxba_imuekf_process: an empty scan");
  if (!dev && (!finite_all(xyz, (size_t)3 * n) || (toff && !finite_all(toff, (size_t)n)))) return vxu::fail(h, VXBA_ERR_ARG, "vxba_imuekf_process: a scan value is not finite");
  if (h->f.last_pcl_end_time - beg_time > 0.01) return vxu::fail(h, VXBA_ERR_ARG, "vxba_imuekf_process: LiDAR time regress");
  if (!notime && !dev) for (int64_t i = 1; i < n; i++) if (toff[i] < toff[i - 1]) return vxu::fail(h, VXBA_ERR_ARG, "vxba_imuekf_process: toff is not non-decreasing");
  if (stamps[0] < h->f.last_imu[0]) return vxu::fail(h, VXBA_ERR_ARG, "vxba_imuekf_process: IMU stamps go back behind the last message");
  for (int t = 1; t < K; t++) if (stamps[t] < stamps[t - 1]) return vxu::fail(h, VXBA_ERR_ARG, "vxba_imuekf_process: IMU stamps are not non-decreasing");

  // propagation on copies: a refusal leaves the handle, state and cov as they were
  vxek::Filter f = h->f;
  double st[vxek::STATE_LEN], cv[vxek::DIM * vxek::DIM], table[vxek::MAX_HEADS * vxek::POSE_LEN];
  std::memcpy(st, state, sizeof st); std::memcpy(cv, cov, sizeof cv);
  int M = 0;
  std::vector<double> edited((size_t)7 * (K + 1));
  const int pr = vxek::propagate(f, noise_of(h->prm), K, stamps, gyr, acc, beg_time, end_time, st, cv, table, &M, edited.data());
  if (pr == vxek::PROP_NO_PAIR) return vxu::fail(h, VXBA_ERR_ARG, "vxba_imuekf_process: no IMU pair reaches the last scan's end");
  if (pr == vxek::PROP_TOO_MANY) return vxu::fail(h, VXBA_ERR_UNSUPPORTED, "vxba_imuekf_process: more than 64 IMU heads in one scan");

  VX_HIP(h, hipSetDevice(h->device));
  h->launches = 0; h->waits = 0; h->passes = 0;
  if (const int rc = ek_reserve(h, n)) return rc;
  if (h->staged_pending) {                                   // the staging block's last upload: complete long ago unless calls come back to back
    if (hipEventQuery(h->ev_staged) != hipSuccess) { VX_HIP(h, vxwait::event_wait(h->ev_staged)); h->waits += 1; }
    h->staged_pending = false;
  }
  const int Mk = notime ? 0 : M;                             // point_notime: no head, every point is copied through
  double* t24 = (double*)h->h_stage.get();
  for (int i = 0; i < Mk; i++) vxek::hoist_row(table + (size_t)vxek::POSE_LEN * i, t24 + (size_t)vxek::DEV_POSE_LEN * i);
  float* s_xyz = (float*)(h->h_stage + vxek::TABLE_BYTES);
  float* s_t = s_xyz + 3 * (size_t)n;
  if (!dev) {
    std::memcpy(s_xyz, xyz, (size_t)n * 12);
    if (toff) std::memcpy(s_t, toff, (size_t)n * 4); else std::memset(s_t, 0, (size_t)n * 4);
  }
  h->prof_deskew = false; h->prof_filter = false;
  if (h->profiling) VX_HIP(h, hipEventRecord(h->ev_prof[0], h->s));
  if (dev) VX_HIP(h, hipStreamWaitEvent(h->s, dev->ev, 0));   // the intake's gather
  VX_HIP(h, hipMemcpyAsync(h->d_in, h->h_stage, vxek::TABLE_BYTES + (dev ? 0 : (size_t)n * 16), hipMemcpyHostToDevice, h->s));
  VX_HIP(h, hipEventRecord(h->ev_staged, h->s));
  h->staged_pending = true;
  vxek::DeskewArg a;
  std::memcpy(a.xc, st, sizeof a.xc); std::memcpy(a.ext, h->prm.ext, sizeof a.ext);
  const float* d_xyz = dev ? dev->d_xyz : (const float*)(h->d_in + vxek::TABLE_BYTES);
  const float* d_toff = dev ? dev->d_toff : d_xyz + 3 * (size_t)n;
  vxek::imuekf_deskew_kernel<<<vxu::blocks_for(n), 256, 0, h->s>>>((const double*)h->d_in.get(), Mk, d_xyz, d_toff, (long long)n, a, h->d_desk);
  VX_HIP(h, hipGetLastError());
  h->launches += 1;
  if (h->profiling) { VX_HIP(h, hipEventRecord(h->ev_prof[1], h->s)); h->prof_deskew = true; }

  // commit
  h->f = f; h->M = M; h->n = n; h->n_filt = 0;
  std::memcpy(h->table, table, sizeof(double) * (size_t)vxek::POSE_LEN * M);
  std::memcpy(state, st, sizeof st); std::memcpy(cov, cv, sizeof cv);
  if (imus_out) std::memcpy(imus_out, edited.data(), edited.size() * sizeof(double));
  if (K_out) *K_out = K + 1;
  if (info) {
    int64_t moved = 0, apps = 0;
    if (!notime && dev) {                                    // the points compensated would take a host wait to count
      moved = -1;
      for (int i = 0; i < M; i++) apps += table[(size_t)vxek::POSE_LEN * i] < (double)dev->toff_first ? 1 : 0;
    } else if (!notime) {
      const double t0 = table[0];
      int64_t lo = 0, hi = n;                                // the first point with toff > t_0
      while (lo < hi) { const int64_t mid = (lo + hi) / 2; if ((double)toff[mid] > t0) hi = mid; else lo = mid + 1; }
      moved = n - lo;
      for (int i = 0; i < M; i++) apps += table[(size_t)vxek::POSE_LEN * i] < (double)toff[0] ? 1 : 0;
    }
    info[0] = 1.0; info[1] = (double)M; info[2] = (double)moved; info[3] = (double)apps; info[4] = end_time; info[5] = h->f.scale_gravity;
    info[6] = (double)h->f.init_num; info[7] = 0.0;
  }
  return VXBA_OK;
}

int vxba_imuekf_process(vxba_imuekf* h, int64_t n, const float* xyz, const float* toff, int K, const double* stamps, const double* gyr, const double* acc, double beg_time,
                        double end_time, double* state, double* cov, double* imus_out, int* K_out, double* info) {
  return ek_process(h, n, xyz, toff, nullptr, K, stamps, gyr, acc, beg_time, end_time, state, cov, imus_out, K_out, info);
}

int vxba_imuekf_process_device(vxba_imuekf* h, vxba_intake* intake, int K, const double* stamps, const double* gyr, const double* acc, double beg_time, double end_time,
                               double* state, double* cov, double* imus_out, int* K_out, double* info) {
  if (!h || !intake) return h ? vxu::fail(h, VXBA_ERR_ARG, "vxba_imuekf_process_device: bad argument") : VXBA_ERR_ARG;
  DevScan dev;
  long long n = 0;
  void* ev = nullptr;
  int device = -1;
  if (vxba_internal_intake_view(intake, &dev.d_xyz, &dev.d_toff, &n, &dev.toff_first, &ev, &device) != VXBA_OK || device != h->device)
    return vxu::fail(h, VXBA_ERR_ARG, "vxba_imuekf_process_device: the intake lives on another device");
  dev.ev = (hipEvent_t)ev;
  return ek_process(h, (int64_t)n, nullptr, nullptr, &dev, K, stamps, gyr, acc, beg_time, end_time, state, cov, imus_out, K_out, info);
}

int vxba_imuekf_read_scan(vxba_imuekf* h, float* xyz_out) {
  if (!h || !xyz_out) return VXBA_ERR_ARG;
  EK_LOCK(h);
  if (h->n == 0) return vxu::fail(h, VXBA_ERR_STATE, "vxba_imuekf_read_scan: no scan");
  VX_HIP(h, hipSetDevice(h->device));
  VX_HIP(h, hipMemcpyAsync(xyz_out, h->d_desk, (size_t)h->n * 12, hipMemcpyDeviceToHost, h->s));
  VX_HIP(h, hipStreamSynchronize(h->s));
  return VXBA_OK;
}

int vxba_imuekf_pose_table(const vxba_imuekf* h, double* table) {
  if (!h || !table) return VXBA_ERR_ARG;
  if (h->M > 0) std::memcpy(table, h->table, sizeof(double) * (size_t)vxek::POSE_LEN * h->M);
  return VXBA_OK;
}

int vxba_imuekf_filter(vxba_imuekf* h, double down_size, int64_t min_points, int64_t* n_out) {
  if (!h || !n_out || !std::isfinite(down_size)) return VXBA_ERR_ARG;
  EK_LOCK(h);
  *n_out = 0;
  if (h->n == 0) return vxu::fail(h, VXBA_ERR_STATE, "vxba_imuekf_filter: no scan");
  VX_HIP(h, hipSetDevice(h->device));
  h->n_filt = 0; h->passes = 0;
  int64_t kept = 0;
  double size = down_size;
  h->prof_filter = false;
  if (h->profiling) VX_HIP(h, hipEventRecord(h->ev_prof[2], h->s));
  for (int pass = 0; pass < 2; pass++, size = down_size / 2) {            // voxelslam.cpp:1574-1581: too few points -> again from the full cloud at half the size
    const int rc = vxd::downsample_device(h->ds, h->s, h->d_desk, h->n, size, h->d_filt, &kept);
    if (rc != VXBA_OK) return vxu::fail(h, rc, "vxba_imuekf_filter: the voxel filter failed (a point beyond 2^20 voxels of the origin?)");
    h->passes += 1;
    if (size >= 0.001) { h->launches += 3; h->waits += 1; }               // key, widen, mean; the wait for the voxel count
    if (kept >= min_points) break;
  }
  VX_HIP(h, hipEventRecord(h->ev_filtered, h->s));
  if (h->profiling) { VX_HIP(h, hipEventRecord(h->ev_prof[3], h->s)); h->prof_filter = true; }
  h->n_filt = kept;
  *n_out = kept;
  return VXBA_OK;
}

int vxba_imuekf_filter_passes(const vxba_imuekf* h) { return h ? h->passes : -1; }

int vxba_imuekf_filtered(vxba_imuekf* h, float* xyz_out) {
  if (!h || (h->n_filt > 0 && !xyz_out)) return VXBA_ERR_ARG;
  EK_LOCK(h);
  if (h->n_filt == 0) return VXBA_OK;
  VX_HIP(h, hipSetDevice(h->device));
  VX_HIP(h, hipMemcpyAsync(xyz_out, h->d_filt, (size_t)h->n_filt * 12, hipMemcpyDeviceToHost, h->s));
  VX_HIP(h, hipStreamSynchronize(h->s));
  return VXBA_OK;
}

int vxba_imuekf_filtered_device(vxba_imuekf* h, const float** d_xyz, int64_t* n) {
  if (!h || !d_xyz || !n) return VXBA_ERR_ARG;
  EK_LOCK(h);
  *d_xyz = h->n_filt > 0 ? h->d_filt : nullptr;
  *n = h->n_filt;
  return VXBA_OK;
}

int vxba_imuekf_set_profiling(vxba_imuekf* h, int enable) {
  if (!h) return VXBA_ERR_ARG;
  EK_LOCK(h);
  VX_HIP(h, hipSetDevice(h->device));
  for (vxu::Event& e : h->ev_prof) if (enable) VX_HIP(h, e.create());
  h->profiling = enable != 0;
  h->prof_deskew = false; h->prof_filter = false;
  return VXBA_OK;
}

int vxba_imuekf_stage_times(vxba_imuekf* h, double out_ms[2]) {
  if (!h || !out_ms) return VXBA_ERR_ARG;
  EK_LOCK(h);
  out_ms[0] = out_ms[1] = -1.0;
  if (!h->profiling) return vxu::fail(h, VXBA_ERR_STATE, "vxba_imuekf_stage_times: profiling is off");
  VX_HIP(h, hipSetDevice(h->device));
  VX_HIP(h, hipStreamSynchronize(h->s));
  float ms = 0.f;
  if (h->prof_deskew) { VX_HIP(h, hipEventElapsedTime(&ms, h->ev_prof[0], h->ev_prof[1])); out_ms[0] = (double)ms; }
  if (h->prof_filter) { VX_HIP(h, hipEventElapsedTime(&ms, h->ev_prof[2], h->ev_prof[3])); out_ms[1] = (double)ms; }
  return VXBA_OK;
}

int vxba_imuekf_stats(const vxba_imuekf* h, int64_t out[4]) {
  if (!h || !out) return VXBA_ERR_ARG;
  out[0] = h->launches; out[1] = h->waits; out[2] = h->n; out[3] = h->n_filt;
  return VXBA_OK;
}

}  // extern "C"
