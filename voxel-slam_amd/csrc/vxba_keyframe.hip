// Keyframes on the GPU (include/vxba.h: vxba_keyframe_*): the front half of thd_loop_closure (voxelslam.cpp:1898-1977) -- the ScanPose buffer, the
// keyframe rule, the merge of win_size marginalised scans into the newest pose's frame -- and down_sampling_pvec(voxel_size / 10)
// (voxel_map.hpp:24-65).  What local mapping hands over (a pose, its v6 and the scan's body points with their covariances) goes in; what the loop
// chain (`plbtc`, :1967-1974 -> vxba_loopreg_add_keyframe_device) and the hierarchical BA (`smp->plptr`, :1965 -> vxba_hba_add_keyframes_device)
// start from comes out, and stays on the device in between.
//
// The handle keeps the buffered scans resident: body points n x 3 float64 and the DIAGONAL of every point's covariance (every later operation
// on `var` is element-wise and only var(0,0), var(1,1), var(2,2) are emitted).  Upstream carries `var` through the merge UNROTATED -- pv.pnt is
// transformed, pv.var is not (:1950-1954) -- although the frame changes; that oddity is kept: the variances are copied as they came.
//
// Launch plan of an emitting push, N = sum of the buffered scans' points:
//   kf_assemble_kernel  one lane per point, grid (blocks of the longest scan, win_size): q = delta_R pnt + delta_p in float64, the `full` row in
//                       float32, the (q, var diagonal) row the filter gathers from, the 63-bit voxel key and the point's index; a coordinate that
//                       is not finite or a voxel index outside (-2^20, 2^20) raises a flag word in mapped host memory.
//   rocPRIM             stable radix_sort_pairs (key, index); run_length_encode; exclusive_scan of the counts over N + 1 words (the number of
//                       occupied voxels stays on the device, so nothing has to be waited for).
//   kf_filter_kernel    one lane per occupied voxel replays upstream's running mean over its points in input order -- per element
//                       m = (m * c + v) / (c + 1), a true division, nothing fused -- and writes the `down` row in float32; rows ascend by voxel index.
// Five enqueues and one memset, whatever N; ONE host wait at the end reads the flag and the voxel count.  The outputs are double-buffered: a push
// that fails (VXBA_ERR_ARG) leaves the previous keyframe readable and the buffer, buf_base, x_key and jour as they were.
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdint>
#include <cstring>
#include <deque>
#include <string>
#include <vector>

#include "../../include/vxba.h"
#include "vxba_dev.hpp"
#include "vxba_keyframe_math.hpp"
#include "vxba_wait.hpp"

namespace vxkf {

constexpr int MAX_WIN = 64;
constexpr int BLK = 256;
constexpr int64_t MAX_SCAN = (int64_t)1 << 26;     // points per scan: N = win_size scans stays below 2^32

struct ScanEntry {      // one buffered scan as the assembly kernel sees it
  double dR[9], dp[3];
  const double* pnt;    // n x 3
  const double* var;    // n x 3 (diagonal)
  long long n, off;     // points, and the first row of the scan in the keyframe
};

// the device-pointer route of a push: body points and the covariance diagonal into the handle's slot; flags[0] <- 1 at a coordinate that is not finite
__global__ void __launch_bounds__(BLK) kf_ingest_kernel(const double* __restrict__ pnt, const double* __restrict__ var9, long long n, double* __restrict__ out_pnt,
                                                        double* __restrict__ out_var, unsigned int* __restrict__ flags) {
  const long long j = (long long)blockIdx.x * BLK + threadIdx.x;
  if (j >= n) return;
  const double x = pnt[3 * j], y = pnt[3 * j + 1], z = pnt[3 * j + 2];
  if (!(isfinite(x) && isfinite(y) && isfinite(z))) flags[0] = 1u;
  out_pnt[3 * j] = x; out_pnt[3 * j + 1] = y; out_pnt[3 * j + 2] = z;
  out_var[3 * j] = var9 ? var9[9 * j] : 0.0; out_var[3 * j + 1] = var9 ? var9[9 * j + 4] : 0.0; out_var[3 * j + 2] = var9 ? var9[9 * j + 8] : 0.0;
}

__global__ void __launch_bounds__(BLK) kf_assemble_kernel(const ScanEntry* __restrict__ tab, double vs, float* __restrict__ full, double* __restrict__ rows,
                                                          unsigned long long* __restrict__ key, unsigned int* __restrict__ idx, unsigned int* __restrict__ flags) {
#pragma clang fp contract(off)
  const ScanEntry& e = tab[blockIdx.y];
  const long long j = (long long)blockIdx.x * BLK + threadIdx.x;
  if (j >= e.n) return;
  const double p[3] = {e.pnt[3 * j], e.pnt[3 * j + 1], e.pnt[3 * j + 2]};
  double q[3];
  transform_point(e.dR, e.dp, p, q);
  const size_t g = (size_t)(e.off + j);
  full[3 * g] = (float)q[0]; full[3 * g + 1] = (float)q[1]; full[3 * g + 2] = (float)q[2];
  rows[6 * g] = q[0]; rows[6 * g + 1] = q[1]; rows[6 * g + 2] = q[2];
  rows[6 * g + 3] = e.var[3 * j]; rows[6 * g + 4] = e.var[3 * j + 1]; rows[6 * g + 5] = e.var[3 * j + 2];
  unsigned long long k;
  if (!voxel_key(q, vs, &k)) flags[2] = 1u;
  key[g] = k;
  idx[g] = (unsigned int)g;
}

__global__ void __launch_bounds__(BLK) kf_filter_kernel(const double* __restrict__ rows, const unsigned int* __restrict__ idx_s, const unsigned int* __restrict__ cell_ptr,
                                                        const unsigned int* __restrict__ n_cells, float* __restrict__ down, float* __restrict__ down_xyz, unsigned int* __restrict__ flags) {
#pragma clang fp contract(off)
  const unsigned int runs = *n_cells;
  const long long c = (long long)blockIdx.x * BLK + threadIdx.x;
  if (c == 0) flags[1] = runs;
  if (c >= (long long)runs) return;
  unsigned int q = cell_ptr[c];
  const unsigned int end = cell_ptr[c + 1];
  const double* r = rows + 6 * (size_t)idx_s[q];
  double m[6] = {r[0], r[1], r[2], r[3], r[4], r[5]};
  int cnt = 1;
  for (q++; q < end; q++, cnt++) {
    r = rows + 6 * (size_t)idx_s[q];
    VXK_UNROLL for (int k = 0; k < 6; k++) m[k] = mean_step(m[k], cnt, r[k]);
  }
  VXK_UNROLL for (int k = 0; k < 6; k++) down[6 * (size_t)c + k] = (float)m[k];
  VXK_UNROLL for (int k = 0; k < 3; k++) down_xyz[3 * (size_t)c + k] = (float)m[k];     // the packed copy the hierarchical BA takes
}

}  // namespace vxkf

struct vxba_keyframe {
  int device = 0;
  std::string err;
  vxu::Stream s;
  int win = 10;
  double voxel_size = 1.0, ang_deg = 5.0, len_thr = 0.1;
  // every ScanPose since clear, and the rule's state (voxelslam.cpp:1851-1852, 1928-1942)
  std::vector<double> poses, v6s;
  int64_t buf_base = 0;
  double jour = 0.0, x_key[12] = {0};
  // the buffered scans (bl_local): device slots [pnt cap x 3 | var diagonal cap x 3], recycled
  struct Scan {
    vxu::Dev<double> d; int64_t n = 0; int64_t pose = 0;
    size_t cap() const { return d.capacity() / 6; }
  };
  std::deque<Scan> ring;
  std::vector<Scan> spare;
  // host-mapped words the kernels write: [0] ingest found a coordinate that is not finite, [1] occupied voxels, [2] assembly found a bad point
  vxu::Pin<unsigned int> flags;
  vxu::Pin<double> stage;                                 // pinned staging of the host route
  vxu::Pin<vxkf::ScanEntry> h_tab; vxu::Dev<vxkf::ScanEntry> d_tab;
  vxu::Arena work;                                        // sort / group work space
  vxu::Dev<unsigned int> d_runs;
  // the keyframe: front is readable, back is being written
  vxu::Dev<float> full[2], down[2], down_xyz[2];
  int front = 0;
  bool has_kf = false;
  int64_t kf_id = 0, n_full = 0, n_down = 0;
  double kf_pose[12] = {0}, kf_jour = 0.0;
  int64_t stats[4] = {0, 0, 0, 0};                        // launches, host waits, bytes D2H, bytes H2D of the last push
  bool profiling = false, ev_valid = false;               // vxba_keyframe_set_profiling: events between the stages of an emitting push
  vxu::Event ev[4];
};

using namespace vxkf;

using vxu::blocks_for, vxu::fail;

static int take_slot(vxba_keyframe* h, int64_t n, vxba_keyframe::Scan* out) {
  vxba_keyframe::Scan sc;
  if (!h->spare.empty()) { sc = std::move(h->spare.back()); h->spare.pop_back(); }
  VX_HIP(h, sc.d.reserve((size_t)n * 6, ((size_t)n + (size_t)n / 4 + 64) * 6));
  sc.n = n;
  *out = std::move(sc);
  return VXBA_OK;
}

// the kernels of one keyframe on the handle's stream; nothing is waited for
static int enqueue_keyframe(vxba_keyframe* h, int64_t N, int64_t n_max) {
  const int W = h->win, back = h->front ^ 1;
  const double* xc = h->poses.data() + 12 * h->ring.back().pose;
  int64_t off = 0;
  for (int i = 0; i < W; i++) {
    const vxba_keyframe::Scan& sc = h->ring[i];
    ScanEntry& e = h->h_tab[i];
    delta_pose(xc, h->poses.data() + 12 * sc.pose, e.dR, e.dp);     // for the newest scan too: xc.R^T xc.R is the identity only up to rounding
    e.pnt = sc.d; e.var = sc.d ? sc.d + 3 * sc.cap() : nullptr; e.n = sc.n; e.off = off;
    off += sc.n;
  }
  if (N == 0) return VXBA_OK;
  const size_t n = (size_t)N, want = n + n / 4;
  VX_HIP(h, h->full[back].reserve(3 * n, 3 * want));
  VX_HIP(h, h->down[back].reserve(6 * n, 6 * want));
  VX_HIP(h, h->down_xyz[back].reserve(3 * n, 3 * want));
  double* d_rows = nullptr;
  vxu::Cells<unsigned int> c;
  bool synced = false;
  VX_HIP(h, c.size(n, 3 * KEY_BITS, h->s));
  VX_HIP(h, h->work.layout([&](vxu::Arena& a) { d_rows = a.take<double>(6 * n); c.carve(a, n); }, h->s, &synced));
  if (synced) h->stats[1] += 1;
  VX_HIP(h, hipMemcpyAsync(h->d_tab, h->h_tab, sizeof(ScanEntry) * W, hipMemcpyHostToDevice, h->s));
  h->stats[3] += (int64_t)sizeof(ScanEntry) * W;
  VX_HIP(h, hipMemsetAsync(c.cnt, 0, (n + 1) * 4, h->s));     // the scan runs over N + 1 counts, of which the encode writes only the occupied voxels'
  h->ev_valid = false;
  if (h->profiling) VX_HIP(h, hipEventRecord(h->ev[0], h->s));
  hipLaunchKernelGGL(kf_assemble_kernel, dim3(blocks_for(n_max, BLK), W), dim3(BLK), 0, h->s, (const ScanEntry*)h->d_tab, h->voxel_size / 10, h->full[back], d_rows, c.key, c.idx, h->flags);
  VX_HIP(h, hipGetLastError());
  if (h->profiling) VX_HIP(h, hipEventRecord(h->ev[1], h->s));
  VX_HIP(h, vxu::sort(c.temp, c.key, c.key_s, c.idx, c.idx_s, n, 3 * KEY_BITS, h->s));
  VX_HIP(h, vxu::encode(c.temp, c.key_s, n, c.ukey, c.cnt, h->d_runs, h->s));
  VX_HIP(h, vxu::scan(c.temp, c.cnt, c.ptr, n + 1, h->s));
  if (h->profiling) VX_HIP(h, hipEventRecord(h->ev[2], h->s));
  hipLaunchKernelGGL(kf_filter_kernel, dim3(blocks_for(N, BLK)), dim3(BLK), 0, h->s, (const double*)d_rows, (const unsigned int*)c.idx_s, (const unsigned int*)c.ptr,
                     (const unsigned int*)h->d_runs, h->down[back], h->down_xyz[back], h->flags);
  VX_HIP(h, hipGetLastError());
  if (h->profiling) { VX_HIP(h, hipEventRecord(h->ev[3], h->s)); h->ev_valid = true; }
  h->stats[0] += 5;      // two kernels of the handle's own, and a library sort, encode or scan counts as one
  return VXBA_OK;
}

static int push_scan(vxba_keyframe* h, const double* pose, const double* v6, int64_t n, const double* pnt, const double* var, bool on_device, int* emitted) {
  if (!h) return VXBA_ERR_ARG;
  if (!pose || !v6 || !emitted || n < 0 || n > MAX_SCAN || (n > 0 && !pnt)) return fail(h, VXBA_ERR_ARG, "keyframe_push_scan: bad argument");
  *emitted = 0;
  for (int k = 0; k < 12; k++) if (!std::isfinite(pose[k])) return fail(h, VXBA_ERR_ARG, "keyframe_push_scan: the pose is not finite");
  h->stats[0] = h->stats[1] = h->stats[2] = h->stats[3] = 0;
  VX_HIP(h, hipSetDevice(h->device));
  vxba_keyframe::Scan sc;
  int rc = take_slot(h, n, &sc);
  if (rc != VXBA_OK) return rc;
  auto give_back = [&](vxba_keyframe::Scan& s) { s.n = 0; h->spare.push_back(std::move(s)); };
  h->flags[0] = h->flags[1] = h->flags[2] = 0u;
  if (n > 0 && !on_device) {
    if (h->stage.reserve((size_t)n * 6, ((size_t)n + (size_t)n / 4 + 64) * 6) != hipSuccess) { give_back(sc); return fail(h, VXBA_ERR_HIP, "keyframe_push_scan: pinned staging"); }
    double* sp = h->stage;
    double* sv = h->stage + 3 * (size_t)n;
    for (int64_t k = 0; k < 3 * n; k++) {
      if (!std::isfinite(pnt[k])) { give_back(sc); return fail(h, VXBA_ERR_ARG, "keyframe_push_scan: point " + std::to_string(k / 3) + " is not finite"); }
      sp[k] = pnt[k];
    }
    for (int64_t j = 0; j < n; j++) {
      sv[3 * j] = var ? var[9 * j] : 0.0; sv[3 * j + 1] = var ? var[9 * j + 4] : 0.0; sv[3 * j + 2] = var ? var[9 * j + 8] : 0.0;
    }
    hipError_t e = hipMemcpyAsync(sc.d, sp, (size_t)n * 24, hipMemcpyHostToDevice, h->s);
    if (e == hipSuccess) e = hipMemcpyAsync(sc.d + 3 * sc.cap(), sv, (size_t)n * 24, hipMemcpyHostToDevice, h->s);
    if (e != hipSuccess) { give_back(sc); return fail(h, VXBA_ERR_HIP, std::string("keyframe_push_scan: ") + hipGetErrorString(e)); }
    h->stats[3] += n * 48;
  } else if (n > 0) {
    hipLaunchKernelGGL(kf_ingest_kernel, dim3(blocks_for(n, BLK)), dim3(BLK), 0, h->s, pnt, var, (long long)n, sc.d.get(), sc.d + 3 * sc.cap(), h->flags.get());
    const hipError_t e = hipGetLastError();
    if (e != hipSuccess) { give_back(sc); return fail(h, VXBA_ERR_HIP, std::string("keyframe_push_scan: ") + hipGetErrorString(e)); }
    h->stats[0] += 1;
  }

  // the rule, :1928-1942; everything it changes is put back if the push fails
  const int64_t base0 = h->buf_base;
  double key0[12];
  std::memcpy(key0, h->x_key, sizeof key0);
  sc.pose = (int64_t)(h->poses.size() / 12);
  h->poses.insert(h->poses.end(), pose, pose + 12);
  h->v6s.insert(h->v6s.end(), v6, v6 + 6);
  h->ring.push_back(std::move(sc));
  if (h->buf_base == 0) std::memcpy(h->x_key, pose, sizeof key0);
  h->buf_base += 1;
  auto roll_back = [&]() {
    give_back(h->ring.back());
    h->ring.pop_back();
    h->poses.resize(h->poses.size() - 12); h->v6s.resize(h->v6s.size() - 6);
    h->buf_base = base0;
    std::memcpy(h->x_key, key0, sizeof key0);
  };
  bool emit = false, drop = false;
  double ang = 0.0, len = 0.0;
  int64_t N = 0, n_max = 0;
  if ((int)h->ring.size() >= h->win) {
    rule_metrics(h->x_key, pose, &ang, &len);
    if (ang < h->ang_deg && len < h->len_thr && h->buf_base > h->win) drop = true;
    else emit = true;
  }
  if (emit) {
    for (const auto& s : h->ring) { N += s.n; if (s.n > n_max) n_max = s.n; }
    rc = N < ((int64_t)1 << 31) ? enqueue_keyframe(h, N, n_max) : fail(h, VXBA_ERR_ARG, "keyframe_push_scan: a keyframe holds fewer than 2^31 points");
    if (rc != VXBA_OK) { hipStreamSynchronize(h->s); roll_back(); return rc; }
  }
  if (n > 0 || (emit && N > 0)) {     // the one wait: the staging buffer is free again, the flag words and the voxel count are in
    const hipError_t e = vxwait::stream_wait(h->s);
    h->stats[1] += 1;
    if (e != hipSuccess) { roll_back(); return fail(h, VXBA_ERR_HIP, std::string("keyframe_push_scan: ") + hipGetErrorString(e)); }
    h->stats[2] += 12;
  }
  const unsigned int bad_in = ((volatile unsigned int*)h->flags)[0], runs = ((volatile unsigned int*)h->flags)[1], bad_kf = ((volatile unsigned int*)h->flags)[2];
  if (bad_in) { roll_back(); return fail(h, VXBA_ERR_ARG, "keyframe_push_scan: a point is not finite"); }
  if (bad_kf) { roll_back(); return fail(h, VXBA_ERR_ARG, "keyframe_push_scan: a merged point is not finite or lies 2^20 voxels or more from the keyframe's origin"); }
  if (drop) { give_back(h->ring.front()); h->ring.pop_front(); }
  if (emit) {
    h->jour += len;
    std::memcpy(h->x_key, pose, sizeof key0);
    h->front ^= 1;
    h->has_kf = true;
    h->kf_id = h->buf_base - 1; h->kf_jour = h->jour; h->n_full = N; h->n_down = N > 0 ? (int64_t)runs : 0;
    std::memcpy(h->kf_pose, pose, sizeof key0);
    while (!h->ring.empty()) { give_back(h->ring.front()); h->ring.pop_front(); }
    *emitted = 1;
  }
  return VXBA_OK;
}

extern "C" {

int vxba_keyframe_create(int device, const vxba_keyframe_params* p, vxba_keyframe** out) {
  if (!out) return VXBA_ERR_ARG;
  *out = nullptr;
  const int win = p && p->win_size > 0 ? p->win_size : 10;
  if (win > MAX_WIN) return VXBA_ERR_ARG;
  if (const int rc = vxu::select_device(device)) return rc;
  vxba_keyframe* h = new vxba_keyframe();
  h->device = device;
  h->win = win;
  h->voxel_size = p && p->voxel_size > 0 ? p->voxel_size : 1.0;
  h->ang_deg = p && p->ang_deg > 0 ? p->ang_deg : 5.0;
  h->len_thr = p && p->len > 0 ? p->len : 0.1;
  if (h->s.create() != hipSuccess || h->flags.reserve(16) != hipSuccess || h->h_tab.reserve(MAX_WIN) != hipSuccess || h->d_tab.reserve(MAX_WIN) != hipSuccess ||
      h->d_runs.reserve(64) != hipSuccess) {
    delete h;
    return VXBA_ERR_HIP;
  }
  *out = h;
  return VXBA_OK;
}

int vxba_keyframe_destroy(vxba_keyframe* h) {
  if (!h) return VXBA_OK;
  hipSetDevice(h->device);
  if (h->s) hipStreamSynchronize(h->s);
  h->work.release();
  delete h;
  return VXBA_OK;
}

const char* vxba_keyframe_last_error(const vxba_keyframe* h) { return h ? h->err.c_str() : "null handle"; }

int vxba_keyframe_clear(vxba_keyframe* h) {
  if (!h) return VXBA_ERR_ARG;
  while (!h->ring.empty()) { h->ring.front().n = 0; h->spare.push_back(std::move(h->ring.front())); h->ring.pop_front(); }
  h->poses.clear(); h->v6s.clear();
  h->buf_base = 0; h->jour = 0.0;
  h->has_kf = false;
  return VXBA_OK;
}

int vxba_keyframe_push_scan(vxba_keyframe* h, const double pose[12], const double v6[6], int64_t n, const double* pnt_body, const double* var, int* emitted) {
  return push_scan(h, pose, v6, n, pnt_body, var, false, emitted);
}

int vxba_keyframe_push_scan_device(vxba_keyframe* h, const double pose[12], const double v6[6], int64_t n, const double* d_pnt_body, const double* d_var, int* emitted) {
  return push_scan(h, pose, v6, n, d_pnt_body, d_var, true, emitted);
}

int vxba_keyframe_info(const vxba_keyframe* h, int64_t* id, double pose[12], double* jour, int64_t* n_full, int64_t* n_down) {
  if (!h) return VXBA_ERR_ARG;
  if (!h->has_kf) return VXBA_ERR_STATE;
  if (id) *id = h->kf_id;
  if (pose) std::memcpy(pose, h->kf_pose, sizeof h->kf_pose);
  if (jour) *jour = h->kf_jour;
  if (n_full) *n_full = h->n_full;
  if (n_down) *n_down = h->n_down;
  return VXBA_OK;
}

int vxba_keyframe_read(vxba_keyframe* h, float* full_xyz, float* down_xyzv) {
  if (!h) return VXBA_ERR_ARG;
  if (!h->has_kf) return fail(h, VXBA_ERR_STATE, "keyframe_read: no keyframe yet");
  VX_HIP(h, hipSetDevice(h->device));
  if (full_xyz && h->n_full > 0) VX_HIP(h, hipMemcpyAsync(full_xyz, h->full[h->front], (size_t)h->n_full * 3 * sizeof(float), hipMemcpyDeviceToHost, h->s));
  if (down_xyzv && h->n_down > 0) VX_HIP(h, hipMemcpyAsync(down_xyzv, h->down[h->front], (size_t)h->n_down * 6 * sizeof(float), hipMemcpyDeviceToHost, h->s));
  VX_HIP(h, hipStreamSynchronize(h->s));
  return VXBA_OK;
}

int vxba_keyframe_device(const vxba_keyframe* h, const float** d_full, const float** d_down) {
  if (!h) return VXBA_ERR_ARG;
  if (!h->has_kf) return VXBA_ERR_STATE;
  if (d_full) *d_full = h->n_full > 0 ? h->full[h->front].get() : nullptr;
  if (d_down) *d_down = h->n_down > 0 ? h->down[h->front].get() : nullptr;
  return VXBA_OK;
}

int vxba_keyframe_device_down_xyz(const vxba_keyframe* h, const float** d_down_xyz) {
  if (!h || !d_down_xyz) return VXBA_ERR_ARG;
  if (!h->has_kf) return VXBA_ERR_STATE;
  *d_down_xyz = h->n_down > 0 ? h->down_xyz[h->front].get() : nullptr;
  return VXBA_OK;
}

int64_t vxba_keyframe_num_scans(const vxba_keyframe* h) { return h ? (int64_t)(h->poses.size() / 12) : 0; }

int vxba_keyframe_num_buffered(const vxba_keyframe* h) { return h ? (int)h->ring.size() : 0; }

int vxba_keyframe_scan_poses(const vxba_keyframe* h, int64_t first, int64_t count, double* poses, double* v6) {
  if (!h) return VXBA_ERR_ARG;
  const int64_t total = (int64_t)(h->poses.size() / 12);
  if (first < 0 || count < 0 || first + count > total) return VXBA_ERR_ARG;
  if (poses && count) std::memcpy(poses, h->poses.data() + 12 * first, sizeof(double) * 12 * count);
  if (v6 && count) std::memcpy(v6, h->v6s.data() + 6 * first, sizeof(double) * 6 * count);
  return VXBA_OK;
}

int vxba_keyframe_set_profiling(vxba_keyframe* h, int enable) {
  if (!h) return VXBA_ERR_ARG;
  VX_HIP(h, hipSetDevice(h->device));
  for (vxu::Event& e : h->ev) if (enable) VX_HIP(h, e.create());
  h->profiling = enable != 0;
  h->ev_valid = false;
  return VXBA_OK;
}

int vxba_keyframe_stage_times(vxba_keyframe* h, double ms[3]) {
  if (!h || !ms) return VXBA_ERR_ARG;
  if (!h->ev_valid) return fail(h, VXBA_ERR_STATE, "keyframe_stage_times: the last emitting push was not profiled");
  for (int k = 0; k < 3; k++) {
    float t = 0.f;
    VX_HIP(h, hipEventElapsedTime(&t, h->ev[k], h->ev[k + 1]));
    ms[k] = (double)t;
  }
  return VXBA_OK;
}

int vxba_keyframe_stats(const vxba_keyframe* h, int64_t out[4]) {
  if (!h || !out) return VXBA_ERR_ARG;
  for (int k = 0; k < 4; k++) out[k] = h->stats[k];
  return VXBA_OK;
}

}  // extern "C"
