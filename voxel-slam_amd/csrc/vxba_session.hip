// Saved sessions on the GPU (include/vxba.h: vxba_session_*, vxba_globalmap): the per-point half of previous_map_read (voxelslam.cpp:307-448) and
// pub_globalmap (:108-150).  The files are read on the host (voxel_slam_amd/sessionio.py); what arrives here is every saved scan of a session
// (body-frame float32 points, as save_pcd wrote them) and the scan poses of alidarState.txt.  The handle keeps the scans resident and makes
//   the keyframes        scans [g win, (g + 1) win) merged into the frame of the group's last scan, voxel-filtered at voxel_size / 10   (:331-372)
//   the descriptor clouds  keyframes [i, i + acsize) merged into the frame of keyframe i + acsize - 1 under the x0 poses               (:377-395)
// and vxba_globalmap gathers every jump-th point of any number of keyframe sets under their poses into one x, y, z, id map.
//
// Launch plan of vxba_session_build_keyframes, N = the points of the scans that fill a group.  Nothing depends on K:
//   ss_merge_kernel   one lane per point: its scan by binary search in the offset table, the scan's (delta_R, delta_p) from a table the host fills
//                     with vxkf::delta_pose, the merged float32 point, its 63-bit voxel key (on the FLOAT point, as down_sampling_voxel takes it),
//                     its keyframe; a key out of range raises a flag word in mapped host memory.
//   rocPRIM           stable radix_sort_pairs (voxel key, point); ss_gather_kernel (the keyframe of every sorted point); stable radix_sort_pairs
//                     (keyframe, point): rows now ascend by (keyframe, voxel key) and keep the input order inside a voxel.
//   ss_heads_kernel   one lane per row: 1 where the (keyframe, key) pair differs from the row before.  rocPRIM exclusive_scan over N + 1 flags.
//   ss_table_kernel   one lane per row: a head writes its voxel's first row into the cell table; the first row of a keyframe writes the keyframe's
//                     offset (and those of the empty keyframes before it) into device memory and into mapped host memory.
//   ss_mean_kernel    one lane per occupied voxel replays down_sampling_voxel's float running mean over its rows in input order.
// Eight enqueues and ONE host wait, whatever N and K.  The keyframe clouds are double-buffered: a build that is refused leaves the previous
// keyframes readable.
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdint>
#include <cstring>
#include <string>
#include <vector>

#include "../../include/vxba.h"
#include "vxba_dev.hpp"
#include "vxba_session_math.hpp"
#include "vxba_wait.hpp"

namespace vxss {

constexpr int BLK = 256;
constexpr int64_t MAX_POINTS = (int64_t)1 << 31;     // rows of one build / one window: indices stay in 32 bits

struct Rel { double dR[9], dp[3]; };     // a scan (a keyframe) in the frame it is merged into

__global__ void __launch_bounds__(BLK) ss_merge_kernel(const float* __restrict__ xyz, const long long* __restrict__ scan_ptr, long long n_scans, long long n,
                                                       const Rel* __restrict__ rel, int win, double vs, int with_key, float* __restrict__ merged,
                                                       unsigned long long* __restrict__ key, unsigned int* __restrict__ idx, unsigned int* __restrict__ kf,
                                                       unsigned int* __restrict__ flags) {
#pragma clang fp contract(off)
  const long long g = (long long)blockIdx.x * BLK + threadIdx.x;
  if (g >= n) return;
  const long long s = owner_of(scan_ptr, n_scans, g);
  const Rel& r = rel[s];
  const float v[3] = {xyz[3 * g], xyz[3 * g + 1], xyz[3 * g + 2]};
  float q[3];
  move_point(r.dR, r.dp, v, q);
  merged[3 * g] = q[0]; merged[3 * g + 1] = q[1]; merged[3 * g + 2] = q[2];
  unsigned long long k;
  if (!voxel_key(q, vs, &k) && with_key) flags[0] = 1u;      // without the filter (voxel_size / 10 < 0.001) no point is refused
  key[g] = k;
  idx[g] = (unsigned int)g;
  kf[g] = (unsigned int)(s / win);
}

__global__ void __launch_bounds__(BLK) ss_gather_kernel(const unsigned int* __restrict__ kf, const unsigned int* __restrict__ idx_s, long long n, unsigned int* __restrict__ kf_s) {
  const long long i = (long long)blockIdx.x * BLK + threadIdx.x;
  if (i < n) kf_s[i] = kf[idx_s[i]];
}

__device__ __forceinline__ bool is_head(const unsigned int* kf_s, const unsigned int* idx_s, const unsigned long long* key, long long i) {
  return i == 0 || kf_s[i] != kf_s[i - 1] || key[idx_s[i]] != key[idx_s[i - 1]];
}

// flag[i] for i < n, and flag[n] = 0: the scan's last output is then the number of occupied voxels
__global__ void __launch_bounds__(BLK) ss_heads_kernel(const unsigned int* __restrict__ kf_s, const unsigned int* __restrict__ idx_s, const unsigned long long* __restrict__ key,
                                                       long long n, unsigned int* __restrict__ flag) {
  const long long i = (long long)blockIdx.x * BLK + threadIdx.x;
  if (i > n) return;
  flag[i] = i < n && is_head(kf_s, idx_s, key, i) ? 1u : 0u;
}

// cell[c] = the first row of occupied voxel c (cell[runs] = n); kfp[k] = the first voxel of keyframe k (kfp[K] = runs), to the device and to the host
__global__ void __launch_bounds__(BLK) ss_table_kernel(const unsigned int* __restrict__ kf_s, const unsigned int* __restrict__ idx_s, const unsigned long long* __restrict__ key,
                                                       const unsigned int* __restrict__ pos, long long n, long long K, unsigned int* __restrict__ cell,
                                                       unsigned int* __restrict__ d_kfp, unsigned int* __restrict__ h_kfp) {
  const long long i = (long long)blockIdx.x * BLK + threadIdx.x;
  if (i >= n) return;
  const unsigned int p = pos[i], k = kf_s[i];
  if (is_head(kf_s, idx_s, key, i)) cell[p] = (unsigned int)i;
  if (i == 0 || kf_s[i - 1] != k) {
    const long long from = i == 0 ? 0 : (long long)kf_s[i - 1] + 1;
    for (long long j = from; j <= (long long)k && j <= K; j++) { d_kfp[j] = p; h_kfp[j] = p; }
  }
  if (i == n - 1) {
    const unsigned int runs = pos[n];
    cell[runs] = (unsigned int)n;
    for (long long j = (long long)k + 1; j <= K; j++) { d_kfp[j] = runs; h_kfp[j] = runs; }
  }
}

// pp = (pp * curvature + p) / (curvature + 1), curvature += 1   (tools.hpp:227-230), float, unfused, in input order
__global__ void __launch_bounds__(BLK) ss_mean_kernel(const float* __restrict__ merged, const unsigned int* __restrict__ idx_s, const unsigned int* __restrict__ cell,
                                                      const unsigned int* __restrict__ n_cells, float* __restrict__ out) {
#pragma clang fp contract(off)
  const long long c = (long long)blockIdx.x * BLK + threadIdx.x;
  if (c >= (long long)*n_cells) return;
  unsigned int q = cell[c];
  const unsigned int end = cell[c + 1];
  size_t i = idx_s[q];
  float x = merged[3 * i], y = merged[3 * i + 1], z = merged[3 * i + 2], cur = 1.0f;
  for (q++; q < end; q++) {
    i = idx_s[q];
    x = mean_step(x, cur, merged[3 * i]);
    y = mean_step(y, cur, merged[3 * i + 1]);
    z = mean_step(z, cur, merged[3 * i + 2]);
    cur = cur + 1.0f;
  }
  out[3 * c] = x; out[3 * c + 1] = y; out[3 * c + 2] = z;
}

// rows [base, base + n) of the packed keyframe clouds, keyframes [k0, k0 + count): each into the frame rel[k - k0] gives
__global__ void __launch_bounds__(BLK) ss_window_kernel(const float* __restrict__ kf_xyz, const unsigned int* __restrict__ kfp, long long k0, long long count, long long n,
                                                        const Rel* __restrict__ rel, float* __restrict__ out) {
#pragma clang fp contract(off)
  const long long g = (long long)blockIdx.x * BLK + threadIdx.x;
  if (g >= n) return;
  const long long row = (long long)kfp[k0] + g;
  const long long k = owner_of(kfp + k0, count, row);
  const Rel& r = rel[k];
  const float v[3] = {kf_xyz[3 * row], kf_xyz[3 * row + 1], kf_xyz[3 * row + 2]};
  float q[3];
  move_point(r.dR, r.dp, v, q);
  out[3 * g] = q[0]; out[3 * g + 1] = q[1]; out[3 * g + 2] = q[2];
}

struct MapKf { double R[9], p[3]; const float* src; float intensity; };

// output point o: keyframe by binary search in the output offsets, its point (o - off) * jump, moved by the keyframe's pose
__global__ void __launch_bounds__(BLK) gm_gather_kernel(const MapKf* __restrict__ tab, const long long* __restrict__ out_off, long long n_kf, long long n_out, long long jump,
                                                        float4* __restrict__ out) {
#pragma clang fp contract(off)
  const long long o = (long long)blockIdx.x * BLK + threadIdx.x;
  if (o >= n_out) return;
  const long long k = owner_of(out_off, n_kf, o);
  const MapKf& e = tab[k];
  const long long j = (o - out_off[k]) * jump;
  const float v[3] = {e.src[3 * j], e.src[3 * j + 1], e.src[3 * j + 2]};
  float q[3];
  move_point(e.R, e.p, v, q);
  out[o] = make_float4(q[0], q[1], q[2], e.intensity);
}

}  // namespace vxss

struct vxba_session {
  int device = 0;
  std::string err;
  vxu::Stream s;
  // the saved scans: offsets and poses on the host, the points and the offsets on the device
  std::vector<int64_t> scan_ptr{0};
  std::vector<double> poses;
  vxu::Dev<float> d_scan;
  vxu::Dev<long long> d_scan_ptr;
  // the keyframes: front is readable, back is being written
  vxu::Dev<float> d_kf[2];
  vxu::Dev<unsigned int> d_kfp[2];
  int front = 0, win = 0;
  std::vector<int64_t> kf_ptr{0}, ids;
  std::vector<double> x0;
  // tables the host fills (pinned) and their device copies; flags[0]: the merge met a key out of range
  vxu::Pin<vxss::Rel> h_rel; vxu::Dev<vxss::Rel> d_rel;
  vxu::Pin<unsigned int> flags, h_kfp;
  vxu::Arena work;
  // the descriptor cloud of the last vxba_session_window_cloud
  vxu::Dev<float> d_win; int64_t n_win = 0;
  int64_t launches = 0, waits = 0;     // of the last build_keyframes / window_cloud
  bool profiling = false, ev_valid = false;     // vxba_session_set_profiling: events between the stages of a build
  vxu::Event ev[4];
};

using namespace vxss;
using vxu::blocks_for, vxu::fail;

static int64_t num_kf(const vxba_session* h) { return (int64_t)h->kf_ptr.size() - 1; }

// room for `count` Rel records on both sides; the stream is idle between calls, so the old blocks can go
static int rel_room(vxba_session* h, size_t count) {
  const size_t want = count + count / 4 + 16;
  VX_HIP(h, h->h_rel.reserve(count, want));
  VX_HIP(h, h->d_rel.reserve(count, want));
  return VXBA_OK;
}

extern "C" {

int vxba_session_create(int device, vxba_session** out) {
  if (!out) return VXBA_ERR_ARG;
  *out = nullptr;
  if (const int rc = vxu::select_device(device)) return rc;
  vxba_session* h = new vxba_session();
  h->device = device;
  if (h->s.create() != hipSuccess || h->flags.reserve(16) != hipSuccess) { delete h; return VXBA_ERR_HIP; }
  *out = h;
  return VXBA_OK;
}

int vxba_session_destroy(vxba_session* h) {
  if (!h) return VXBA_OK;
  hipSetDevice(h->device);
  if (h->s) hipStreamSynchronize(h->s);
  h->work.release();
  delete h;
  return VXBA_OK;
}

const char* vxba_session_last_error(const vxba_session* h) { return h ? h->err.c_str() : "null handle"; }

int vxba_session_clear(vxba_session* h) {
  if (!h) return VXBA_ERR_ARG;
  h->scan_ptr.assign(1, 0); h->poses.clear();
  h->kf_ptr.assign(1, 0); h->ids.clear(); h->x0.clear();
  h->n_win = 0; h->win = 0;
  return VXBA_OK;
}

int vxba_session_load_scans(vxba_session* h, int64_t n_scans, const int64_t* scan_ptr, const float* xyz, const double* poses) {
  if (!h) return VXBA_ERR_ARG;
  if (n_scans < 0 || !scan_ptr || scan_ptr[0] != 0 || (n_scans > 0 && !poses)) return fail(h, VXBA_ERR_ARG, "session_load_scans: bad argument");
  for (int64_t k = 0; k < n_scans; k++)
    if (scan_ptr[k + 1] < scan_ptr[k]) return fail(h, VXBA_ERR_ARG, "session_load_scans: scan_ptr decreases at scan " + std::to_string(k));
  for (int64_t k = 0; k < 12 * n_scans; k++)
    if (!std::isfinite(poses[k])) return fail(h, VXBA_ERR_ARG, "session_load_scans: the pose of scan " + std::to_string(k / 12) + " is not finite");
  const int64_t n = scan_ptr[n_scans];
  if (n >= MAX_POINTS || (n > 0 && !xyz)) return fail(h, VXBA_ERR_ARG, "session_load_scans: null points, or 2^31 points or more");
  VX_HIP(h, hipSetDevice(h->device));
  VX_HIP(h, h->d_scan.reserve((size_t)n * 3));
  VX_HIP(h, h->d_scan_ptr.reserve((size_t)n_scans + 1));
  if (n > 0) VX_HIP(h, hipMemcpy(h->d_scan, xyz, (size_t)n * 3 * sizeof(float), hipMemcpyHostToDevice));
  static_assert(sizeof(long long) == sizeof(int64_t), "the offset table is uploaded as it is");
  VX_HIP(h, hipMemcpy(h->d_scan_ptr, scan_ptr, ((size_t)n_scans + 1) * sizeof(int64_t), hipMemcpyHostToDevice));
  VX_HIP(h, hipStreamSynchronize(nullptr));      // the kernels run on the handle's own non-blocking stream: the copies must have landed before any of them starts
  h->scan_ptr.assign(scan_ptr, scan_ptr + n_scans + 1);
  h->poses.assign(poses, poses + 12 * n_scans);
  h->kf_ptr.assign(1, 0); h->ids.clear(); h->x0.clear();      // keyframes of other scans are gone
  h->n_win = 0; h->win = 0;
  return VXBA_OK;
}

int64_t vxba_session_num_scans(const vxba_session* h) { return h ? (int64_t)h->scan_ptr.size() - 1 : 0; }
int64_t vxba_session_num_keyframes(const vxba_session* h) { return h ? num_kf(h) : 0; }

int vxba_session_build_keyframes(vxba_session* h, int win_size, double voxel_size, int64_t* n_keyframes) {
  if (!h) return VXBA_ERR_ARG;
  if (win_size <= 0 || !(voxel_size > 0) || !n_keyframes) return fail(h, VXBA_ERR_ARG, "session_build_keyframes: bad argument");
  h->launches = h->waits = 0;
  const int64_t n_scans = (int64_t)h->scan_ptr.size() - 1, K = n_scans / win_size, used = K * win_size;
  const int64_t N = h->scan_ptr[used];
  const double vs = voxel_size / 10;      // in double, as upstream (:362)
  const bool filter = !(vs < 0.001);      // down_sampling_voxel returns the cloud untouched below 0.001 (tools.hpp:203)
  const int back = h->front ^ 1;
  std::vector<int64_t> kf_ptr(K + 1, 0);
  VX_HIP(h, hipSetDevice(h->device));
  if (N > 0) {
    VX_HIP(h, h->d_kf[back].reserve((size_t)N * 3, ((size_t)N + (size_t)N / 4) * 3));
    VX_HIP(h, h->d_kfp[back].reserve((size_t)K + 1, (size_t)K + 65));
    VX_HIP(h, h->h_kfp.reserve((size_t)K + 1, (size_t)K + 65));
    if (const int rc = rel_room(h, (size_t)used)) return rc;
    for (int64_t s = 0; s < used; s++) {
      const int64_t last = (s / win_size) * win_size + win_size - 1;
      // for the group's last scan too: xc.R^T xc.R is the identity only up to rounding, and upstream multiplies by it (:350-356)
      vxkf::delta_pose(h->poses.data() + 12 * last, h->poses.data() + 12 * s, h->h_rel[s].dR, h->h_rel[s].dp);
    }
    const size_t n = (size_t)N;
    unsigned int bits = 1;
    while (((int64_t)1 << bits) < K) bits++;
    float* d_merged = nullptr;
    unsigned long long *key = nullptr, *key_s = nullptr;
    unsigned int *idx = nullptr, *idx_s = nullptr, *idx_ss = nullptr, *kf = nullptr, *kf_g = nullptr, *kf_s = nullptr, *flag = nullptr, *pos = nullptr, *cell = nullptr;
    vxu::Temp temp;
    VX_HIP(h, (vxu::sort_temp<unsigned long long, unsigned int>(temp.bytes, n, 63, h->s)));
    VX_HIP(h, (vxu::sort_temp<unsigned int, unsigned int>(temp.bytes, n, bits, h->s)));
    VX_HIP(h, vxu::scan_temp<unsigned int>(temp.bytes, n + 1, h->s));
    bool synced = false;
    VX_HIP(h, h->work.layout([&](vxu::Arena& a) {
      d_merged = filter ? a.take<float>(3 * n) : nullptr;
      key = a.take<unsigned long long>(n); key_s = a.take<unsigned long long>(n);
      idx = a.take<unsigned int>(n); idx_s = a.take<unsigned int>(n); idx_ss = a.take<unsigned int>(n);
      kf = a.take<unsigned int>(n); kf_g = a.take<unsigned int>(n); kf_s = a.take<unsigned int>(n);
      flag = a.take<unsigned int>(n + 1); pos = a.take<unsigned int>(n + 1); cell = a.take<unsigned int>(n + 1);
      temp.p = a.take<char>(temp.bytes);
    }, h->s, &synced));
    if (synced) h->waits += 1;
    h->flags[0] = 0u;
    VX_HIP(h, hipMemcpyAsync(h->d_rel, h->h_rel, sizeof(Rel) * (size_t)used, hipMemcpyHostToDevice, h->s));
    h->ev_valid = false;
    const bool prof = h->profiling && filter;
    if (prof) VX_HIP(h, hipEventRecord(h->ev[0], h->s));
    hipLaunchKernelGGL(ss_merge_kernel, dim3(blocks_for(N, BLK)), dim3(BLK), 0, h->s, (const float*)h->d_scan, (const long long*)h->d_scan_ptr, (long long)used, (long long)N,
                       (const Rel*)h->d_rel, win_size, filter ? vs : 1.0, filter ? 1 : 0, filter ? d_merged : h->d_kf[back].get(), key, idx, kf, h->flags);
    VX_HIP(h, hipGetLastError());
    h->launches += 1;
    if (prof) VX_HIP(h, hipEventRecord(h->ev[1], h->s));
    if (filter) {
      VX_HIP(h, vxu::sort(temp, key, key_s, idx, idx_s, n, 63, h->s));
      hipLaunchKernelGGL(ss_gather_kernel, dim3(blocks_for(N, BLK)), dim3(BLK), 0, h->s, (const unsigned int*)kf, (const unsigned int*)idx_s, (long long)N, kf_g);
      VX_HIP(h, hipGetLastError());
      VX_HIP(h, vxu::sort(temp, kf_g, kf_s, idx_s, idx_ss, n, bits, h->s));
      hipLaunchKernelGGL(ss_heads_kernel, dim3(blocks_for(N + 1, BLK)), dim3(BLK), 0, h->s, (const unsigned int*)kf_s, (const unsigned int*)idx_ss, (const unsigned long long*)key,
                         (long long)N, flag);
      VX_HIP(h, hipGetLastError());
      VX_HIP(h, vxu::scan(temp, flag, pos, n + 1, h->s));
      hipLaunchKernelGGL(ss_table_kernel, dim3(blocks_for(N, BLK)), dim3(BLK), 0, h->s, (const unsigned int*)kf_s, (const unsigned int*)idx_ss, (const unsigned long long*)key,
                         (const unsigned int*)pos, (long long)N, (long long)K, cell, h->d_kfp[back], h->h_kfp);
      VX_HIP(h, hipGetLastError());
      if (prof) VX_HIP(h, hipEventRecord(h->ev[2], h->s));
      hipLaunchKernelGGL(ss_mean_kernel, dim3(blocks_for(N, BLK)), dim3(BLK), 0, h->s, (const float*)d_merged, (const unsigned int*)idx_ss, (const unsigned int*)cell,
                         (const unsigned int*)(pos + n), h->d_kf[back]);
      VX_HIP(h, hipGetLastError());
      if (prof) { VX_HIP(h, hipEventRecord(h->ev[3], h->s)); h->ev_valid = true; }
      h->launches += 7;      // a library sort or scan counts as one
    }
    const hipError_t e = vxwait::stream_wait(h->s);
    h->waits += 1;
    if (e != hipSuccess) return fail(h, VXBA_ERR_HIP, std::string("session_build_keyframes: ") + hipGetErrorString(e));
    if (((volatile unsigned int*)h->flags)[0])
      return fail(h, VXBA_ERR_ARG, "session_build_keyframes: a merged point is not finite or lies 2^20 voxels or more from its keyframe's origin");
    if (filter) {
      for (int64_t k = 0; k <= K; k++) kf_ptr[k] = (int64_t)((volatile unsigned int*)h->h_kfp)[k];
    } else {
      // the merged clouds as they are: the offsets are the groups'
      std::vector<unsigned int> kp(K + 1);
      for (int64_t k = 0; k <= K; k++) { kf_ptr[k] = h->scan_ptr[k * win_size]; kp[k] = (unsigned int)kf_ptr[k]; }
      VX_HIP(h, hipMemcpy(h->d_kfp[back], kp.data(), sizeof(unsigned int) * (size_t)(K + 1), hipMemcpyHostToDevice));
      VX_HIP(h, hipStreamSynchronize(nullptr));
    }
    h->front = back;
  }
  h->win = win_size;
  h->kf_ptr = kf_ptr;
  h->ids.resize(K); h->x0.resize(12 * K);
  for (int64_t k = 0; k < K; k++) {
    h->ids[k] = k * win_size + win_size - 1;
    std::memcpy(h->x0.data() + 12 * k, h->poses.data() + 12 * h->ids[k], 12 * sizeof(double));
  }
  h->n_win = 0;
  *n_keyframes = K;
  return VXBA_OK;
}

int vxba_session_keyframes(const vxba_session* h, int64_t* kf_ptr, int64_t* ids, double* poses) {
  if (!h) return VXBA_ERR_ARG;
  const int64_t K = num_kf(h);
  if (kf_ptr) std::memcpy(kf_ptr, h->kf_ptr.data(), sizeof(int64_t) * (size_t)(K + 1));
  if (ids && K) std::memcpy(ids, h->ids.data(), sizeof(int64_t) * (size_t)K);
  if (poses && K) std::memcpy(poses, h->x0.data(), sizeof(double) * 12 * (size_t)K);
  return VXBA_OK;
}

int vxba_session_read_keyframes(vxba_session* h, float* xyz) {
  if (!h) return VXBA_ERR_ARG;
  const int64_t n = h->kf_ptr.back();
  if (n > 0 && !xyz) return fail(h, VXBA_ERR_ARG, "session_read_keyframes: null output");
  VX_HIP(h, hipSetDevice(h->device));
  if (n > 0) VX_HIP(h, hipMemcpy(xyz, h->d_kf[h->front], (size_t)n * 3 * sizeof(float), hipMemcpyDeviceToHost));
  return VXBA_OK;
}

int vxba_session_device(const vxba_session* h, const float** d_xyz) {
  if (!h || !d_xyz) return VXBA_ERR_ARG;
  *d_xyz = h->kf_ptr.back() > 0 ? h->d_kf[h->front].get() : nullptr;
  return VXBA_OK;
}

int vxba_session_set_scan_poses(vxba_session* h, const double* poses) {
  if (!h) return VXBA_ERR_ARG;
  const int64_t n_scans = (int64_t)h->scan_ptr.size() - 1;
  if (n_scans > 0 && !poses) return fail(h, VXBA_ERR_ARG, "session_set_scan_poses: null poses");
  for (int64_t k = 0; k < 12 * n_scans; k++)
    if (!std::isfinite(poses[k])) return fail(h, VXBA_ERR_ARG, "session_set_scan_poses: the pose of scan " + std::to_string(k / 12) + " is not finite");
  if (n_scans) h->poses.assign(poses, poses + 12 * n_scans);
  for (size_t k = 0; k < h->ids.size(); k++) std::memcpy(h->x0.data() + 12 * k, h->poses.data() + 12 * h->ids[k], 12 * sizeof(double));      // kf->x0 = scanPoses[kf->id]->x
  return VXBA_OK;
}

int vxba_session_num_windows(int64_t K, int acsize, int mgsize) {
  if (acsize <= 0 || mgsize <= 0) return 0;
  int n = 0;
  for (int64_t i = 0; i + acsize < K; i += mgsize) n++;      // strict, as upstream (:377): exactly acsize keyframes make no window
  return n;
}

int vxba_session_window_cloud(vxba_session* h, int w, int acsize, int mgsize, int64_t* n_out, const float** d_xyz, int64_t* frame_id) {
  if (!h) return VXBA_ERR_ARG;
  const int64_t K = num_kf(h);
  if (!n_out || !d_xyz || w < 0 || w >= vxba_session_num_windows(K, acsize, mgsize)) return fail(h, VXBA_ERR_ARG, "session_window_cloud: bad argument, or no such window");
  h->launches = h->waits = 0;
  const int64_t i = (int64_t)w * mgsize, up = i + acsize;
  const int64_t n = h->kf_ptr[up] - h->kf_ptr[i];
  *n_out = 0; *d_xyz = nullptr;
  h->n_win = 0;
  if (frame_id) *frame_id = h->ids[up - 1];
  if (n == 0) return VXBA_OK;
  VX_HIP(h, hipSetDevice(h->device));
  VX_HIP(h, h->d_win.reserve((size_t)n * 3, ((size_t)n + (size_t)n / 4) * 3));
  if (const int rc = rel_room(h, (size_t)acsize)) return rc;
  const double* xc = h->x0.data() + 12 * (up - 1);
  for (int64_t j = i; j < up; j++) vxkf::delta_pose(xc, h->x0.data() + 12 * j, h->h_rel[j - i].dR, h->h_rel[j - i].dp);
  VX_HIP(h, hipMemcpyAsync(h->d_rel, h->h_rel, sizeof(Rel) * (size_t)acsize, hipMemcpyHostToDevice, h->s));
  hipLaunchKernelGGL(ss_window_kernel, dim3(blocks_for(n, BLK)), dim3(BLK), 0, h->s, (const float*)h->d_kf[h->front], (const unsigned int*)h->d_kfp[h->front], (long long)i,
                     (long long)acsize, (long long)n, (const Rel*)h->d_rel, h->d_win);
  VX_HIP(h, hipGetLastError());
  h->launches += 1;
  const hipError_t e = vxwait::stream_wait(h->s);      // the consumers run on streams of their own
  h->waits += 1;
  if (e != hipSuccess) return fail(h, VXBA_ERR_HIP, std::string("session_window_cloud: ") + hipGetErrorString(e));
  h->n_win = n;
  *n_out = n; *d_xyz = h->d_win;
  return VXBA_OK;
}

int vxba_session_read_window(vxba_session* h, float* xyz) {
  if (!h) return VXBA_ERR_ARG;
  if (h->n_win > 0 && !xyz) return fail(h, VXBA_ERR_ARG, "session_read_window: null output");
  VX_HIP(h, hipSetDevice(h->device));
  if (h->n_win > 0) VX_HIP(h, hipMemcpy(xyz, h->d_win, (size_t)h->n_win * 3 * sizeof(float), hipMemcpyDeviceToHost));
  return VXBA_OK;
}

int vxba_session_set_profiling(vxba_session* h, int enable) {
  if (!h) return VXBA_ERR_ARG;
  VX_HIP(h, hipSetDevice(h->device));
  for (vxu::Event& e : h->ev) if (enable) VX_HIP(h, e.create());
  h->profiling = enable != 0;
  h->ev_valid = false;
  return VXBA_OK;
}

int vxba_session_stage_times(vxba_session* h, double ms[3]) {
  if (!h || !ms) return VXBA_ERR_ARG;
  if (!h->ev_valid) return fail(h, VXBA_ERR_STATE, "session_stage_times: the last build was not profiled, or held no point");
  for (int k = 0; k < 3; k++) {
    float t = 0.f;
    VX_HIP(h, hipEventElapsedTime(&t, h->ev[k], h->ev[k + 1]));
    ms[k] = (double)t;
  }
  return VXBA_OK;
}

int vxba_session_stats(const vxba_session* h, int64_t out[4]) {
  if (!h || !out) return VXBA_ERR_ARG;
  out[0] = h->launches; out[1] = h->waits; out[2] = h->scan_ptr.back(); out[3] = num_kf(h);
  return VXBA_OK;
}

int vxba_globalmap(int device, int n_sets, const float* const* d_xyz, const int64_t* const* cloud_ptr, const int64_t* n_keyframes, const double* const* poses,
                   const float* intensity, int64_t interval_size, float* out_xyzi, int64_t capacity, int64_t* n_out, int64_t* chunk_ptr, int64_t* n_chunks) {
  if (n_sets < 0 || interval_size <= 0 || capacity < 0 || !n_out || (n_sets > 0 && (!d_xyz || !cloud_ptr || !n_keyframes || !poses || !intensity))) return VXBA_ERR_ARG;
  *n_out = 0;
  if (n_chunks) *n_chunks = 0;
  int64_t psize = 0, n_kf = 0;
  for (int s = 0; s < n_sets; s++) {
    const int64_t K = n_keyframes[s];
    if (K < 0 || !cloud_ptr[s] || (K > 0 && !poses[s])) return VXBA_ERR_ARG;
    for (int64_t k = 0; k < K; k++) if (cloud_ptr[s][k + 1] < cloud_ptr[s][k]) return VXBA_ERR_ARG;
    for (int64_t k = 0; k < 12 * K; k++) if (!std::isfinite(poses[s][k])) return VXBA_ERR_ARG;
    if (cloud_ptr[s][K] > cloud_ptr[s][0] && !d_xyz[s]) return VXBA_ERR_ARG;
    psize += cloud_ptr[s][K] - cloud_ptr[s][0];
    n_kf += K;
  }
  const long long jump = map_jump(psize, interval_size);
  std::vector<MapKf> tab((size_t)n_kf);
  std::vector<long long> off((size_t)n_kf + 1, 0);
  std::vector<int64_t> chunks{0};
  int64_t t = 0, pending = 0;
  for (int s = 0; s < n_sets; s++)
    for (int64_t k = 0; k < n_keyframes[s]; k++, t++) {
      MapKf& e = tab[t];
      std::memcpy(e.R, poses[s] + 12 * k, 9 * sizeof(double));
      std::memcpy(e.p, poses[s] + 12 * k + 9, 3 * sizeof(double));
      e.src = d_xyz[s] ? d_xyz[s] + 3 * cloud_ptr[s][k] : nullptr;
      e.intensity = intensity[s];
      const long long c = map_count(cloud_ptr[s][k + 1] - cloud_ptr[s][k], jump);
      off[t + 1] = off[t] + c;
      pending += c;
      if (pending > interval_size) { chunks.push_back(off[t + 1]); pending = 0; }      // the flush after a keyframe (:141-146)
    }
  const int64_t total = off[n_kf];
  chunks.push_back(total);                                                             // the last publish (:149), empty or not
  *n_out = total;
  if (total > capacity || (total > 0 && !out_xyzi)) return VXBA_ERR_ARG;               // *n_out tells how much room it takes
  if (chunk_ptr) std::memcpy(chunk_ptr, chunks.data(), sizeof(int64_t) * chunks.size());
  if (n_chunks) *n_chunks = (int64_t)chunks.size() - 1;
  if (total == 0) return VXBA_OK;
  if (const int rc = vxu::select_device(device)) return rc;
  vxu::Lease lease(device);
  MapKf* d_tab = nullptr; long long* d_off = nullptr; float4* d_out = nullptr;
  VX_HIP_RC(lease.layout([&](vxu::Arena& a) { d_tab = a.take<MapKf>((size_t)n_kf); d_off = a.take<long long>((size_t)n_kf + 1); d_out = a.take<float4>((size_t)total); }));
  VX_HIP_RC(hipMemcpy(d_tab, tab.data(), sizeof(MapKf) * (size_t)n_kf, hipMemcpyHostToDevice));
  VX_HIP_RC(hipMemcpy(d_off, off.data(), sizeof(long long) * ((size_t)n_kf + 1), hipMemcpyHostToDevice));
  hipLaunchKernelGGL(gm_gather_kernel, dim3(blocks_for(total, BLK)), dim3(BLK), 0, nullptr, (const MapKf*)d_tab, (const long long*)d_off, (long long)n_kf, (long long)total, jump,
                     d_out);
  VX_HIP_RC(hipGetLastError());
  VX_HIP_RC(hipMemcpy(out_xyzi, d_out, sizeof(float4) * (size_t)total, hipMemcpyDeviceToHost));
  return VXBA_OK;
}

}  // extern "C"
