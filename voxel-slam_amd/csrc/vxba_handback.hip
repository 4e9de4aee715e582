// The loop hand-back on the GPU (include/vxba.h: vxba_kfarchive_*): the running session's `keyframes` vector resident on the device, and the three
// places of the reference that turn keyframe clouds into world-frame fixed points of the local map -- keyframe_loading (voxelslam.cpp:1189-1228),
// the map_loop build at the tail of thd_loop_closure's optimisation branch (:2131-2150) and the buffered scans of loop_update (:1161-1168).
//
// The archive: one packed store of `down` rows (x, y, z, var00, var11, var22 float32, as vxba_keyframe_device hands them out) that grows
// geometrically; offsets, ids, x0, jour and the exist flags live on the host, as do the float32 snapshot of the history positions and the
// radius search over it (K is a few thousand at most).
//
// Launch plan of vxba_kfarchive_map_loop / _map_loop_scans / _load_near, N = the output points:
//   one pinned copy    [output offsets S + 1 | poses S x 12 | sources S] of the S selected segments (a keyframe listed once per cloud that holds it:
//                      the cumulative form simply lists keyframes repeatedly)
//   hb_world_kernel    one lane per output point: the segment by binary search in the offset table, q = R double(v) + p through
//                      vxkf::transform_point into shared memory; then the workgroup writes its 256 rows of `pnt` (768 doubles) and of `var`
//                      (2304 doubles, the zeros included: fix_divide reads all nine) with lane-consecutive 8-byte stores -- a wave's 64 stores are
//                      512 contiguous bytes, where a row per lane would be 24- and 72-byte strides
// One launch and one host wait whatever S and N.
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdint>
#include <cstring>
#include <string>
#include <vector>

#include "../../include/vxba.h"
#include "vxba_dev.hpp"
#include "vxba_handback_math.hpp"
#include "vxba_wait.hpp"

namespace vxhb {

constexpr int BLK = 256;
constexpr int MAX_INIT = 64;           // keyframes of a map_loop
constexpr int MAX_PENDING = 1024;      // buffered scans of a map_loop_scans
constexpr int64_t MAX_POINTS = (int64_t)0x3fffffff;     // what vxba_map_cut_voxel_fix takes in one cloud

struct Seg {              // where a segment's rows come from
  const float* xyzv;      // a keyframe: rows of 6 float32 ...
  const double* pnt;      // ... or a buffered scan: body points n x 3
  const double* var9;     // and its variances n x 9 (may be NULL: zeros)
};

__global__ void __launch_bounds__(BLK) hb_world_kernel(const long long* __restrict__ off, const double* __restrict__ pose, const Seg* __restrict__ seg, long long n_seg, long long n,
                                                       int with_var, double* __restrict__ out_pnt, double* __restrict__ out_var) {
#pragma clang fp contract(off)
  __shared__ double s_q[3 * BLK];
  __shared__ float s_d[3 * BLK];        // a keyframe point's variance columns
  __shared__ long long s_row[BLK];      // a scan point's row in its segment; -1: a keyframe point
  __shared__ int s_seg[BLK];
  const long long base = (long long)blockIdx.x * BLK;
  const int t = threadIdx.x;
  const long long g = base + t;
  if (g < n) {
    const long long s = vxss::owner_of(off, n_seg, g);
    const long long j = g - off[s];
    const Seg e = seg[s];
    const double* P = pose + 12 * s;
    double q[3];
    if (e.xyzv) {
      const float* r = e.xyzv + 6 * j;
      const float v[3] = {r[0], r[1], r[2]};
      world_point(P, v, q);
      s_d[3 * t] = r[3]; s_d[3 * t + 1] = r[4]; s_d[3 * t + 2] = r[5];
      s_row[t] = -1;
    } else {
      const double v[3] = {e.pnt[3 * j], e.pnt[3 * j + 1], e.pnt[3 * j + 2]};
      world_point(P, v, q);
      s_row[t] = j;
    }
    s_seg[t] = (int)s;
    s_q[3 * t] = q[0]; s_q[3 * t + 1] = q[1]; s_q[3 * t + 2] = q[2];
  }
  __syncthreads();
  const long long left = n - base;
  const int m = left < BLK ? (int)left : BLK;      // rows of this workgroup
  for (int e = t; e < 3 * m; e += BLK) out_pnt[3 * base + e] = s_q[e];
  if (!with_var) return;
  for (int e = t; e < 9 * m; e += BLK) {
    const int pt = e / 9, c = e - 9 * pt;
    const long long j = s_row[pt];
    double v = 0.0;
    if (j < 0) v = diag_entry(s_d[3 * pt], s_d[3 * pt + 1], s_d[3 * pt + 2], c);
    else { const double* var9 = seg[s_seg[pt]].var9; if (var9) v = var9[9 * j + c]; }
    out_var[9 * base + e] = v;
  }
}

}  // namespace vxhb

struct vxba_kfarchive {
  int device = 0;
  std::string err;
  vxu::Stream s;
  // the keyframes: packed rows on the device, everything else on the host
  vxu::Dev<float> store;                 // capacity in floats; rows of 6
  std::vector<int64_t> off{0};           // K + 1 offsets (points)
  std::vector<int64_t> ids;
  std::vector<double> x0, jour;          // K x 12, K
  std::vector<unsigned char> exist;
  // arm_history's snapshot: what the search reads
  std::vector<float> snap;               // n_hist x 3
  int64_t n_hist = 0, history_kfsize = 0;
  // one call's tables and outputs
  vxu::Pin<char> h_tab; vxu::Dev<char> d_tab;
  vxu::Dev<double> out_pnt, out_var;
  int64_t stats[4] = {0, 0, 0, 0};       // launches, host waits, bytes D2H, bytes H2D of the last call
};

using namespace vxhb;
using vxu::blocks_for, vxu::fail;

namespace {

inline int64_t num_kf(const vxba_kfarchive* h) { return (int64_t)h->ids.size(); }

inline void zero_stats(vxba_kfarchive* h) { h->stats[0] = h->stats[1] = h->stats[2] = h->stats[3] = 0; }

inline bool finite12(const double* p) {
  for (int k = 0; k < 12; k++) if (!std::isfinite(p[k])) return false;
  return true;
}

// room for `rows` more rows; the rows already there are kept
int grow_store(vxba_kfarchive* h, int64_t rows) {
  const size_t have = (size_t)h->off.back() * 6, need = have + (size_t)rows * 6;
  if (need <= h->store.capacity()) return VXBA_OK;
  vxu::Dev<float> nb;
  VX_HIP(h, nb.reserve(need, need + need / 2 + 6 * 1024));
  if (have) {
    VX_HIP(h, hipMemcpyAsync(nb, h->store, have * sizeof(float), hipMemcpyDeviceToDevice, h->s));
    VX_HIP(h, vxwait::stream_wait(h->s));
    h->stats[1] += 1;
  }
  h->store = std::move(nb);
  return VXBA_OK;
}

int add_impl(vxba_kfarchive* h, int64_t id, const double* pose, double jour, int64_t n, const float* xyzv, bool on_device) {
  if (!h) return VXBA_ERR_ARG;
  if (!pose || n < 0 || n > MAX_POINTS || (n > 0 && !xyzv)) return fail(h, VXBA_ERR_ARG, "kfarchive_add: bad argument");
  if (!finite12(pose) || !std::isfinite(jour)) return fail(h, VXBA_ERR_ARG, "kfarchive_add: the pose is not finite");
  zero_stats(h);
  VX_HIP(h, hipSetDevice(h->device));
  if (n > 0) {
    if (const int rc = grow_store(h, n)) return rc;
    VX_HIP(h, hipMemcpyAsync(h->store + 6 * (size_t)h->off.back(), xyzv, (size_t)n * 6 * sizeof(float), on_device ? hipMemcpyDeviceToDevice : hipMemcpyHostToDevice, h->s));
    VX_HIP(h, vxwait::stream_wait(h->s));      // the source is the caller's again when the call returns
    h->stats[1] += 1;
    if (!on_device) h->stats[3] += n * 24;
  }
  h->off.push_back(h->off.back() + n);
  h->ids.push_back(id);
  h->x0.insert(h->x0.end(), pose, pose + 12);
  h->jour.push_back(jour);
  h->exist.push_back(0);      // Keyframe's constructor
  return VXBA_OK;
}

struct Sel { int64_t n; const double* pose; Seg seg; };      // one segment of a launch

// the one launch: the segments in order, clouds given by cloud_ptr over them on the caller's side
int run_world(vxba_kfarchive* h, const std::vector<Sel>& sel, bool with_var, const char* what) {
  const size_t S = sel.size();
  int64_t N = 0;
  for (const Sel& e : sel) N += e.n;
  if (N == 0) return VXBA_OK;
  if (N > MAX_POINTS) return fail(h, VXBA_ERR_ARG, std::string(what) + ": more than 2^30 - 1 output points");
  const size_t b_off = (S + 1) * sizeof(long long), b_pose = S * 12 * sizeof(double), b_seg = S * sizeof(Seg), bytes = b_off + b_pose + b_seg;
  VX_HIP(h, h->h_tab.reserve(bytes, 2 * bytes));
  VX_HIP(h, h->d_tab.reserve(bytes, 2 * bytes));
  VX_HIP(h, h->out_pnt.reserve(3 * (size_t)N, 3 * ((size_t)N + (size_t)N / 4)));
  if (with_var) VX_HIP(h, h->out_var.reserve(9 * (size_t)N, 9 * ((size_t)N + (size_t)N / 4)));
  long long* t_off = (long long*)h->h_tab.get();
  double* t_pose = (double*)(h->h_tab.get() + b_off);
  Seg* t_seg = (Seg*)(h->h_tab.get() + b_off + b_pose);
  t_off[0] = 0;
  for (size_t s = 0; s < S; s++) {
    t_off[s + 1] = t_off[s] + sel[s].n;
    std::memcpy(t_pose + 12 * s, sel[s].pose, 12 * sizeof(double));
    t_seg[s] = sel[s].seg;
  }
  VX_HIP(h, hipMemcpyAsync(h->d_tab, h->h_tab, bytes, hipMemcpyHostToDevice, h->s));
  h->stats[3] += (int64_t)bytes;
  hipLaunchKernelGGL(hb_world_kernel, dim3(blocks_for(N, BLK)), dim3(BLK), 0, h->s, (const long long*)h->d_tab.get(), (const double*)(h->d_tab.get() + b_off),
                     (const Seg*)(h->d_tab.get() + b_off + b_pose), (long long)S, (long long)N, with_var ? 1 : 0, h->out_pnt.get(), with_var ? h->out_var.get() : nullptr);
  VX_HIP(h, hipGetLastError());
  h->stats[0] += 1;
  VX_HIP(h, vxwait::stream_wait(h->s));      // the map reads the outputs on its own stream: they are complete when the call returns
  h->stats[1] += 1;
  return VXBA_OK;
}

int map_loop_impl(vxba_kfarchive* h, int init_num, int cumulative, int n_pending, const double* pending_poses, const int64_t* pending_n, const double* const* d_pending_pnt,
                  const double* const* d_pending_var, int64_t* cloud_ptr, int* n_clouds, const double** d_pnt_world, const double** d_var) {
  if (!h) return VXBA_ERR_ARG;
  if (init_num <= 0) init_num = 5;
  if (!cloud_ptr || !n_clouds || !d_pnt_world || !d_var || init_num > MAX_INIT || n_pending < 0 || n_pending > MAX_PENDING ||
      (n_pending > 0 && (!pending_poses || !pending_n || !d_pending_pnt)))
    return fail(h, VXBA_ERR_ARG, "kfarchive_map_loop: bad argument");
  for (int i = 0; i < n_pending; i++) {
    if (pending_n[i] < 0 || pending_n[i] > MAX_POINTS || (pending_n[i] > 0 && !d_pending_pnt[i])) return fail(h, VXBA_ERR_ARG, "kfarchive_map_loop: bad buffered scan");
    if (!finite12(pending_poses + 12 * i)) return fail(h, VXBA_ERR_ARG, "kfarchive_map_loop: a buffered scan's pose is not finite");
  }
  zero_stats(h);
  VX_HIP(h, hipSetDevice(h->device));
  const int64_t K = num_kf(h), first = K > init_num ? K - init_num : 0;
  std::vector<Sel> sel;
  int nc = 0;
  cloud_ptr[0] = 0;
  for (int64_t k = first; k < K; k++, nc++) {      // cloud nc: keyframe k alone, or (upstream: pvec_tem is never cleared) keyframes first .. k
    int64_t pts = 0;
    for (int64_t a = cumulative ? first : k; a <= k; a++) {
      const int64_t n = h->off[a + 1] - h->off[a];
      sel.push_back({n, h->x0.data() + 12 * a, {n > 0 ? h->store.get() + 6 * (size_t)h->off[a] : nullptr, nullptr, nullptr}});
      pts += n;
    }
    cloud_ptr[nc + 1] = cloud_ptr[nc] + pts;
  }
  for (int i = 0; i < n_pending; i++, nc++) {
    sel.push_back({pending_n[i], pending_poses + 12 * i, {nullptr, d_pending_pnt[i], d_pending_var ? d_pending_var[i] : nullptr}});
    cloud_ptr[nc + 1] = cloud_ptr[nc] + pending_n[i];
  }
  // a segment without points owns no output row, so its NULL source is never read
  if (const int rc = run_world(h, sel, true, "kfarchive_map_loop")) return rc;
  *n_clouds = nc;
  const bool any = cloud_ptr[nc] > 0;
  *d_pnt_world = any ? h->out_pnt.get() : nullptr;
  *d_var = any ? h->out_var.get() : nullptr;
  return VXBA_OK;
}

}  // namespace

extern "C" {

int vxba_kfarchive_create(int device, vxba_kfarchive** out) {
  if (!out) return VXBA_ERR_ARG;
  *out = nullptr;
  if (const int rc = vxu::select_device(device)) return rc;
  vxba_kfarchive* h = new vxba_kfarchive();
  h->device = device;
  if (h->s.create() != hipSuccess) { delete h; return VXBA_ERR_HIP; }
  *out = h;
  return VXBA_OK;
}

int vxba_kfarchive_destroy(vxba_kfarchive* h) {
  if (!h) return VXBA_OK;
  hipSetDevice(h->device);
  if (h->s) hipStreamSynchronize(h->s);
  delete h;
  return VXBA_OK;
}

const char* vxba_kfarchive_last_error(const vxba_kfarchive* h) { return h ? h->err.c_str() : "null handle"; }

int vxba_kfarchive_clear(vxba_kfarchive* h) {
  if (!h) return VXBA_ERR_ARG;
  h->off.assign(1, 0);
  h->ids.clear(); h->x0.clear(); h->jour.clear(); h->exist.clear(); h->snap.clear();
  h->n_hist = h->history_kfsize = 0;
  zero_stats(h);
  return VXBA_OK;
}

int vxba_kfarchive_add(vxba_kfarchive* h, int64_t id, const double pose[12], double jour, int64_t n, const float* down_xyzv) {
  return add_impl(h, id, pose, jour, n, down_xyzv, false);
}

int vxba_kfarchive_add_device(vxba_kfarchive* h, int64_t id, const double pose[12], double jour, int64_t n, const float* d_down_xyzv) {
  return add_impl(h, id, pose, jour, n, d_down_xyzv, true);
}

int64_t vxba_kfarchive_num(const vxba_kfarchive* h) { return h ? num_kf(h) : 0; }

int vxba_kfarchive_info(const vxba_kfarchive* h, int64_t k, int64_t* id, double pose[12], double* jour, int64_t* n, int* exist) {
  if (!h || k < 0 || k >= num_kf(h)) return VXBA_ERR_ARG;
  if (id) *id = h->ids[k];
  if (pose) std::memcpy(pose, h->x0.data() + 12 * k, 12 * sizeof(double));
  if (jour) *jour = h->jour[k];
  if (n) *n = h->off[k + 1] - h->off[k];
  if (exist) *exist = h->exist[k];
  return VXBA_OK;
}

int vxba_kfarchive_read(vxba_kfarchive* h, int64_t k, float* out) {
  if (!h) return VXBA_ERR_ARG;
  if (k < 0 || k >= num_kf(h)) return fail(h, VXBA_ERR_ARG, "kfarchive_read: no such keyframe");
  const int64_t n = h->off[k + 1] - h->off[k];
  if (n == 0) return VXBA_OK;
  if (!out) return fail(h, VXBA_ERR_ARG, "kfarchive_read: bad argument");
  VX_HIP(h, hipSetDevice(h->device));
  VX_HIP(h, hipMemcpyAsync(out, h->store + 6 * (size_t)h->off[k], (size_t)n * 6 * sizeof(float), hipMemcpyDeviceToHost, h->s));
  VX_HIP(h, hipStreamSynchronize(h->s));
  return VXBA_OK;
}

int vxba_kfarchive_device(const vxba_kfarchive* h, const float** d_xyzv, const int64_t** cloud_ptr) {
  if (!h) return VXBA_ERR_ARG;
  if (d_xyzv) *d_xyzv = h->off.back() > 0 ? h->store.get() : nullptr;
  if (cloud_ptr) *cloud_ptr = h->off.data();
  return VXBA_OK;
}

int vxba_kfarchive_set_poses(vxba_kfarchive* h, const double* x0) {
  if (!h) return VXBA_ERR_ARG;
  const int64_t K = num_kf(h);
  if (K > 0 && !x0) return fail(h, VXBA_ERR_ARG, "kfarchive_set_poses: bad argument");
  for (int64_t k = 0; k < K; k++)
    if (!finite12(x0 + 12 * k)) return fail(h, VXBA_ERR_ARG, "kfarchive_set_poses: pose " + std::to_string(k) + " is not finite");
  if (K > 0) std::memcpy(h->x0.data(), x0, sizeof(double) * 12 * K);
  return VXBA_OK;
}

int vxba_kfarchive_arm_history(vxba_kfarchive* h, int init_num) {
  if (!h) return VXBA_ERR_ARG;
  if (init_num <= 0) init_num = 5;
  const int64_t K = num_kf(h);
  h->history_kfsize = 0;                                                            // :2103
  for (int64_t k = K > init_num ? K - init_num : 0; k < K; k++) h->exist[k] = 0;    // :2138
  if (K > init_num) {                                                               // :2152-2167
    h->n_hist = K - init_num;
    h->snap.resize(3 * (size_t)h->n_hist);
    for (int64_t k = 0; k < h->n_hist; k++) {
      h->exist[k] = 1;
      for (int j = 0; j < 3; j++) h->snap[3 * k + j] = (float)h->x0[12 * k + 9 + j];
    }
    h->history_kfsize = h->n_hist;
  }
  return VXBA_OK;
}

int64_t vxba_kfarchive_history_size(const vxba_kfarchive* h) { return h ? h->history_kfsize : 0; }

int vxba_kfarchive_load_near(vxba_kfarchive* h, const double p_curr[3], double radius, int* k_loaded, int64_t* n, const double** d_pnt_world) {
  if (!h) return VXBA_ERR_ARG;
  if (!p_curr || !k_loaded || !n || !d_pnt_world || !std::isfinite(p_curr[0]) || !std::isfinite(p_curr[1]) || !std::isfinite(p_curr[2]) || std::isnan(radius))
    return fail(h, VXBA_ERR_ARG, "kfarchive_load_near: bad argument");
  zero_stats(h);
  *k_loaded = -1; *n = 0; *d_pnt_world = nullptr;
  if (h->history_kfsize <= 0) return VXBA_OK;                                       // :1191
  if (radius <= 0) radius = 10.0;
  const float pc[3] = {(float)p_curr[0], (float)p_curr[1], (float)p_curr[2]};
  // the snapshot covers keyframes [0, n_hist); a keyframe added since is not in it
  const long long k = nearest_existing(h->snap.data(), h->n_hist, h->exist.data(), pc, (float)(radius * radius));
  if (k < 0) return VXBA_OK;
  VX_HIP(h, hipSetDevice(h->device));
  const int64_t pts = h->off[k + 1] - h->off[k];
  std::vector<Sel> sel{{pts, h->x0.data() + 12 * k, {pts > 0 ? h->store.get() + 6 * (size_t)h->off[k] : nullptr, nullptr, nullptr}}};
  if (const int rc = run_world(h, sel, false, "kfarchive_load_near")) return rc;
  h->exist[k] = 0;                                                                  // :1222-1223
  h->history_kfsize--;
  *k_loaded = (int)k; *n = pts; *d_pnt_world = pts > 0 ? h->out_pnt.get() : nullptr;
  return VXBA_OK;
}

int vxba_kfarchive_map_loop(vxba_kfarchive* h, int init_num, int cumulative, int64_t* cloud_ptr, int* n_clouds, const double** d_pnt_world, const double** d_var) {
  return map_loop_impl(h, init_num, cumulative, 0, nullptr, nullptr, nullptr, nullptr, cloud_ptr, n_clouds, d_pnt_world, d_var);
}

int vxba_kfarchive_map_loop_scans(vxba_kfarchive* h, int init_num, int cumulative, int n_pending, const double* pending_poses, const int64_t* pending_n,
                                  const double* const* d_pending_pnt, const double* const* d_pending_var, int64_t* cloud_ptr, int* n_clouds, const double** d_pnt_world,
                                  const double** d_var) {
  return map_loop_impl(h, init_num, cumulative, n_pending, pending_poses, pending_n, d_pending_pnt, d_pending_var, cloud_ptr, n_clouds, d_pnt_world, d_var);
}

int vxba_kfarchive_stats(const vxba_kfarchive* h, int64_t out[4]) {
  if (!h || !out) return VXBA_ERR_ARG;
  for (int k = 0; k < 4; k++) out[k] = h->stats[k];
  return VXBA_OK;
}

}  // extern "C"
