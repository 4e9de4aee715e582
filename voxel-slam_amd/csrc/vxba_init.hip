// Scan-to-cloud odometry of the initialisation on the GPU -- self-contained translation unit: the device-resident world cloud, the exact
// five-nearest search, the per-point plane fit and the `vxba_initodom_*` entry points of include/vxba.h.
//
// What it replaces (VoxelSLAM/src): `lio_state_estimation_kdtree` voxelslam.cpp:960-1098 with its kd-tree (`pl_tree`, `kd_map`).
//
// For the first win_size scans there is no plane map.  The reference aligns each scan against a growing point cloud: five nearest
// neighbours per point from a kd-tree, a plane through them, and the iterated EKF of the regular odometry.  Here the search is brute force,
// because brute force is exact and the clouds of win_size scans filtered at 0.5 m are small:
//
//   init_sweep_kernel   four lanes per scan point, 64 scan points per workgroup.  The cloud passes through LDS in tiles of 1024 float4; lane j
//                       of a point's group scans the entries j, j + 4, ... of every tile and keeps its five best in registers (statically
//                       indexed compare-exchange), ordered by (float32 squared distance, index).  The four lists are merged by the same order,
//                       so the result is the one an ascending scan over the whole cloud gives, whatever the tile and lane split; equal
//                       distances go to the lower index.  The group's first lane then fits the plane (vxba_init_math.hpp), applies the gate,
//                       stores (n, d) for the iterations that do not search again, and accumulates the 21 + 6 + 1 sums.  Sums: the workgroup's
//                       64 leaders through LDS, added in point order, one partial row per workgroup; lio_ekf_kernel<1> adds the rows in a fixed
//                       order.  No float atomics: two runs give identical bits.
//   lio_ekf_kernel<1>   (vxba_lio.hip) the 15 x 15 update, the refind / rematch schedule.
//   init_append_kernel  the scan under a state, rounded to float, behind the cloud.
// vxba_initodom_step enqueues four rounds of (sweep, EKF) -- the kernels of a finished call return at their first instruction --, the append
// and the voxel filter (vxba_downsample.hip) and waits once, inside the filter, for the voxel count.  Own kernel launches per step: 9 + the
// filter's 4, whatever the cloud size (rocPRIM's sort, run-length encode and scan inside the filter choose their own launches).  A step that
// has to grow the scan or cloud buffers waits once more per buffer (counted), and so does the filter when its scratch grows (not counted:
// it is the filter's).  The filter's wait comes BEFORE its last three launches (widen, scan, mean): the step returns with the new cloud still
// being written.  Every later use of the cloud -- search, sweep, append, read-back -- is enqueued on the handle's one stream, behind them.
#include "vxba_wait.hpp"
#include <hip/hip_runtime.h>

#include <algorithm>
#include <chrono>
#include <cmath>
#include <cstdint>
#include <cstring>
#include <limits>
#include <mutex>
#include <string>
#include <vector>

#include "../../include/vxba.h"
#include "vxba_dev.hpp"
#include "vxba_downsample.h"
#include "vxba_imu.hpp"
#include "vxba_init_math.hpp"
#include "vxba_internal.h"
#include "vxba_lio_ctl.hpp"
#include "vxba_math.hpp"

namespace vxin {

constexpr int BLK = 256;          // four waves
constexpr int LPQ = 4;            // lanes per query
constexpr int QPB = BLK / LPQ;    // queries per workgroup
constexpr int TILE = 1024;        // cloud points per LDS tile
constexpr int MAX_GRID = 256;     // partial rows lio_ekf_kernel adds; larger scans loop inside the workgroups
constexpr int NACC = 28;          // HTH upper triangle 21 | HTz 6 | valid
constexpr int NO_INDEX = 0x7fffffff;
constexpr int64_t SEED_MIN = 100; // pl_tree->size() < 100: the scan only seeds the cloud

struct Top5 {
  float d[NMATCH];
  int i[NMATCH];
};

__device__ __forceinline__ void top_insert(Top5& t, float d, int i) {
  if (closer(d, i, t.d[NMATCH - 1], t.i[NMATCH - 1])) {
    t.d[NMATCH - 1] = d; t.i[NMATCH - 1] = i;
#pragma unroll
    for (int k = NMATCH - 1; k >= 1; k--) {
      const bool sw = closer(t.d[k], t.i[k], t.d[k - 1], t.i[k - 1]);
      const float da = t.d[k - 1], db = t.d[k];
      const int ia = t.i[k - 1], ib = t.i[k];
      t.d[k - 1] = sw ? db : da; t.d[k] = sw ? da : db;
      t.i[k - 1] = sw ? ib : ia; t.i[k] = sw ? ia : ib;
    }
  }
}

// The five nearest cloud points of (qx, qy, qz), ascending by (distance, index); fewer than five cloud points leave (inf, NO_INDEX) entries.
// Every lane of the workgroup takes part (the tile loads and the barriers are the workgroup's); the LPQ lanes of a query end with the same list.
__device__ __forceinline__ void search5(const float* __restrict__ cloud, int M, float qx, float qy, float qz, float4* tile, Top5& t) {
#pragma unroll
  for (int k = 0; k < NMATCH; k++) { t.d[k] = std::numeric_limits<float>::infinity(); t.i[k] = NO_INDEX; }
  const int j = threadIdx.x & (LPQ - 1);
  for (int t0 = 0; t0 < M; t0 += TILE) {
    __syncthreads();                                     // the previous tile has been read by every lane
    const int m = min(TILE, M - t0);
    for (int k = threadIdx.x; k < m; k += BLK) {
      const float* c = cloud + 3 * (size_t)(t0 + k);
      tile[k] = make_float4(c[0], c[1], c[2], 0.f);
    }
    __syncthreads();
#pragma unroll 4
    for (int k = j; k < m; k += LPQ) {
      const float4 c = tile[k];
      top_insert(t, sqdist(c.x, c.y, c.z, qx, qy, qz), t0 + k);
    }
  }
#pragma unroll
  for (int off = 1; off < LPQ; off <<= 1) {              // the group's lanes are neighbours inside one wave
    float od[NMATCH];
    int oi[NMATCH];
#pragma unroll
    for (int k = 0; k < NMATCH; k++) { od[k] = __shfl_xor(t.d[k], off, 64); oi[k] = __shfl_xor(t.i[k], off, 64); }
#pragma unroll
    for (int k = 0; k < NMATCH; k++) top_insert(t, od[k], oi[k]);
  }
}

// inspection: the search alone on float queries
__global__ __launch_bounds__(BLK) void init_search_kernel(const float* __restrict__ cloud, int M, const float* __restrict__ qry, long long n, int* __restrict__ idx,
                                                          float* __restrict__ sqd) {
  __shared__ float4 tile[TILE];
  const long long q = (long long)blockIdx.x * QPB + threadIdx.x / LPQ;
  const bool live = q < n;
  const float qx = live ? qry[3 * q] : 0.f, qy = live ? qry[3 * q + 1] : 0.f, qz = live ? qry[3 * q + 2] : 0.f;
  Top5 t;
  search5(cloud, M, qx, qy, qz, tile, t);
  if (live && (threadIdx.x & (LPQ - 1)) == 0) {
#pragma unroll
    for (int k = 0; k < NMATCH; k++) { idx[NMATCH * q + k] = t.i[k] == NO_INDEX ? -1 : t.i[k]; sqd[NMATCH * q + k] = t.d[k]; }
  }
}

// One pass of voxelslam.cpp:1001-1053.  pts: n x 3 body points; nn / ok / plane: the per-point records of the four iterations, iteration `it`
// at offset it * cap points.  M >= 5 (the caller enters with M >= 100).
__global__ __launch_bounds__(BLK) void init_sweep_kernel(const vxl::LioCtl* __restrict__ ctl, const double* __restrict__ pts, long long n, long long cap,
                                                         const float* __restrict__ cloud, int M, int* __restrict__ nn, int* __restrict__ ok,
                                                         double* __restrict__ plane, double* __restrict__ partials) {
  __shared__ float4 tile[TILE];
  __shared__ double red[QPB][NACC];
  if (ctl->done) return;
  double R[9], tr[3];
#pragma unroll
  for (int k = 0; k < 9; k++) R[k] = ctl->state[k];
#pragma unroll
  for (int k = 0; k < 3; k++) tr[k] = ctl->state[9 + k];
  const int refind = ctl->refind;
  const long long wr = (long long)ctl->iter * cap, rd = (long long)ctl->slot * cap;   // records written when searching, read otherwise
  double s[NACC];
#pragma unroll
  for (int k = 0; k < NACC; k++) s[k] = 0.0;
  const bool lead = (threadIdx.x & (LPQ - 1)) == 0;
  const long long nblk = (n + QPB - 1) / QPB;
  for (long long qb = blockIdx.x; qb < nblk; qb += gridDim.x) {
    const long long q = qb * QPB + threadIdx.x / LPQ;
    const bool live = q < n;
    double p[3] = {0.0, 0.0, 0.0}, w[3];
    if (live) { p[0] = pts[3 * q]; p[1] = pts[3 * q + 1]; p[2] = pts[3 * q + 2]; }
    world_point(R, tr, p, w);
    bool good = false;
    double nr[3] = {0.0, 0.0, 0.0}, d = 0.0;
    if (refind) {
      Top5 t;
      search5(cloud, M, (float)w[0], (float)w[1], (float)w[2], tile, t);
      if (live && lead && t.i[NMATCH - 1] == NO_INDEX) {   // a query no distance compares with (the host turns such scans away): no plane
#pragma unroll
        for (int k = 0; k < NMATCH; k++) nn[NMATCH * (wr + q) + k] = -1;
        ok[wr + q] = 0;
      } else if (live && lead) {
        double A[3 * NMATCH], direct[3], worst;
#pragma unroll
        for (int k = 0; k < NMATCH; k++) {
          const float* c = cloud + 3 * (size_t)t.i[k];
          A[3 * k] = (double)c[0]; A[3 * k + 1] = (double)c[1]; A[3 * k + 2] = (double)c[2];
        }
        fit_plane5(A, direct);
        good = gate5(A, direct, worst);
        plane_of(direct, nr, d);
#pragma unroll
        for (int k = 0; k < NMATCH; k++) nn[NMATCH * (wr + q) + k] = t.i[k];
        ok[wr + q] = good ? 1 : 0;
        double* pl = plane + 4 * (wr + q);
        pl[0] = nr[0]; pl[1] = nr[1]; pl[2] = nr[2]; pl[3] = d;
      }
    } else if (live && lead) {
      good = ok[rd + q] != 0;
      const double* pl = plane + 4 * (rd + q);
      nr[0] = pl[0]; nr[1] = pl[1]; nr[2] = pl[2]; d = pl[3];
    }
    if (good) {
      double jac[6], resid;
      jac_row(R, p, nr, d, w, jac, resid);
      int k = 0;
#pragma unroll
      for (int r = 0; r < 6; r++)
#pragma unroll
        for (int c = r; c < 6; c++, k++) s[k] += jac[r] * jac[c];
#pragma unroll
      for (int r = 0; r < 6; r++) s[21 + r] += jac[r] * resid;
      s[27] += 1.0;
    }
  }
  __syncthreads();
  if (lead) {
#pragma unroll
    for (int k = 0; k < NACC; k++) red[threadIdx.x / LPQ][k] = s[k];
  }
  __syncthreads();
  if (threadIdx.x < vxl::NSUM) {   // the row lio_ekf_kernel reads: HTH 21 | HTz 6 | nnt 6 (not used here) | count
    const int src = threadIdx.x < 27 ? threadIdx.x : (threadIdx.x == 33 ? 27 : -1);
    double tsum = 0.0;
    if (src >= 0)
      for (int qq = 0; qq < QPB; qq++) tsum += red[qq][src];
    partials[(size_t)blockIdx.x * vxl::NSUM + threadIdx.x] = tsum;
  }
}

// the scan under the control block's state, rounded to float, into out (n x 3)
__global__ void init_append_kernel(const vxl::LioCtl* __restrict__ ctl, const double* __restrict__ pts, long long n, float* __restrict__ out) {
  const long long q = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  if (q >= n) return;
  const double p[3] = {pts[3 * q], pts[3 * q + 1], pts[3 * q + 2]};
  double w[3];
  world_point(ctl->state, ctl->state + 9, p, w);
  out[3 * q] = (float)w[0]; out[3 * q + 1] = (float)w[1]; out[3 * q + 2] = (float)w[2];
}

// de-skew: one lane per OUTPUT slot; the host has laid out upstream's sequence (which point, under which IMU pose) before the launch
__global__ void init_deskew_kernel(const float* __restrict__ xyz, const float* __restrict__ toff, const int* __restrict__ src, const int* __restrict__ head,
                                   long long m, const double* __restrict__ table, const double* __restrict__ xc_ext /* xc 12 | ext 12 */, double* __restrict__ out) {
  const long long q = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  if (q >= m) return;
  const int i = src[q], k = head[q];
  double o[3];
  if (k < 0) extrinsic_point(xc_ext + 12, xyz + 3 * (size_t)i, o);
  else deskew_point(table + (size_t)POSE_LEN * k, xc_ext, xc_ext + 12, xyz + 3 * (size_t)i, (double)toff[i], o);
  out[3 * q] = o[0]; out[3 * q + 1] = o[1]; out[3 * q + 2] = o[2];
}

// sum of n n^T over the factor's cached plane normals (eig_vectors[a].col(0)): one workgroup, lanes stride over the voxels, then a fixed LDS tree
__global__ __launch_bounds__(256) void init_scatter_kernel(const double* __restrict__ eigvec, int VS, int V, double* __restrict__ out6) {
  __shared__ double red[256][6];
  double s[6] = {0, 0, 0, 0, 0, 0};
  for (int a = threadIdx.x; a < V; a += 256) {
    const double x = eigvec[a], y = eigvec[(size_t)VS + a], z = eigvec[2 * (size_t)VS + a];   // plane k = 3 col + row, col 0
    s[0] += x * x; s[1] += x * y; s[2] += x * z; s[3] += y * y; s[4] += y * z; s[5] += z * z;
  }
#pragma unroll
  for (int k = 0; k < 6; k++) red[threadIdx.x][k] = s[k];
  __syncthreads();
  for (int off = 128; off >= 1; off >>= 1) {
    if (threadIdx.x < off) {
#pragma unroll
      for (int k = 0; k < 6; k++) red[threadIdx.x][k] += red[threadIdx.x + off][k];
    }
    __syncthreads();
  }
  if (threadIdx.x < 6) out6[threadIdx.x] = red[0][threadIdx.x];
}

// calcBodyVar (voxelslam.hpp:164-185) on a de-skewed body point followed by pvec_update (:203-215) -- the converged rounds of motion_init --, or the identity
// variance of motion_blur's pointVar (first-phase rounds); the world point either way.  One lane per point.
struct PointVarArg { double R[9], p[3], rot_var[9], tsl_var[9]; float range_inc; double dir_var; int with_var; };
__global__ void init_pointvar_kernel(double* __restrict__ body, long long m, PointVarArg a, double* __restrict__ var9, double* __restrict__ pwld) {
  const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= m) return;
  double pb[3] = {body[3 * i], body[3 * i + 1], body[3 * i + 2]};
  double O[9] = {1, 0, 0, 0, 1, 0, 0, 0, 1};
  if (a.with_var) {
    double V[9];
    body_var(pb, a.range_inc, a.dir_var, V);        // rewrites a zero z, as upstream does
    body[3 * i + 2] = pb[2];
    world_var(a.R, pb, V, a.rot_var, a.tsl_var, O);
  }
  for (int k = 0; k < 9; k++) var9[9 * i + k] = O[k];
  double w[3];
  world_point(a.R, a.p, pb, w);
  pwld[3 * i] = w[0]; pwld[3 * i + 1] = w[1]; pwld[3 * i + 2] = w[2];
}

}  // namespace vxin

struct vxba_initodom {
  int device = 0;
  vxu::Stream stream;
  vxu::Dev<float> d_cloud[2];               // the resident cloud is d_cloud[cur]; the filter writes the other one.  Both grow together
  int cur = 0;
  int64_t M = 0;
  int64_t cloud_cap() const { return (int64_t)d_cloud[0].capacity() / 3; }
  // the resident scan and its records, one block carved for pts_cap() points: n x 3 body points | nn 4 x cap x 5 | ok 4 x cap | plane 4 x cap x 4
  static constexpr size_t PT_BYTES = 3 * 8 + 4 * vxin::NMATCH * 4 + 4 * 4 + 4 * 4 * 8;
  vxu::Dev<char> d_scan;
  int64_t pts_cap() const { return (int64_t)(d_scan.capacity() / PT_BYTES); }
  double* d_pts() const { return (double*)d_scan.get(); }
  int* d_nn() const { return (int*)(d_scan.get() + pts_cap() * 24); }
  int* d_ok() const { return d_nn() + pts_cap() * 4 * vxin::NMATCH; }
  double* d_plane() const { return (double*)(d_ok() + pts_cap() * 4); }
  int64_t n_pts = 0;
  int refound[4] = {0, 0, 0, 0};            // which iterations of the last step searched (their records are readable)
  vxu::Dev<vxl::LioCtl> d_ctl;
  vxu::Dev<double> d_partials;
  vxd::Scratch ds;
  vxu::Arena work;                          // vxba_initodom_search: queries up, indices and distances down
  int64_t launches = 0, syncs = 0;
  std::string err;
  std::recursive_mutex mtx;
};

namespace {

#define IO_LOCK(h) std::lock_guard<std::recursive_mutex> lk__((h)->mtx)

// room for `want` cloud points in both buffers; the resident cloud is kept
int io_cloud_reserve(vxba_initodom* h, int64_t want) {
  if (want <= h->cloud_cap()) return VXBA_OK;
  int64_t cap = std::max<int64_t>(h->cloud_cap(), (int64_t)1 << 18);
  while (cap < want) cap *= 2;
  vxu::Dev<float> nb[2];                    // gone with the scope unless both are there and the cloud has been copied
  VX_HIP(h, nb[0].reserve((size_t)cap * 3));
  VX_HIP(h, nb[1].reserve((size_t)cap * 3));
  if (h->M) VX_HIP(h, hipMemcpyAsync(nb[0], h->d_cloud[h->cur], (size_t)h->M * 3 * sizeof(float), hipMemcpyDeviceToDevice, h->stream));
  VX_HIP(h, hipStreamSynchronize(h->stream));
  h->syncs += 1;
  h->d_cloud[0] = std::move(nb[0]); h->d_cloud[1] = std::move(nb[1]); h->cur = 0;
  return VXBA_OK;
}

int io_scan_reserve(vxba_initodom* h, int64_t n) {
  if (n > h->pts_cap()) {
    VX_HIP(h, hipStreamSynchronize(h->stream));
    h->syncs += 1;
    const int64_t cap = (std::max<int64_t>(n, 2 * h->pts_cap()) + 255) / 256 * 256;
    VX_HIP(h, h->d_scan.reserve((size_t)cap * vxba_initodom::PT_BYTES));
  }
  h->n_pts = n;
  for (int k = 0; k < 4; k++) h->refound[k] = 0;
  return VXBA_OK;
}

}  // namespace

extern "C" {

int vxba_initodom_create(int device, vxba_initodom** out) {
  if (!out) return VXBA_ERR_ARG;
  *out = nullptr;
  if (const int rc = vxu::select_device(device)) return rc;
  vxba_initodom* h = new vxba_initodom();
  h->device = device;
  if (h->stream.create() != hipSuccess || h->d_ctl.reserve(1) != hipSuccess || h->d_partials.reserve((size_t)vxin::MAX_GRID * vxl::NSUM) != hipSuccess) {
    delete h;
    return VXBA_ERR_HIP;
  }
  *out = h;
  return VXBA_OK;
}

int vxba_initodom_destroy(vxba_initodom* h) {
  if (!h) return VXBA_ERR_ARG;
  hipSetDevice(h->device);
  if (h->stream) hipStreamSynchronize(h->stream);
  h->ds.release(); h->work.release();
  delete h;
  return VXBA_OK;
}

const char* vxba_initodom_last_error(const vxba_initodom* h) { return h ? h->err.c_str() : "null handle"; }

int vxba_initodom_clear(vxba_initodom* h) {
  if (!h) return VXBA_ERR_ARG;
  IO_LOCK(h);
  h->M = 0;
  return VXBA_OK;
}

int64_t vxba_initodom_cloud_size(const vxba_initodom* h) { return h ? h->M : -1; }

int vxba_initodom_cloud(vxba_initodom* h, float* xyz) {
  if (!h || (h->M > 0 && !xyz)) return VXBA_ERR_ARG;
  IO_LOCK(h);
  if (h->M == 0) return VXBA_OK;
  VX_HIP(h, hipSetDevice(h->device));
  VX_HIP(h, hipMemcpyAsync(xyz, h->d_cloud[h->cur], (size_t)h->M * 3 * sizeof(float), hipMemcpyDeviceToHost, h->stream));
  VX_HIP(h, hipStreamSynchronize(h->stream));
  return VXBA_OK;
}

int vxba_initodom_search(vxba_initodom* h, int64_t n, const float* qry, int32_t* idx, float* sqd) {
  if (!h || n < 0 || (n > 0 && (!qry || !idx || !sqd))) return VXBA_ERR_ARG;
  if (n == 0) return VXBA_OK;
  IO_LOCK(h);
  if (n > (int64_t)0x7fffffff / vxin::NMATCH) return vxu::fail(h, VXBA_ERR_ARG, "vxba_initodom_search: too many queries");
  VX_HIP(h, hipSetDevice(h->device));
  float *d_q = nullptr, *d_s = nullptr; int* d_i = nullptr;
  VX_HIP(h, h->work.layout([&](vxu::Arena& a) { d_q = a.take<float>((size_t)n * 3); d_i = a.take<int>((size_t)n * vxin::NMATCH); d_s = a.take<float>((size_t)n * vxin::NMATCH); }, h->stream));
  hipError_t e = hipMemcpyAsync(d_q, qry, (size_t)n * 3 * sizeof(float), hipMemcpyHostToDevice, h->stream);
  if (e == hipSuccess) {
    vxin::init_search_kernel<<<(unsigned)((n + vxin::QPB - 1) / vxin::QPB), vxin::BLK, 0, h->stream>>>(h->d_cloud[h->cur], (int)h->M, d_q, n, d_i, d_s);
    e = hipGetLastError();
  }
  if (e == hipSuccess) e = hipMemcpyAsync(idx, d_i, (size_t)n * vxin::NMATCH * sizeof(int), hipMemcpyDeviceToHost, h->stream);
  if (e == hipSuccess) e = hipMemcpyAsync(sqd, d_s, (size_t)n * vxin::NMATCH * sizeof(float), hipMemcpyDeviceToHost, h->stream);
  const hipError_t e2 = hipStreamSynchronize(h->stream);      // also when something above failed: nothing of this call is in flight afterwards
  if (e == hipSuccess) e = e2;
  if (e != hipSuccess) { h->err = std::string("vxba_initodom_search: ") + hipGetErrorString(e); return VXBA_ERR_HIP; }
  return VXBA_OK;
}

int vxba_initodom_step(vxba_initodom* h, int64_t n, const double* pnt_body, double* state, double* cov, double* info, double* sweeps_out) {
  if (!h || n < 0 || !state || !cov || (n > 0 && !pnt_body)) return VXBA_ERR_ARG;
  IO_LOCK(h);
  if (h->M + n >= ((int64_t)1 << 31) / 4) return vxu::fail(h, VXBA_ERR_ARG, "vxba_initodom_step: cloud + scan beyond 2^29 points");
  for (int k = 0; k < VXBA_STATE_LEN; k++)
    if (!std::isfinite(state[k])) return vxu::fail(h, VXBA_ERR_ARG, "vxba_initodom_step: state is not finite");
  for (int64_t k = 0; k < 3 * n; k++)
    if (!std::isfinite(pnt_body[k])) return vxu::fail(h, VXBA_ERR_ARG, "vxba_initodom_step: a scan point is not finite");
  VX_HIP(h, hipSetDevice(h->device));
  h->launches = h->syncs = 0;
  if (info) std::memset(info, 0, sizeof(double) * VXBA_INITODOM_INFO_LEN);
  int rc = io_scan_reserve(h, n);
  if (rc != VXBA_OK) return rc;
  const bool seed = h->M < vxin::SEED_MIN;
  constexpr int D = 15;
  static thread_local vxl::LioCtl hc;
  std::memset(&hc, 0, sizeof hc);
  std::memcpy(hc.state, state, sizeof hc.state); std::memcpy(hc.x_prop, state, sizeof hc.x_prop);
  if (!seed) {
    double lu[D * D];
    int perm[D];
    if (!vxi::dm_inverse(D, cov, hc.cov_inv, lu, perm)) return vxu::fail(h, VXBA_ERR_ARG, "vxba_initodom_step: singular state covariance");
    for (int k = 0; k < D * D; k++) hc.cov_inv[k] = hc.cov_inv[k] / 1000;   // K_1 = (H_T_H + cov_inv / 1000)^-1
    std::memcpy(hc.cov, cov, sizeof hc.cov);
    hc.refind = 1;
  }
  rc = io_cloud_reserve(h, h->M + n);
  if (rc != VXBA_OK) return rc;
  if (n) VX_HIP(h, hipMemcpyAsync(h->d_pts(), pnt_body, (size_t)n * 3 * sizeof(double), hipMemcpyHostToDevice, h->stream));
  VX_HIP(h, hipMemcpyAsync(h->d_ctl, &hc, sizeof hc, hipMemcpyHostToDevice, h->stream));
  float* cloud = h->d_cloud[h->cur];
  const unsigned agrid = (unsigned)std::max<int64_t>(1, (n + 255) / 256);
  if (seed) {   // no filter in this branch, the state stays as it is
    if (n) {
      vxin::init_append_kernel<<<agrid, 256, 0, h->stream>>>(h->d_ctl, h->d_pts(), n, cloud + 3 * h->M);
      VX_HIP(h, hipGetLastError());
      h->launches += 1;
    }
    VX_HIP(h, vxwait::stream_wait(h->stream));
    h->syncs += 1;
    h->M += n;
    if (info) info[0] = 1.0;
    return VXBA_OK;
  }
  if (n) {
    const unsigned grid = (unsigned)std::min<int64_t>((n + vxin::QPB - 1) / vxin::QPB, vxin::MAX_GRID);
    for (int it = 0; it < VXBA_LIO_MAX_ITER; it++) {
      vxin::init_sweep_kernel<<<grid, vxin::BLK, 0, h->stream>>>(h->d_ctl, h->d_pts(), n, h->pts_cap(), cloud, (int)h->M, h->d_nn(), h->d_ok(), h->d_plane(), h->d_partials);
      VX_HIP(h, hipGetLastError());
      rc = vxba_internal_lio_ekf_init_launch((void*)h->stream, h->d_ctl, h->d_partials, (int)grid);
      if (rc != VXBA_OK) return vxu::fail(h, rc, "vxba_initodom_step: the EKF kernel did not launch");
      h->launches += 2;
    }
    vxin::init_append_kernel<<<agrid, 256, 0, h->stream>>>(h->d_ctl, h->d_pts(), n, cloud + 3 * h->M);
    VX_HIP(h, hipGetLastError());
    h->launches += 1;
    VX_HIP(h, hipMemcpyAsync(&hc, h->d_ctl, sizeof hc, hipMemcpyDeviceToHost, h->stream));
  }
  // down_sampling_voxel(*pl_tree, 0.5): waits (once) for the voxel count, and with it for everything above
  int64_t kept = 0;
  rc = vxd::downsample_device(h->ds, h->stream, cloud, h->M + n, 0.5, h->d_cloud[1 - h->cur], &kept);
  h->launches += 4; h->syncs += 1;
  if (rc != VXBA_OK) {
    hipStreamSynchronize(h->stream);
    h->M = 0;
    return vxu::fail(h, rc, "vxba_initodom_step: the voxel filter failed (a point beyond 2^20 voxels of the origin?); the cloud is cleared");
  }
  h->cur = 1 - h->cur; h->M = kept;
  if (n) {
    std::memcpy(state, hc.state, sizeof hc.state); std::memcpy(cov, hc.cov, sizeof hc.cov);
    const int iters = (int)hc.info[1];
    for (int k = 0; k < 4; k++) h->refound[k] = k < iters ? hc.refind_trace[k] : 0;
    if (info) {
      info[1] = iters; info[2] = hc.info[2]; info[3] = hc.rematch_num;
      for (int k = 0; k < 4; k++) info[4 + k] = h->refound[k];
    }
    if (sweeps_out) std::memcpy(sweeps_out, hc.sweeps, sizeof(double) * vxl::SWEEP_OUT * iters);
  }
  return VXBA_OK;
}

int vxba_initodom_inspect(vxba_initodom* h, int iteration, int32_t* nn, int32_t* ok, double* plane) {
  if (!h || iteration < 0 || iteration >= VXBA_LIO_MAX_ITER || !nn || !ok || !plane) return VXBA_ERR_ARG;
  IO_LOCK(h);
  if (!h->refound[iteration]) return vxu::fail(h, VXBA_ERR_STATE, "vxba_initodom_inspect: the last step did not search in this iteration");
  VX_HIP(h, hipSetDevice(h->device));
  const int64_t n = h->n_pts, off = (int64_t)iteration * h->pts_cap();
  VX_HIP(h, hipMemcpyAsync(nn, h->d_nn() + vxin::NMATCH * off, (size_t)n * vxin::NMATCH * sizeof(int), hipMemcpyDeviceToHost, h->stream));
  VX_HIP(h, hipMemcpyAsync(ok, h->d_ok() + off, (size_t)n * sizeof(int), hipMemcpyDeviceToHost, h->stream));
  VX_HIP(h, hipMemcpyAsync(plane, h->d_plane() + 4 * off, (size_t)n * 4 * sizeof(double), hipMemcpyDeviceToHost, h->stream));
  VX_HIP(h, hipStreamSynchronize(h->stream));
  return VXBA_OK;
}

int vxba_initodom_stats(const vxba_initodom* h, int64_t out[4]) {
  if (!h || !out) return VXBA_ERR_ARG;
  out[0] = h->launches; out[1] = h->syncs; out[2] = h->M; out[3] = h->n_pts;
  return VXBA_OK;
}

// ---- motion_init's pieces ------------------------------------------------------------------------------------------------------------
int vxba_init_pose_table(int K, const double* stamps, const double* gyr, const double* acc, double beg_time, const double* xc, const double* bias_from, double scale,
                         double* table) {
  if (K < 1 || !stamps || !gyr || !acc || !xc || !bias_from || (K > 1 && !table)) return VXBA_ERR_ARG;
  double R[9], p[3], v[3];
  std::memcpy(R, xc, sizeof R); std::memcpy(p, xc + 9, sizeof p); std::memcpy(v, xc + 12, sizeof v);
  const double *bg = bias_from + 15, *ba = bias_from + 18, *g = xc + 21;
  for (int t = K - 1, e = 0; t >= 1; t--, e++) {     // tail = message t, head = message t - 1
    double rate[3], a[3], acc_imu[3];
    vxin::midpoint_sample(gyr + 3 * (t - 1), gyr + 3 * t, acc + 3 * (t - 1), acc + 3 * t, bg, ba, scale, rate, a);
    vxin::pose_step(R, p, v, rate, a, g, stamps[t - 1] - stamps[t], acc_imu);
    double* o = table + (size_t)vxin::POSE_LEN * e;
    o[0] = stamps[t - 1] - beg_time;
    std::memcpy(o + 1, R, sizeof R); std::memcpy(o + 10, p, sizeof p); std::memcpy(o + 13, v, sizeof v); std::memcpy(o + 16, rate, sizeof rate); std::memcpy(o + 19, acc_imu, sizeof acc_imu);
  }
  return VXBA_OK;
}

int vxba_init_deskew(int device, int64_t n, const float* xyz, const float* toff, int K, const double* stamps, const double* gyr, const double* acc, double beg_time,
                     const double* xc, const double* bias_from, const double* ext, double scale, int point_notime, int64_t capacity, double* out, int32_t* src_out,
                     int64_t* n_out) {
  if (n < 0 || !n_out || !xc || !ext || (n > 0 && (!xyz || !out)) || n >= ((int64_t)1 << 30) || K < 0 || K > (1 << 20)) return VXBA_ERR_ARG;
  *n_out = 0;
  if (!point_notime && (K < 1 || !toff || !stamps || !gyr || !acc || !bias_from)) return VXBA_ERR_ARG;
  if (n == 0) return VXBA_OK;
  // upstream's walk (:534-560), on the host: it knows the times and the table's offsets, so every output slot and its pose are fixed before the launch
  std::vector<int> src, head;
  std::vector<double> table;
  if (point_notime) {
    src.resize(n); head.assign(n, -1);
    for (int64_t i = 0; i < n; i++) src[i] = (int)i;
  } else {
    table.resize((size_t)vxin::POSE_LEN * std::max(K - 1, 1));
    int rc = vxba_init_pose_table(K, stamps, gyr, acc, beg_time, xc, bias_from, scale, table.data());
    if (rc != VXBA_OK) return rc;
    int64_t it = n - 1;
    for (int k = 0; k < K - 1; k++) {
      const double offt = table[(size_t)vxin::POSE_LEN * k];
      for (; (double)toff[it] > offt; it--) {
        src.push_back((int)it); head.push_back(k);
        if (it == 0) break;                          // leaves the inner loop only: the first point comes again under every earlier head that it is later than
      }
    }
  }
  const int64_t m = (int64_t)src.size();
  *n_out = m;
  if (m > capacity) return VXBA_ERR_ARG;
  if (src_out) std::memcpy(src_out, src.data(), (size_t)m * sizeof(int));
  if (m == 0) return VXBA_OK;
  if (const int rc = vxu::select_device(device)) return rc;
  vxu::Lease lease(device);
  float *d_xyz = nullptr, *d_t = nullptr; int *d_src = nullptr, *d_head = nullptr; double *d_tab = nullptr, *d_x = nullptr, *d_o = nullptr;
  VX_HIP_RC(lease.layout([&](vxu::Arena& a) {
    d_xyz = a.take<float>((size_t)n * 3); d_t = a.take<float>((size_t)n); d_src = a.take<int>((size_t)m); d_head = a.take<int>((size_t)m);
    d_tab = a.take<double>(std::max<size_t>(table.size(), 1)); d_x = a.take<double>(24); d_o = a.take<double>((size_t)m * 3);
  }));
  double xe[24];
  std::memcpy(xe, xc, 12 * sizeof(double)); std::memcpy(xe + 12, ext, 12 * sizeof(double));
  hipError_t e = hipMemcpy(d_xyz, xyz, (size_t)n * 12, hipMemcpyHostToDevice);
  if (e == hipSuccess && !point_notime) e = hipMemcpy(d_t, toff, (size_t)n * 4, hipMemcpyHostToDevice);
  if (e == hipSuccess) e = hipMemcpy(d_src, src.data(), (size_t)m * 4, hipMemcpyHostToDevice);
  if (e == hipSuccess) e = hipMemcpy(d_head, head.data(), (size_t)m * 4, hipMemcpyHostToDevice);
  if (e == hipSuccess && !table.empty()) e = hipMemcpy(d_tab, table.data(), table.size() * 8, hipMemcpyHostToDevice);
  if (e == hipSuccess) e = hipMemcpy(d_x, xe, sizeof xe, hipMemcpyHostToDevice);
  if (e == hipSuccess) {
    vxin::init_deskew_kernel<<<(unsigned)((m + 255) / 256), 256>>>(d_xyz, d_t, d_src, d_head, m, d_tab, d_x, d_o);
    e = hipGetLastError();
  }
  if (e == hipSuccess) e = hipMemcpy(out, d_o, (size_t)m * 24, hipMemcpyDeviceToHost);
  return e == hipSuccess ? VXBA_OK : VXBA_ERR_HIP;
}

int vxba_init_normal_scatter(vxba_factor* f, double* nnt9) {
  if (!f || !nnt9) return VXBA_ERR_ARG;
  const double *ev = nullptr, *U = nullptr, *mg = nullptr;
  int VS = 0, V = 0;
  int rc = vxba_internal_cache_view(f, &ev, &U, &mg, &VS, &V);
  if (rc != VXBA_OK) return rc;
  if (V > 0 && !U) return VXBA_ERR_STATE;
  const int device = vxba_internal_factor_device(f);
  if (hipSetDevice(device) != hipSuccess) return VXBA_ERR_HIP;
  vxu::Lease lease(device);
  double* d6 = nullptr;
  VX_HIP_RC(lease.layout([&](vxu::Arena& a) { d6 = a.take<double>(6); }));
  vxin::init_scatter_kernel<<<1, 256>>>(U, VS, V, d6);
  double s[6];
  hipError_t e = hipGetLastError();
  if (e == hipSuccess) e = hipMemcpy(s, d6, sizeof s, hipMemcpyDeviceToHost);
  if (e != hipSuccess) return VXBA_ERR_HIP;
  nnt9[0] = s[0]; nnt9[1] = s[1]; nnt9[2] = s[2]; nnt9[3] = s[1]; nnt9[4] = s[3]; nnt9[5] = s[4]; nnt9[6] = s[2]; nnt9[7] = s[4]; nnt9[8] = s[5];
  return VXBA_OK;
}

int vxba_imu_push(double* imu, int K, const double* stamps, const double* gyr, const double* acc, double scale, const double* noise_meas, const double* noise_walk) {
  if (!imu || K < 0 || (K > 0 && (!stamps || !gyr || !acc)) || !noise_meas || !noise_walk) return VXBA_ERR_ARG;
  for (int t = 1; t < K; t++) {
    double rate[3], a[3];
    vxin::midpoint_sample(gyr + 3 * (t - 1), gyr + 3 * t, acc + 3 * (t - 1), acc + 3 * t, imu + vxi::O_BG, imu + vxi::O_BA, scale, rate, a);
    vxi::imu_add(imu, rate, a, stamps[t] - stamps[t - 1], noise_meas, noise_walk);
  }
  return VXBA_OK;
}

static thread_local double g_motion_us[4] = {0, 0, 0, 0};   // de-skew | map build (variances, cut, recut) | LM | re-preintegration (+ scatter) of the last call

int vxba_init_motion_times(double out_us[4]) {
  if (!out_us) return VXBA_ERR_ARG;
  std::memcpy(out_us, g_motion_us, sizeof g_motion_us);
  return VXBA_OK;
}

// Initialization::motion_init (voxelslam.cpp:563-713): the rounds, the convergence rule, align_gravity, the switch of plane thresholds, the three exits.
// Host shell over the entry points of this library; per scan and round one de-skew launch, one variance / world-point launch and the map's cut.
int vxba_init_motion(vxba_map* m, vxba_factor* f, int win_size, const int64_t* scan_ptr, const float* xyz, const float* toff, const double* beg_times,
                     const int64_t* imu_ptr, const double* stamps, const double* gyr, const double* acc, double* states, const double* covs, const double* ext,
                     const vxba_init_motion_params* prm, double* imus, double* hess_out, double* report, double* traces, int* n_rounds, double* eigvalue, int* flag) {
  if (!m || !f || win_size < 2 || win_size > VXBA_MAX_WIN || !scan_ptr || !xyz || !beg_times || !imu_ptr || !stamps || !gyr || !acc || !states || !covs || !ext || !prm ||
      !imus || !hess_out || !report || !n_rounds || !eigvalue || !flag || (!prm->point_notime && !toff))
    return VXBA_ERR_ARG;
  const int W = win_size;
  if (scan_ptr[0] != 0 || imu_ptr[0] != 0) return VXBA_ERR_ARG;
  int64_t n_max = 0;
  for (int i = 0; i < W; i++) {
    if (scan_ptr[i + 1] < scan_ptr[i] || imu_ptr[i + 1] < imu_ptr[i] || imu_ptr[i + 1] - imu_ptr[i] > (1 << 20)) return VXBA_ERR_ARG;
    n_max = std::max(n_max, scan_ptr[i + 1] - scan_ptr[i] + (imu_ptr[i + 1] - imu_ptr[i]) + 1);
  }
  *n_rounds = 0; *flag = 0;
  eigvalue[0] = eigvalue[1] = eigvalue[2] = 0.0;
  std::memset(report, 0, sizeof(double) * VXBA_INIT_MAX_ROUNDS * VXBA_INIT_REPORT_LEN);
  if (traces) std::memset(traces, 0, sizeof(double) * VXBA_INIT_MAX_ROUNDS * 3 * VXBA_TRACE_COLS);
  const int device = vxba_internal_factor_device(f);
  if (hipSetDevice(device) != hipSuccess) return VXBA_ERR_HIP;
  const double first_thre[4] = {0.25, 0.25, 0.25, 0.25};
  const float range_inc = (float)prm->dept_err, degree_inc = (float)prm->beam_err;
  const double dir_var = std::pow(std::sin((degree_inc) * 0.017453293), 2);   // pow(sin(DEG2RAD(degree_inc)), 2), PCL's DEG2RAD
  std::vector<double> body((size_t)n_max * 3), Rp((size_t)W * 12);
  // body 3 | var 9 | world 3 per point.  An owner of its own and no lease: it is held across vxba_init_deskew and vxba_init_normal_scatter, which take one
  vxu::Dev<double> d_buf;
  VX_HIP_RC(d_buf.reserve((size_t)n_max * 15));
  int rc = VXBA_OK, converge_flag = 0;
  double converge_thre = 0.05;
  using clk = std::chrono::steady_clock;
  auto since = [](clk::time_point t) { return std::chrono::duration<double, std::micro>(clk::now() - t).count(); };
  for (double& t : g_motion_us) t = 0;
  bool is_degrade = true;
  for (int iter = 0; iter < VXBA_INIT_MAX_ROUNDS && rc == VXBA_OK; iter++) {
    double* rep = report + (size_t)VXBA_INIT_REPORT_LEN * iter;
    *n_rounds = iter + 1;
    rep[7] = converge_flag; rep[10] = converge_thre;
    if ((rc = vxba_map_clear(m))) break;
    if ((rc = converge_flag ? vxba_map_set_plane_thresholds(m, prm->min_eigen_value, prm->plane_eigen_value_thre) : vxba_map_set_plane_thresholds(m, 0.02, first_thre))) break;
    for (int i = 0; i < W && rc == VXBA_OK; i++) {
      const int64_t n = scan_ptr[i + 1] - scan_ptr[i], k0 = imu_ptr[i];
      const int K = (int)(imu_ptr[i + 1] - k0), l = i == 0 ? 0 : i - 1;
      const double* xc = states + (size_t)VXBA_STATE_LEN * i;
      int64_t mo = 0;
      clk::time_point t0 = clk::now();
      rc = vxba_init_deskew(device, n, xyz + 3 * scan_ptr[i], toff ? toff + scan_ptr[i] : nullptr, K, stamps + k0, gyr + 3 * k0, acc + 3 * k0, beg_times[i], xc,
                            states + (size_t)VXBA_STATE_LEN * l, ext, prm->imupre_scale_gravity, prm->point_notime, n_max, body.data(), nullptr, &mo);
      g_motion_us[0] += since(t0);
      if (rc != VXBA_OK || mo == 0) continue;
      t0 = clk::now();
      vxin::PointVarArg a;
      std::memcpy(a.R, xc, sizeof a.R); std::memcpy(a.p, xc + 9, sizeof a.p);
      const double* cv = covs + (size_t)225 * i;
      for (int c = 0; c < 3; c++)
        for (int r = 0; r < 3; r++) { a.rot_var[3 * c + r] = cv[15 * c + r]; a.tsl_var[3 * c + r] = cv[15 * (3 + c) + 3 + r]; }
      a.range_inc = range_inc; a.dir_var = dir_var; a.with_var = converge_flag;
      hipError_t e = hipMemcpy(d_buf, body.data(), (size_t)mo * 3 * sizeof(double), hipMemcpyHostToDevice);
      if (e == hipSuccess) {
        vxin::init_pointvar_kernel<<<(unsigned)((mo + 255) / 256), 256>>>(d_buf, mo, a, d_buf + 3 * (size_t)n_max, d_buf + 12 * (size_t)n_max);
        e = hipGetLastError();
      }
      if (e == hipSuccess) e = hipStreamSynchronize(nullptr);
      if (e != hipSuccess) { rc = VXBA_ERR_HIP; break; }
      rc = vxba_map_cut_voxel_device(m, i, mo, d_buf, d_buf + 3 * (size_t)n_max, d_buf + 12 * (size_t)n_max);
      if (rc == VXBA_OK && hipDeviceSynchronize() != hipSuccess) rc = VXBA_ERR_HIP;   // the buffer is written again for the next scan
      g_motion_us[1] += since(t0);
    }
    if (rc != VXBA_OK) break;
    clk::time_point t0 = clk::now();
    if ((rc = vxba_clear(f))) break;
    for (int i = 0; i < W; i++) std::memcpy(&Rp[12 * (size_t)i], states + (size_t)VXBA_STATE_LEN * i, 12 * sizeof(double));
    int64_t nv = 0;
    if ((rc = vxba_map_recut(m, W, Rp.data(), f, &nv))) break;
    rep[0] = (double)nv;
    g_motion_us[1] += since(t0);
    if (nv < 10) break;                                                          // `if(voxhess.plvec_voxels.size() < 10) break;`
    double resis[2] = {0, 0}, tr[3 * VXBA_TRACE_COLS] = {0};
    int nt = 0;
    t0 = clk::now();
    if ((rc = vxba_li_damping_iter_gravity(f, states, imus, prm->imu_coef, 3, hess_out, resis, tr, &nt))) break;
    g_motion_us[2] += since(t0);
    t0 = clk::now();
    if (traces) std::memcpy(traces + (size_t)iter * 3 * VXBA_TRACE_COLS, tr, sizeof tr);
    rep[1] = resis[0]; rep[2] = resis[1]; rep[3] = states[21]; rep[4] = states[22]; rep[5] = states[23]; rep[8] = nt; rep[9] = 1.0;
    const double ratio = std::fabs(resis[0] - resis[1]) / resis[0];
    rep[6] = ratio;
    for (int i = 1; i < W && rc == VXBA_OK; i++) {                               // new factors at the new biases
      double* blob = imus + (size_t)VXBA_IMU_LEN * (i - 1);
      const double* xl = states + (size_t)VXBA_STATE_LEN * (i - 1);
      rc = vxba_imu_init(blob, xl + 15, xl + 18);
      if (rc == VXBA_OK)
        rc = vxba_imu_push(blob, (int)(imu_ptr[i + 1] - imu_ptr[i]), stamps + imu_ptr[i], gyr + 3 * imu_ptr[i], acc + 3 * imu_ptr[i], prm->imupre_scale_gravity,
                           prm->noise_meas, prm->noise_walk);
    }
    if (rc != VXBA_OK) break;
    g_motion_us[3] += since(t0);
    if (ratio < converge_thre && iter >= 2) {
      double nnt[9], lam[3], U[9];
      if ((rc = vxba_init_normal_scatter(f, nnt))) break;
      const double c6[6] = {nnt[0], nnt[3], nnt[6], nnt[4], nnt[7], nnt[8]};
      vxm::eig_sym3(c6, lam, U);
      eigvalue[0] = lam[0]; eigvalue[1] = lam[1]; eigvalue[2] = lam[2];
      is_degrade = lam[0] < 15;
      converge_thre = 0.01;
      rep[11] = 1.0;
      if (converge_flag == 0) {
        vxin::align_gravity(states, W);
        converge_flag = 1;
        continue;
      }
      break;
    }
  }
  if (rc != VXBA_OK) return rc;
  const double* g = states + (size_t)VXBA_STATE_LEN * (W - 1) + 21;
  const double gnm = std::sqrt((g[0] * g[0] + g[1] * g[1]) + g[2] * g[2]);
  if (is_degrade || gnm < 9.6 || gnm > 10.0) converge_flag = 0;
  if (converge_flag == 0) {                                                      // upstream tears the map down; the factor goes with it here
    if ((rc = vxba_map_clear(m))) return rc;
    if ((rc = vxba_map_set_plane_thresholds(m, prm->min_eigen_value, prm->plane_eigen_value_thre))) return rc;
    if ((rc = vxba_clear(f))) return rc;
  }
  *flag = converge_flag;
  return VXBA_OK;
}

}  // extern "C"
