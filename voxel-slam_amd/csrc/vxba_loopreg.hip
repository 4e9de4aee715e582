// Loop-edge registration below the C ABI (include/vxba.h: vxba_loopreg_*): plane clouds, the verify score and the normal-gated ICP.
//
// Reference: STDescManager::init_voxel_map / BTCOctoTree::init_plane / get_plane (BTC.cpp:96-139, 279-338: a keyframe cloud -> one (centre,
// normal) per voxel that holds a plane), STDescManager::plane_geometric_verify (BTC.cpp:1422-1479: the score of a candidate) and icp_normal
// (loop_refine.hpp:47-145).  All three sit on one primitive: transform a source plane cloud by a pose hypothesis, find the nearest target
// centre of every source point, gate the pair (vxba_loopreg_math.hpp).
//
// Launch plan:
//   associate_kernel<MODE>  sixteen lanes per source point, sixteen source points per workgroup, grid (source blocks, pairs).  The target cloud
//                           passes through LDS in tiles of 1024 centres; lane j of a point's group scans the centres j, j + 16, ... in ascending
//                           index with a strict <, the group keeps the smaller distance and of equal ones the lower index: the nearest
//                           neighbour is exact in float32 and ties go to the lowest index.  MODE picks the consumer: per-point output (inspection), an integer count per pair
//                           (score), or the 35 sums of an ICP iteration reduced wave -> workgroup -> one partial row per workgroup.
//   icp_step_kernel         one wave per pair: the partial rows summed in a fixed order, the 6 x 6 solve, the pose update, the state machine,
//                           and -- for the pair that stops -- the eigenvalues of sum n_t n_t^T and the report row.
// vxba_loopreg_icp enqueues max_iter rounds of the two and synchronises once; the workgroups of a finished pair return at their first
// instruction.  No floating-point atomics: two runs give identical bits, and a pair's result does not depend on the batch around it (its
// partial rows are per block of sixteen source points, whatever the grid).
//   keyframe -> plane cloud: (widen_kernel for a float32 cloud already on the device,) key_kernel (voxel key per point), rocPRIM radix sort of (key, index), plane_kernel (the first point of every
//   voxel sums its run in input order, eigen-decomposition, plane test), rocPRIM scan + scatter of the plane rows in key order.
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdint>
#include <cstring>
#include <limits>
#include <string>
#include <vector>

#include "../../include/vxba.h"
#include "vxba_dev.hpp"
#include "vxba_loopreg_internal.hpp"
#include "vxba_loopreg_math.hpp"
#include "vxba_math.hpp"

namespace vxlr {

constexpr int BLK = 256;               // lanes per workgroup
constexpr int TS = 16;                 // lanes that share the target scan of one source point
constexpr int SPB = BLK / TS;          // source points per workgroup
constexpr int WAVES = BLK / 64;
constexpr int TILE = 1024;             // target centres per LDS tile: 16 KiB
constexpr int REPORT_LEN = VXBA_ICP_REPORT_LEN;
constexpr int KEY_BITS = 21, KEY_OFF = 1 << 20;

enum Mode { MODE_INSPECT = 0, MODE_SCORE = 1, MODE_ICP = 2 };

struct PairState {
  double pose[12];
  double norm[6];       // sum n_t n_t^T of the last iteration (upper triangle)
  double resi, match;   // of the last iteration
  IcpState st;
};

struct Args {
  const PairDesc* pairs;
  const double* poses;       // B x 12 (inspect, score)
  PairState* state;          // B (icp)
  double g0[4], g1[4];       // gates: g0 everywhere; the icp takes g1 once is_converge is set
  int32_t* nn;               // inspect: S
  uint8_t* matched;          // inspect: S
  int* useful;               // score: B
  double* partial;           // icp: B x nblk x ACC_LEN
  int nblk;                  // partial rows reserved per pair
  double* report;            // icp: B x REPORT_LEN
  double step_tol, icp_eigval;
  int max_iter;
};

// nearest target centre of (qx, qy, qz) in float32: squared distance (dx dx + dy dy) + dz dz without contraction.  The TS lanes of a source
// point share the work: lane j of the group takes the targets j, j + TS, ... of every tile in ascending order with a strict <, so it holds the
// lowest index among the nearest of ITS targets; the group then keeps the smaller distance and, of equal distances, the lower index -- the
// same answer as one ascending scan with a strict <.  Every lane of the workgroup takes part (the tile loads and the barriers are the workgroup's).
__device__ __forceinline__ int nearest(const float* __restrict__ tar, int T, float qx, float qy, float qz, float4* tile) {
  float best = std::numeric_limits<float>::infinity();
  int bi = 0x7fffffff;
  const int j = threadIdx.x & (TS - 1);
  for (int t0 = 0; t0 < T; t0 += TILE) {
    __syncthreads();                                     // the previous tile has been read by every lane
    const int m = min(TILE, T - t0);
    for (int k = threadIdx.x; k < m; k += BLK) {
      const float* c = tar + 6 * (size_t)(t0 + k);
      tile[k] = make_float4(c[0], c[1], c[2], 0.f);
    }
    __syncthreads();
#pragma unroll 4
    for (int k = j; k < m; k += TS) {
      const float4 c = tile[k];
      const float dx = __fsub_rn(c.x, qx), dy = __fsub_rn(c.y, qy), dz = __fsub_rn(c.z, qz);
      const float d = __fadd_rn(__fadd_rn(__fmul_rn(dx, dx), __fmul_rn(dy, dy)), __fmul_rn(dz, dz));
      if (d < best) { best = d; bi = t0 + k; }
    }
  }
#pragma unroll
  for (int off = TS / 2; off >= 1; off >>= 1) {          // the group's lanes are neighbours inside one wave
    const float ob = __shfl_xor(best, off, 64);
    const int oi = __shfl_xor(bi, off, 64);
    if (ob < best || (ob == best && oi < bi)) { best = ob; bi = oi; }
  }
  return bi == 0x7fffffff ? 0 : bi;                      // no target compared below (a distance that is not a number): index 0, as one scan gives
}

template <int MODE>
__global__ void __launch_bounds__(BLK) associate_kernel(Args a) {
  __shared__ float4 tile[TILE];
  __shared__ double s_red[MODE == MODE_ICP ? WAVES * ACC_LEN : 1];
  __shared__ int s_cnt[WAVES];
  const int b = blockIdx.y;
  if (MODE == MODE_ICP && a.state[b].st.done) return;    // uniform: written by the previous launch only
  const PairDesc pd = a.pairs[b];
  const int s0 = blockIdx.x * SPB;
  if (s0 >= pd.S) return;
  const int s = s0 + threadIdx.x / TS;
  const bool live = s < pd.S;
  const bool lead = (threadIdx.x & (TS - 1)) == 0;         // the lane of the group that gates, counts and accumulates
  double P[12];
  const double* Pin = MODE == MODE_ICP ? a.state[b].pose : a.poses + 12 * (size_t)b;
#pragma unroll
  for (int k = 0; k < 12; k++) P[k] = Pin[k];
  double g[4];
  const bool tight = MODE == MODE_ICP && a.state[b].st.is_converge;
#pragma unroll
  for (int k = 0; k < 4; k++) g[k] = tight ? a.g1[k] : a.g0[k];

  float sp[6] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
  if (live) {
#pragma unroll
    for (int k = 0; k < 6; k++) sp[k] = pd.src[6 * (size_t)s + k];
  }
  double p[3], n[3];
  transform_plane(P, sp, p, n);
  const int bi = nearest(pd.tar, pd.T, (float)p[0], (float)p[1], (float)p[2], tile);
  bool ok = false;
  double rr = 0.0;
  float tp[6] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
  if (live && lead && pd.T > 0) {
#pragma unroll
    for (int k = 0; k < 6; k++) tp[k] = pd.tar[6 * (size_t)bi + k];
    ok = gate(p, n, tp, g, rr);
  }
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  if (MODE == MODE_INSPECT) {
    if (live && lead) { a.nn[s] = pd.T > 0 ? bi : -1; a.matched[s] = ok ? 1 : 0; }
  } else if (MODE == MODE_SCORE) {
    const int c = __popcll(__ballot(ok));
    if (lane == 0) s_cnt[wave] = c;
    __syncthreads();
    if (threadIdx.x == 0) {
      int t = 0;
#pragma unroll
      for (int w = 0; w < WAVES; w++) t += s_cnt[w];
      if (t) atomicAdd(a.useful + b, t);                 // integers: any order gives the same sum
    }
  } else {
    double acc[ACC_LEN];
#pragma unroll
    for (int k = 0; k < ACC_LEN; k++) acc[k] = 0.0;
    if (ok) {
      double jac[6];
      jac_row(P, sp, tp, jac);
      accumulate(jac, tp, rr, acc);
    }
#pragma unroll
    for (int k = 0; k < ACC_LEN; k++) {
      double v = acc[k];
#pragma unroll
      for (int off = 32; off >= 1; off >>= 1) v += __shfl_xor(v, off, 64);
      if (lane == 0) s_red[wave * ACC_LEN + k] = v;
    }
    __syncthreads();
    if (threadIdx.x < ACC_LEN) {
      double v = 0.0;
#pragma unroll
      for (int w = 0; w < WAVES; w++) v += s_red[w * ACC_LEN + threadIdx.x];
      a.partial[((size_t)b * a.nblk + blockIdx.x) * ACC_LEN + threadIdx.x] = v;
    }
  }
}

// one wave per pair
__global__ void __launch_bounds__(64) icp_step_kernel(Args a) {
  const int b = blockIdx.x, lane = threadIdx.x;
  PairState* ps = a.state + b;
  IcpState st;
  st.iter = ps->st.iter; st.done = ps->st.done; st.is_converge = ps->st.is_converge; st.failed = ps->st.failed;
  if (st.done) return;
  const int S = a.pairs[b].S;
  const int nb = (S + SPB - 1) / SPB;
  double acc[ACC_LEN];
#pragma unroll
  for (int k = 0; k < ACC_LEN; k++) acc[k] = 0.0;
  for (int r = lane; r < nb; r += 64) {                  // rows lane, lane + 64, ...: a fixed order for a given S
    const double* row = a.partial + ((size_t)b * a.nblk + r) * ACC_LEN;
#pragma unroll
    for (int k = 0; k < ACC_LEN; k++) acc[k] += row[k];
  }
#pragma unroll
  for (int k = 0; k < ACC_LEN; k++) {
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) acc[k] += __shfl_xor(acc[k], off, 64);
  }
  // every lane holds the same sums from here on and computes the same bits; lane 0 writes
  double P[12], dx[6], Pn[12];
#pragma unroll
  for (int k = 0; k < 12; k++) P[k] = ps->pose[k];
  solve6(acc, acc + ACC_JACT, dx);
  const bool apply = icp_advance(st, acc[ACC_COUNT], dx, a.step_tol, a.max_iter);
  if (apply) retract(P, dx, Pn);
  else {
#pragma unroll
    for (int k = 0; k < 12; k++) Pn[k] = P[k];
  }
  if (lane == 0) {
#pragma unroll
    for (int k = 0; k < 12; k++) ps->pose[k] = Pn[k];
#pragma unroll
    for (int k = 0; k < 6; k++) ps->norm[k] = acc[ACC_NORM + k];
    ps->resi = acc[ACC_RESI]; ps->match = acc[ACC_COUNT];
    ps->st.iter = st.iter; ps->st.done = st.done; ps->st.is_converge = st.is_converge; ps->st.failed = st.failed;
  }
  if (st.done) {
    double lam[3], U[9];
    vxm::eig_sym3(acc + ACC_NORM, lam, U);
    const bool accept = lam[0] > a.icp_eigval && st.is_converge == 1 && !st.failed;
    if (lane == 0) {
      double* rep = a.report + REPORT_LEN * (size_t)b;
      rep[0] = accept ? 1.0 : 0.0; rep[1] = (double)st.is_converge; rep[2] = (double)st.iter; rep[3] = acc[ACC_COUNT];
      rep[4] = lam[0]; rep[5] = lam[1]; rep[6] = lam[2]; rep[7] = acc[ACC_RESI];
    }
  }
}

// ---- keyframe -> plane cloud -------------------------------------------------------------------------------------------------------
// the float32 cloud of vxba_loopreg_add_keyframe_device as the float64 the kernels below read (exact)
__global__ void __launch_bounds__(256) widen_kernel(const float* __restrict__ src, long long n3, double* __restrict__ dst) {
  const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
  if (i < n3) dst[i] = (double)src[i];
}

__global__ void __launch_bounds__(256) key_kernel(const double* __restrict__ xyz, long long n, double voxel_size, unsigned long long* __restrict__ key,
                                                 unsigned int* __restrict__ idx, int* __restrict__ err) {
  const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
  if (i >= n) return;
  unsigned long long k = 0;
  bool bad = false;
#pragma unroll
  for (int c = 0; c < 3; c++) {
    const double v = xyz[3 * i + c];
    long long l = 0;
    if (fabs(v / voxel_size) < (double)(KEY_OFF - 2)) l = voxel_coord(v, voxel_size);    // false for values that are not finite, too
    else bad = true;
    k = (k << KEY_BITS) | (unsigned long long)(l + KEY_OFF);
  }
  if (bad) *err = 1;                                     // every writer stores the same value
  key[i] = k;
  idx[i] = (unsigned int)i;
}

// the first point of every run of equal keys sums the run in input order (the sort is stable) and decides; one row and one flag per point slot
__global__ void __launch_bounds__(256) plane_kernel(const double* __restrict__ xyz, const unsigned long long* __restrict__ key, const unsigned int* __restrict__ idx,
                                                   long long n, int voxel_init_num, double thre, float* __restrict__ rows, unsigned int* __restrict__ flag) {
  const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
  if (i >= n) return;
  const unsigned long long k = key[i];
  unsigned int f = 0;
  if (i == 0 || key[i - 1] != k) {
    double P[6] = {0, 0, 0, 0, 0, 0}, v[3] = {0, 0, 0};
    long long j = i;
    for (; j < n && key[j] == k; j++) {
      const double* q = xyz + 3 * (size_t)idx[j];
      const double x = q[0], y = q[1], z = q[2];
      P[0] += x * x; P[1] += x * y; P[2] += x * z; P[3] += y * y; P[4] += y * z; P[5] += z * z;
      v[0] += x; v[1] += y; v[2] += z;
    }
    const long long N = j - i;
    if (N > voxel_init_num) {
      const double Nd = (double)N;
      const double c[3] = {v[0] / Nd, v[1] / Nd, v[2] / Nd};
      const double C[6] = {P[0] / Nd - c[0] * c[0], P[1] / Nd - c[0] * c[1], P[2] / Nd - c[0] * c[2], P[3] / Nd - c[1] * c[1], P[4] / Nd - c[1] * c[2], P[5] / Nd - c[2] * c[2]};
      double lam[3], U[9];
      vxm::eig_sym3(C, lam, U);
      if (lam[0] < thre) {
        double nx = U[0], ny = U[3], nz = U[6];
        // the sign: the component of largest magnitude (the first of equals) is positive
        const double ax = fabs(nx), ay = fabs(ny), az = fabs(nz);
        const double lead = (ax >= ay && ax >= az) ? nx : (ay >= az ? ny : nz);
        if (lead < 0) { nx = -nx; ny = -ny; nz = -nz; }
        float* r = rows + 6 * (size_t)i;
        r[0] = (float)c[0]; r[1] = (float)c[1]; r[2] = (float)c[2]; r[3] = (float)nx; r[4] = (float)ny; r[5] = (float)nz;
        f = 1;
      }
    }
  }
  flag[i] = f;
}

__global__ void __launch_bounds__(256) scatter_kernel(const float* __restrict__ rows, const unsigned int* __restrict__ flag, const unsigned int* __restrict__ pos, long long n,
                                                     float* __restrict__ out, unsigned int* __restrict__ total) {
  const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
  if (i >= n) return;
  if (flag[i]) {
#pragma unroll
    for (int k = 0; k < 6; k++) out[6 * (size_t)pos[i] + k] = rows[6 * (size_t)i + k];
  }
  if (i == n - 1) *total = pos[i] + flag[i];
}

}  // namespace vxlr

// ---- host ------------------------------------------------------------------------------------------------------------------------
struct vxba_loopreg {
  int device = 0;
  std::string err;
  vxu::Stream s;
  struct Cloud { vxu::Dev<float> d; int n = 0; };
  std::vector<Cloud> clouds;
  // batch buffers, grown on demand
  vxu::Dev<vxlr::PairDesc> d_pairs; vxu::Dev<double> d_poses; vxu::Dev<vxlr::PairState> d_state; vxu::Dev<int> d_useful; vxu::Dev<double> d_report;
  vxu::Dev<double> d_partial;
  vxu::Dev<int32_t> d_nn; vxu::Dev<uint8_t> d_matched;
  vxu::Arena work;                                 // the temporaries of add_keyframe: kept across vxba_loopreg_clear
  int64_t launches = 0, syncs = 0, last_B = 0;     // of the last score / icp / associate call
  unsigned long long generation = 0;               // counts vxba_loopreg_clear: device pointers handed out before it are dead (vxba_loopsearch holds some)
};

namespace vxlr {

using vxu::blocks_for, vxu::fail;

static int new_cloud(vxba_loopreg* h, int n, const float* d_rows /* device, may be null when n == 0 */, int* id) {
  vxba_loopreg::Cloud c;
  c.n = n;
  VX_HIP(h, c.d.reserve((size_t)(n ? n : 1) * 6));
  if (n) VX_HIP(h, hipMemcpyAsync(c.d, d_rows, (size_t)n * 6 * sizeof(float), hipMemcpyDeviceToDevice, h->s));
  h->clouds.push_back(std::move(c));
  *id = (int)h->clouds.size() - 1;
  return VXBA_OK;
}

// the pairs of a batch checked and on the device; returns the largest source size through max_s
static int stage_pairs(vxba_loopreg* h, const char* what, int B, const int32_t* src_tar, const double* poses, int* max_s) {
  if (B <= 0 || !src_tar || !poses) return fail(h, VXBA_ERR_ARG, std::string(what) + ": bad argument");
  const int nc = (int)h->clouds.size();
  std::vector<PairDesc> pd(B);
  int ms = 0;
  for (int b = 0; b < B; b++) {
    const int si = src_tar[2 * b], ti = src_tar[2 * b + 1];
    if (si < 0 || si >= nc || ti < 0 || ti >= nc)
      return fail(h, VXBA_ERR_ARG, std::string(what) + ": pair " + std::to_string(b) + " (" + std::to_string(si) + ", " + std::to_string(ti) + ") is out of range for " + std::to_string(nc) + " clouds");
    for (int k = 0; k < 12; k++) if (!std::isfinite(poses[12 * (size_t)b + k])) return fail(h, VXBA_ERR_ARG, std::string(what) + ": the pose of pair " + std::to_string(b) + " is not finite");
    pd[b] = PairDesc{h->clouds[si].d, h->clouds[ti].d, h->clouds[si].n, h->clouds[ti].n};
    if (pd[b].S > ms) ms = pd[b].S;
  }
  VX_HIP(h, hipSetDevice(h->device));
  VX_HIP(h, h->d_pairs.reserve(B)); VX_HIP(h, h->d_poses.reserve((size_t)B * 12)); VX_HIP(h, h->d_state.reserve(B)); VX_HIP(h, h->d_useful.reserve(B)); VX_HIP(h, h->d_report.reserve((size_t)B * REPORT_LEN));
  VX_HIP(h, hipMemcpyAsync(h->d_pairs, pd.data(), sizeof(PairDesc) * B, hipMemcpyHostToDevice, h->s));
  VX_HIP(h, hipMemcpyAsync(h->d_poses, poses, sizeof(double) * 12 * B, hipMemcpyHostToDevice, h->s));
  VX_HIP(h, hipStreamSynchronize(h->s));                  // pd leaves scope; counted by the callers
  *max_s = ms;
  return VXBA_OK;
}

static void set_gates(double g[4], const double* v) { for (int k = 0; k < 4; k++) g[k] = v[k]; }

// ---- what vxba_loopsearch.hip uses (vxba_loopreg_internal.hpp) ----
hipStream_t stream_of(vxba_loopreg* h) { return h->s; }
unsigned long long generation_of(const vxba_loopreg* h) { return h->generation; }
bool cloud_of(const vxba_loopreg* h, int id, const float** d, int* n) {
  if (id < 0 || id >= (int)h->clouds.size()) return false;
  *d = h->clouds[id].d; *n = h->clouds[id].n;
  return true;
}
void enqueue_score(vxba_loopreg* h, int B, int max_s, const PairDesc* d_pairs, const double* d_poses, int* d_useful, double normal_thr, double dis_thr) {
  Args a{};
  a.pairs = d_pairs; a.poses = d_poses; a.useful = d_useful;
  const double g[4] = {normal_thr, normal_thr, dis_thr, std::numeric_limits<double>::infinity()};
  set_gates(a.g0, g); set_gates(a.g1, g);
  hipLaunchKernelGGL(associate_kernel<MODE_SCORE>, dim3(blocks_for(max_s > 0 ? max_s : 1, SPB), B), dim3(BLK), 0, h->s, a);
}

}  // namespace vxlr

using namespace vxlr;

extern "C" {

int vxba_loopreg_create(int device, vxba_loopreg** out) {
  if (!out) return VXBA_ERR_ARG;
  *out = nullptr;
  if (const int rc = vxu::select_device(device)) return rc;
  vxba_loopreg* h = new vxba_loopreg();
  h->device = device;
  if (h->s.create() != hipSuccess) { delete h; return VXBA_ERR_HIP; }
  *out = h;
  return VXBA_OK;
}

int vxba_loopreg_clear(vxba_loopreg* h) {
  if (!h) return VXBA_ERR_ARG;
  hipSetDevice(h->device);
  if (h->s) hipStreamSynchronize(h->s);
  h->clouds.clear();
  h->generation += 1;
  return VXBA_OK;
}

int vxba_loopreg_destroy(vxba_loopreg* h) {
  if (!h) return VXBA_OK;
  vxba_loopreg_clear(h);
  h->work.release();
  delete h;
  return VXBA_OK;
}

const char* vxba_loopreg_last_error(const vxba_loopreg* h) { return h ? h->err.c_str() : "null handle"; }

int vxba_loopreg_num_clouds(const vxba_loopreg* h) { return h ? (int)h->clouds.size() : 0; }

int64_t vxba_loopreg_cloud_size(const vxba_loopreg* h, int id) { return (h && id >= 0 && id < (int)h->clouds.size()) ? (int64_t)h->clouds[id].n : -1; }

int vxba_loopreg_read_cloud(vxba_loopreg* h, int id, float* xyzn) {
  if (!h) return VXBA_ERR_ARG;
  if (id < 0 || id >= (int)h->clouds.size()) return fail(h, VXBA_ERR_ARG, "loopreg_read_cloud: cloud " + std::to_string(id) + " is out of range for " + std::to_string(h->clouds.size()) + " clouds");
  const auto& c = h->clouds[id];
  if (c.n == 0) return VXBA_OK;
  if (!xyzn) return fail(h, VXBA_ERR_ARG, "loopreg_read_cloud: bad argument");
  VX_HIP(h, hipSetDevice(h->device));
  VX_HIP(h, hipMemcpyAsync(xyzn, c.d, (size_t)c.n * 6 * sizeof(float), hipMemcpyDeviceToHost, h->s));
  VX_HIP(h, hipStreamSynchronize(h->s));
  return VXBA_OK;
}

int vxba_loopreg_add_cloud(vxba_loopreg* h, int64_t n, const float* xyzn, int* id) {
  if (!h || n < 0 || n > INT32_MAX / 8 || (n > 0 && !xyzn) || !id) return fail(h, VXBA_ERR_ARG, "loopreg_add_cloud: bad argument");
  for (int64_t k = 0; k < 6 * n; k++) if (!std::isfinite(xyzn[k])) return fail(h, VXBA_ERR_ARG, "loopreg_add_cloud: row " + std::to_string(k / 6) + " is not finite");
  VX_HIP(h, hipSetDevice(h->device));
  vxba_loopreg::Cloud c;
  c.n = (int)n;
  VX_HIP(h, c.d.reserve((size_t)(n ? n : 1) * 6));
  if (n) {
    hipError_t e = hipMemcpyAsync(c.d, xyzn, (size_t)n * 6 * sizeof(float), hipMemcpyHostToDevice, h->s);
    if (e == hipSuccess) e = hipStreamSynchronize(h->s);
    if (e != hipSuccess) return fail(h, VXBA_ERR_HIP, std::string("loopreg_add_cloud: ") + hipGetErrorString(e));
  }
  h->clouds.push_back(std::move(c));
  *id = (int)h->clouds.size() - 1;
  return VXBA_OK;
}

// xyz: n_points x 3 float64 on the host, or -- xyz_f32_device -- n_points x 3 float32 in device memory, widened exactly
static int add_keyframe(vxba_loopreg* h, int64_t n_points, const double* xyz, const float* xyz_f32_device, const vxba_planecloud_params* prm, int* id, int64_t* n_planes) {
  if (!h || n_points < 0 || n_points > (int64_t)1 << 30 || (n_points > 0 && !xyz && !xyz_f32_device) || !id) return fail(h, VXBA_ERR_ARG, "loopreg_add_keyframe: bad argument");
  const double voxel_size = prm && prm->voxel_size > 0 ? prm->voxel_size : 1.0;
  const int init_num = prm && prm->voxel_init_num >= 0 ? prm->voxel_init_num : 10;
  const double thre = prm && prm->plane_detection_thre > 0 ? prm->plane_detection_thre : 0.01;
  if (n_planes) *n_planes = 0;
  VX_HIP(h, hipSetDevice(h->device));
  if (n_points == 0) return new_cloud(h, 0, nullptr, id);
  const long long n = n_points;
  double* d_xyz = nullptr; unsigned long long *d_key = nullptr, *d_key_s = nullptr; unsigned int *d_idx = nullptr, *d_idx_s = nullptr, *d_flag = nullptr, *d_pos = nullptr, *d_total = nullptr;
  float *d_rows = nullptr, *d_out = nullptr; int* d_err = nullptr;
  vxu::Temp temp;
  VX_HIP(h, vxu::sort_temp<unsigned long long, unsigned int>(temp.bytes, (size_t)n, 3 * KEY_BITS, h->s));
  VX_HIP(h, vxu::scan_temp<unsigned int>(temp.bytes, (size_t)n, h->s));
  VX_HIP(h, h->work.layout([&](vxu::Arena& a) {
    d_xyz = a.take<double>(3 * n); d_key = a.take<unsigned long long>(n); d_key_s = a.take<unsigned long long>(n);
    d_idx = a.take<unsigned int>(n); d_idx_s = a.take<unsigned int>(n); d_flag = a.take<unsigned int>(n); d_pos = a.take<unsigned int>(n);
    d_total = a.take<unsigned int>(1); d_rows = a.take<float>(6 * n); d_out = a.take<float>(6 * n); d_err = a.take<int>(1); temp.p = a.take<char>(temp.bytes);
  }, h->s));
  if (xyz_f32_device) hipLaunchKernelGGL(widen_kernel, dim3(blocks_for(3 * n)), dim3(256), 0, h->s, xyz_f32_device, 3 * n, d_xyz);
  else VX_HIP(h, hipMemcpyAsync(d_xyz, xyz, sizeof(double) * 3 * n, hipMemcpyHostToDevice, h->s));
  VX_HIP(h, hipMemsetAsync(d_err, 0, 4, h->s));
  hipLaunchKernelGGL(key_kernel, dim3(blocks_for(n)), dim3(256), 0, h->s, (const double*)d_xyz, n, voxel_size, d_key, d_idx, d_err);
  VX_HIP(h, vxu::sort(temp, d_key, d_key_s, d_idx, d_idx_s, (size_t)n, 3 * KEY_BITS, h->s));
  hipLaunchKernelGGL(plane_kernel, dim3(blocks_for(n)), dim3(256), 0, h->s, (const double*)d_xyz, (const unsigned long long*)d_key_s, (const unsigned int*)d_idx_s, n, init_num, thre, d_rows, d_flag);
  VX_HIP(h, vxu::scan(temp, d_flag, d_pos, (size_t)n, h->s));
  hipLaunchKernelGGL(scatter_kernel, dim3(blocks_for(n)), dim3(256), 0, h->s, (const float*)d_rows, (const unsigned int*)d_flag, (const unsigned int*)d_pos, n, d_out, d_total);
  VX_HIP(h, hipGetLastError());
  unsigned int total = 0; int bad = 0;
  VX_HIP(h, hipMemcpyAsync(&total, d_total, 4, hipMemcpyDeviceToHost, h->s));
  VX_HIP(h, hipMemcpyAsync(&bad, d_err, 4, hipMemcpyDeviceToHost, h->s));
  VX_HIP(h, hipStreamSynchronize(h->s));
  int rc = VXBA_OK;
  if (bad) rc = fail(h, VXBA_ERR_ARG, "loopreg_add_keyframe: a point is not finite or lies beyond 2^20 voxels of the origin");
  else {
    rc = new_cloud(h, (int)total, d_out, id);
    if (rc == VXBA_OK) { hipError_t e = hipStreamSynchronize(h->s); if (e != hipSuccess) rc = fail(h, VXBA_ERR_HIP, std::string("loopreg_add_keyframe: ") + hipGetErrorString(e)); }
    if (rc == VXBA_OK && n_planes) *n_planes = total;
  }
  return rc;
}

int vxba_loopreg_add_keyframe(vxba_loopreg* h, int64_t n_points, const double* xyz, const vxba_planecloud_params* prm, int* id, int64_t* n_planes) {
  return add_keyframe(h, n_points, xyz, nullptr, prm, id, n_planes);
}

int vxba_loopreg_add_keyframe_device(vxba_loopreg* h, int64_t n_points, const float* d_xyz, const vxba_planecloud_params* prm, int* id, int64_t* n_planes) {
  if (n_points > 0 && !d_xyz) return fail(h, VXBA_ERR_ARG, "loopreg_add_keyframe_device: bad argument");
  return add_keyframe(h, n_points, nullptr, d_xyz, prm, id, n_planes);
}

int vxba_loopreg_associate(vxba_loopreg* h, int src, int tar, const double pose[12], const double gates[4], int32_t* nn, uint8_t* matched) {
  if (!h || !pose || !gates) return fail(h, VXBA_ERR_ARG, "loopreg_associate: bad argument");
  const int32_t st[2] = {src, tar};
  int S = 0;
  h->launches = h->syncs = 0; h->last_B = 1;
  int rc = stage_pairs(h, "loopreg_associate", 1, st, pose, &S);
  if (rc != VXBA_OK) return rc;
  h->syncs += 1;
  if (S == 0) return VXBA_OK;
  if (!nn || !matched) return fail(h, VXBA_ERR_ARG, "loopreg_associate: bad argument");
  VX_HIP(h, h->d_nn.reserve(S)); VX_HIP(h, h->d_matched.reserve(S));
  Args a{};
  a.pairs = h->d_pairs; a.poses = h->d_poses; a.nn = h->d_nn; a.matched = h->d_matched;
  set_gates(a.g0, gates); set_gates(a.g1, gates);
  hipLaunchKernelGGL(associate_kernel<MODE_INSPECT>, dim3(blocks_for(S, SPB), 1), dim3(BLK), 0, h->s, a);
  h->launches += 1;
  VX_HIP(h, hipGetLastError());
  VX_HIP(h, hipMemcpyAsync(nn, h->d_nn, sizeof(int32_t) * S, hipMemcpyDeviceToHost, h->s));
  VX_HIP(h, hipMemcpyAsync(matched, h->d_matched, S, hipMemcpyDeviceToHost, h->s));
  VX_HIP(h, hipStreamSynchronize(h->s));
  h->syncs += 1;
  return VXBA_OK;
}

int vxba_loopreg_score(vxba_loopreg* h, int B, const int32_t* src_tar, const double* poses, double normal_thr, double dis_thr, double* score, int64_t* useful) {
  if (!h || !score) return fail(h, VXBA_ERR_ARG, "loopreg_score: bad argument");
  int S = 0;
  h->launches = h->syncs = 0; h->last_B = B;
  int rc = stage_pairs(h, "loopreg_score", B, src_tar, poses, &S);
  if (rc != VXBA_OK) return rc;
  h->syncs += 1;
  VX_HIP(h, hipMemsetAsync(h->d_useful, 0, sizeof(int) * B, h->s));
  Args a{};
  a.pairs = h->d_pairs; a.poses = h->d_poses; a.useful = h->d_useful;
  const double g[4] = {normal_thr, normal_thr, dis_thr, std::numeric_limits<double>::infinity()};    // no point-to-point gate (BTC.cpp:1471-1473)
  set_gates(a.g0, g); set_gates(a.g1, g);
  if (S > 0) {
    hipLaunchKernelGGL(associate_kernel<MODE_SCORE>, dim3(blocks_for(S, SPB), B), dim3(BLK), 0, h->s, a);
    h->launches += 1;
    VX_HIP(h, hipGetLastError());
  }
  std::vector<int> cnt(B);
  VX_HIP(h, hipMemcpyAsync(cnt.data(), h->d_useful, sizeof(int) * B, hipMemcpyDeviceToHost, h->s));
  VX_HIP(h, hipStreamSynchronize(h->s));
  h->syncs += 1;
  for (int b = 0; b < B; b++) {
    const int Sb = h->clouds[src_tar[2 * b]].n;
    score[b] = Sb > 0 ? (double)cnt[b] / (double)Sb : 0.0;      // an empty source has no useful match (the reference divides 0 by 0)
    if (useful) useful[b] = cnt[b];
  }
  return VXBA_OK;
}

int vxba_loopreg_icp(vxba_loopreg* h, int B, const int32_t* src_tar, double* poses, const vxba_icp_options* opt, double* report) {
  if (!h) return VXBA_ERR_ARG;
  int S = 0;
  h->launches = h->syncs = 0; h->last_B = B;
  int rc = stage_pairs(h, "loopreg_icp", B, src_tar, poses, &S);
  if (rc != VXBA_OK) return rc;
  h->syncs += 1;
  const int max_iter = opt && opt->max_iter > 0 ? opt->max_iter : 20;
  static const double G0[4] = {0.2, 0.2, 0.5, 3.0}, G1[4] = {0.1, 0.1, 0.1, 1.0};
  Args a{};
  set_gates(a.g0, opt && opt->gates0[0] > 0 ? opt->gates0 : G0);
  set_gates(a.g1, opt && opt->gates1[0] > 0 ? opt->gates1 : G1);
  a.step_tol = opt && opt->step_tol > 0 ? opt->step_tol : 1e-3;
  a.icp_eigval = opt && opt->icp_eigval > 0 ? opt->icp_eigval : 14.0;
  a.max_iter = max_iter;
  const int nblk = (int)blocks_for(S > 0 ? S : 1, SPB);
  const size_t need = (size_t)B * nblk * ACC_LEN;
  VX_HIP(h, h->d_partial.reserve(need));
  std::vector<PairState> st(B);
  for (int b = 0; b < B; b++) { std::memset(&st[b], 0, sizeof(PairState)); std::memcpy(st[b].pose, poses + 12 * (size_t)b, sizeof(double) * 12); }
  VX_HIP(h, hipMemcpyAsync(h->d_state, st.data(), sizeof(PairState) * B, hipMemcpyHostToDevice, h->s));
  VX_HIP(h, hipMemsetAsync(h->d_report, 0, sizeof(double) * REPORT_LEN * B, h->s));
  a.pairs = h->d_pairs; a.state = h->d_state; a.partial = h->d_partial; a.nblk = nblk; a.report = h->d_report;
  for (int it = 0; it < max_iter; it++) {
    hipLaunchKernelGGL(associate_kernel<MODE_ICP>, dim3(nblk, B), dim3(BLK), 0, h->s, a);
    hipLaunchKernelGGL(icp_step_kernel, dim3(B), dim3(64), 0, h->s, a);
    h->launches += 2;
  }
  VX_HIP(h, hipGetLastError());
  std::vector<double> rep((size_t)B * REPORT_LEN);
  VX_HIP(h, hipMemcpyAsync(st.data(), h->d_state, sizeof(PairState) * B, hipMemcpyDeviceToHost, h->s));
  VX_HIP(h, hipMemcpyAsync(rep.data(), h->d_report, sizeof(double) * rep.size(), hipMemcpyDeviceToHost, h->s));
  VX_HIP(h, hipStreamSynchronize(h->s));
  h->syncs += 1;
  for (int b = 0; b < B; b++) std::memcpy(poses + 12 * (size_t)b, st[b].pose, sizeof(double) * 12);
  if (report) std::memcpy(report, rep.data(), sizeof(double) * rep.size());
  return VXBA_OK;
}

int vxba_loopreg_stats(const vxba_loopreg* h, int64_t out[4]) {
  if (!h || !out) return VXBA_ERR_ARG;
  out[0] = h->launches; out[1] = h->syncs; out[2] = (int64_t)h->clouds.size(); out[3] = h->last_B;
  return VXBA_OK;
}

}  // extern "C"
