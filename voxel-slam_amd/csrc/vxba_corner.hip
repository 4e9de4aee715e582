// Corner extraction on the GPU (include/vxba.h: vxba_corner_*): STDescManager::GenerateSTDescs without its last step -- init_voxel_map / init_plane,
// get_project_plane, merge_plane, binary_extractor, extract_binary and non_maxi_suppression (BTC.cpp:90-139, 156-186, 279-321, 340-977).  A keyframe's
// `full` cloud goes in; the corner set vxba_loopsearch_describe takes comes out.  The arithmetic is vxba_corner_math.hpp's, restated by
// tests/_corner_ref.py; this unit is built without floating-point contraction.
//
// Launch plan, n points, P plane voxels, M merged planes, U <= proj_plane_num used planes, E = n U:
//   cn_widen_kernel        the device route only: float32 -> float64, exact
//   cn_key_kernel          one lane per point: 63-bit voxel key and index; a bad coordinate raises a flag word in mapped host memory
//   rocPRIM                stable radix sort (key, index), run-length encode, exclusive scan
//   cn_big_kernel + scan   the runs with more than voxel_init_num points get a record slot, in key order
//   cn_plane_kernel        one lane per such voxel folds its points in input order, solves, decides; scan of the verdicts
//   cn_plane_scatter       the plane records in key order = ascending (x, y, z) voxel coordinate            -> wait 1: P
//   cn_pair_kernel         P x P pair tests, one bit each, row i word w = columns 64 w ..                     -> wait 2: the bit matrix
//   host                   the reference's sequential labelling, the folds of the groups, the stable sort by N
//   cn_pair_kernel         M x M over the merged list                                                        -> wait 3
//   host                   merge_plane, the sort, the gate of binary_extractor: the used planes
//   cn_project_kernel      one lane per (point, used plane): min / max of px, py and the kept count, reduced down a fixed tree per block
//   cn_bounds_kernel       one block per used plane reduces the block partials and fixes the image's origin, sizes and segment counts
//   cn_cellkey_kernel      the key (plane, segment x, segment y, x in segment, y in segment) per (point, plane); pairs outside every image sort last
//   rocPRIM                stable radix sort, run-length encode, exclusive scan over E
//   cn_cell_kernel         one lane per occupied cell replays its points in input order: count, sum px, sum py, occupancy word
//   cn_segment_kernel      the first cell of every segment scans the segment's cells (adjacent in key order), picks the winner, applies the summary,
//                          touch, border and line filters (neighbours by binary search in the sorted cell keys); scan of the verdicts
//   cn_cand_scatter        the candidates in (plane, segment x, segment y) order with their locations
//   cn_suppress_kernel     brute force over LDS tiles: the verdict of non_maxi_suppression per candidate     -> wait 4: counts, wait 5: the candidates
//   host                   the kept candidates in order and the cut (a stable sort by summary of at most MAX_CAND entries)
// The number of launches and waits depends on the route (host, device, with_planes) only.  Nothing is summed with atomics; every order-dependent
// sum is replayed in input order.  Results are committed at the end: a failed call leaves the previous result readable.
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdint>
#include <cstring>
#include <string>
#include <vector>

#include "../../include/vxba.h"
#include "vxba_corner_math.hpp"
#include "vxba_dev.hpp"
#include "vxba_wait.hpp"

namespace vxcn {

constexpr int BLK = 256;
constexpr int MAX_PLANES = 16384;       // rows of a pair test (plane voxels, merged planes)
constexpr int MAX_CAND = 65536;         // candidates ahead of the suppression
constexpr int64_t MAX_POINTS = (int64_t)1 << 28;     // E = 8 n stays below 2^31

struct Cand {      // one candidate as the host reads it
  double loc[3];
  unsigned long long occ;
  int plane, cx, cy, count, summary, keep;
};

struct ImgArgs {
  double res, high_inc, dis_min, dis_max, summary_min, radius;
  int cut_num, line_filter, touch_filter, n_used;
};

__global__ void __launch_bounds__(BLK) cn_widen_kernel(const float* __restrict__ src, long long n3, double* __restrict__ dst) {
  const long long i = (long long)blockIdx.x * BLK + threadIdx.x;
  if (i < n3) dst[i] = (double)src[i];
}

__global__ void __launch_bounds__(BLK) cn_key_kernel(const double* __restrict__ xyz, long long n, double vs, unsigned long long* __restrict__ key, unsigned int* __restrict__ idx,
                                                     unsigned int* __restrict__ flags) {
  const long long i = (long long)blockIdx.x * BLK + threadIdx.x;
  if (i >= n) return;
  const double q[3] = {xyz[3 * i], xyz[3 * i + 1], xyz[3 * i + 2]};
  unsigned long long k;
  if (!voxel_key(q, vs, &k)) flags[0] = 1u;       // every writer stores the same value
  key[i] = k;
  idx[i] = (unsigned int)i;
}

// big[r] = 1 where run r holds more than voxel_init_num points; big has n + 1 entries, zeroed beforehand
__global__ void __launch_bounds__(BLK) cn_big_kernel(const unsigned int* __restrict__ cnt, const unsigned int* __restrict__ n_runs, int voxel_init_num, unsigned int* __restrict__ big) {
  const long long r = (long long)blockIdx.x * BLK + threadIdx.x;
  if (r >= (long long)*n_runs) return;
  big[r] = cnt[r] > (unsigned int)voxel_init_num ? 1u : 0u;
}

__global__ void __launch_bounds__(BLK) cn_plane_kernel(const double* __restrict__ xyz, const unsigned int* __restrict__ idx_s, const unsigned int* __restrict__ ptr,
                                                       const unsigned int* __restrict__ n_runs, const unsigned int* __restrict__ big, const unsigned int* __restrict__ slot, double thre,
                                                       double* __restrict__ recs, unsigned int* __restrict__ is_plane) {
  const long long r = (long long)blockIdx.x * BLK + threadIdx.x;
  if (r >= (long long)*n_runs || !big[r]) return;
  double P[6] = {0, 0, 0, 0, 0, 0}, v[3] = {0, 0, 0};
  const unsigned int beg = ptr[r], end = ptr[r + 1];
  for (unsigned int q = beg; q < end; q++) {
    const double* p = xyz + 3 * (size_t)idx_s[q];
    const double x = p[0], y = p[1], z = p[2];
    P[0] += x * x; P[1] += x * y; P[2] += x * z; P[3] += y * y; P[4] += y * z; P[5] += z * z;
    v[0] += x; v[1] += y; v[2] += z;
  }
  double rec[REC];
  const bool ok = record_from_sums(P, v, (long long)(end - beg), thre, rec);
  const unsigned int s = slot[r];
  if (ok) {
#pragma unroll
    for (int k = 0; k < REC; k++) recs[(size_t)REC * s + k] = rec[k];
  }
  is_plane[s] = ok ? 1u : 0u;
}

// is_plane / pos have `slots` + 1 entries (the last flag is 0): pos[slots] is the number of planes
__global__ void __launch_bounds__(BLK) cn_plane_scatter(const double* __restrict__ recs, const unsigned int* __restrict__ is_plane, const unsigned int* __restrict__ pos, long long slots,
                                                        double* __restrict__ planes, unsigned int* __restrict__ flags) {
  const long long s = (long long)blockIdx.x * BLK + threadIdx.x;
  if (s == 0) flags[1] = pos[slots];
  if (s >= slots || !is_plane[s]) return;
  const unsigned int o = pos[s];
  if (o >= (unsigned int)MAX_PLANES) return;
#pragma unroll
  for (int k = 0; k < REC; k++) planes[(size_t)REC * o + k] = recs[(size_t)REC * s + k];
}

// bit (i, j) of the pair test, j < i; row i holds W words
__global__ void __launch_bounds__(BLK) cn_pair_kernel(const double* __restrict__ planes, int P, int W, double normal_thre, double dis_thre, unsigned long long* __restrict__ bits) {
  const long long t = (long long)blockIdx.x * BLK + threadIdx.x;
  if (t >= (long long)P * W) return;
  const int i = (int)(t / W), w = (int)(t % W);
  unsigned long long word = 0;
  const double* a = planes + (size_t)REC * i;
  for (int b = 0; b < 64; b++) {
    const int j = 64 * w + b;
    if (j >= i) break;
    if (pair_test(a, planes + (size_t)REC * j, normal_thre, dis_thre)) word |= 1ull << b;
  }
  bits[t] = word;
}

// min / max of px and py and the kept count of one block of points for plane blockIdx.y; part: [plane][block][4], cnt: [plane][block]
__global__ void __launch_bounds__(BLK) cn_project_kernel(const double* __restrict__ xyz, long long n, const Proj* __restrict__ proj, ImgArgs a, double* __restrict__ part,
                                                         unsigned int* __restrict__ part_cnt) {
  __shared__ double s_lo_x[BLK], s_hi_x[BLK], s_lo_y[BLK], s_hi_y[BLK];
  __shared__ unsigned int s_cnt[BLK];
  const int u = blockIdx.y, t = threadIdx.x;
  const long long i = (long long)blockIdx.x * BLK + t;
  double lo_x = INFINITY, hi_x = -INFINITY, lo_y = INFINITY, hi_y = -INFINITY;
  unsigned int c = 0;
  if (i < n) {
    const double q[3] = {xyz[3 * i], xyz[3 * i + 1], xyz[3 * i + 2]};
    double dis, px, py;
    if (project_point(proj[u], q, a.dis_min, a.dis_max, &dis, &px, &py)) { lo_x = hi_x = px; lo_y = hi_y = py; c = 1; }
  }
  s_lo_x[t] = lo_x; s_hi_x[t] = hi_x; s_lo_y[t] = lo_y; s_hi_y[t] = hi_y; s_cnt[t] = c;
  __syncthreads();
  for (int off = BLK / 2; off >= 1; off >>= 1) {
    if (t < off) {
      s_lo_x[t] = fmin(s_lo_x[t], s_lo_x[t + off]); s_hi_x[t] = fmax(s_hi_x[t], s_hi_x[t + off]);
      s_lo_y[t] = fmin(s_lo_y[t], s_lo_y[t + off]); s_hi_y[t] = fmax(s_hi_y[t], s_hi_y[t + off]);
      s_cnt[t] += s_cnt[t + off];
    }
    __syncthreads();
  }
  if (t == 0) {
    const size_t o = (size_t)u * gridDim.x + blockIdx.x;
    part[4 * o] = s_lo_x[0]; part[4 * o + 1] = s_hi_x[0]; part[4 * o + 2] = s_lo_y[0]; part[4 * o + 3] = s_hi_y[0];
    part_cnt[o] = s_cnt[0];
  }
}

__global__ void __launch_bounds__(BLK) cn_bounds_kernel(const double* __restrict__ part, const unsigned int* __restrict__ part_cnt, int nb, ImgArgs a, Img* __restrict__ img, Img* __restrict__ img_host) {
  __shared__ double s_lo_x[BLK], s_hi_x[BLK], s_lo_y[BLK], s_hi_y[BLK];
  __shared__ unsigned long long s_cnt[BLK];
  const int u = blockIdx.x, t = threadIdx.x;
  double lo_x = INFINITY, hi_x = -INFINITY, lo_y = INFINITY, hi_y = -INFINITY;
  unsigned long long c = 0;
  for (int b = t; b < nb; b += BLK) {
    const size_t o = (size_t)u * nb + b;
    lo_x = fmin(lo_x, part[4 * o]); hi_x = fmax(hi_x, part[4 * o + 1]); lo_y = fmin(lo_y, part[4 * o + 2]); hi_y = fmax(hi_y, part[4 * o + 3]);
    c += part_cnt[o];
  }
  s_lo_x[t] = lo_x; s_hi_x[t] = hi_x; s_lo_y[t] = lo_y; s_hi_y[t] = hi_y; s_cnt[t] = c;
  __syncthreads();
  for (int off = BLK / 2; off >= 1; off >>= 1) {
    if (t < off) {
      s_lo_x[t] = fmin(s_lo_x[t], s_lo_x[t + off]); s_hi_x[t] = fmax(s_hi_x[t], s_hi_x[t + off]);
      s_lo_y[t] = fmin(s_lo_y[t], s_lo_y[t + off]); s_hi_y[t] = fmax(s_hi_y[t], s_hi_y[t + off]);
      s_cnt[t] += s_cnt[t + off];
    }
    __syncthreads();
  }
  if (t == 0) {
    Img g;
    make_img(s_lo_x[0], s_hi_x[0], s_lo_y[0], s_hi_y[0], (long long)s_cnt[0], a.res, &g);
    img[u] = g;
    img_host[u] = g;
  }
}

// element e = u n + i: plane-major, so that the stable sort keeps the points of a cell in input order
__global__ void __launch_bounds__(BLK) cn_cellkey_kernel(const double* __restrict__ xyz, long long n, const Proj* __restrict__ proj, const Img* __restrict__ img, ImgArgs a,
                                                         unsigned long long* __restrict__ key, unsigned int* __restrict__ idx) {
  const int u = blockIdx.y;
  const long long i = (long long)blockIdx.x * BLK + threadIdx.x;
  if (i >= n) return;
  const size_t e = (size_t)u * (size_t)n + (size_t)i;
  unsigned long long k = CELL_NONE;
  if (img[u].valid) {
    const double q[3] = {xyz[3 * i], xyz[3 * i + 1], xyz[3 * i + 2]};
    double dis, px, py;
    if (project_point(proj[u], q, a.dis_min, a.dis_max, &dis, &px, &py)) k = cell_key(u, cell_index(px, img[u].min_x, a.res), cell_index(py, img[u].min_y, a.res));
  }
  key[e] = k;
  idx[e] = (unsigned int)e;
}

__global__ void __launch_bounds__(BLK) cn_cell_kernel(const double* __restrict__ xyz, long long n, const Proj* __restrict__ proj, ImgArgs a, const unsigned long long* __restrict__ ukey,
                                                      const unsigned int* __restrict__ idx_s, const unsigned int* __restrict__ ptr, const unsigned int* __restrict__ n_runs,
                                                      unsigned int* __restrict__ c_cnt, double* __restrict__ c_sx, double* __restrict__ c_sy, unsigned long long* __restrict__ c_occ) {
  const long long r = (long long)blockIdx.x * BLK + threadIdx.x;
  if (r >= (long long)*n_runs) return;
  const unsigned long long k = ukey[r];
  if (k >= CELL_NONE) return;
  const int u = key_plane(k);
  const Proj pj = proj[u];
  double sx = 0, sy = 0;
  unsigned long long occ = 0;
  const unsigned int beg = ptr[r], end = ptr[r + 1];
  for (unsigned int q = beg; q < end; q++) {
    const size_t i = (size_t)idx_s[q] - (size_t)u * (size_t)n;
    const double p[3] = {xyz[3 * i], xyz[3 * i + 1], xyz[3 * i + 2]};
    double dis, px, py;
    project_point(pj, p, a.dis_min, a.dis_max, &dis, &px, &py);
    sx += px; sy += py;
    const int b = height_bin(dis, a.dis_min, a.high_inc);
    if (b >= 0 && b < a.cut_num) occ |= 1ull << b;      // dis == dis_max lands on cut_num: counted, no bit (the reference writes out of bounds there)
  }
  c_cnt[r] = end - beg; c_sx[r] = sx; c_sy[r] = sy; c_occ[r] = occ;
}

// the summary of cell (u, cx, cy), 0 where it is empty or outside the image
__device__ __forceinline__ int cell_summary(const unsigned long long* __restrict__ ukey, const unsigned long long* __restrict__ c_occ, unsigned int runs, int u, int cx, int cy) {
  if (cx < 0 || cy < 0) return 0;
  const unsigned long long want = cell_key(u, cx, cy);
  unsigned int lo = 0, hi = runs;
  while (lo < hi) {
    const unsigned int mid = lo + (hi - lo) / 2;
    if (ukey[mid] < want) lo = mid + 1; else hi = mid;
  }
  return (lo < runs && ukey[lo] == want) ? __popcll(c_occ[lo]) : 0;
}

// flag has E + 1 entries, zeroed beforehand; win[r] the winning run of the segment that run r heads
__global__ void __launch_bounds__(BLK) cn_segment_kernel(const unsigned long long* __restrict__ ukey, const unsigned long long* __restrict__ c_occ, const unsigned int* __restrict__ n_runs,
                                                         const Img* __restrict__ img, ImgArgs a, unsigned int* __restrict__ flag, unsigned int* __restrict__ win) {
  const long long r = (long long)blockIdx.x * BLK + threadIdx.x;
  const unsigned int runs = *n_runs;
  if (r >= (long long)runs) return;
  const unsigned long long k = ukey[r];
  if (k >= CELL_NONE) return;
  const unsigned long long seg = k >> 6;
  if (r > 0 && (ukey[r - 1] >> 6) == seg) return;
  int best = 0;
  unsigned int bt = (unsigned int)r;
  for (unsigned int t = (unsigned int)r; t < runs && (ukey[t] >> 6) == seg; t++) {
    const int s = __popcll(c_occ[t]);
    if (s > best) { best = s; bt = t; }
  }
  if (best == 0 || !((double)best >= a.summary_min)) return;
  const unsigned long long kw = ukey[bt], occ = c_occ[bt];
  if (a.touch_filter && !(occ & 15ull)) return;
  const int u = key_plane(kw), cx = key_cx(kw), cy = key_cy(kw);
  const Img g = img[u];
  if (cx / SEG >= g.x_seg || cy / SEG >= g.y_seg) return;      // the reference scans x_seg x y_seg segments
  if (cx <= 0 || cx >= g.x_len - 1 || cy <= 0 || cy >= g.y_len - 1) return;
  if (a.line_filter) {
    bool hit = false;
    hit |= line_hit(best, cell_summary(ukey, c_occ, runs, u, cx, cy + 1), cell_summary(ukey, c_occ, runs, u, cx, cy - 1));
    hit |= line_hit(best, cell_summary(ukey, c_occ, runs, u, cx + 1, cy), cell_summary(ukey, c_occ, runs, u, cx - 1, cy));
    hit |= line_hit(best, cell_summary(ukey, c_occ, runs, u, cx + 1, cy + 1), cell_summary(ukey, c_occ, runs, u, cx - 1, cy - 1));
    hit |= line_hit(best, cell_summary(ukey, c_occ, runs, u, cx + 1, cy - 1), cell_summary(ukey, c_occ, runs, u, cx - 1, cy + 1));
    if (hit) return;
  }
  flag[r] = 1u;
  win[r] = bt;
}

__global__ void __launch_bounds__(BLK) cn_cand_scatter(const unsigned long long* __restrict__ ukey, const unsigned int* __restrict__ n_runs, const unsigned int* __restrict__ flag,
                                                       const unsigned int* __restrict__ pos, long long E, const unsigned int* __restrict__ win, const unsigned int* __restrict__ c_cnt,
                                                       const double* __restrict__ c_sx, const double* __restrict__ c_sy, const unsigned long long* __restrict__ c_occ,
                                                       const Proj* __restrict__ proj, Cand* __restrict__ cand, unsigned int* __restrict__ n_cand, unsigned int* __restrict__ flags) {
  const long long r = (long long)blockIdx.x * BLK + threadIdx.x;
  if (r == 0) {
    const unsigned int runs = *n_runs;
    *n_cand = pos[E]; flags[2] = pos[E];
    flags[3] = runs - ((runs > 0 && ukey[runs - 1] >= CELL_NONE) ? 1u : 0u);      // occupied cells: the run of the pairs in no image is the last one
  }
  if (r >= (long long)*n_runs || !flag[r]) return;
  const unsigned int o = pos[r];
  if (o >= (unsigned int)MAX_CAND) return;
  const unsigned int w = win[r];
  const unsigned long long k = ukey[w];
  const int u = key_plane(k);
  const double cnt = (double)c_cnt[w];
  const double px = c_sx[w] / cnt, py = c_sy[w] / cnt;
  Cand c;
#pragma unroll
  for (int d = 0; d < 3; d++) c.loc[d] = (py * proj[u].x[d] + px * proj[u].y[d]) + proj[u].c[d];
  c.occ = c_occ[w];
  c.plane = u; c.cx = key_cx(k); c.cy = key_cy(k); c.count = (int)c_cnt[w]; c.summary = __popcll(c_occ[w]); c.keep = 1;
  cand[o] = c;
}

// i is dropped when some near j != i has summary_j >= summary_i
__global__ void __launch_bounds__(BLK) cn_suppress_kernel(Cand* __restrict__ cand, const unsigned int* __restrict__ n_cand, float r2) {
  __shared__ float s_x[BLK], s_y[BLK], s_z[BLK];
  __shared__ int s_sum[BLK];
  const unsigned int C = min(*n_cand, (unsigned int)MAX_CAND);
  if (blockIdx.x * BLK >= C) return;
  const unsigned int i = blockIdx.x * BLK + threadIdx.x;
  float me[3] = {0.f, 0.f, 0.f};
  int mine = 0;
  if (i < C) { me[0] = (float)cand[i].loc[0]; me[1] = (float)cand[i].loc[1]; me[2] = (float)cand[i].loc[2]; mine = cand[i].summary; }
  int keep = 1;
  for (unsigned int base = 0; base < C; base += BLK) {
    const unsigned int j = base + threadIdx.x;
    __syncthreads();
    if (j < C) { s_x[threadIdx.x] = (float)cand[j].loc[0]; s_y[threadIdx.x] = (float)cand[j].loc[1]; s_z[threadIdx.x] = (float)cand[j].loc[2]; s_sum[threadIdx.x] = cand[j].summary; }
    __syncthreads();
    const unsigned int m = min((unsigned int)BLK, C - base);
    for (unsigned int t = 0; t < m; t++) {
      const float o[3] = {s_x[t], s_y[t], s_z[t]};
      if (base + t != i && nms_near(me, o, r2) && s_sum[t] >= mine) keep = 0;
    }
  }
  if (i < C) cand[i].keep = keep;
}

}  // namespace vxcn

struct vxba_corner {
  int device = 0;
  std::string err;
  vxu::Stream s;
  vxu::Pin<unsigned int> flags;       // mapped host: [0] bad coordinate, [1] planes, [2] candidates, [3] cell runs
  vxu::Pin<vxcn::Img> h_img;          // mapped host: the images of the used planes
  vxu::Pin<vxcn::Proj> h_proj; vxu::Dev<vxcn::Proj> d_proj;
  vxu::Dev<vxcn::Img> d_img;
  vxu::Dev<unsigned int> d_runs, d_ncand;
  vxu::Dev<double> d_planes;                              // MAX_PLANES records: the pair kernel's rows
  vxu::Dev<unsigned long long> d_bits;
  vxu::Dev<vxcn::Cand> d_cand;
  vxu::Arena work;
  // the last result
  std::vector<double> planes; std::vector<int> plane_id;            // stage 1-2: records and labels
  std::vector<double> proj_list; std::vector<int> proj_used;        // stage 3-4: final sorted list, position among the used or -1
  std::vector<vxcn::Cand> cand;                                      // stage 5-6
  std::vector<int> out;                                              // stage 7: indices into cand
  int64_t stats[6] = {0, 0, 0, 0, 0, 0};      // launches, host waits, bytes D2H, bytes H2D, occupied cells, candidates
  bool profiling = false, ev_valid = false;
  vxu::Event ev[12];
};

using namespace vxcn;
using vxu::blocks_for, vxu::fail;

namespace {

int wait(vxba_corner* h) {
  const hipError_t e = vxwait::stream_wait(h->s);
  h->stats[1] += 1;
  if (e != hipSuccess) return fail(h, VXBA_ERR_HIP, std::string("corner_extract: ") + hipGetErrorString(e));
  return VXBA_OK;
}

int check_params(vxba_corner* h, const vxba_corner_params* p, int* cut_num) {
  auto bad = [&](const char* m) { return fail(h, VXBA_ERR_ARG, std::string("corner_extract: ") + m); };
  if (!(p->proj_image_resolution > 0) || !(p->proj_image_high_inc > 0) || !(p->voxel_size > 0) || !(p->non_max_suppression_radius > 0))
    return bad("a resolution, increment, voxel size or radius is not positive");
  if (!std::isfinite(p->proj_image_resolution) || !std::isfinite(p->proj_image_high_inc) || !std::isfinite(p->voxel_size) || !std::isfinite(p->non_max_suppression_radius) ||
      !std::isfinite(p->proj_dis_min) || !std::isfinite(p->proj_dis_max) || !std::isfinite(p->plane_merge_normal_thre) || !std::isfinite(p->plane_merge_dis_thre) ||
      !std::isfinite(p->plane_detection_thre) || !std::isfinite(p->summary_min_thre))
    return bad("a parameter is not finite");
  if (!(p->proj_dis_max > p->proj_dis_min)) return bad("proj_dis_max <= proj_dis_min");
  const double cn = (p->proj_dis_max - p->proj_dis_min) / p->proj_image_high_inc;
  if (!(cn >= 4.0 && cn < 65.0)) return bad("cut_num outside 4..64");
  *cut_num = (int)cn;
  if (p->proj_plane_num < 1 || p->proj_plane_num > MAX_USED) return bad("proj_plane_num outside 1..8");
  if (p->useful_corner_num < 1 || p->useful_corner_num > VXBA_LOOPSEARCH_MAX_CORNERS) return bad("useful_corner_num outside 1..VXBA_LOOPSEARCH_MAX_CORNERS");
  if (p->voxel_init_num < 0) return bad("voxel_init_num is negative");
  return VXBA_OK;
}

// rows (count x REC, on the host) through the pair kernel: the bit matrix, W words a row
int pair_bits(vxba_corner* h, const std::vector<double>& rows, bool upload, const vxba_corner_params* p, std::vector<unsigned long long>& bits, int* W_out) {
  const int P = (int)(rows.size() / REC), W = (P + 63) / 64;
  *W_out = W;
  const size_t words = (size_t)P * W;
  VX_HIP(h, h->d_bits.reserve(words, words + words / 4));
  if (upload && P > 0) { VX_HIP(h, hipMemcpyAsync(h->d_planes, rows.data(), rows.size() * sizeof(double), hipMemcpyHostToDevice, h->s)); h->stats[3] += (int64_t)(rows.size() * sizeof(double)); }
  hipLaunchKernelGGL(cn_pair_kernel, dim3(blocks_for((long long)words, BLK)), dim3(BLK), 0, h->s, (const double*)h->d_planes, P, W, p->plane_merge_normal_thre, p->plane_merge_dis_thre, h->d_bits);
  VX_HIP(h, hipGetLastError());
  h->stats[0] += 1;
  bits.assign(words, 0ull);
  if (words) { VX_HIP(h, hipMemcpyAsync(bits.data(), h->d_bits, words * 8, hipMemcpyDeviceToHost, h->s)); h->stats[2] += (int64_t)words * 8; }
  return wait(h);
}

struct Ev {      // events around a stage when profiling
  vxba_corner* h; int k;
  void begin() { if (h->profiling) hipEventRecord(h->ev[2 * k], h->s); }
  void end() { if (h->profiling) hipEventRecord(h->ev[2 * k + 1], h->s); }
};

// mode 0: host cloud, 1: device float32 cloud, 2: host cloud and a caller's plane list
int extract(vxba_corner* h, int mode, int64_t n, const void* src, int64_t m, const double* centres, const double* normals, const vxba_corner_params* p_in, int64_t* n_corners) {
  if (!h) return VXBA_ERR_ARG;
  vxba_corner_params prm;
  if (p_in) prm = *p_in; else vxba_corner_default_params(&prm, 0);
  const vxba_corner_params* p = &prm;
  if (!n_corners || n < 0 || n > MAX_POINTS || (n > 0 && !src)) return fail(h, VXBA_ERR_ARG, "corner_extract: bad argument");
  int cut_num = 0;
  if (const int rc = check_params(h, p, &cut_num)) return rc;
  if (mode == 2) {
    if (m < 1 || m > MAX_PLANES || !centres || !normals) return fail(h, VXBA_ERR_ARG, "corner_extract_with_planes: 1..16384 planes");
    for (int64_t k = 0; k < 3 * m; k++) if (!std::isfinite(centres[k]) || !std::isfinite(normals[k])) return fail(h, VXBA_ERR_ARG, "corner_extract_with_planes: a plane is not finite");
    for (int64_t k = 0; k < m; k++) if (normals[3 * k] == 0 && normals[3 * k + 1] == 0 && normals[3 * k + 2] == 0) return fail(h, VXBA_ERR_ARG, "corner_extract_with_planes: a zero normal");
  }
  if (mode != 1 && n > 0) {
    const double* x = (const double*)src;
    for (int64_t k = 0; k < 3 * n; k++) {
      if (!std::isfinite(x[k]) || !(std::fabs(x[k] / p->voxel_size) < (double)(KEY_OFF - 2)))
        return fail(h, VXBA_ERR_ARG, "corner_extract: point " + std::to_string(k / 3) + " is not finite or lies 2^20 voxels or more from the origin");
    }
  }
  for (int64_t& v : h->stats) v = 0;
  h->ev_valid = false;
  std::vector<double> planes, proj_list;
  std::vector<int> plane_id, proj_used;
  std::vector<Cand> cand;
  std::vector<int> out;
  auto commit = [&]() {
    h->planes.swap(planes); h->plane_id.swap(plane_id); h->proj_list.swap(proj_list); h->proj_used.swap(proj_used); h->cand.swap(cand); h->out.swap(out);
    *n_corners = (int64_t)h->out.size();
    return VXBA_OK;
  };
  if (n == 0) return commit();
  VX_HIP(h, hipSetDevice(h->device));

  // one layout for the whole call: the cloud, the voxel cells over n, the image cells over E = n proj_plane_num
  const size_t N = (size_t)n, EU = N * (size_t)p->proj_plane_num, slots = N / ((size_t)p->voxel_init_num + 1) + 1;
  const int nb = (int)blocks_for(n, BLK);
  double *d_xyz = nullptr, *d_recs = nullptr, *d_part = nullptr, *c_sx = nullptr, *c_sy = nullptr;
  unsigned int *d_big = nullptr, *d_slot = nullptr, *d_isp = nullptr, *d_ppos = nullptr, *d_pcnt = nullptr, *c_cnt = nullptr, *d_flag = nullptr, *d_fpos = nullptr, *d_win = nullptr;
  unsigned long long* c_occ = nullptr;
  vxu::Cells<unsigned int> c1, c2;
  VX_HIP(h, c1.size(N, 3 * KEY_BITS, h->s));
  VX_HIP(h, c2.size(EU, 54, h->s));
  VX_HIP(h, vxu::scan_temp<unsigned int>(c1.temp.bytes, slots + 1, h->s));
  bool synced = false;
  VX_HIP(h, h->work.layout([&](vxu::Arena& a) {
    d_xyz = a.take<double>(3 * N);
    c1.carve(a, N);
    d_big = a.take<unsigned int>(N + 1); d_slot = a.take<unsigned int>(N + 1);
    d_recs = a.take<double>(REC * slots); d_isp = a.take<unsigned int>(slots + 1); d_ppos = a.take<unsigned int>(slots + 1);
    d_part = a.take<double>(4 * (size_t)nb * MAX_USED); d_pcnt = a.take<unsigned int>((size_t)nb * MAX_USED);
    c2.carve(a, EU);
    c_cnt = a.take<unsigned int>(EU); c_sx = a.take<double>(EU); c_sy = a.take<double>(EU); c_occ = a.take<unsigned long long>(EU);
    d_flag = a.take<unsigned int>(EU + 1); d_fpos = a.take<unsigned int>(EU + 1); d_win = a.take<unsigned int>(EU);
  }, h->s, &synced));
  if (synced) h->stats[1] += 1;
  h->flags[0] = h->flags[1] = h->flags[2] = h->flags[3] = 0u;

  if (mode == 1) {
    hipLaunchKernelGGL(cn_widen_kernel, dim3(blocks_for(3 * n, BLK)), dim3(BLK), 0, h->s, (const float*)src, (long long)(3 * n), d_xyz);
    VX_HIP(h, hipGetLastError());
    h->stats[0] += 1;
  } else {
    VX_HIP(h, hipMemcpyAsync(d_xyz, src, N * 24, hipMemcpyHostToDevice, h->s));
    h->stats[3] += n * 24;
  }

  double first[3] = {0, 0, 0};      // the fallback plane's centre (:173-179)
  if (mode != 2) {
    // ---- stage 1: plane records ----
    Ev e0{h, 0};
    e0.begin();
    VX_HIP(h, hipMemsetAsync(c1.cnt, 0, (N + 1) * 4, h->s));
    VX_HIP(h, hipMemsetAsync(d_big, 0, (N + 1) * 4, h->s));
    VX_HIP(h, hipMemsetAsync(d_isp, 0, (slots + 1) * 4, h->s));
    hipLaunchKernelGGL(cn_key_kernel, dim3(nb), dim3(BLK), 0, h->s, (const double*)d_xyz, (long long)n, p->voxel_size, c1.key, c1.idx, h->flags);
    VX_HIP(h, hipGetLastError());
    VX_HIP(h, vxu::sort(c1.temp, c1.key, c1.key_s, c1.idx, c1.idx_s, N, 3 * KEY_BITS, h->s));
    VX_HIP(h, vxu::encode(c1.temp, c1.key_s, N, c1.ukey, c1.cnt, h->d_runs, h->s));
    VX_HIP(h, vxu::scan(c1.temp, c1.cnt, c1.ptr, N + 1, h->s));
    hipLaunchKernelGGL(cn_big_kernel, dim3(nb), dim3(BLK), 0, h->s, (const unsigned int*)c1.cnt, (const unsigned int*)h->d_runs, p->voxel_init_num, d_big);
    VX_HIP(h, hipGetLastError());
    VX_HIP(h, vxu::scan(c1.temp, d_big, d_slot, N + 1, h->s));
    hipLaunchKernelGGL(cn_plane_kernel, dim3(nb), dim3(BLK), 0, h->s, (const double*)d_xyz, (const unsigned int*)c1.idx_s, (const unsigned int*)c1.ptr, (const unsigned int*)h->d_runs,
                       (const unsigned int*)d_big, (const unsigned int*)d_slot, p->plane_detection_thre, d_recs, d_isp);
    VX_HIP(h, hipGetLastError());
    VX_HIP(h, vxu::scan(c1.temp, d_isp, d_ppos, slots + 1, h->s));
    hipLaunchKernelGGL(cn_plane_scatter, dim3(blocks_for((long long)slots, BLK)), dim3(BLK), 0, h->s, (const double*)d_recs, (const unsigned int*)d_isp, (const unsigned int*)d_ppos,
                       (long long)slots, h->d_planes, h->flags);
    VX_HIP(h, hipGetLastError());
    if (mode == 1) { VX_HIP(h, hipMemcpyAsync(first, d_xyz, 24, hipMemcpyDeviceToHost, h->s)); h->stats[2] += 24; }
    else std::memcpy(first, src, 24);
    e0.end();
    h->stats[0] += 9;
    if (const int rc = wait(h)) return rc;
    h->stats[2] += 8;
    if (((volatile unsigned int*)h->flags)[0]) return fail(h, VXBA_ERR_ARG, "corner_extract: a point is not finite or lies 2^20 voxels or more from the origin");
    const unsigned int P = ((volatile unsigned int*)h->flags)[1];
    if (P > (unsigned int)MAX_PLANES) return fail(h, VXBA_ERR_ARG, "corner_extract: more than 16384 plane voxels");
    // ---- stage 2: pair tests, labels, groups ----
    planes.resize((size_t)REC * P);
    if (P) { VX_HIP(h, hipMemcpyAsync(planes.data(), h->d_planes, planes.size() * 8, hipMemcpyDeviceToHost, h->s)); h->stats[2] += (int64_t)planes.size() * 8; }
    std::vector<unsigned long long> bits;
    int W = 0;
    Ev e1{h, 1};
    e1.begin();
    if (const int rc = pair_bits(h, planes, false, p, bits, &W)) return rc;
    e1.end();
    label_rows((int)P, [&](int i, int j) { return (bits[(size_t)i * W + j / 64] >> (j % 64)) & 1ull; }, plane_id);
    fold_groups(planes, plane_id, false, proj_list);
    // ---- stage 3: sort, merge_plane, sort ----
    sort_by_size(proj_list);
    Ev e2{h, 2};
    e2.begin();
    if (const int rc = pair_bits(h, proj_list, true, p, bits, &W)) return rc;
    e2.end();
    const int M = (int)(proj_list.size() / REC);
    if (M == 0) {
      proj_list.assign(REC, 0.0);
      for (int k = 0; k < 3; k++) proj_list[k] = first[k];
      proj_list[R_NRM + 2] = 1.0;
    } else if (M > 1) {
      std::vector<int> id2;
      std::vector<double> merged;
      label_rows(M, [&](int i, int j) { return (bits[(size_t)i * W + j / 64] >> (j % 64)) & 1ull; }, id2);
      fold_groups(proj_list, id2, true, merged);
      proj_list.swap(merged);
      sort_by_size(proj_list);
    }
  } else {
    proj_list.assign((size_t)REC * m, 0.0);
    for (int64_t i = 0; i < m; i++)
      for (int k = 0; k < 3; k++) { proj_list[(size_t)REC * i + k] = centres[3 * i + k]; proj_list[(size_t)REC * i + R_NRM + k] = normals[3 * i + k]; }
  }

  // ---- stage 4: the gate ----
  const int M = (int)(proj_list.size() / REC);
  std::vector<double> nrm((size_t)3 * M);
  for (int i = 0; i < M; i++) for (int k = 0; k < 3; k++) nrm[3 * i + k] = proj_list[(size_t)REC * i + R_NRM + k];
  std::vector<int> used;
  gate_planes(M, nrm.data(), p->proj_plane_num, used);
  proj_used.assign((size_t)M, -1);
  const int U = (int)used.size();
  for (int u = 0; u < U; u++) {
    proj_used[used[u]] = u;
    make_proj(proj_list.data() + (size_t)REC * used[u], proj_list.data() + (size_t)REC * used[u] + R_NRM, &h->h_proj[u]);
  }
  if (U == 0) return commit();

  // ---- stage 5: images ----
  ImgArgs a;
  a.res = p->proj_image_resolution; a.high_inc = p->proj_image_high_inc; a.dis_min = p->proj_dis_min; a.dis_max = p->proj_dis_max; a.summary_min = p->summary_min_thre;
  a.radius = p->non_max_suppression_radius; a.cut_num = cut_num; a.line_filter = p->line_filter_enable; a.touch_filter = p->touch_filter_enable; a.n_used = U;
  const size_t E = N * (size_t)U;
  VX_HIP(h, hipMemcpyAsync(h->d_proj, h->h_proj, sizeof(Proj) * U, hipMemcpyHostToDevice, h->s));
  h->stats[3] += (int64_t)sizeof(Proj) * U;
  Ev e3{h, 3};
  e3.begin();
  hipLaunchKernelGGL(cn_project_kernel, dim3(nb, U), dim3(BLK), 0, h->s, (const double*)d_xyz, (long long)n, (const Proj*)h->d_proj, a, d_part, d_pcnt);
  VX_HIP(h, hipGetLastError());
  hipLaunchKernelGGL(cn_bounds_kernel, dim3(U), dim3(BLK), 0, h->s, (const double*)d_part, (const unsigned int*)d_pcnt, nb, a, h->d_img, h->h_img);
  VX_HIP(h, hipGetLastError());
  hipLaunchKernelGGL(cn_cellkey_kernel, dim3(nb, U), dim3(BLK), 0, h->s, (const double*)d_xyz, (long long)n, (const Proj*)h->d_proj, (const Img*)h->d_img, a, c2.key, c2.idx);
  VX_HIP(h, hipGetLastError());
  e3.end();
  Ev e4{h, 4};
  e4.begin();
  VX_HIP(h, hipMemsetAsync(c2.cnt, 0, (E + 1) * 4, h->s));
  VX_HIP(h, hipMemsetAsync(d_flag, 0, (E + 1) * 4, h->s));
  VX_HIP(h, vxu::sort(c2.temp, c2.key, c2.key_s, c2.idx, c2.idx_s, E, 54, h->s));
  VX_HIP(h, vxu::encode(c2.temp, c2.key_s, E, c2.ukey, c2.cnt, h->d_runs, h->s));
  VX_HIP(h, vxu::scan(c2.temp, c2.cnt, c2.ptr, E + 1, h->s));
  e4.end();
  Ev e5{h, 5};
  e5.begin();
  const unsigned eb = blocks_for((long long)E, BLK);
  hipLaunchKernelGGL(cn_cell_kernel, dim3(eb), dim3(BLK), 0, h->s, (const double*)d_xyz, (long long)n, (const Proj*)h->d_proj, a, (const unsigned long long*)c2.ukey,
                     (const unsigned int*)c2.idx_s, (const unsigned int*)c2.ptr, (const unsigned int*)h->d_runs, c_cnt, c_sx, c_sy, c_occ);
  VX_HIP(h, hipGetLastError());
  hipLaunchKernelGGL(cn_segment_kernel, dim3(eb), dim3(BLK), 0, h->s, (const unsigned long long*)c2.ukey, (const unsigned long long*)c_occ, (const unsigned int*)h->d_runs,
                     (const Img*)h->d_img, a, d_flag, d_win);
  VX_HIP(h, hipGetLastError());
  VX_HIP(h, vxu::scan(c2.temp, d_flag, d_fpos, E + 1, h->s));
  hipLaunchKernelGGL(cn_cand_scatter, dim3(eb), dim3(BLK), 0, h->s, (const unsigned long long*)c2.ukey, (const unsigned int*)h->d_runs, (const unsigned int*)d_flag,
                     (const unsigned int*)d_fpos, (long long)E, (const unsigned int*)d_win, (const unsigned int*)c_cnt, (const double*)c_sx, (const double*)c_sy,
                     (const unsigned long long*)c_occ, (const Proj*)h->d_proj, h->d_cand, h->d_ncand, h->flags);
  VX_HIP(h, hipGetLastError());
  // ---- stage 6: suppression ----
  const float r2 = (float)(p->non_max_suppression_radius * p->non_max_suppression_radius);
  hipLaunchKernelGGL(cn_suppress_kernel, dim3(MAX_CAND / BLK), dim3(BLK), 0, h->s, h->d_cand, (const unsigned int*)h->d_ncand, r2);
  VX_HIP(h, hipGetLastError());
  e5.end();
  h->stats[0] += 11;
  if (const int rc = wait(h)) return rc;
  h->stats[2] += 8 + (int64_t)sizeof(Img) * U;
  for (int u = 0; u < U; u++) if (((volatile Img*)h->h_img)[u].too_big) return fail(h, VXBA_ERR_ARG, "corner_extract: an image axis of 2^24 cells or more");
  const unsigned int C = ((volatile unsigned int*)h->flags)[2];
  h->stats[4] = (int64_t)((volatile unsigned int*)h->flags)[3]; h->stats[5] = (int64_t)C;
  if (C > (unsigned int)MAX_CAND) return fail(h, VXBA_ERR_UNSUPPORTED, "corner_extract: more than 65536 candidates ahead of the suppression");
  cand.resize(C);
  if (C) {
    VX_HIP(h, hipMemcpyAsync(cand.data(), h->d_cand, sizeof(Cand) * C, hipMemcpyDeviceToHost, h->s));
    h->stats[2] += (int64_t)sizeof(Cand) * C;
  }
  if (const int rc = wait(h)) return rc;
  // ---- stage 7: the kept candidates in order, and the cut ----
  std::vector<int> kept, summary(C);
  for (unsigned int i = 0; i < C; i++) { summary[i] = cand[i].summary; if (cand[i].keep) kept.push_back((int)i); }
  cut_order(kept, summary, p->useful_corner_num, out);
  if (h->profiling) h->ev_valid = (mode != 2);
  return commit();
}

}  // namespace

extern "C" {

void vxba_corner_default_params(vxba_corner_params* p, int is_high_fly) {
  if (!p) return;
  const bool f = is_high_fly != 0;
  p->useful_corner_num = f ? 200 : 100;
  p->plane_merge_normal_thre = f ? 0.3 : 0.1;
  p->plane_merge_dis_thre = f ? 0.6 : 0.3;
  p->plane_detection_thre = f ? 0.05 : 0.01;
  p->voxel_size = f ? 2.0 : 1.0;
  p->voxel_init_num = 10;
  p->proj_plane_num = f ? 1 : 2;
  p->proj_image_resolution = 0.5;
  p->proj_image_high_inc = f ? 0.2 : 0.1;
  p->proj_dis_min = 0.0;
  p->proj_dis_max = f ? 10.0 : 5.0;
  p->summary_min_thre = f ? 6.0 : 10.0;
  p->line_filter_enable = f ? 0 : 1;
  p->touch_filter_enable = 0;
  p->non_max_suppression_radius = f ? 3.0 : 2.0;
}

int vxba_corner_create(int device, vxba_corner** out) {
  if (!out) return VXBA_ERR_ARG;
  *out = nullptr;
  if (const int rc = vxu::select_device(device)) return rc;
  vxba_corner* h = new vxba_corner();
  h->device = device;
  if (h->s.create() != hipSuccess || h->flags.reserve(16) != hipSuccess || h->h_img.reserve(MAX_USED) != hipSuccess || h->h_proj.reserve(MAX_USED) != hipSuccess ||
      h->d_proj.reserve(MAX_USED) != hipSuccess || h->d_img.reserve(MAX_USED) != hipSuccess || h->d_runs.reserve(64) != hipSuccess || h->d_ncand.reserve(64) != hipSuccess ||
      h->d_planes.reserve((size_t)REC * MAX_PLANES) != hipSuccess || h->d_cand.reserve(MAX_CAND) != hipSuccess) {
    delete h;
    return VXBA_ERR_HIP;
  }
  *out = h;
  return VXBA_OK;
}

int vxba_corner_destroy(vxba_corner* h) {
  if (!h) return VXBA_OK;
  hipSetDevice(h->device);
  if (h->s) hipStreamSynchronize(h->s);
  h->work.release();
  delete h;
  return VXBA_OK;
}

const char* vxba_corner_last_error(const vxba_corner* h) { return h ? h->err.c_str() : "null handle"; }

int vxba_corner_extract(vxba_corner* h, int64_t n, const double* xyz, const vxba_corner_params* params, int64_t* n_corners) {
  return extract(h, 0, n, xyz, 0, nullptr, nullptr, params, n_corners);
}

int vxba_corner_extract_device(vxba_corner* h, int64_t n, const float* d_xyz, const vxba_corner_params* params, int64_t* n_corners) {
  return extract(h, 1, n, d_xyz, 0, nullptr, nullptr, params, n_corners);
}

int vxba_corner_extract_with_planes(vxba_corner* h, int64_t n, const double* xyz, int64_t m, const double* centres, const double* normals, const vxba_corner_params* params,
                                    int64_t* n_corners) {
  return extract(h, 2, n, xyz, m, centres, normals, params, n_corners);
}

int vxba_corner_read(vxba_corner* h, double* locations, uint64_t* occupancy, int32_t* summary) {
  if (!h) return VXBA_ERR_ARG;
  for (size_t k = 0; k < h->out.size(); k++) {
    const Cand& c = h->cand[(size_t)h->out[k]];
    if (locations) { locations[3 * k] = c.loc[0]; locations[3 * k + 1] = c.loc[1]; locations[3 * k + 2] = c.loc[2]; }
    if (occupancy) occupancy[k] = c.occ;
    if (summary) summary[k] = c.summary;
  }
  return VXBA_OK;
}

int vxba_corner_planes(vxba_corner* h, int64_t* n_planes, double* records, int32_t* labels) {
  if (!h) return VXBA_ERR_ARG;
  if (n_planes) *n_planes = (int64_t)h->plane_id.size();
  if (records && !h->planes.empty()) std::memcpy(records, h->planes.data(), h->planes.size() * sizeof(double));
  if (labels) for (size_t k = 0; k < h->plane_id.size(); k++) labels[k] = h->plane_id[k];
  return VXBA_OK;
}

int vxba_corner_projection_planes(vxba_corner* h, int64_t* n_planes, double* records, int32_t* used) {
  if (!h) return VXBA_ERR_ARG;
  if (n_planes) *n_planes = (int64_t)h->proj_used.size();
  if (records && !h->proj_list.empty()) std::memcpy(records, h->proj_list.data(), h->proj_list.size() * sizeof(double));
  if (used) for (size_t k = 0; k < h->proj_used.size(); k++) used[k] = h->proj_used[k];
  return VXBA_OK;
}

int vxba_corner_candidates(vxba_corner* h, int64_t* n_candidates, int32_t* ints, uint64_t* occupancy, double* locations) {
  if (!h) return VXBA_ERR_ARG;
  if (n_candidates) *n_candidates = (int64_t)h->cand.size();
  for (size_t k = 0; k < h->cand.size(); k++) {
    const Cand& c = h->cand[k];
    if (ints) { int32_t* r = ints + VXBA_CORNER_CAND_INTS * k; r[0] = c.plane; r[1] = c.cx; r[2] = c.cy; r[3] = c.count; r[4] = c.summary; r[5] = c.keep; }
    if (occupancy) occupancy[k] = c.occ;
    if (locations) { locations[3 * k] = c.loc[0]; locations[3 * k + 1] = c.loc[1]; locations[3 * k + 2] = c.loc[2]; }
  }
  return VXBA_OK;
}

int vxba_corner_stats(const vxba_corner* h, int64_t out[6]) {
  if (!h || !out) return VXBA_ERR_ARG;
  for (int k = 0; k < 6; k++) out[k] = h->stats[k];
  return VXBA_OK;
}

int vxba_corner_set_profiling(vxba_corner* h, int enable) {
  if (!h) return VXBA_ERR_ARG;
  VX_HIP(h, hipSetDevice(h->device));
  for (vxu::Event& e : h->ev) if (enable) VX_HIP(h, e.create());
  h->profiling = enable != 0;
  h->ev_valid = false;
  return VXBA_OK;
}

int vxba_corner_stage_times(vxba_corner* h, double ms[VXBA_CORNER_STAGES]) {
  if (!h || !ms) return VXBA_ERR_ARG;
  if (!h->ev_valid) return fail(h, VXBA_ERR_STATE, "corner_stage_times: the last extract was not profiled, held no points or used no plane");
  for (int k = 0; k < VXBA_CORNER_STAGES; k++) {
    float t = 0.f;
    VX_HIP(h, hipEventElapsedTime(&t, h->ev[2 * k], h->ev[2 * k + 1]));
    ms[k] = (double)t;
  }
  return VXBA_OK;
}

}  // extern "C"
