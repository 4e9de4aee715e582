// Arithmetic of the corner extraction (include/vxba.h: vxba_corner_*), host + device: vxba_corner.hip runs it on the GPU and in its host shell,
// tests/hostmath/corner_hostcheck.cpp compiles the same text with g++ for the CPU suite.
//
// Reference: STDescManager::GenerateSTDescs without generate_std -- init_voxel_map / init_plane (BTC.cpp:279-321, 90-139), get_project_plane
// (:340-458), merge_plane (:460-569), binary_extractor (:571-611), extract_binary (:613-924), non_maxi_suppression (:926-977).
// Association (what tests/_corner_ref.py restates in numpy): float64 throughout, every 3-term inner product is (a0 b0 + a1 b1) + a2 b2, nothing is
// fused.  Both translation units that include this file are compiled WITHOUT floating-point contraction.
//
// Layout: a plane record is REC = 16 doubles [c 3 | cov xx xy xz yy yz zz | N | normal 3 | d | radius | lambda_min].
#pragma once
#include <math.h>
#include <stdint.h>

#include <algorithm>
#include <vector>

#include "vxba_math.hpp"

#if defined(__HIPCC__)
#define VXC_HD __host__ __device__ __forceinline__
#else
#define VXC_HD inline
#endif

namespace vxcn {

constexpr int KEY_BITS = 21;
constexpr long long KEY_OFF = 1ll << 20;
constexpr int REC = 16;
constexpr int R_C = 0, R_COV = 3, R_N = 9, R_NRM = 10, R_D = 13, R_RAD = 14, R_LMIN = 15;
constexpr int SEG = 5;                               // segmen_base_num (:717)
constexpr int MAX_USED = 8;                          // proj_plane_num at most
constexpr long long MAX_AXIS = 1ll << 24;            // cells per image axis, exclusive
constexpr unsigned long long CELL_NONE = 15ull << 50;   // the key of a (point, plane) pair that is in no image: sorts behind every cell

VXC_HD double dot3(const double* a, const double* b) { return (a[0] * b[0] + a[1] * b[1]) + a[2] * b[2]; }

// voxel coordinate of :287-295: divide, subtract 1.0 where negative, truncate; false where not finite or outside (-2^20, 2^20)
VXC_HD bool voxel_key(const double* q, double vs, unsigned long long* key) {
  unsigned long long k = 0;
  bool ok = true;
  for (int j = 0; j < 3; j++) {
    double l = q[j] / vs;
    long long pos = 0;
    if (fabs(l) < (double)(KEY_OFF - 2)) {      // false for values that are not finite, too
      if (l < 0) l -= 1.0;
      pos = (long long)l;
    } else {
      ok = false;
    }
    k = (k << KEY_BITS) | (unsigned long long)(pos + KEY_OFF);
  }
  *key = k;
  return ok;
}

// normal (sign: the component of largest magnitude, the first of equals, is positive), d = -n.c, radius = sqrt(lambda_max), lambda_min from the
// record's covariance and centre (:110-129, :429-443)
VXC_HD void solve_record(double* r) {
  double lam[3], U[9];
  vxm::eig_sym3(r + R_COV, lam, U);
  double nx = U[0], ny = U[3], nz = U[6];
  const double ax = fabs(nx), ay = fabs(ny), az = fabs(nz);
  const double lead = (ax >= ay && ax >= az) ? nx : (ay >= az ? ny : nz);
  if (lead < 0) { nx = -nx; ny = -ny; nz = -nz; }
  r[R_NRM] = nx; r[R_NRM + 1] = ny; r[R_NRM + 2] = nz;
  r[R_D] = -((nx * r[0] + ny * r[1]) + nz * r[2]);
  r[R_RAD] = sqrt(lam[2]);
  r[R_LMIN] = lam[0];
}

// sums of p (v) and p p^T (P, xx xy xz yy yz zz) over N points -> the record; true when it is a plane (:96-139)
VXC_HD bool record_from_sums(const double* P, const double* v, long long N, double thre, double* r) {
  const double Nd = (double)N;
  r[0] = v[0] / Nd; r[1] = v[1] / Nd; r[2] = v[2] / Nd;
  r[3] = P[0] / Nd - r[0] * r[0]; r[4] = P[1] / Nd - r[0] * r[1]; r[5] = P[2] / Nd - r[0] * r[2];
  r[6] = P[3] / Nd - r[1] * r[1]; r[7] = P[4] / Nd - r[1] * r[2]; r[8] = P[5] / Nd - r[2] * r[2];
  r[R_N] = Nd;
  solve_record(r);
  return r[R_LMIN] < thre;
}

// the reference's update of (cov, c, N) of a by b (:405-424); a's normal, d and radius are stale afterwards
VXC_HD void fold_record(double* a, const double* b) {
  const double Na = a[R_N], Nb = b[R_N], Ns = Na + Nb;
  const int I[6] = {0, 0, 0, 1, 1, 2}, J[6] = {0, 1, 2, 1, 2, 2};
  double m[3];
  for (int k = 0; k < 3; k++) m[k] = (a[k] * Na + b[k] * Nb) / Ns;
  double cov[6];
  for (int k = 0; k < 6; k++) {
    const double p1 = (a[R_COV + k] + a[I[k]] * a[J[k]]) * Na;
    const double p2 = (b[R_COV + k] + b[I[k]] * b[J[k]]) * Nb;
    cov[k] = (p1 + p2) / Ns - m[I[k]] * m[J[k]];
  }
  for (int k = 0; k < 6; k++) a[R_COV + k] = cov[k];
  for (int k = 0; k < 3; k++) a[k] = m[k];
  a[R_N] = Ns;
}

// the pair test of get_project_plane and merge_plane (:357-370)
VXC_HD bool pair_test(const double* a, const double* b, double normal_thre, double dis_thre) {
  const double* na = a + R_NRM;
  const double* nb = b + R_NRM;
  const double d0 = na[0] - nb[0], d1 = na[1] - nb[1], d2 = na[2] - nb[2];
  const double s0 = na[0] + nb[0], s1 = na[1] + nb[1], s2 = na[2] + nb[2];
  const double nd = sqrt((d0 * d0 + d1 * d1) + d2 * d2), ns = sqrt((s0 * s0 + s1 * s1) + s2 * s2);
  const double dis1 = fabs(dot3(na, b) + a[R_D]);
  const double dis2 = fabs(dot3(nb, a) + b[R_D]);
  return (nd < normal_thre || ns < normal_thre) && dis1 < dis_thre && dis2 < dis_thre;
}

// a projection plane as the image kernels read it
struct Proj {
  double c[3], n[3], x[3], y[3], D, dx, dy;
};

// x_axis from (1, 1, -(A+B)/C) with its two fall-backs, y_axis = n x x_axis, both normalised (:626-654)
VXC_HD void make_proj(const double* c, const double* n, Proj* p) {
  const double A = n[0], B = n[1], Cc = n[2];
  double x[3] = {1, 1, 0};
  if (Cc != 0) x[2] = -(A + B) / Cc;
  else if (B != 0) x[1] = -A / B;
  else { x[0] = 0; x[1] = 1; }
  const double xn = sqrt((x[0] * x[0] + x[1] * x[1]) + x[2] * x[2]);
  x[0] /= xn; x[1] /= xn; x[2] /= xn;
  double y[3] = {n[1] * x[2] - n[2] * x[1], n[2] * x[0] - n[0] * x[2], n[0] * x[1] - n[1] * x[0]};
  const double yn = sqrt((y[0] * y[0] + y[1] * y[1]) + y[2] * y[2]);
  y[0] /= yn; y[1] /= yn; y[2] /= yn;
  for (int k = 0; k < 3; k++) { p->c[k] = c[k]; p->n[k] = n[k]; p->x[k] = x[k]; p->y[k] = y[k]; }
  p->D = -dot3(n, c);
  p->dx = -dot3(x, c);
  p->dy = -dot3(y, c);
}

// dis, project_x (along y_axis) and project_y (along x_axis) of one point (:660-689); true when dis_min <= dis <= dis_max
VXC_HD bool project_point(const Proj& p, const double* q, double dis_min, double dis_max, double* dis, double* px, double* py) {
  const double A = p.n[0], B = p.n[1], Cc = p.n[2], D = p.D, x = q[0], y = q[1], z = q[2];
  const double d = fabs(((x * A + y * B) + z * Cc) + D);
  *dis = d;
  if (!(d >= dis_min && d <= dis_max)) return false;
  const double den = (A * A + B * B) + Cc * Cc;
  const double c0 = (-A * ((B * y + Cc * z) + D) + x * (B * B + Cc * Cc)) / den;
  const double c1 = (-B * ((A * x + Cc * z) + D) + y * (A * A + Cc * Cc)) / den;
  const double c2 = (-Cc * ((A * x + B * y) + D) + z * (A * A + B * B)) / den;
  *px = ((c0 * p.y[0] + c1 * p.y[1]) + c2 * p.y[2]) + p.dy;
  *py = ((c0 * p.x[0] + c1 * p.x[1]) + c2 * p.x[2]) + p.dx;
  return true;
}

// the image of one used plane (:695-722)
struct Img {
  double min_x, min_y;
  int x_len, y_len, x_seg, y_seg;
  int valid;        // more than five points kept
  int too_big;      // an axis of 2^24 cells or more
  long long kept;
};

VXC_HD void make_img(double lo_x, double hi_x, double lo_y, double hi_y, long long kept, double res, Img* g) {
  const double min_x = lo_x < 10.0 ? lo_x : 10.0, max_x = hi_x > -10.0 ? hi_x : -10.0;
  const double min_y = lo_y < 10.0 ? lo_y : 10.0, max_y = hi_y > -10.0 ? hi_y : -10.0;
  g->min_x = min_x; g->min_y = min_y; g->kept = kept;
  g->valid = kept > 5 ? 1 : 0;
  g->too_big = 0;
  g->x_len = g->y_len = g->x_seg = g->y_seg = 0;
  if (!g->valid) return;
  const double seg_len = SEG * res;
  const double wx = (max_x - min_x) / res + SEG, wy = (max_y - min_y) / res + SEG;
  if (!(wx < (double)MAX_AXIS && wy < (double)MAX_AXIS)) { g->too_big = 1; g->valid = 0; return; }
  g->x_seg = (int)((max_x - min_x) / seg_len + 1);
  g->y_seg = (int)((max_y - min_y) / seg_len + 1);
  g->x_len = (int)wx;
  g->y_len = (int)wy;
}

VXC_HD int cell_index(double p, double lo, double res) { return (int)((p - lo) / res); }
VXC_HD int height_bin(double dis, double dis_min, double high_inc) { return (int)((dis - dis_min) / high_inc); }

// sorted key order = (plane, segment x, segment y, x in segment, y in segment): the reference's scan order (:803-820)
VXC_HD unsigned long long cell_key(int plane, int cx, int cy) {
  return ((unsigned long long)plane << 50) | ((unsigned long long)(cx / SEG) << 28) | ((unsigned long long)(cy / SEG) << 6) | ((unsigned long long)(cx % SEG) << 3) |
         (unsigned long long)(cy % SEG);
}
VXC_HD int key_plane(unsigned long long k) { return (int)(k >> 50); }
VXC_HD int key_cx(unsigned long long k) { return (int)((k >> 28) & 0x3fffff) * SEG + (int)((k >> 3) & 7); }
VXC_HD int key_cy(unsigned long long k) { return (int)((k >> 6) & 0x3fffff) * SEG + (int)(k & 7); }

// one direction of the line filter (:867-889): s the winner's summary, s1 / s2 its two neighbours'
VXC_HD bool line_hit(int s, int s1, int s2) {
  const double v = (double)s, a = (double)s1, b = (double)s2, thr = v - 3;
  bool hit = false;
  if (a >= thr && b >= 0.5 * v) hit = true;
  if (b >= thr && a >= 0.5 * v) hit = true;
  if (a >= thr && b >= thr) hit = true;
  return hit;
}

// non_maxi_suppression's distance (:926-965): locations rounded to float32, float32 squared distance < float32(radius^2)
VXC_HD bool nms_near(const float* a, const float* b, float r2) {
  const float dx = a[0] - b[0], dy = a[1] - b[1], dz = a[2] - b[2];
  return (dx * dx + dy * dy) + dz * dz < r2;
}

// ---- the sequential parts, on the host ---------------------------------------------------------------------------------------------

// the reference's labelling (:350-382): outer index from the last row down to 1, inner from 0 up to outer - 1; pred(outer, inner)
template <class Pred>
inline void label_rows(int P, Pred pred, std::vector<int>& id) {
  id.assign((size_t)P, 0);
  int cur = 1;
  for (int i = P - 1; i >= 1; i--)
    for (int j = 0; j < i; j++) {
      if (!pred(i, j)) continue;
      if (id[i] == 0 && id[j] == 0) { id[i] = cur; id[j] = cur; cur++; }
      else if (id[i] == 0 && id[j] != 0) id[i] = id[j];
      else if (id[i] != 0 && id[j] == 0) id[j] = id[i];
    }
}

// groups in ascending i (:386-456, :500-568): a group folds every other member ascending and is re-solved once; keep_unlabelled: merge_plane's
// rule for id-0 rows (kept as they are at their position), false: get_project_plane's (dropped)
inline void fold_groups(const std::vector<double>& rows, const std::vector<int>& id, bool keep_unlabelled, std::vector<double>& out) {
  const int P = (int)id.size();
  out.clear();
  std::vector<int> seen;
  for (int i = 0; i < P; i++) {
    if (std::find(seen.begin(), seen.end(), id[i]) != seen.end()) continue;
    if (id[i] == 0) {
      if (keep_unlabelled) out.insert(out.end(), rows.begin() + (size_t)REC * i, rows.begin() + (size_t)REC * (i + 1));
      continue;
    }
    double r[REC];
    for (int k = 0; k < REC; k++) r[k] = rows[(size_t)REC * i + k];
    bool merged = false;
    for (int j = 0; j < P; j++) {
      if (j == i || id[j] != id[i]) continue;
      merged = true;
      fold_record(r, rows.data() + (size_t)REC * j);
    }
    if (merged) {
      solve_record(r);
      seen.push_back(id[i]);
      out.insert(out.end(), r, r + REC);
    }
  }
}

// stable sort by N descending (:181, :183 with ties keeping their order)
inline void sort_by_size(std::vector<double>& rows) {
  const int P = (int)(rows.size() / REC);
  std::vector<int> ord((size_t)P);
  for (int i = 0; i < P; i++) ord[i] = i;
  std::stable_sort(ord.begin(), ord.end(), [&](int a, int b) { return rows[(size_t)REC * a + R_N] > rows[(size_t)REC * b + R_N]; });
  std::vector<double> out(rows.size());
  for (int i = 0; i < P; i++) std::copy(rows.begin() + (size_t)REC * ord[i], rows.begin() + (size_t)REC * (ord[i] + 1), out.begin() + (size_t)REC * i);
  rows.swap(out);
}

// the gate of binary_extractor (:578-598) over centres / normals (m x 3 each): the indices of the planes used, proj_plane_num at most
inline void gate_planes(int m, const double* normals, int proj_plane_num, std::vector<int>& used) {
  used.clear();
  double last[3] = {0, 0, 0};
  for (int i = 0; i < m; i++) {
    const double* n = normals + 3 * i;
    const double d0 = n[0] - last[0], d1 = n[1] - last[1], d2 = n[2] - last[2];
    const double s0 = n[0] + last[0], s1 = n[1] + last[1], s2 = n[2] + last[2];
    if (sqrt((d0 * d0 + d1 * d1) + d2 * d2) < 0.3 || sqrt((s0 * s0 + s1 * s1) + s2 * s2) > 0.3) {
      last[0] = n[0]; last[1] = n[1]; last[2] = n[2];
      used.push_back(i);
      if ((int)used.size() == proj_plane_num) break;
    }
  }
}

// the cut (:601-609): kept candidates in order; with useful <= count a stable sort by summary descending and the first `useful`
inline void cut_order(const std::vector<int>& kept, const std::vector<int>& summary, int useful, std::vector<int>& out) {
  out = kept;
  if ((size_t)useful > kept.size()) return;
  std::stable_sort(out.begin(), out.end(), [&](int a, int b) { return summary[a] > summary[b]; });
  out.resize((size_t)useful);
}

}  // namespace vxcn
