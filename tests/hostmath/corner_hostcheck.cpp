// Host build of csrc/vxba_corner_math.hpp for tests/test_corner_cpu.py: the whole extraction on the CPU with the arithmetic the kernels run, the
// per-point and per-cell work as plain loops in the order the kernels replay it.  Built by the test with g++ -ffp-contract=off.
#include <cstdint>
#include <cstring>
#include <map>
#include <vector>

#include "../../voxel-slam_amd/csrc/vxba_corner_math.hpp"

using namespace vxcn;

namespace {

struct Params {      // the fields of vxba_corner_params, all as doubles, in the struct's order
  double useful_corner_num, plane_merge_normal_thre, plane_merge_dis_thre, plane_detection_thre, voxel_size, voxel_init_num, proj_plane_num, proj_image_resolution,
      proj_image_high_inc, proj_dis_min, proj_dis_max, summary_min_thre, line_filter_enable, touch_filter_enable, non_max_suppression_radius;
};

struct Cell { unsigned int cnt = 0; double sx = 0, sy = 0; unsigned long long occ = 0; };

struct Result {
  std::vector<double> planes, proj;
  std::vector<int> labels, used;
  std::vector<int> cand_ints;      // 6 per candidate
  std::vector<unsigned long long> cand_occ;
  std::vector<double> cand_loc;
  std::vector<int> out;
} R;

void label_by_test(const std::vector<double>& rows, const Params& p, std::vector<int>& id) {
  const int P = (int)(rows.size() / REC);
  label_rows(P, [&](int i, int j) { return pair_test(rows.data() + (size_t)REC * i, rows.data() + (size_t)REC * j, p.plane_merge_normal_thre, p.plane_merge_dis_thre); }, id);
}

int summary_at(const std::map<unsigned long long, Cell>& cells, int u, int cx, int cy) {
  if (cx < 0 || cy < 0) return 0;
  auto it = cells.find(cell_key(u, cx, cy));
  return it == cells.end() ? 0 : __builtin_popcountll(it->second.occ);
}

}  // namespace

extern "C" {

// returns the number of corners; m > 0: stages 4-7 on the caller's planes
int cnh_extract(int n, const double* xyz, const double* prm, int m, const double* centres, const double* normals) {
  Params p;
  std::memcpy(&p, prm, sizeof p);
  R = Result();
  if (n == 0) return 0;
  const int cut_num = (int)((p.proj_dis_max - p.proj_dis_min) / p.proj_image_high_inc);
  if (m <= 0) {
    std::map<unsigned long long, std::vector<int>> vox;
    for (int i = 0; i < n; i++) {
      unsigned long long k;
      if (!voxel_key(xyz + 3 * i, p.voxel_size, &k)) return -1;
      vox[k].push_back(i);
    }
    for (auto& kv : vox) {
      if ((long long)kv.second.size() <= (long long)p.voxel_init_num) continue;
      double P[6] = {0, 0, 0, 0, 0, 0}, v[3] = {0, 0, 0};
      for (int i : kv.second) {
        const double x = xyz[3 * i], y = xyz[3 * i + 1], z = xyz[3 * i + 2];
        P[0] += x * x; P[1] += x * y; P[2] += x * z; P[3] += y * y; P[4] += y * z; P[5] += z * z;
        v[0] += x; v[1] += y; v[2] += z;
      }
      double rec[REC];
      if (record_from_sums(P, v, (long long)kv.second.size(), p.plane_detection_thre, rec)) R.planes.insert(R.planes.end(), rec, rec + REC);
    }
    label_by_test(R.planes, p, R.labels);
    fold_groups(R.planes, R.labels, false, R.proj);
    sort_by_size(R.proj);
    const int M = (int)(R.proj.size() / REC);
    if (M == 0) {
      R.proj.assign(REC, 0.0);
      for (int k = 0; k < 3; k++) R.proj[k] = xyz[k];
      R.proj[R_NRM + 2] = 1.0;
    } else if (M > 1) {
      std::vector<int> id2;
      std::vector<double> merged;
      label_by_test(R.proj, p, id2);
      fold_groups(R.proj, id2, true, merged);
      R.proj.swap(merged);
      sort_by_size(R.proj);
    }
  } else {
    R.proj.assign((size_t)REC * m, 0.0);
    for (int i = 0; i < m; i++)
      for (int k = 0; k < 3; k++) { R.proj[(size_t)REC * i + k] = centres[3 * i + k]; R.proj[(size_t)REC * i + R_NRM + k] = normals[3 * i + k]; }
  }
  const int M = (int)(R.proj.size() / REC);
  std::vector<double> nrm((size_t)3 * M);
  for (int i = 0; i < M; i++) for (int k = 0; k < 3; k++) nrm[3 * i + k] = R.proj[(size_t)REC * i + R_NRM + k];
  std::vector<int> used;
  gate_planes(M, nrm.data(), (int)p.proj_plane_num, used);
  R.used.assign((size_t)M, -1);
  for (size_t u = 0; u < used.size(); u++) R.used[used[u]] = (int)u;

  for (size_t u = 0; u < used.size(); u++) {
    Proj pj;
    make_proj(R.proj.data() + (size_t)REC * used[u], R.proj.data() + (size_t)REC * used[u] + R_NRM, &pj);
    double lo_x = INFINITY, hi_x = -INFINITY, lo_y = INFINITY, hi_y = -INFINITY;
    long long kept = 0;
    for (int i = 0; i < n; i++) {
      double dis, px, py;
      if (!project_point(pj, xyz + 3 * i, p.proj_dis_min, p.proj_dis_max, &dis, &px, &py)) continue;
      kept++;
      lo_x = fmin(lo_x, px); hi_x = fmax(hi_x, px); lo_y = fmin(lo_y, py); hi_y = fmax(hi_y, py);
    }
    Img g;
    make_img(lo_x, hi_x, lo_y, hi_y, kept, p.proj_image_resolution, &g);
    if (g.too_big) return -2;
    if (!g.valid) continue;
    std::map<unsigned long long, Cell> cells;
    for (int i = 0; i < n; i++) {
      double dis, px, py;
      if (!project_point(pj, xyz + 3 * i, p.proj_dis_min, p.proj_dis_max, &dis, &px, &py)) continue;
      Cell& c = cells[cell_key((int)u, cell_index(px, g.min_x, p.proj_image_resolution), cell_index(py, g.min_y, p.proj_image_resolution))];
      c.cnt++; c.sx += px; c.sy += py;
      const int b = height_bin(dis, p.proj_dis_min, p.proj_image_high_inc);
      if (b >= 0 && b < cut_num) c.occ |= 1ull << b;
    }
    for (auto it = cells.begin(); it != cells.end();) {
      const unsigned long long seg = it->first >> 6;
      int best = 0;
      auto bt = it;
      for (; it != cells.end() && (it->first >> 6) == seg; ++it) {
        const int s = __builtin_popcountll(it->second.occ);
        if (s > best) { best = s; bt = it; }
      }
      if (best == 0 || !((double)best >= p.summary_min_thre)) continue;
      const Cell& w = bt->second;
      if (p.touch_filter_enable != 0 && !(w.occ & 15ull)) continue;
      const int cx = key_cx(bt->first), cy = key_cy(bt->first), uu = (int)u;
      if (cx / SEG >= g.x_seg || cy / SEG >= g.y_seg) continue;
      if (cx <= 0 || cx >= g.x_len - 1 || cy <= 0 || cy >= g.y_len - 1) continue;
      if (p.line_filter_enable != 0) {
        bool hit = false;
        hit |= line_hit(best, summary_at(cells, uu, cx, cy + 1), summary_at(cells, uu, cx, cy - 1));
        hit |= line_hit(best, summary_at(cells, uu, cx + 1, cy), summary_at(cells, uu, cx - 1, cy));
        hit |= line_hit(best, summary_at(cells, uu, cx + 1, cy + 1), summary_at(cells, uu, cx - 1, cy - 1));
        hit |= line_hit(best, summary_at(cells, uu, cx + 1, cy - 1), summary_at(cells, uu, cx - 1, cy + 1));
        if (hit) continue;
      }
      const double px = w.sx / (double)w.cnt, py = w.sy / (double)w.cnt;
      for (int d = 0; d < 3; d++) R.cand_loc.push_back((py * pj.x[d] + px * pj.y[d]) + pj.c[d]);
      R.cand_occ.push_back(w.occ);
      const int row[6] = {uu, cx, cy, (int)w.cnt, best, 1};
      R.cand_ints.insert(R.cand_ints.end(), row, row + 6);
    }
  }
  const int Cn = (int)R.cand_occ.size();
  const float r2 = (float)(p.non_max_suppression_radius * p.non_max_suppression_radius);
  std::vector<int> kept, summary((size_t)Cn);
  for (int i = 0; i < Cn; i++) {
    summary[i] = R.cand_ints[6 * i + 4];
    const float a[3] = {(float)R.cand_loc[3 * i], (float)R.cand_loc[3 * i + 1], (float)R.cand_loc[3 * i + 2]};
    int keep = 1;
    for (int j = 0; j < Cn; j++) {
      const float b[3] = {(float)R.cand_loc[3 * j], (float)R.cand_loc[3 * j + 1], (float)R.cand_loc[3 * j + 2]};
      if (j != i && nms_near(a, b, r2) && R.cand_ints[6 * j + 4] >= R.cand_ints[6 * i + 4]) keep = 0;
    }
    R.cand_ints[6 * i + 5] = keep;
    if (keep) kept.push_back(i);
  }
  cut_order(kept, summary, (int)p.useful_corner_num, R.out);
  return (int)R.out.size();
}

void cnh_counts(int* out) { out[0] = (int)R.labels.size(); out[1] = (int)R.used.size(); out[2] = (int)R.cand_occ.size(); out[3] = (int)R.out.size(); }

void cnh_read(double* planes, int* labels, double* proj, int* used, int* cand_ints, unsigned long long* cand_occ, double* cand_loc, int* out) {
  std::memcpy(planes, R.planes.data(), R.planes.size() * 8);
  std::memcpy(labels, R.labels.data(), R.labels.size() * 4);
  std::memcpy(proj, R.proj.data(), R.proj.size() * 8);
  std::memcpy(used, R.used.data(), R.used.size() * 4);
  std::memcpy(cand_ints, R.cand_ints.data(), R.cand_ints.size() * 4);
  std::memcpy(cand_occ, R.cand_occ.data(), R.cand_occ.size() * 8);
  std::memcpy(cand_loc, R.cand_loc.data(), R.cand_loc.size() * 8);
  std::memcpy(out, R.out.data(), R.out.size() * 4);
}

// pieces, for the term-by-term tests
void cnh_solve(double* rec) { solve_record(rec); }
void cnh_fold(double* a, const double* b) { fold_record(a, b); }
void cnh_label(int P, const unsigned char* pred, int* id) {
  std::vector<int> v;
  label_rows(P, [&](int i, int j) { return pred[(size_t)i * P + j] != 0; }, v);
  std::memcpy(id, v.data(), v.size() * 4);
}

}  // extern "C"
