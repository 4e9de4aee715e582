// Harness for make_golden_map_fix.py: the reference's fix-form cut_voxel (voxel_map.hpp:1641-1671), the teardown of loop_update (voxelslam.cpp:1105-1112,
// 1158-1159), its single-thread window cut_voxel (:1170-1177) and its recut of every root (:1179-1180) behind the ref_capi surface.  One translation unit
// on top of oracle/ref_capi.cpp (found through -I oracle, not modified); needed only where the golden is generated.
#include "ref_capi.cpp"
extern "C" {
void vxr_localmap_cut_voxel_fix(void* m, int64_t n, const double* pnt_world, const double* var, double jour) {
  RefLocalMap* lm = (RefLocalMap*)m;
  lm->bind();
  PVec pvec((size_t)n);
  for (int64_t i = 0; i < n; i++) {
    pvec[i].pnt = unpack_v3(pnt_world + 3 * i);
    if (var) pvec[i].var = unpack_m3(var + 9 * i); else pvec[i].var.setZero();
  }
  cut_voxel(lm->surf_map, pvec, lm->win_size, jour);
}
void vxr_localmap_clear(void* m) {
  RefLocalMap* lm = (RefLocalMap*)m;
  lm->bind();
  for (auto& kv : lm->surf_map) free_tree(kv.second);
  lm->surf_map.clear(); lm->surf_map_slide.clear();
  for (int i = 0; i < lm->win_size; i++) lm->mp_store[i] = i;
}
// pwld as loop_update builds it: x_buf[i].R * pv.pnt + x_buf[i].p
void vxr_localmap_cut_voxel_single(void* m, int ord, int64_t n, const double* pnt, const double* var, const double* Rp) {
  RefLocalMap* lm = (RefLocalMap*)m;
  lm->bind();
  std::vector<IMUST> xs = unpack_poses(Rp, 1);
  PVecPtr pvec(new PVec((size_t)n));
  PLV(3) pwld;
  for (int64_t i = 0; i < n; i++) { (*pvec)[i].pnt = unpack_v3(pnt + 3 * i); (*pvec)[i].var = unpack_m3(var + 9 * i); }
  for (pointVar& pv : *pvec) pwld.push_back(xs[0].R * pv.pnt + xs[0].p);
  cut_voxel(lm->surf_map, pvec, ord, lm->surf_map_slide, lm->win_size, pwld, lm->sws[0]);
}
void vxr_localmap_recut_all(void* m, int win_count, const double* Rp) {
  RefLocalMap* lm = (RefLocalMap*)m;
  lm->bind();
  std::vector<IMUST> xs = unpack_poses(Rp, win_count);
  for (auto iter = lm->surf_map.begin(); iter != lm->surf_map.end(); ++iter) iter->second->recut(win_count, xs, lm->sws[0]);
}
}
