// Harness for make_golden_keyframe.py: one keyframe the way the front half of thd_loop_closure builds it (voxelslam.cpp:1944-1974), behind one
// extern "C" call.  One translation unit on top of oracle/ref_capi.cpp (found through -I oracle, not modified; it already includes voxel_map.hpp);
// needed only where the golden is generated.  The merge of the buffered scans into the newest pose's frame sits inside the reference's thread
// function and cannot be called, so it is restated here on the shim's Eigen types (oracle/shim/Eigen/Core: products summed left to right, one
// rounding per operation); the filter is the reference's own down_sampling_pvec.
#include <array>

#include "ref_capi.cpp"
extern "C" {
// poses W x 12 [R column-major 9 | t 3], oldest scan first, the last one is the keyframe's; scan_ptr W + 1 offsets in points; pnt N x 3; var N x 9
// column-major.  full N x 3 float32 (the cloud handed to the loop chain), down capacity N x 6 float32 (x, y, z, normal_x, normal_y, normal_z of
// pl_keep, in the map's iteration order), down_index N x 3 the voxel index of every down row (recomputed the way down_sampling_pvec does, so the
// caller can sort).  Returns the number of down rows.
int64_t vxr_keyframe(int W, const double* poses, const int64_t* scan_ptr, const double* pnt, const double* var, double voxel_size, float* full, float* down,
                     int64_t* down_index) {
  const std::vector<IMUST> xs = unpack_poses(poses, W);
  const IMUST& xc = xs[W - 1];
  PVec merged;
  for (int i = 0; i < W; i++) {
    const Eigen::Vector3d dp = xc.R.transpose() * (xs[i].p - xc.p);
    const Eigen::Matrix3d dR = xc.R.transpose() * xs[i].R;
    for (int64_t k = scan_ptr[i]; k < scan_ptr[i + 1]; k++) {
      pointVar pv;
      pv.pnt << pnt[3 * k], pnt[3 * k + 1], pnt[3 * k + 2];
      for (int c = 0; c < 3; c++) for (int r = 0; r < 3; r++) pv.var(r, c) = var[9 * k + 3 * c + r];
      pv.pnt = dR * pv.pnt + dp;
      merged.push_back(pv);
    }
  }
  pcl::PointCloud<PointType> keep;
  down_sampling_pvec(merged, voxel_size / 10, keep);
  for (size_t k = 0; k < merged.size(); k++)     // the float fields of the point type the loop chain's cloud is made of (the shim has no PointXYZI)
    for (int j = 0; j < 3; j++) full[3 * k + j] = (float)merged[k].pnt[j];
  // the voxel a down row came from: pl_keep does not carry it.  A second run of the reference's filter over the FIRST point of every voxel inserts
  // the same keys in the same order, so its map iterates in the same order; each of those points carries its voxel's number through the filter
  {
    PVec firsts;
    std::vector<std::array<int64_t, 3>> index;
    std::map<std::array<int64_t, 3>, int> seen;
    const double vs = voxel_size / 10;
    for (size_t k = 0; k < merged.size(); k++) {
      float loc[3];
      std::array<int64_t, 3> pos;
      for (int j = 0; j < 3; j++) {
        loc[j] = merged[k].pnt[j] / vs;
        if (loc[j] < 0) loc[j] -= 1.0;
        pos[j] = (int64_t)loc[j];
      }
      if (seen.emplace(pos, 1).second) {
        pointVar tag = merged[k];
        tag.var(0, 0) = (double)index.size();      // the row's identity travels in a field the filter copies through for a voxel of one point
        firsts.push_back(tag);
        index.push_back(pos);
      }
    }
    pcl::PointCloud<PointType> order;
    down_sampling_pvec(firsts, vs, order);
    if (order.size() != keep.size()) return -1;
    for (size_t r = 0; r < keep.size(); r++) {
      const size_t id = (size_t)order[r].normal_x;
      for (int j = 0; j < 3; j++) down_index[3 * r + j] = index[id][j];
    }
  }
  for (size_t r = 0; r < keep.size(); r++) {
    down[6 * r] = keep[r].x; down[6 * r + 1] = keep[r].y; down[6 * r + 2] = keep[r].z;
    down[6 * r + 3] = keep[r].normal_x; down[6 * r + 4] = keep[r].normal_y; down[6 * r + 5] = keep[r].normal_z;
  }
  return (int64_t)keep.size();
}
}
