// Harness for make_golden_loop_icp.py: the reference's icp_normal (loop_refine.hpp:47-145) behind one extern "C" call.  One translation unit on
// top of oracle/ref_capi.cpp (found through -I oracle, not modified; it already includes loop_refine.hpp); needed only where the golden is
// generated.  The KdTreeFLANN icp_normal searches with is the shim's (oracle/shim/pcl/kdtree/kdtree_flann.h): a brute-force float32 search with
// lowest-index ties, not PCL's tree.
#include "ref_capi.cpp"
extern "C" {
// src ns x 6, tar nt x 6 float32 (x, y, z, nx, ny, nz); pose12 [R column-major 9 | t 3] in and out.  Returns icp_normal's verdict.
int vxr_icp_normal(int64_t ns, const float* src, int64_t nt, const float* tar, double* pose12, double icp_eigval) {
  pcl::PointCloud<PointType> pl_src, pl_tar;
  for (int64_t i = 0; i < ns; i++) {
    PointType p;
    p.x = src[6 * i]; p.y = src[6 * i + 1]; p.z = src[6 * i + 2]; p.normal_x = src[6 * i + 3]; p.normal_y = src[6 * i + 4]; p.normal_z = src[6 * i + 5];
    pl_src.push_back(p);
  }
  for (int64_t i = 0; i < nt; i++) {
    PointType p;
    p.x = tar[6 * i]; p.y = tar[6 * i + 1]; p.z = tar[6 * i + 2]; p.normal_x = tar[6 * i + 3]; p.normal_y = tar[6 * i + 4]; p.normal_z = tar[6 * i + 5];
    pl_tar.push_back(p);
  }
  std::pair<Eigen::Vector3d, Eigen::Matrix3d> pose;
  for (int r = 0; r < 3; r++) {
    for (int c = 0; c < 3; c++) pose.second(r, c) = pose12[3 * c + r];
    pose.first[r] = pose12[9 + r];
  }
  const bool ok = icp_normal(pl_src, pl_tar, pose, icp_eigval);
  for (int r = 0; r < 3; r++) {
    for (int c = 0; c < 3; c++) pose12[3 * c + r] = pose.second(r, c);
    pose12[9 + r] = pose.first[r];
  }
  return ok ? 1 : 0;
}
}
