// csrc/vxba_map_math.hpp compiled for the host (g++ -ffp-contract=off): the local map's pure arithmetic behind a C surface for tests/test_map_cpu.py.
#include "../../voxel-slam_amd/csrc/vxba_map_math.hpp"
#include "../../voxel-slam_amd/csrc/vxba_math.hpp"

extern "C" {

// n points pushed one after the other into a leaf's running sums: the world cluster, the scan's local cluster, cov_add (column-major 9x9)
void maph_push(long long n, const double* body, const double* world, const double* var9, double* cl_local, double* cl_add, double* cov_add) {
  for (long long i = 0; i < n; i++) {
    vxmap::cl_push(cl_local, body + 3 * i);
    vxmap::cl_push(cl_add, world + 3 * i);
    vxmap::cov_add_point(cov_add, world + 3 * i, var9 + 9 * i);
  }
}
void maph_to_world(long long n, const double* Rp, const double* body, double* world) {
  for (long long i = 0; i < n; i++) vxmap::to_world(Rp, body + 3 * i, world + 3 * i);
}
void maph_octant(long long n, const double* world, const double* centre, int* oct) {
  for (long long i = 0; i < n; i++) oct[i] = vxmap::octant_of(world + 3 * i, centre);
}
void maph_voxel_index(long long n, const double* w, double voxel_size, long long* loc) {
  for (long long i = 0; i < n; i++) loc[i] = vxmap::voxel_index(w[i], voxel_size);
}
// the eigen-decomposition as map_judge_kernel and map_margi_kernel take it: cluster_cov, eig_sym3, eigenvectors stored 3 * column + row
void maph_eig(const double* cluster, double* eig_val, double* eig_vec) {
  double Cm[6], lam[3], U[9];
  vxm::cluster_cov(cluster, cluster + 6, cluster[9], Cm);
  vxm::eig_sym3(Cm, lam, U);
  for (int k = 0; k < 3; k++) eig_val[k] = lam[k];
  for (int col = 0; col < 3; col++)
    for (int row = 0; row < 3; row++) eig_vec[3 * col + row] = U[3 * row + col];
}
void maph_transform(const double* cluster, const double* Rp, double* out) { vxmap::cl_transform(cluster, Rp, out); }
void maph_plane_update(const double* cov_add, const double* cluster, const double* eig_vec, const double* eig_val, double* centre, double* plane_var) {
  double ca9[9];
  for (int q = 0; q < 3; q++)
    for (int r = 0; r < 3; r++) ca9[3 * q + r] = cov_add[9 * (6 + q) + 6 + r];
  vxmap::plane_update_math(cov_add, ca9, cluster, eig_vec, eig_val, centre, plane_var);
}

}  // extern "C"
