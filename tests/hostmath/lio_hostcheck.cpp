// Host build of the odometry sweep's per-point arithmetic (voxel-slam_amd/csrc/vxba_lio_math.hpp) for tests/test_lio_cpu.py:
//   g++ -O2 -std=c++17 -fPIC -shared -ffp-contract=off -o liblio_hostcheck.so lio_hostcheck.cpp
// The same text lio_sweep_kernel runs: the float-typed voxel index, the leaf test (both gates, sigma, the residual) and the column
// bookkeeping of the wave's reduce-scatter.
#include "../../voxel-slam_amd/csrc/vxba_lio_math.hpp"

extern "C" {

// n points against one plane record each (rec: n x PLANE_LEN; has[i] == 0: no leaf, nothing is tested).  arg: R 9 | p 3 | rot_var 9 | tsl_var 9,
// column-major.  pts: n x 9 (pnt 3 | var upper triangle 6).  Out: loc n x 3, packed (0 where the index is out of range), flag, sigma, resi.
void lioh_points(long long n, const double* pts, const double* rec, const int* has, const double* arg, double voxel_size, long long* loc, int* packed, int* flag,
                 double* sigma, double* resi) {
  vxl::SweepArg a;
  for (int k = 0; k < 9; k++) { a.R[k] = arg[k]; a.rot_var[k] = arg[12 + k]; a.tsl_var[k] = arg[21 + k]; }
  for (int k = 0; k < 3; k++) a.p[k] = arg[9 + k];
  for (long long i = 0; i < n; i++) {
    const double* pnt = pts + 9 * i;
    const double* var = pts + 9 * i + 3;
    const double w[3] = {a.R[0] * pnt[0] + a.R[3] * pnt[1] + a.R[6] * pnt[2] + a.p[0], a.R[1] * pnt[0] + a.R[4] * pnt[1] + a.R[7] * pnt[2] + a.p[1],
                         a.R[2] * pnt[0] + a.R[5] * pnt[1] + a.R[8] * pnt[2] + a.p[2]};
    for (int k = 0; k < 3; k++) loc[3 * i + k] = vxl::voxel_index(w[k], voxel_size);
    unsigned long long key;
    packed[i] = vxl::pack_key(loc[3 * i], loc[3 * i + 1], loc[3 * i + 2], key) ? 1 : 0;
    double sg = 0.0, nrm[3], rs = 0.0;
    flag[i] = has[i] ? (vxl::plane_test(rec + vxl::PLANE_LEN * i, w, a, pnt, var, sg, nrm, rs) ? 1 : 0) : 0;
    sigma[i] = flag[i] ? sg : 0.0;
    resi[i] = rs;
  }
}

// the reduce-scatter's bookkeeping for all 64 lanes: the column each lane ends with and whether it holds a real sum (real >= 1)
void lioh_scatter(int* col, int* real) {
  for (int lane = 0; lane < 64; lane++) {
    int c = 0, r = vxl::NSUM, N = vxl::NSUM;
    for (int off = 32; off >= 1; off /= 2) {
      const int M = (N + 1) / 2;
      vxl::scatter_step((lane & off) != 0, M, c, r);
      N = M;
    }
    col[lane] = c; real[lane] = r;
  }
}

}  // extern "C"
