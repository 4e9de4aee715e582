// Pose-graph optimisation below the C ABI (include/vxba.h: vxba_pgo_*): the top-down half of the global BA.
//
// Reference: topDownProcess (voxelslam.cpp:2231-2317) and build_graph (:1741-1802) hand BetweenFactor<Pose3> / PriorFactor<Pose3> with diagonal
// variances to GTSAM's ISAM2.  Here the same least-squares problem is solved by Levenberg-Marquardt (the damping rule of the LiDAR optimisers,
// vxba_kernels.hip lm_decide) around a block-Jacobi preconditioned conjugate-gradient solve of (H + u diag(H)) dx = -g.
//
// Launch plan.  One outer iteration is six launches and no host synchronisation:
//   pgo_lin_kernel       one lane per factor: residual, Jacobians, the weighted products J^T W J (both ends), J_i^T W J_j, J^T W e
//   pgo_assemble_kernel  one lane per node: D_i, g_i summed over the node's factors in CSR order; (D_i + u diag D_i)^-1
//   pgo_solve_kernel     ONE workgroup of 512 lanes: the whole CG solve (six lanes per 6 x 6 block, one per row: products per factor, sums
//                        per node) and the decrease the model predicts -- workgroup barriers only, however many iterations it takes
//   pgo_retract_kernel   one lane per node: the trial poses
//   pgo_cost_kernel      one lane per factor: the cost at the trial poses
//   pgo_decide_kernel    one workgroup: the trial cost summed, accept / reject, the damping schedule, the report row
// The host enqueues max_iter rounds of the six and synchronises once; a finished optimisation makes the remaining launches return at
// their first instruction.  No floating-point atomics: every sum runs in CSR order or down a fixed tree, so two runs give identical bits.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <cstdint>
#include <cstring>
#include <numeric>
#include <string>
#include <vector>

#include "../../include/vxba.h"
#include "vxba_dev.hpp"
#include "vxba_pgo_math.hpp"

namespace vxpgo {

constexpr int STEP_THREADS = 1024;                       // the decision's workgroup
constexpr int SOLVE_THREADS = 512;                       // the solve's: eight waves, so that a lane may keep 256 registers -- FB factors in flight
constexpr int SOLVE_WAVES = SOLVE_THREADS / 64;
constexpr int SLOTS_PER_WAVE = 10;                       // six lanes per node, ten nodes per wave, four lanes idle
constexpr int STEP_SLOTS = SOLVE_WAVES * SLOTS_PER_WAVE;
constexpr int LDS_MAX_N = 4800;                          // unknowns whose four CG vectors (x, r, p, A p) fit the workgroup's LDS: 153 600 B of 160 KiB
constexpr int REPORT_LEN = VXBA_PGO_REPORT_LEN;
constexpr int FB = 4;                                    // factors in flight per lane in the solve's product

struct Ctl {            // device-resident state of one optimize call
  double u, v, cost;    // damping, rejection factor, cost at the current poses (valid from the first decision on)
  double q1, rz_rel;    // of the last solve: predicted decrease, relative preconditioned residual at its end
  int cg_it, capped;
  int iter, done, n_accept, n_reject;
};

struct Args {
  int K, F, n;                       // nodes, factors, unknowns
  const int* adj_ptr;                // K + 1
  const int* adj_code;               // per adjacency entry: 2 * factor + (0: the node is the factor's i, 1: its j)
  const int* fpos;                   // F x 2: the adjacency entries of the factor in the rows of its i and of its j (-1 for a prior's j)
  const int* fi;                     // F: node i of the factor
  const int* fj;                     // F: node j, -1 for a prior
  const double* Z;                   // F x 12 measurement records
  const double* w;                   // F x 6 weights 1 / v6
  double* X;                         // K x 12 current poses
  double* Xt;                        // K x 12 trial poses
  double* B;                         // F x 36   J_i^T W J_j
  double* Dc;                        // F x 72   J_i^T W J_i | J_j^T W J_j
  double* gc;                        // F x 12   J_i^T W e | J_j^T W e
  double* ce;                        // F        cost of the factor at X
  double* D;                         // K x 36
  double* g;                         // K x 6
  double* Minv;                      // K x 36
  double* vec;                       // 4 n: the CG vectors of a graph too large for LDS
  double* contrib;                   // 6 per adjacency entry: the off-diagonal products of the CG iteration in progress
  double* dx;                        // n: the step of the last solve
  double* ce_t;                      // F: cost of the factor at Xt
  Ctl* ctl;
  double* report;                    // max_iter x REPORT_LEN
  int max_iter, cg_cap;
  double cg_tol2, rel_tol;
};

// ---- per factor ------------------------------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(256) pgo_lin_kernel(Args a) {
  const int f = blockIdx.x * 256 + threadIdx.x;
  if (a.ctl->done || f >= a.F) return;
  const int i = a.fi[f], j = a.fj[f];
  double e[6], Ji[36], Jj[36], w[6];
#pragma unroll
  for (int k = 0; k < 6; k++) w[k] = a.w[6 * (size_t)f + k];
  const bool between = j >= 0;
  if (between) between_lin(a.X + 12 * (size_t)i, a.X + 12 * (size_t)j, a.Z + 12 * (size_t)f, e, Ji, Jj);
  else {
    prior_lin(a.X + 12 * (size_t)i, a.Z + 12 * (size_t)f, e, Ji);
#pragma unroll
    for (int k = 0; k < 36; k++) Jj[k] = 0.0;
  }
  a.ce[f] = half_wsq(e, w);
  double* B = a.B + 36 * (size_t)f;
  double* Dc = a.Dc + 72 * (size_t)f;
  double* gc = a.gc + 12 * (size_t)f;
#pragma unroll
  for (int r = 0; r < 6; r++) {
#pragma unroll
    for (int c = 0; c < 6; c++) {
      B[6 * r + c] = jtwj(Ji, w, Jj, r, c);
      Dc[6 * r + c] = jtwj(Ji, w, Ji, r, c);
      Dc[36 + 6 * r + c] = jtwj(Jj, w, Jj, r, c);
    }
    gc[r] = jtwe(Ji, w, e, r);
    gc[6 + r] = jtwe(Jj, w, e, r);
  }
}

// cost (and, where asked for, the 6 residuals) of every factor at the poses X: vxba_pgo_cost, and the trial poses of every step
__global__ void __launch_bounds__(256) pgo_cost_kernel(Args a, const double* __restrict__ X, double* __restrict__ ce, double* __restrict__ resid, int in_loop) {
  const int f = blockIdx.x * 256 + threadIdx.x;
  if ((in_loop && a.ctl->done) || f >= a.F) return;
  const int i = a.fi[f], j = a.fj[f];
  double e[6], w[6];
#pragma unroll
  for (int k = 0; k < 6; k++) w[k] = a.w[6 * (size_t)f + k];
  if (j >= 0) between_residual(X + 12 * (size_t)i, X + 12 * (size_t)j, a.Z + 12 * (size_t)f, e);
  else prior_residual(X + 12 * (size_t)i, a.Z + 12 * (size_t)f, e);
  if (resid) {
#pragma unroll
    for (int k = 0; k < 6; k++) resid[6 * (size_t)f + k] = e[k];
  }
  ce[f] = half_wsq(e, w);
}

// trial poses X (+) dx; a node without factors keeps its pose bit for bit
__global__ void __launch_bounds__(256) pgo_retract_kernel(Args a) {
  const int node = blockIdx.x * 256 + threadIdx.x;
  if (a.ctl->done || node >= a.K) return;
  const double* P = a.X + 12 * (size_t)node;
  double* T = a.Xt + 12 * (size_t)node;
  if (a.adj_ptr[node + 1] == a.adj_ptr[node]) {
#pragma unroll
    for (int k = 0; k < 12; k++) T[k] = P[k];
  } else {
    double dx[6];
#pragma unroll
    for (int k = 0; k < 6; k++) dx[k] = a.dx[6 * (size_t)node + k];
    retract(P, dx, T);
  }
}

// ---- per node --------------------------------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(256) pgo_assemble_kernel(Args a) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (a.ctl->done || i >= a.K) return;
  double D[36], g[6];
#pragma unroll
  for (int k = 0; k < 36; k++) D[k] = 0.0;
#pragma unroll
  for (int k = 0; k < 6; k++) g[k] = 0.0;
  const int a0 = a.adj_ptr[i], a1 = a.adj_ptr[i + 1];
  for (int q = a0; q < a1; q++) {                      // CSR order: the order the factors were added in
    const int code = a.adj_code[q];
    const double* Dc = a.Dc + 72 * (size_t)(code >> 1) + 36 * (code & 1);
    const double* gc = a.gc + 12 * (size_t)(code >> 1) + 6 * (code & 1);
#pragma unroll
    for (int k = 0; k < 36; k++) D[k] += Dc[k];
#pragma unroll
    for (int k = 0; k < 6; k++) g[k] += gc[k];
  }
#pragma unroll
  for (int k = 0; k < 36; k++) a.D[36 * (size_t)i + k] = D[k];
#pragma unroll
  for (int k = 0; k < 6; k++) a.g[6 * (size_t)i + k] = g[k];
  if (a1 > a0) {
    const double u = a.ctl->u;
#pragma unroll
    for (int k = 0; k < 6; k++) D[7 * k] += u * D[7 * k];
    inv6_spd(D);
  }                                                     // a node without factors: zero block, zero step
#pragma unroll
  for (int k = 0; k < 36; k++) a.Minv[36 * (size_t)i + k] = D[k];
}

// ---- the solve: one workgroup ----------------------------------------------------------------------------------------------------
// Sum over the workgroup, the same bits in every lane: xor butterfly inside each wave, the wave sums through LDS, added in wave order.
// Two buffers alternate, so a wave that is already writing the next sum cannot overwrite what a slower wave still reads.
template <int WAVES>
__device__ __forceinline__ double block_sum(double v, double (*buf)[WAVES], int& flip) {
#pragma unroll
  for (int off = 32; off >= 1; off >>= 1) v += __shfl_xor(v, off, 64);
  double* b = buf[flip];
  flip ^= 1;
  if ((threadIdx.x & 63) == 0) b[threadIdx.x >> 6] = v;
  __syncthreads();
  double s = 0.0;
#pragma unroll
  for (int k = 0; k < WAVES; k++) s += b[k];
  return s;
}

template <bool IN_LDS>
__global__ void __launch_bounds__(SOLVE_THREADS) pgo_solve_kernel(Args a) {
  __shared__ double s_red[2][SOLVE_WAVES];
  __shared__ double s_vec[IN_LDS ? 4 * LDS_MAX_N : 1];
  Ctl* ctl = a.ctl;
  if (ctl->done) return;                                // uniform: written by the previous launch only
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int n = a.n;
  double* x = IN_LDS ? s_vec : a.vec;
  double* r = x + n;
  double* p = r + n;
  double* Ap = p + n;
  int flip = 0;
  const double u = ctl->u;

  // six lanes per node, one per row of its blocks; a node's lanes sit in one wave
  const bool active = lane < 6 * SLOTS_PER_WAVE;
  const int slot_in_wave = lane / 6, row = lane - 6 * slot_in_wave, lane0 = 6 * slot_in_wave;
  const int slot = wave * SLOTS_PER_WAVE + slot_in_wave;

  // x = 0, r = b = -g, z = M^-1 r, p = z
  double part = 0.0;
  if (active) for (int node = slot; node < a.K; node += STEP_SLOTS) {
    const int idx = 6 * node + row;
    const double rv = -a.g[idx];
    const double* Mi = a.Minv + 36 * (size_t)node + 6 * row;
    double z = 0.0;
#pragma unroll
    for (int c = 0; c < 6; c++) z += Mi[c] * __shfl(rv, lane0 + c, 64);
    x[idx] = 0.0; r[idx] = rv; p[idx] = z;
    part += rv * z;
  }
  double rz = block_sum(part, s_red, flip);             // its barrier also publishes p
  const double rz0 = rz;
  int cg_it = 0, capped = 0;
  double rz_end = rz0;
  if (rz0 > 0.0) {
    for (;;) {
      // A p = (H + u diag H) p in two phases.  Per factor (dealt round-robin to the 80 lane groups, so a node of degree 130 costs what any
      // other does): lane r reads row r and column r of B once and leaves (B p_j)[r] and (B^T p_i)[r] at the factor's two places in the
      // CSR-ordered contribution list.  FB factors are in flight per lane: the loads of a batch are issued before its arithmetic.
      if (active) for (int f0 = slot; f0 < a.F; f0 += FB * STEP_SLOTS) {
        int ni[FB], nj[FB], qi[FB], qj[FB];
#pragma unroll
        for (int k = 0; k < FB; k++) {
          const int f = f0 + k * STEP_SLOTS;
          const bool ok = f < a.F;
          ni[k] = ok ? a.fi[f] : 0; nj[k] = ok ? a.fj[f] : -1;
          qi[k] = ok ? a.fpos[2 * f] : -1; qj[k] = ok ? a.fpos[2 * f + 1] : -1;
        }
        double br[FB][6], bc[FB][6];
#pragma unroll
        for (int k = 0; k < FB; k++) {
          const double* Bf = a.B + 36 * (size_t)(nj[k] >= 0 ? f0 + k * STEP_SLOTS : 0);
#pragma unroll
          for (int c = 0; c < 6; c++) { br[k][c] = Bf[6 * row + c]; bc[k][c] = Bf[6 * c + row]; }
        }
#pragma unroll
        for (int k = 0; k < FB; k++) {
          if (qi[k] < 0) continue;
          double ci = 0.0, cj = 0.0;
          if (nj[k] >= 0) {
            const double* pi = p + 6 * ni[k];
            const double* pj = p + 6 * nj[k];
#pragma unroll
            for (int c = 0; c < 6; c++) { ci += br[k][c] * pj[c]; cj += bc[k][c] * pi[c]; }
            a.contrib[6 * (size_t)qj[k] + row] = cj;
          }
          a.contrib[6 * (size_t)qi[k] + row] = ci;       // a prior has no off-diagonal block: zero
        }
      }
      __syncthreads();
      // per node: the diagonal block, then the contributions in CSR order (the order the factors were added in)
      part = 0.0;
      if (active) for (int node = slot; node < a.K; node += STEP_SLOTS) {
        const int idx = 6 * node + row;
        const double* Di = a.D + 36 * (size_t)node + 6 * row;
        const double* pn = p + 6 * node;
        double acc = u * Di[row] * pn[row];
#pragma unroll
        for (int c = 0; c < 6; c++) acc += Di[c] * pn[c];
        const int q1 = a.adj_ptr[node + 1];
        const double* cq = a.contrib + row;
#pragma unroll 8
        for (int q = a.adj_ptr[node]; q < q1; q++) acc += cq[6 * (size_t)q];
        Ap[idx] = acc;
        part += pn[row] * acc;
      }
      const double pAp = block_sum(part, s_red, flip);
      const double alpha = rz / pAp;
      // x += alpha p, r -= alpha A p, z = M^-1 r (kept where A p was)
      part = 0.0;
      if (active) for (int node = slot; node < a.K; node += STEP_SLOTS) {
        const int idx = 6 * node + row;
        x[idx] += alpha * p[idx];
        const double rv = r[idx] - alpha * Ap[idx];
        r[idx] = rv;
        const double* Mi = a.Minv + 36 * (size_t)node + 6 * row;
        double z = 0.0;
#pragma unroll
        for (int c = 0; c < 6; c++) z += Mi[c] * __shfl(rv, lane0 + c, 64);
        Ap[idx] = z;
        part += rv * z;
      }
      const double rzn = block_sum(part, s_red, flip);
      cg_it++;
      rz_end = rzn;
      if (!(rzn > a.cg_tol2 * rz0)) break;               // converged (or not a number: the trial cost below then rejects the step)
      if (cg_it >= a.cg_cap) { capped = 1; break; }
      const double beta = rzn / rz;
      rz = rzn;
      if (active) for (int node = slot; node < a.K; node += STEP_SLOTS) {
        const int idx = 6 * node + row;
        p[idx] = Ap[idx] + beta * p[idx];
      }
      __syncthreads();
    }
  }

  // decrease the quadratic model predicts for x: with r = b - (H + u D) x, -g.x - x.H x / 2 = x.(b + r + u D x) / 2, D = diag H
  part = 0.0;
  if (active) for (int node = slot; node < a.K; node += STEP_SLOTS) {
    const int idx = 6 * node + row;
    const double xv = x[idx];
    part += xv * (-a.g[idx] + r[idx] + u * a.D[36 * (size_t)node + 7 * row] * xv);
  }
  const double q1 = 0.5 * block_sum(part, s_red, flip);
  if (active) for (int node = slot; node < a.K; node += STEP_SLOTS) a.dx[6 * node + row] = x[6 * node + row];
  if (tid == 0) { ctl->q1 = q1; ctl->cg_it = cg_it; ctl->capped = capped; ctl->rz_rel = rz0 > 0.0 ? sqrt(rz_end / rz0) : 0.0; }
}

// accept / reject and the damping schedule (lm_decide, vxba_kernels.hip); every lane computes the same bits
__global__ void __launch_bounds__(STEP_THREADS) pgo_decide_kernel(Args a) {
  __shared__ double s_red[2][STEP_THREADS / 64];
  Ctl* ctl = a.ctl;
  if (ctl->done) return;
  const int tid = threadIdx.x;
  int flip = 0;
  const double u = ctl->u, v = ctl->v, q1 = ctl->q1;
  const int iter = ctl->iter;
  // cost at the current poses: the linearisation's per-factor costs before the first step, carried afterwards
  double p0 = 0.0, p1 = 0.0;
  for (int f = tid; f < a.F; f += STEP_THREADS) { if (iter == 0) p0 += a.ce[f]; p1 += a.ce_t[f]; }
  const double s0 = block_sum(p0, s_red, flip);
  const double cost1 = block_sum(p1, s_red, flip);
  const double cost0 = iter == 0 ? s0 : ctl->cost;
  const double q = cost0 - cost1;
  const bool accept = q > 0;                             // false for a cost that is not a number: a rejected step
  double un, vn;
  if (accept) {
    const double one_three = 1.0 / 3;
    const double t = 2 * (q / q1) - 1;
    const double gf = 1 - t * t * t;
    un = u * (gf > one_three ? gf : one_three);
    vn = 2;
    for (int k = tid; k < 12 * a.K; k += STEP_THREADS) a.X[k] = a.Xt[k];
  } else {
    un = u * v;
    vn = 2 * v;
  }
  __syncthreads();                                       // every lane has read ctl
  if (tid == 0) {
    double* rep = a.report + REPORT_LEN * (size_t)iter;
    rep[0] = cost0; rep[1] = cost1; rep[2] = accept ? 1.0 : 0.0; rep[3] = u; rep[4] = (double)ctl->cg_it; rep[5] = (double)ctl->capped; rep[6] = q1;
    rep[7] = ctl->rz_rel;
    ctl->u = un; ctl->v = vn;
    ctl->cost = accept ? cost1 : cost0;
    ctl->iter = iter + 1;
    ctl->n_accept += accept ? 1 : 0;
    ctl->n_reject += accept ? 0 : 1;
    ctl->done = (fabs(q / cost0) < a.rel_tol || iter + 1 >= a.max_iter) ? 1 : 0;
  }
}

}  // namespace vxpgo

// ---- host ------------------------------------------------------------------------------------------------------------------------
struct vxba_pgo {
  int device = 0;
  std::string err;
  vxu::Stream s;
  int K = 0;
  std::vector<double> poses;                 // K x 12
  std::vector<int> fi, fj;                   // factors in the order they were added; fj = -1: prior
  std::vector<double> Z, w;                  // F x 12, F x 6
  bool graph_dirty = true;
  // device
  vxu::Dev<int> d_adj_ptr, d_adj_code, d_fpos, d_fi, d_fj;
  vxu::Dev<double> d_Z, d_w, d_X, d_Xt, d_B, d_Dc, d_gc, d_ce, d_D, d_g, d_Minv, d_vec, d_dx, d_ce_t, d_contrib, d_report, d_resid;
  vxu::Dev<vxpgo::Ctl> d_ctl;
  int64_t launches = 0, syncs = 0;           // of the last optimize call
};

namespace vxpgo {

using vxu::fail;

static bool finite_all(const double* p, size_t n) { for (size_t k = 0; k < n; k++) if (!std::isfinite(p[k])) return false; return true; }

// a component that has factors between its nodes but no prior is free to move as a whole (GTSAM throws there): name one of its nodes
static int check_gauge(vxba_pgo* h) {
  const int K = h->K;
  std::vector<int> parent(K);
  std::iota(parent.begin(), parent.end(), 0);
  auto find = [&](int x) { while (parent[x] != x) { parent[x] = parent[parent[x]]; x = parent[x]; } return x; };
  for (size_t f = 0; f < h->fi.size(); f++) if (h->fj[f] >= 0) { const int ra = find(h->fi[f]), rb = find(h->fj[f]); if (ra != rb) parent[std::max(ra, rb)] = std::min(ra, rb); }
  std::vector<char> has_prior(K, 0), has_edge(K, 0);
  for (size_t f = 0; f < h->fi.size(); f++) { if (h->fj[f] < 0) has_prior[find(h->fi[f])] = 1; else has_edge[find(h->fi[f])] = 1; }
  for (int k = 0; k < K; k++) if (find(k) == k && has_edge[k] && !has_prior[k])
    return fail(h, VXBA_ERR_ARG, "pgo_optimize: the component of node " + std::to_string(k) + " has no prior (its gauge is free)");
  return VXBA_OK;
}

// factors -> device, CSR adjacency in the order the factors were added
static int upload_graph(vxba_pgo* h) {
  const int K = h->K, F = (int)h->fi.size();
  std::vector<int> ptr(K + 1, 0);
  for (int f = 0; f < F; f++) { ptr[h->fi[f] + 1]++; if (h->fj[f] >= 0) ptr[h->fj[f] + 1]++; }
  for (int k = 0; k < K; k++) ptr[k + 1] += ptr[k];
  const int A = ptr[K];
  std::vector<int> code(std::max(A, 1)), fpos(2 * (size_t)std::max(F, 1), -1), fill(ptr.begin(), ptr.end() - 1);
  for (int f = 0; f < F; f++) {
    int q = fill[h->fi[f]]++;
    code[q] = 2 * f; fpos[2 * f] = q;
    if (h->fj[f] >= 0) { q = fill[h->fj[f]]++; code[q] = 2 * f + 1; fpos[2 * f + 1] = q; }
  }
  const size_t k = (size_t)K, f = (size_t)F, a = (size_t)A;
  VX_HIP(h, h->d_adj_ptr.reserve(k + 1)); VX_HIP(h, h->d_X.reserve(k * 12)); VX_HIP(h, h->d_Xt.reserve(k * 12)); VX_HIP(h, h->d_D.reserve(k * 36));
  VX_HIP(h, h->d_g.reserve(k * 6)); VX_HIP(h, h->d_Minv.reserve(k * 36)); VX_HIP(h, h->d_vec.reserve(k * 24)); VX_HIP(h, h->d_dx.reserve(k * 6));
  VX_HIP(h, h->d_fi.reserve(f)); VX_HIP(h, h->d_fj.reserve(f)); VX_HIP(h, h->d_fpos.reserve(2 * f)); VX_HIP(h, h->d_Z.reserve(f * 12)); VX_HIP(h, h->d_w.reserve(f * 6)); VX_HIP(h, h->d_B.reserve(f * 36));
  VX_HIP(h, h->d_Dc.reserve(f * 72)); VX_HIP(h, h->d_gc.reserve(f * 12)); VX_HIP(h, h->d_ce.reserve(f)); VX_HIP(h, h->d_ce_t.reserve(f)); VX_HIP(h, h->d_resid.reserve(f * 6));
  VX_HIP(h, h->d_adj_code.reserve(a)); VX_HIP(h, h->d_contrib.reserve(6 * a));
  VX_HIP(h, h->d_ctl.reserve(1));
  VX_HIP(h, hipMemcpy(h->d_adj_ptr, ptr.data(), sizeof(int) * (K + 1), hipMemcpyHostToDevice));
  if (A) VX_HIP(h, hipMemcpy(h->d_adj_code, code.data(), sizeof(int) * A, hipMemcpyHostToDevice));
  if (F) {
    VX_HIP(h, hipMemcpy(h->d_fi, h->fi.data(), sizeof(int) * F, hipMemcpyHostToDevice)); VX_HIP(h, hipMemcpy(h->d_fj, h->fj.data(), sizeof(int) * F, hipMemcpyHostToDevice));
    VX_HIP(h, hipMemcpy(h->d_fpos, fpos.data(), sizeof(int) * 2 * F, hipMemcpyHostToDevice));
    VX_HIP(h, hipMemcpy(h->d_Z, h->Z.data(), sizeof(double) * 12 * F, hipMemcpyHostToDevice)); VX_HIP(h, hipMemcpy(h->d_w, h->w.data(), sizeof(double) * 6 * F, hipMemcpyHostToDevice));
  }
  h->graph_dirty = false;
  return VXBA_OK;
}

static Args make_args(vxba_pgo* h) {
  Args a{};
  a.K = h->K; a.F = (int)h->fi.size(); a.n = 6 * h->K;
  a.adj_ptr = h->d_adj_ptr; a.adj_code = h->d_adj_code; a.fpos = h->d_fpos; a.contrib = h->d_contrib; a.fi = h->d_fi; a.fj = h->d_fj; a.Z = h->d_Z; a.w = h->d_w;
  a.X = h->d_X; a.Xt = h->d_Xt; a.B = h->d_B; a.Dc = h->d_Dc; a.gc = h->d_gc; a.ce = h->d_ce; a.D = h->d_D; a.g = h->d_g; a.Minv = h->d_Minv; a.vec = h->d_vec; a.dx = h->d_dx; a.ce_t = h->d_ce_t;
  a.ctl = h->d_ctl; a.report = h->d_report;
  return a;
}

// the graph and the poses in device memory, ready for a kernel
static int stage(vxba_pgo* h, const char* what) {
  if (h->K == 0) return fail(h, VXBA_ERR_STATE, std::string(what) + ": no poses (vxba_pgo_set_poses first)");
  VX_HIP(h, hipSetDevice(h->device));
  if (h->graph_dirty) { const int rc = upload_graph(h); if (rc != VXBA_OK) return rc; }
  VX_HIP(h, hipMemcpyAsync(h->d_X, h->poses.data(), sizeof(double) * 12 * h->K, hipMemcpyHostToDevice, h->s));
  return VXBA_OK;
}

}  // namespace vxpgo

using namespace vxpgo;

extern "C" {

int vxba_pgo_create(int device, vxba_pgo** out) {
  if (!out) return VXBA_ERR_ARG;
  *out = nullptr;
  if (const int rc = vxu::select_device(device)) return rc;
  vxba_pgo* h = new vxba_pgo();
  h->device = device;
  if (h->s.create() != hipSuccess) { delete h; return VXBA_ERR_HIP; }
  *out = h;
  return VXBA_OK;
}

int vxba_pgo_destroy(vxba_pgo* h) {
  if (!h) return VXBA_OK;
  hipSetDevice(h->device);
  if (h->s) hipStreamSynchronize(h->s);
  delete h;
  return VXBA_OK;
}

const char* vxba_pgo_last_error(const vxba_pgo* h) { return h ? h->err.c_str() : "null handle"; }

int vxba_pgo_clear(vxba_pgo* h) {
  if (!h) return VXBA_ERR_ARG;
  h->K = 0; h->poses.clear(); h->fi.clear(); h->fj.clear(); h->Z.clear(); h->w.clear();
  h->graph_dirty = true;
  return VXBA_OK;
}

int vxba_pgo_num_nodes(const vxba_pgo* h) { return h ? h->K : 0; }
int64_t vxba_pgo_num_factors(const vxba_pgo* h) { return h ? (int64_t)h->fi.size() : 0; }

int vxba_pgo_set_poses(vxba_pgo* h, int n, const double* poses) {
  if (!h || n <= 0 || !poses) return fail(h, VXBA_ERR_ARG, "pgo_set_poses: bad argument");
  if (!h->fi.empty() && n != h->K) return fail(h, VXBA_ERR_ARG, "pgo_set_poses: " + std::to_string(n) + " poses for a graph over " + std::to_string(h->K) + " nodes (vxba_pgo_clear first)");
  if (!finite_all(poses, (size_t)12 * n)) return fail(h, VXBA_ERR_ARG, "pgo_set_poses: a pose is not finite");
  if (n != h->K) h->graph_dirty = true;
  h->K = n;
  h->poses.assign(poses, poses + (size_t)12 * n);
  return VXBA_OK;
}

int vxba_pgo_read_poses(vxba_pgo* h, double* poses) {
  if (!h || !poses) return fail(h, VXBA_ERR_ARG, "pgo_read_poses: bad argument");
  std::memcpy(poses, h->poses.data(), sizeof(double) * h->poses.size());
  return VXBA_OK;
}

int vxba_pgo_add_edges(vxba_pgo* h, int64_t n, int node_offset_i, int node_offset_j, const int32_t* edge_ij, const double* edge_data) {
  if (!h || n < 0 || (n > 0 && (!edge_ij || !edge_data))) return fail(h, VXBA_ERR_ARG, "pgo_add_edges: bad argument");
  if (h->K == 0) return fail(h, VXBA_ERR_STATE, "pgo_add_edges: no poses (vxba_pgo_set_poses first)");
  for (int64_t k = 0; k < n; k++) {          // everything is checked before anything is added
    const int64_t i = (int64_t)node_offset_i + edge_ij[2 * k], j = (int64_t)node_offset_j + edge_ij[2 * k + 1];
    if (i < 0 || i >= h->K || j < 0 || j >= h->K) return fail(h, VXBA_ERR_ARG, "pgo_add_edges: edge " + std::to_string(k) + " (" + std::to_string(i) + ", " + std::to_string(j) + ") is out of range for " + std::to_string(h->K) + " nodes");
    if (i == j) return fail(h, VXBA_ERR_ARG, "pgo_add_edges: edge " + std::to_string(k) + " joins node " + std::to_string(i) + " to itself");
    const double* d = edge_data + 18 * k;
    if (!finite_all(d, 18)) return fail(h, VXBA_ERR_ARG, "pgo_add_edges: edge " + std::to_string(k) + " is not finite");
    for (int q = 12; q < 18; q++) if (!(d[q] > 0)) return fail(h, VXBA_ERR_ARG, "pgo_add_edges: edge " + std::to_string(k) + " has a variance <= 0");
  }
  for (int64_t k = 0; k < n; k++) {
    const double* d = edge_data + 18 * k;
    h->fi.push_back(node_offset_i + edge_ij[2 * k]); h->fj.push_back(node_offset_j + edge_ij[2 * k + 1]);
    h->Z.insert(h->Z.end(), d, d + 12);
    for (int q = 12; q < 18; q++) h->w.push_back(1.0 / d[q]);
  }
  if (n) h->graph_dirty = true;
  return VXBA_OK;
}

int vxba_pgo_add_priors(vxba_pgo* h, int64_t n, const int32_t* node, const double* pose12, const double* v6) {
  if (!h || n < 0 || (n > 0 && (!node || !pose12 || !v6))) return fail(h, VXBA_ERR_ARG, "pgo_add_priors: bad argument");
  if (h->K == 0) return fail(h, VXBA_ERR_STATE, "pgo_add_priors: no poses (vxba_pgo_set_poses first)");
  for (int64_t k = 0; k < n; k++) {
    if (node[k] < 0 || node[k] >= h->K) return fail(h, VXBA_ERR_ARG, "pgo_add_priors: prior " + std::to_string(k) + " on node " + std::to_string(node[k]) + " is out of range for " + std::to_string(h->K) + " nodes");
    if (!finite_all(pose12 + 12 * k, 12) || !finite_all(v6 + 6 * k, 6)) return fail(h, VXBA_ERR_ARG, "pgo_add_priors: prior " + std::to_string(k) + " is not finite");
    for (int q = 0; q < 6; q++) if (!(v6[6 * k + q] > 0)) return fail(h, VXBA_ERR_ARG, "pgo_add_priors: prior " + std::to_string(k) + " has a variance <= 0");
  }
  for (int64_t k = 0; k < n; k++) {
    h->fi.push_back(node[k]); h->fj.push_back(-1);
    double z[12];
    pose_R(pose12 + 12 * k, z);                // the measurement record holds the rotation row-major
    for (int q = 0; q < 3; q++) z[9 + q] = pose12[12 * k + 9 + q];
    h->Z.insert(h->Z.end(), z, z + 12);
    for (int q = 0; q < 6; q++) h->w.push_back(1.0 / v6[6 * k + q]);
  }
  if (n) h->graph_dirty = true;
  return VXBA_OK;
}

int vxba_pgo_cost(vxba_pgo* h, double* cost, double* residuals) {
  if (!h || !cost) return fail(h, VXBA_ERR_ARG, "pgo_cost: bad argument");
  const int F = (int)h->fi.size();
  *cost = 0.0;
  if (F == 0) return VXBA_OK;
  int rc = stage(h, "pgo_cost");
  if (rc != VXBA_OK) return rc;
  Args a = make_args(h);
  hipLaunchKernelGGL(pgo_cost_kernel, dim3((F + 255) / 256), dim3(256), 0, h->s, a, (const double*)h->d_X, h->d_ce, residuals ? h->d_resid : nullptr, 0);
  VX_HIP(h, hipGetLastError());
  std::vector<double> ce(F), res;
  VX_HIP(h, hipMemcpyAsync(ce.data(), h->d_ce, sizeof(double) * F, hipMemcpyDeviceToHost, h->s));
  if (residuals) VX_HIP(h, hipMemcpyAsync(residuals, h->d_resid, sizeof(double) * 6 * F, hipMemcpyDeviceToHost, h->s));
  VX_HIP(h, hipStreamSynchronize(h->s));
  double s = 0.0;
  for (int f = 0; f < F; f++) s += ce[f];
  *cost = s;
  return VXBA_OK;
}

int vxba_pgo_optimize(vxba_pgo* h, const vxba_pgo_options* opt, double* poses_out, double* report, int report_capacity, int* n_outer) {
  if (!h) return VXBA_ERR_ARG;
  if (n_outer) *n_outer = 0;
  h->launches = h->syncs = 0;
  if (h->K == 0) return fail(h, VXBA_ERR_STATE, "pgo_optimize: no poses (vxba_pgo_set_poses first)");
  const int K = h->K, F = (int)h->fi.size(), n = 6 * K;
  const int max_iter = opt && opt->max_iter > 0 ? opt->max_iter : 6;
  const int cg_cap = opt && opt->cg_max_iter > 0 ? opt->cg_max_iter : std::max(200, 2 * n);
  const double cg_tol = opt && opt->cg_tol > 0 ? opt->cg_tol : 1e-8;
  const double rel_tol = opt && opt->rel_cost_tol >= 0 ? opt->rel_cost_tol : 1e-6;
  const double u0 = opt && opt->u0 > 0 ? opt->u0 : VXBA_PGO_DEFAULT_U0;
  const double v0 = opt && opt->v0 > 0 ? opt->v0 : 2.0;
  if (report && report_capacity < max_iter) return fail(h, VXBA_ERR_ARG, "pgo_optimize: report_capacity " + std::to_string(report_capacity) + " < max_iter " + std::to_string(max_iter));
  int rc = check_gauge(h);
  if (rc != VXBA_OK) return rc;
  if (F == 0) {                                  // nothing constrains anything: every pose stays
    if (poses_out) std::memcpy(poses_out, h->poses.data(), sizeof(double) * 12 * K);
    return VXBA_OK;
  }
  rc = stage(h, "pgo_optimize");
  if (rc != VXBA_OK) return rc;
  VX_HIP(h, h->d_report.reserve((size_t)max_iter * REPORT_LEN));
  Ctl c{};
  c.u = u0; c.v = v0;
  VX_HIP(h, hipMemcpyAsync(h->d_ctl, &c, sizeof(Ctl), hipMemcpyHostToDevice, h->s));
  VX_HIP(h, hipMemsetAsync(h->d_report, 0, sizeof(double) * max_iter * REPORT_LEN, h->s));
  Args a = make_args(h);
  a.max_iter = max_iter; a.cg_cap = cg_cap; a.cg_tol2 = cg_tol * cg_tol; a.rel_tol = rel_tol;
  const bool in_lds = n <= LDS_MAX_N;
  for (int it = 0; it < max_iter; it++) {
    hipLaunchKernelGGL(pgo_lin_kernel, dim3((F + 255) / 256), dim3(256), 0, h->s, a);
    hipLaunchKernelGGL(pgo_assemble_kernel, dim3((K + 255) / 256), dim3(256), 0, h->s, a);
    if (in_lds) hipLaunchKernelGGL(pgo_solve_kernel<true>, dim3(1), dim3(SOLVE_THREADS), 0, h->s, a);
    else hipLaunchKernelGGL(pgo_solve_kernel<false>, dim3(1), dim3(SOLVE_THREADS), 0, h->s, a);
    hipLaunchKernelGGL(pgo_retract_kernel, dim3((K + 255) / 256), dim3(256), 0, h->s, a);
    hipLaunchKernelGGL(pgo_cost_kernel, dim3((F + 255) / 256), dim3(256), 0, h->s, a, (const double*)h->d_Xt, h->d_ce_t, (double*)nullptr, 1);
    hipLaunchKernelGGL(pgo_decide_kernel, dim3(1), dim3(STEP_THREADS), 0, h->s, a);
    h->launches += 6;
  }
  VX_HIP(h, hipGetLastError());
  std::vector<double> rep((size_t)max_iter * REPORT_LEN);
  VX_HIP(h, hipMemcpyAsync(h->poses.data(), h->d_X, sizeof(double) * 12 * K, hipMemcpyDeviceToHost, h->s));
  VX_HIP(h, hipMemcpyAsync(rep.data(), h->d_report, sizeof(double) * rep.size(), hipMemcpyDeviceToHost, h->s));
  VX_HIP(h, hipMemcpyAsync(&c, h->d_ctl, sizeof(Ctl), hipMemcpyDeviceToHost, h->s));
  VX_HIP(h, hipStreamSynchronize(h->s));
  h->syncs += 1;
  if (poses_out) std::memcpy(poses_out, h->poses.data(), sizeof(double) * 12 * K);
  if (report) std::memcpy(report, rep.data(), sizeof(double) * (size_t)c.iter * REPORT_LEN);
  if (n_outer) *n_outer = c.iter;
  return VXBA_OK;
}

int vxba_pgo_stats(const vxba_pgo* h, int64_t out[4]) {
  if (!h || !out) return VXBA_ERR_ARG;
  out[0] = h->launches; out[1] = h->syncs; out[2] = h->K; out[3] = (int64_t)h->fi.size();
  return VXBA_OK;
}

}  // extern "C"
