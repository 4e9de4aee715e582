// Loop search below the C ABI (include/vxba.h: vxba_loopsearch_*): triangle descriptors of a keyframe's corners, the device-resident
// database of them, the vote over it and the verification of the candidates.
//
// Reference: STDescManager::generate_std (BTC.cpp:979-1126), AddSTDescs (:258-277), candidate_selector (:1128-1279), candidate_verify and
// triangle_solver (:1281-1420), SearchLoop (:205-256).  The arithmetic that has to round as written is in vxba_loopsearch_math.hpp.
//
// Launch plan:
//   describe  triangle_kernel   one wave per corner: the corners in LDS as float32, K rounds of (distance, index) selection for the K nearest,
//                               then the lanes over the (m, n) pairs: sides, tests, key; one slot per (i, m, n) in loop order
//             rocPRIM stable radix sort of (key, slot); mark_kernel flags the first slot of every run of equal keys; rocPRIM scan;
//             compact_kernel writes the surviving descriptors in slot order into the current set (plane-major SoA)
//   add       rocPRIM stable sort of (cell, index); add_runs_kernel: the first descriptor of every run claims / finds the cell's slot in the
//             open-addressing table (integer CAS) and chains the run behind the cell's list, numbering positions; copy_kernel copies the
//             records into the frame's own block.  Work ~ the keyframe's descriptors; the table doubles when half full (rehash_kernel)
//   search    query_kernel<count>, rocPRIM scan, (host reads the total), query_kernel<emit>: the second pass writes every match at
//             offset[(descriptor, neighbour cell)] + its rank among the cell's matches -- the list is born ordered, no sort, no arrival order
//             select_kernel (one workgroup: candidate_num rounds of first-argmax over the votes), candkey_kernel + rocPRIM stable sort on
//             the candidate slot (the pairs of a candidate contiguous, list order kept), verify_kernel (one workgroup per (hypothesis,
//             candidate)), best_kernel (one wave per candidate: first maximum, the pair descriptor of the score), the score kernel of
//             vxba_loopreg.hip.  9 launches, 2 host synchronisations, whatever the database, the matches and the candidates.
//   search_multi  the same nine over S databases at once: the session is a grid dimension of the query, verify and best kernels
//             (multi_*), the counts of all (session, descriptor, cell) go through one scan, so the list is session-major; the votes are one array over
//             all sessions' frames, one workgroup per session selects, the sort key is (session, candidate slot).  The sessions' table goes up in
//             one pinned copy, everything comes back in one.  The arithmetic is the single search's: the kernels of both share their bodies.
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
#include "vxba_loopsearch_math.hpp"

namespace vxls {

constexpr int MAXN = VXBA_LOOPSEARCH_MAX_CORNERS, MAXK = 32, HYP = VXBA_LOOPSEARCH_MAX_HYPOTHESES, MAXCAND = 64;
constexpr int NF = 15;                                  // float64 planes of a record: triangle 0..2, centre 3..5, locations of A, B, C 6..14
constexpr size_t REC_BYTES = NF * 8 + 3 * 8 + 8 + 4;    // + occupancy of A, B, C + next + position in the cell
constexpr int CI = VXBA_LOOPSEARCH_CAND_INTS, CD = VXBA_LOOPSEARCH_CAND_DOUBLES;

// descriptors as planes: f[p * stride + i]
struct Rec {
  double* f;
  unsigned long long* occ;    // 3 planes
  unsigned long long* next;   // the entry filed before this one in the same cell: frame << 32 | index, KEY_NONE at the end (frames only)
  int* pos;                   // position in the cell, in insertion order (frames only)
  int n, stride;
};
struct Frame {
  Rec r;
  const float* cloud;
  int cloud_n, cloud_id;
};
struct Table {
  unsigned long long* key;    // packed cell, KEY_NONE when empty
  unsigned long long* head;   // the cell's newest entry
  int* count;
  unsigned mask;
};

__device__ __forceinline__ unsigned hash_of(unsigned long long k, unsigned mask) {
  k ^= k >> 33; k *= 0xff51afd7ed558ccdULL; k ^= k >> 33;
  return (unsigned)k & mask;
}

__device__ __forceinline__ int pick3(int v, int a, int b, int c) { return v == 0 ? a : (v == 1 ? b : c); }

// ---- describe ----------------------------------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(64) triangle_kernel(const double* __restrict__ loc, int n, int K, double min_len, double max_len, unsigned long long* __restrict__ key,
                                                      unsigned int* __restrict__ val, int* __restrict__ vert, double* __restrict__ sides) {
  __shared__ float xs[3 * MAXN];
  __shared__ int nb[MAXK];
  const int i = blockIdx.x, lane = threadIdx.x;
  for (int k = lane; k < 3 * n; k += 64) xs[k] = (float)loc[k];
  __syncthreads();
  const float qx = xs[3 * i], qy = xs[3 * i + 1], qz = xs[3 * i + 2];
  float pd = -1.f; int pi = -1;                          // the pair selected last: the next one is the smallest (distance, index) after it
  for (int r = 0; r < K; r++) {
    float best = std::numeric_limits<float>::infinity(); int bi = 0x7fffffff;
    for (int j = lane; j < n; j += 64) {
      const float dx = xs[3 * j] - qx, dy = xs[3 * j + 1] - qy, dz = xs[3 * j + 2] - qz;
      const float d = (dx * dx + dy * dy) + dz * dz;
      if ((d > pd || (d == pd && j > pi)) && d < best) { best = d; bi = j; }
    }
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) {
      const float ob = __shfl_xor(best, off, 64); const int oi = __shfl_xor(bi, off, 64);
      if (ob < best || (ob == best && oi < bi)) { best = ob; bi = oi; }
    }
    if (lane == 0) nb[r] = bi < n ? bi : i;
    pd = best; pi = bi;
  }
  __syncthreads();
  const int P = (K - 1) * (K - 2) / 2;
  for (int p = lane; p < P; p += 64) {
    int m = 1, rem = p;
    while (rem >= K - 1 - m) { rem -= K - 1 - m; m++; }
    const int nn = m + 1 + rem;
    const int i2 = nb[m], i3 = nb[nn];
    double a = side(xs + 3 * i, xs + 3 * i2), b = side(xs + 3 * i, xs + 3 * i3), c = side(xs + 3 * i3, xs + 3 * i2);
    bool ok = sides_in_range(a, b, c, min_len, max_len);
    int v[3];
    sort_sides(a, b, c, v);
    ok = ok && not_collinear(a, b, c);
    const size_t slot = (size_t)i * P + p;
    key[slot] = ok ? pack3(side_key(a), side_key(b), side_key(c)) : KEY_NONE;
    val[slot] = (unsigned int)slot;
    vert[3 * slot] = pick3(v[0], i, i2, i3); vert[3 * slot + 1] = pick3(v[1], i, i2, i3); vert[3 * slot + 2] = pick3(v[2], i, i2, i3);
    sides[3 * slot] = a; sides[3 * slot + 1] = b; sides[3 * slot + 2] = c;
  }
}

// sorted position i: the first of a run of equal keys is the triangle that came first in loop order (the sort is stable)
__global__ void __launch_bounds__(256) mark_kernel(const unsigned long long* __restrict__ key_s, const unsigned int* __restrict__ val_s, int n, unsigned int* __restrict__ flag) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i >= n) return;
  const unsigned long long k = key_s[i];
  flag[val_s[i]] = (k != KEY_NONE && (i == 0 || key_s[i - 1] != k)) ? 1u : 0u;
}

__global__ void __launch_bounds__(256) compact_kernel(int nslots, const unsigned int* __restrict__ flag, const unsigned int* __restrict__ pos, const int* __restrict__ vert,
                                                     const double* __restrict__ sides, const double* __restrict__ loc, const unsigned long long* __restrict__ occ, double scale,
                                                     Rec cur, int* __restrict__ cid, unsigned long long* __restrict__ cell, unsigned int* __restrict__ total) {
  const int s = blockIdx.x * 256 + threadIdx.x;
  if (s >= nslots) return;
  if (s == nslots - 1) *total = pos[s] + flag[s];
  if (!flag[s]) return;
  const int d = (int)pos[s], st = cur.stride;
  if (d >= st) return;
  double t[3], ctr[3] = {0, 0, 0};
#pragma unroll
  for (int k = 0; k < 3; k++) { t[k] = scale * sides[3 * (size_t)s + k]; cur.f[k * st + d] = t[k]; }
  float fc[9];
#pragma unroll
  for (int v = 0; v < 3; v++) {
    const int c = vert[3 * (size_t)s + v];
    cid[v * st + d] = c;
    cur.occ[v * st + d] = occ[c];
#pragma unroll
    for (int k = 0; k < 3; k++) {
      const double x = loc[3 * c + k];
      cur.f[(6 + 3 * v + k) * st + d] = x;
      fc[3 * v + k] = (float)x;
    }
  }
#pragma unroll
  for (int k = 0; k < 3; k++) cur.f[(3 + k) * st + d] = (((double)fc[k] + (double)fc[3 + k]) + (double)fc[6 + k]) / 3.0;
  cell[d] = pack3(cell_add(t[0]), cell_add(t[1]), cell_add(t[2]));
}

// ---- add -----------------------------------------------------------------------------------------------------------------------------
__device__ __forceinline__ unsigned claim_slot(const Table& tb, unsigned long long k) {
  unsigned s = hash_of(k, tb.mask);
  for (;;) {
    const unsigned long long old = atomicCAS(tb.key + s, KEY_NONE, k);
    if (old == KEY_NONE || old == k) return s;
    s = (s + 1) & tb.mask;
  }
}

// the table is kept at most half full by the host, so every probe ends
__global__ void __launch_bounds__(256) add_runs_kernel(const unsigned long long* __restrict__ cell_s, const unsigned int* __restrict__ idx_s, int nd, int frame, Table tb, Rec blk) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i >= nd) return;
  const unsigned long long k = cell_s[i];
  if (i > 0 && cell_s[i - 1] == k) return;
  const unsigned s = claim_slot(tb, k);                 // one run per cell and launch: nobody else touches this slot's head and count
  const int base = tb.count[s];
  unsigned long long prev = base ? tb.head[s] : KEY_NONE;
  int r = 0;
  for (int j = i; j < nd && cell_s[j] == k; j++, r++) {
    const unsigned int e = idx_s[j];                    // ascending inside the run: the sort is stable
    blk.pos[e] = base + r;
    blk.next[e] = prev;
    prev = ((unsigned long long)(unsigned)frame << 32) | e;
  }
  tb.head[s] = prev;
  tb.count[s] = base + r;
}

__global__ void __launch_bounds__(256) iota_kernel(unsigned int* __restrict__ v, int n) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i < n) v[i] = (unsigned int)i;
}

__global__ void __launch_bounds__(256) copy_kernel(Rec cur, Rec blk, int nd) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i >= nd) return;
#pragma unroll
  for (int p = 0; p < NF; p++) blk.f[p * blk.stride + i] = cur.f[p * cur.stride + i];
#pragma unroll
  for (int p = 0; p < 3; p++) blk.occ[p * blk.stride + i] = cur.occ[p * cur.stride + i];
}

__global__ void __launch_bounds__(256) rehash_kernel(Table from, Table to) {
  const unsigned i = blockIdx.x * 256 + threadIdx.x;
  if (i > from.mask) return;
  const unsigned long long k = from.key[i];
  if (k == KEY_NONE) return;
  const unsigned s = claim_slot(to, k);
  to.head[s] = from.head[i];
  to.count[s] = from.count[i];
}

// ---- search --------------------------------------------------------------------------------------------------------------------------
// One searched session as the multi-session kernels see it: its cell table, its frame records and their count, its own skip_near_num, and
// where its frames start in the vote array that runs over all sessions' frames.
struct Sess {
  Table tb;
  const Frame* frames;
  int F, skip, voff;
};

// lane t = (query descriptor, neighbour offset) against one database.  cnt / off: this database's nd * 27 counts and their offsets into the match
// list; votes: this database's frames; fbase: what the list's frame column adds to the frame (0, or the session's vote offset)
template <bool EMIT>
__device__ __forceinline__ void query_body(const Rec& cur, int t, const Table& tb, const Frame* __restrict__ frames, int frame_cur, int skip, double rough, double sim_thr,
                                           int* __restrict__ cnt, const int* __restrict__ off, int* __restrict__ mq, int* __restrict__ mf, int* __restrict__ mi,
                                           int* __restrict__ votes, int fbase) {
  const int q = t / 27, o = t - 27 * q;
  const int inc[3] = {o / 9 - 1, (o / 3) % 3 - 1, o % 3 - 1};
  double tri[3]; int c[3];
  bool in = true;
#pragma unroll
  for (int k = 0; k < 3; k++) {
    tri[k] = cur.f[k * cur.stride + q];
    c[k] = cell_query(tri[k], inc[k]);
    in = in && c[k] >= 0 && c[k] < (1 << KEY_BITS);
  }
  int n = 0;
  if (in && cell_distance(tri, c) < 1.5) {
    const unsigned long long key = pack3(c[0], c[1], c[2]);
    unsigned s = hash_of(key, tb.mask);
    unsigned long long e = KEY_NONE;
    for (;;) {
      const unsigned long long k = tb.key[s];
      if (k == key) { e = tb.head[s]; break; }
      if (k == KEY_NONE) break;
      s = (s + 1) & tb.mask;
    }
    if (e != KEY_NONE) {
      const double thr = norm3(tri[0], tri[1], tri[2]) * rough;
      const unsigned long long bq[3] = {cur.occ[q], cur.occ[cur.stride + q], cur.occ[2 * cur.stride + q]};
      const int last = EMIT ? off[t] + cnt[t] : 0;       // the walk runs newest first: the k-th match found is the k-th from the end
      while (e != KEY_NONE) {
        const int f = (int)(e >> 32), i = (int)(e & 0xffffffffu);
        const Rec r = frames[f].r;
        if (frame_cur - f > skip) {
          const double d = norm3(tri[0] - r.f[i], tri[1] - r.f[r.stride + i], tri[2] - r.f[2 * r.stride + i]);
          if (d < thr) {
            const unsigned long long be[3] = {r.occ[i], r.occ[r.stride + i], r.occ[2 * r.stride + i]};
            if (similarity(bq, be) > sim_thr) {
              n++;
              if (EMIT) {
                const int w = last - n;
                mq[w] = q; mf[w] = fbase + f; mi[w] = i;
                atomicAdd(votes + f, 1);                 // integers: any order gives the same sum
              }
            }
          }
        }
        e = r.next[i];
      }
    }
  }
  if (!EMIT) cnt[t] = n;
}

// one lane per (query descriptor, neighbour offset); cnt has nd * 27 + 1 entries (the last one zero: the scan puts the total there)
template <bool EMIT>
__global__ void __launch_bounds__(256) query_kernel(Rec cur, int nd, Table tb, const Frame* __restrict__ frames, int frame_cur, int skip, double rough, double sim_thr,
                                                   int* __restrict__ cnt, const int* __restrict__ off, int* __restrict__ mq, int* __restrict__ mf, int* __restrict__ mi,
                                                   int* __restrict__ votes) {
  const int t = blockIdx.x * 256 + threadIdx.x;
  if (!EMIT && t == nd * 27) cnt[t] = 0;
  if (t >= nd * 27) return;
  query_body<EMIT>(cur, t, tb, frames, frame_cur, skip, rough, sim_thr, cnt, off, mq, mf, mi, votes, 0);
}

// grid (lanes of one session, S): the counts are session-major, S * nd * 27 + 1 of them under one scan, so the list is born session-major and ordered
// inside every session as the single search orders it.  The second pass also leaves the S + 1 offsets of the sessions' lists in moff.
template <bool EMIT>
__global__ void __launch_bounds__(256) multi_query_kernel(Rec cur, int nd, const Sess* __restrict__ sess, int S, int frame_cur, double rough, double sim_thr, int* __restrict__ cnt,
                                                         const int* __restrict__ off, int* __restrict__ mq, int* __restrict__ mf, int* __restrict__ mi, int* __restrict__ votes,
                                                         int* __restrict__ moff) {
  const int s = blockIdx.y, t = blockIdx.x * 256 + threadIdx.x;
  const size_t nq = (size_t)nd * 27;
  if (t == 0) {
    if (!EMIT && s == 0) cnt[S * nq] = 0;
    if (EMIT) { moff[s] = off[s * nq]; if (s == 0) moff[S] = off[S * nq]; }
  }
  if ((size_t)t >= nq) return;
  const Sess se = sess[s];
  if (se.F == 0) {                                       // a session without frames has no table either
    if (!EMIT) cnt[s * nq + t] = 0;
    return;
  }
  query_body<EMIT>(cur, t, se.tb, se.frames, frame_cur, se.skip, rough, sim_thr, cnt + s * nq, off + s * nq, mq, mf, mi, votes + se.voff, se.voff);
}

// one workgroup: candidate_num rounds of the first maximum of the votes (votes descending, frame ascending), while it is >= 5; base: where the
// database's part of the sorted list starts
__device__ __forceinline__ void select_body(int* __restrict__ votes, int F, int cand_num, int* __restrict__ cand_of_frame, int* __restrict__ cframe,
                                            int* __restrict__ cvotes, int* __restrict__ coff, int* __restrict__ ncand, int base) {
  __shared__ int sv[4], sf[4], stop;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  int total = 0, nc = 0;
  for (int c = 0; c < cand_num; c++) {
    int bv = -1, bf = 0x7fffffff;
    for (int f = threadIdx.x; f < F; f += 256) {
      const int v = votes[f];
      if (v > bv) { bv = v; bf = f; }
    }
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) {
      const int ov = __shfl_xor(bv, off, 64), of = __shfl_xor(bf, off, 64);
      if (ov > bv || (ov == bv && of < bf)) { bv = ov; bf = of; }
    }
    if (lane == 0) { sv[wave] = bv; sf[wave] = bf; }
    __syncthreads();
    if (threadIdx.x == 0) {
      for (int w = 1; w < 4; w++) if (sv[w] > bv || (sv[w] == bv && sf[w] < bf)) { bv = sv[w]; bf = sf[w]; }
      stop = bv < 5;
      if (!stop) {
        votes[bf] = 0; cand_of_frame[bf] = c;
        cframe[c] = bf; cvotes[c] = bv; coff[c] = base + total;
        total += bv; nc = c + 1;
      }
    }
    __syncthreads();
    if (stop) break;
  }
  if (threadIdx.x == 0) *ncand = nc;
}

__global__ void __launch_bounds__(256) select_kernel(int* __restrict__ votes, int F, int cand_num, int* __restrict__ cand_of_frame, int* __restrict__ cframe,
                                                    int* __restrict__ cvotes, int* __restrict__ coff, int* __restrict__ ncand) {
  select_body(votes, F, cand_num, cand_of_frame, cframe, cvotes, coff, ncand, 0);
}

// one workgroup per session, each over its own stretch of the votes
__global__ void __launch_bounds__(256) multi_select_kernel(const Sess* __restrict__ sess, int* __restrict__ votes, int cand_num, int* __restrict__ cand_of_frame,
                                                          int* __restrict__ cframe, int* __restrict__ cvotes, int* __restrict__ coff, int* __restrict__ ncand,
                                                          const int* __restrict__ moff) {
  const int s = blockIdx.x;
  const Sess se = sess[s];
  select_body(votes + se.voff, se.F, cand_num, cand_of_frame + se.voff, cframe + s * cand_num, cvotes + s * cand_num, coff + s * cand_num, ncand + s, moff[s]);
}

__global__ void __launch_bounds__(256) candkey_kernel(const int* __restrict__ mf, int M, const int* __restrict__ cand_of_frame, unsigned int* __restrict__ key, unsigned int* __restrict__ val) {
  const int m = blockIdx.x * 256 + threadIdx.x;
  if (m >= M) return;
  const int c = cand_of_frame[mf[m]];
  key[m] = c < 0 ? 255u : (unsigned int)c;
  val[m] = (unsigned int)m;
}

// the sort key of the multi-session list: (session, candidate slot), 255 for a pair of no candidate; the list's frame column is global
__global__ void __launch_bounds__(256) multi_candkey_kernel(const int* __restrict__ mf, int M, int S, const int* __restrict__ moff, const int* __restrict__ cand_of_frame,
                                                           unsigned int* __restrict__ key, unsigned int* __restrict__ val) {
  const int m = blockIdx.x * 256 + threadIdx.x;
  if (m >= M) return;
  int s = 0;
  while (s + 1 < S && moff[s + 1] <= m) s++;
  const int c = cand_of_frame[mf[m]];
  key[m] = ((unsigned int)s << 8) | (c < 0 ? 255u : (unsigned int)c);
  val[m] = (unsigned int)m;
}

__device__ __forceinline__ void load_pair(const Rec& cur, const Frame* frames, int q, int f, int i, double* sl, double* rl) {
  const Rec r = frames[f].r;
#pragma unroll
  for (int k = 0; k < 9; k++) { sl[k] = cur.f[(6 + k) * cur.stride + q]; rl[k] = r.f[(6 + k) * r.stride + i]; }
}

// workgroup (h, c) of one database: the hypothesis of pair h * skip_len, voted on by every pair of the candidate; fbase: what the list's frame
// column holds on top of the frame
__device__ __forceinline__ void verify_body(const Rec& cur, const Frame* __restrict__ frames, const int* __restrict__ mq, const int* __restrict__ mf, const int* __restrict__ mi,
                                            const unsigned int* __restrict__ sval, const int* __restrict__ cvotes, const int* __restrict__ coff, const int* __restrict__ ncand,
                                            int* __restrict__ hvote, double* __restrict__ hpose, int c, int h, int fbase) {
  __shared__ int s_cnt[4];
  if (c >= *ncand) return;
  const int M = cvotes[c], skip_len = M / 50 + 1, use = M / skip_len;
  if (h >= use) return;
  const int base = coff[c];
  double P[12];
  {
    const int m = (int)sval[base + h * skip_len];
    const int q = mq[m], f = mf[m] - fbase, i = mi[m];
    double sl[9], rl[9], sc[3], rc[3];
    load_pair(cur, frames, q, f, i, sl, rl);
    const Rec r = frames[f].r;
#pragma unroll
    for (int k = 0; k < 3; k++) { sc[k] = cur.f[(3 + k) * cur.stride + q]; rc[k] = r.f[(3 + k) * r.stride + i]; }
    triangle_pose(sl, sc, rl, rc, P);
  }
  const bool fin = finite12(P);
  int n = 0;
  for (int j = threadIdx.x; j < M; j += 256) {
    const int m = (int)sval[base + j];
    double sl[9], rl[9];
    load_pair(cur, frames, mq[m], mf[m] - fbase, mi[m], sl, rl);
    if (fin && pair_votes(P, sl, rl, 3.0)) n++;
  }
#pragma unroll
  for (int off = 32; off >= 1; off >>= 1) n += __shfl_xor(n, off, 64);
  if ((threadIdx.x & 63) == 0) s_cnt[threadIdx.x >> 6] = n;
  __syncthreads();
  if (threadIdx.x == 0) {
    hvote[c * HYP + h] = (s_cnt[0] + s_cnt[1]) + (s_cnt[2] + s_cnt[3]);
#pragma unroll
    for (int k = 0; k < 12; k++) hpose[(size_t)(c * HYP + h) * 12 + k] = P[k];
  }
}

// grid (HYP, candidate_num)
__global__ void __launch_bounds__(256) verify_kernel(Rec cur, const Frame* __restrict__ frames, const int* __restrict__ mq, const int* __restrict__ mf, const int* __restrict__ mi,
                                                    const unsigned int* __restrict__ sval, const int* __restrict__ cvotes, const int* __restrict__ coff, const int* __restrict__ ncand,
                                                    int* __restrict__ hvote, double* __restrict__ hpose) {
  verify_body(cur, frames, mq, mf, mi, sval, cvotes, coff, ncand, hvote, hpose, blockIdx.y, blockIdx.x, 0);
}

// grid (HYP, candidate_num, S): sessions differ in candidates, pairs and skip_len; a workgroup without a hypothesis returns at once
__global__ void __launch_bounds__(256) multi_verify_kernel(Rec cur, const Sess* __restrict__ sess, int NC, const int* __restrict__ mq, const int* __restrict__ mf,
                                                          const int* __restrict__ mi, const unsigned int* __restrict__ sval, const int* __restrict__ cvotes,
                                                          const int* __restrict__ coff, const int* __restrict__ ncand, int* __restrict__ hvote, double* __restrict__ hpose) {
  const int s = blockIdx.z;
  const Sess se = sess[s];
  verify_body(cur, se.frames, mq, mf, mi, sval, cvotes + s * NC, coff + s * NC, ncand + s, hvote + (size_t)s * NC * HYP, hpose + (size_t)s * NC * HYP * 12, blockIdx.y,
              blockIdx.x, se.voff);
}

// one wave per candidate slot c of one database: the first maximum over its hypotheses, its table row and the pair the score kernel reads
__device__ __forceinline__ void best_body(const Frame* __restrict__ frames, const int* __restrict__ cframe, const int* __restrict__ cvotes, const int* __restrict__ ncand,
                                          const int* __restrict__ hvote, const double* __restrict__ hpose, const float* cur_cloud, int cur_n, long long* __restrict__ tab,
                                          double* __restrict__ poses, vxlr::PairDesc* __restrict__ pairs, int c) {
  const int lane = threadIdx.x;
  if (c >= *ncand) {
    if (lane == 0) pairs[c] = vxlr::PairDesc{cur_cloud, cur_cloud, 0, 0};
    if (lane < 12) poses[12 * c + lane] = 0.0;
    return;
  }
  const int M = cvotes[c], skip_len = M / 50 + 1, use = M / skip_len;
  int bv = lane < use ? hvote[c * HYP + lane] : -1, bh = lane;
#pragma unroll
  for (int off = 32; off >= 1; off >>= 1) {
    const int ov = __shfl_xor(bv, off, 64), oh = __shfl_xor(bh, off, 64);
    if (ov > bv || (ov == bv && oh < bh)) { bv = ov; bh = oh; }
  }
  if (lane < 12) poses[12 * c + lane] = hpose[(size_t)(c * HYP + bh) * 12 + lane];
  if (lane == 0) {
    const Frame fr = frames[cframe[c]];
    long long* row = tab + CI * c;
    row[0] = cframe[c]; row[1] = M; row[2] = M; row[3] = use; row[4] = bh; row[5] = bv; row[6] = 0;
    pairs[c] = vxlr::PairDesc{cur_cloud, fr.cloud, bv >= 4 ? cur_n : 0, fr.cloud_n};
  }
}

__global__ void __launch_bounds__(64) best_kernel(const Frame* __restrict__ frames, const int* __restrict__ cframe, const int* __restrict__ cvotes, const int* __restrict__ ncand,
                                                 const int* __restrict__ hvote, const double* __restrict__ hpose, const float* cur_cloud, int cur_n, long long* __restrict__ tab,
                                                 double* __restrict__ poses, vxlr::PairDesc* __restrict__ pairs) {
  best_body(frames, cframe, cvotes, ncand, hvote, hpose, cur_cloud, cur_n, tab, poses, pairs, blockIdx.x);
}

// grid (candidate_num, S): row s * candidate_num + c of the tables, the poses and the score's pairs
__global__ void __launch_bounds__(64) multi_best_kernel(const Sess* __restrict__ sess, int NC, const int* __restrict__ cframe, const int* __restrict__ cvotes,
                                                       const int* __restrict__ ncand, const int* __restrict__ hvote, const double* __restrict__ hpose, const float* cur_cloud,
                                                       int cur_n, long long* __restrict__ tab, double* __restrict__ poses, vxlr::PairDesc* __restrict__ pairs) {
  const int s = blockIdx.y;
  best_body(sess[s].frames, cframe + s * NC, cvotes + s * NC, ncand + s, hvote + (size_t)s * NC * HYP, hpose + (size_t)s * NC * HYP * 12, cur_cloud, cur_n,
            tab + (size_t)s * NC * CI, poses + (size_t)s * NC * 12, pairs + s * NC, blockIdx.x);
}

}  // namespace vxls

// ---- host ------------------------------------------------------------------------------------------------------------------------
using namespace vxls;

struct vxba_loopsearch {
  int device = 0;
  std::string err;
  vxba_loopreg* reg = nullptr;
  hipStream_t s = nullptr;
  unsigned long long reg_generation = 0;
  // the current set
  Rec cur{}; vxu::Dev<char> d_cur; vxu::Dev<int> d_cid; vxu::Dev<unsigned long long> d_cell; int nd = 0;      // cur views d_cur: [f NF x stride | occ 3 x stride]
  // describe scratch
  vxu::Dev<double> d_loc; vxu::Dev<unsigned long long> d_occ;
  vxu::Dev<unsigned long long> d_key, d_key_s; vxu::Dev<unsigned int> d_val, d_val_s, d_flag, d_pos; vxu::Dev<int> d_vert; vxu::Dev<double> d_sides;
  vxu::Dev<unsigned int> d_total;
  vxu::Arena work;                                      // rocPRIM's temp storage
  // the database: a block per frame (frames[k].r views blocks[k]), the frame table, the cell table (tb views tb_mem: key | head | count)
  std::vector<Frame> frames; std::vector<vxu::Dev<char>> blocks;
  vxu::Dev<Frame> d_frames; vxu::Dev<int> d_votes, d_cand_of_frame;
  Table tb{}; vxu::Dev<char> tb_mem; size_t tb_used_ub = 0;
  int64_t n_db = 0, rec_bytes = 0;
  // search
  vxu::Dev<int> d_cnt, d_off;
  vxu::Dev<int> d_mq, d_mf, d_mi; vxu::Dev<unsigned int> d_ck, d_ck_s, d_cv, d_cv_s;
  vxu::Dev<int> d_cframe, d_cvotes, d_coff, d_ncand, d_hvote, d_useful; vxu::Dev<double> d_hpose, d_poses;
  vxu::Dev<long long> d_tab; vxu::Dev<vxlr::PairDesc> d_pairs;
  int64_t n_matches = 0, launches = 0, syncs = 0;
  // the search over several sessions: its match list (kept for read_matches) and sort scratch, the pinned block both of its copies go through,
  // and the S + 1 offsets of the sessions' lists (empty after a single search)
  vxu::Arena mlist; int *m_mq = nullptr, *m_mf = nullptr, *m_mi = nullptr;
  vxu::Pin<char> pin;
  std::vector<int64_t> moff;
};

namespace vxls {

using vxu::blocks_for, vxu::fail;

static void defaults(vxba_loopsearch_params* p) {
  p->descriptor_near_num = 15; p->descriptor_min_len = 2; p->descriptor_max_len = 50; p->std_side_resolution = 0.2;
  p->skip_near_num = 30; p->candidate_num = 20; p->rough_dis_threshold = 0.01; p->similarity_threshold = 0.7; p->icp_threshold = 0.15;
  p->normal_threshold = 0.2; p->dis_threshold = 0.5;
}

static int check_params(vxba_loopsearch* h, const char* what, const vxba_loopsearch_params& p) {
  const std::string w(what);
  if (p.descriptor_near_num < 3 || p.descriptor_near_num > MAXK) return fail(h, VXBA_ERR_ARG, w + ": descriptor_near_num outside 3..32");
  if (!(p.std_side_resolution > 0) || !std::isfinite(p.std_side_resolution) || !(p.descriptor_min_len / p.std_side_resolution >= 2.0))
    return fail(h, VXBA_ERR_ARG, w + ": descriptor_min_len / std_side_resolution must be at least 2");
  if (!(p.descriptor_max_len > p.descriptor_min_len) || !(p.descriptor_max_len <= 2000.0) || !(p.descriptor_max_len / p.std_side_resolution < 1e6))
    return fail(h, VXBA_ERR_ARG, w + ": descriptor_max_len outside (descriptor_min_len, 2000], or more than 1e6 cells long");
  if (p.candidate_num < 1 || p.candidate_num > MAXCAND) return fail(h, VXBA_ERR_ARG, w + ": candidate_num outside 1..64");
  if (!std::isfinite(p.rough_dis_threshold) || !std::isfinite(p.similarity_threshold) || !std::isfinite(p.icp_threshold) || !std::isfinite(p.normal_threshold) ||
      !std::isfinite(p.dis_threshold))
    return fail(h, VXBA_ERR_ARG, w + ": a threshold is not finite");
  return VXBA_OK;
}

static Rec rec_at(void* base, int n) {
  Rec r;
  char* b = (char*)base;
  r.f = (double*)b; b += (size_t)NF * 8 * n;
  r.occ = (unsigned long long*)b; b += (size_t)3 * 8 * n;
  r.next = (unsigned long long*)b; b += (size_t)8 * n;
  r.pos = (int*)b;
  r.n = n; r.stride = n;
  return r;
}

// a cell table of `cap` slots (a power of two) in one block, empty
static int table_alloc(vxba_loopsearch* h, vxu::Dev<char>& mem, Table& t, size_t cap) {
  t = Table{};
  VX_HIP(h, mem.reserve(cap * 20));
  t.key = (unsigned long long*)mem.get(); t.head = (unsigned long long*)(mem.get() + cap * 8); t.count = (int*)(mem.get() + cap * 16);
  VX_HIP(h, hipMemsetAsync(t.key, 0xff, cap * 8, h->s)); VX_HIP(h, hipMemsetAsync(t.count, 0, cap * 4, h->s));
  t.mask = (unsigned)(cap - 1);
  return VXBA_OK;
}

static void drop_database(vxba_loopsearch* h) {
  h->blocks.clear(); h->frames.clear();
  h->tb_mem.release(); h->tb = Table{}; h->tb_used_ub = 0; h->n_db = 0; h->rec_bytes = 0; h->n_matches = 0;
}

}  // namespace vxls

extern "C" {

int vxba_loopsearch_create(int device, vxba_loopreg* clouds, vxba_loopsearch** out) {
  if (!out) return VXBA_ERR_ARG;
  *out = nullptr;
  if (!clouds) return VXBA_ERR_ARG;
  if (const int rc = vxu::select_device(device)) return rc;
  vxba_loopsearch* h = new vxba_loopsearch();
  h->device = device; h->reg = clouds; h->s = vxlr::stream_of(clouds); h->reg_generation = vxlr::generation_of(clouds);
  const int nc = MAXCAND;
  const bool ok = h->d_total.reserve(1) == hipSuccess && h->d_cframe.reserve(nc) == hipSuccess && h->d_cvotes.reserve(nc) == hipSuccess && h->d_coff.reserve(nc) == hipSuccess &&
                  h->d_ncand.reserve(1) == hipSuccess && h->d_hvote.reserve((size_t)nc * HYP) == hipSuccess && h->d_useful.reserve(nc) == hipSuccess &&
                  h->d_hpose.reserve((size_t)12 * nc * HYP) == hipSuccess && h->d_poses.reserve((size_t)12 * nc) == hipSuccess && h->d_tab.reserve((size_t)CI * nc) == hipSuccess &&
                  h->d_pairs.reserve(nc) == hipSuccess;
  if (!ok) { delete h; return VXBA_ERR_HIP; }
  *out = h;
  return VXBA_OK;
}

int vxba_loopsearch_clear(vxba_loopsearch* h) {
  if (!h) return VXBA_ERR_ARG;
  hipSetDevice(h->device);
  hipStreamSynchronize(h->s);
  drop_database(h);
  h->nd = 0;
  h->reg_generation = vxlr::generation_of(h->reg);
  return VXBA_OK;
}

int vxba_loopsearch_destroy(vxba_loopsearch* h) {
  if (!h) return VXBA_OK;
  hipSetDevice(h->device);
  hipStreamSynchronize(h->s);
  h->work.release(); h->mlist.release();
  delete h;
  return VXBA_OK;
}

const char* vxba_loopsearch_last_error(const vxba_loopsearch* h) { return h ? h->err.c_str() : "null handle"; }

int vxba_loopsearch_num_frames(const vxba_loopsearch* h) { return h ? (int)h->frames.size() : 0; }

int64_t vxba_loopsearch_num_descriptors(const vxba_loopsearch* h, int which) {
  if (!h) return -1;
  if (which == -1) return h->n_db;
  if (which == -2) return h->nd;
  return which >= 0 && which < (int)h->frames.size() ? (int64_t)h->frames[which].r.n : -1;
}

void vxba_loopsearch_default_params(vxba_loopsearch_params* p) { if (p) defaults(p); }

int vxba_loopsearch_describe(vxba_loopsearch* h, int64_t n64, const double* loc, const uint64_t* occ, const vxba_loopsearch_params* params, int64_t* n_desc) {
  if (!h) return VXBA_ERR_ARG;
  if (n64 < 0 || n64 > MAXN || (n64 > 0 && (!loc || !occ))) return fail(h, VXBA_ERR_ARG, "loopsearch_describe: bad argument (at most " + std::to_string(MAXN) + " corners)");
  vxba_loopsearch_params p;
  if (params) p = *params; else defaults(&p);
  int rc = check_params(h, "loopsearch_describe", p);
  if (rc != VXBA_OK) return rc;
  const int n = (int)n64;
  for (int k = 0; k < 3 * n; k++)
    if (!(std::fabs(loc[k]) < 1e18)) return fail(h, VXBA_ERR_ARG, "loopsearch_describe: corner " + std::to_string(k / 3) + " is not finite (or beyond 1e18)");
  VX_HIP(h, hipSetDevice(h->device));
  const int K = p.descriptor_near_num < n ? p.descriptor_near_num : n;
  const int P = K >= 3 ? (K - 1) * (K - 2) / 2 : 0;
  const size_t nslots = (size_t)n * P;
  if (n_desc) *n_desc = 0;
  if (nslots == 0) { h->nd = 0; return VXBA_OK; }
  VX_HIP(h, h->d_loc.reserve((size_t)3 * n)); VX_HIP(h, h->d_occ.reserve((size_t)n));
  VX_HIP(h, h->d_key.reserve(nslots)); VX_HIP(h, h->d_key_s.reserve(nslots)); VX_HIP(h, h->d_val.reserve(nslots)); VX_HIP(h, h->d_val_s.reserve(nslots)); VX_HIP(h, h->d_flag.reserve(nslots));
  VX_HIP(h, h->d_pos.reserve(nslots)); VX_HIP(h, h->d_vert.reserve(3 * nslots)); VX_HIP(h, h->d_sides.reserve(3 * nslots));
  if (nslots * (NF * 8 + 3 * 8) > h->d_cur.capacity()) {      // the set, its corner ids and its cells are laid out by one stride: d_cur last, so its capacity says that all three are there
    h->nd = 0; h->cur = Rec{};
    h->d_cur.release();
    VX_HIP(h, h->d_cid.reserve(3 * nslots)); VX_HIP(h, h->d_cell.reserve(nslots)); VX_HIP(h, h->d_cur.reserve(nslots * (NF * 8 + 3 * 8)));
    char* base = h->d_cur.get();
    h->cur.f = (double*)base; h->cur.occ = (unsigned long long*)(base + nslots * NF * 8); h->cur.stride = (int)nslots;
  }
  vxu::Temp temp;
  VX_HIP(h, vxu::sort_temp<unsigned long long, unsigned int>(temp.bytes, nslots, 64, h->s));
  VX_HIP(h, vxu::scan_temp<unsigned int>(temp.bytes, nslots, h->s));
  VX_HIP(h, h->work.layout([&](vxu::Arena& a) { temp.p = a.take<char>(temp.bytes); }, h->s));
  VX_HIP(h, hipMemcpyAsync(h->d_loc, loc, sizeof(double) * 3 * n, hipMemcpyHostToDevice, h->s));
  VX_HIP(h, hipMemcpyAsync(h->d_occ, occ, sizeof(uint64_t) * n, hipMemcpyHostToDevice, h->s));
  hipLaunchKernelGGL(triangle_kernel, dim3(n), dim3(64), 0, h->s, (const double*)h->d_loc, n, K, p.descriptor_min_len, p.descriptor_max_len, h->d_key, h->d_val, h->d_vert, h->d_sides);
  VX_HIP(h, vxu::sort(temp, h->d_key.get(), h->d_key_s.get(), h->d_val.get(), h->d_val_s.get(), nslots, 64, h->s));
  hipLaunchKernelGGL(mark_kernel, dim3(blocks_for(nslots)), dim3(256), 0, h->s, (const unsigned long long*)h->d_key_s, (const unsigned int*)h->d_val_s, (int)nslots, h->d_flag);
  VX_HIP(h, vxu::scan(temp, h->d_flag.get(), h->d_pos.get(), nslots, h->s));
  const double scale = 1.0 / p.std_side_resolution;
  hipLaunchKernelGGL(compact_kernel, dim3(blocks_for(nslots)), dim3(256), 0, h->s, (int)nslots, (const unsigned int*)h->d_flag, (const unsigned int*)h->d_pos, (const int*)h->d_vert,
                     (const double*)h->d_sides, (const double*)h->d_loc, (const unsigned long long*)h->d_occ, scale, h->cur, h->d_cid, h->d_cell, h->d_total);
  VX_HIP(h, hipGetLastError());
  unsigned int total = 0;
  VX_HIP(h, hipMemcpyAsync(&total, h->d_total, 4, hipMemcpyDeviceToHost, h->s));
  VX_HIP(h, hipStreamSynchronize(h->s));
  h->nd = (int)total; h->cur.n = (int)total;
  if (n_desc) *n_desc = total;
  return VXBA_OK;
}

int vxba_loopsearch_read_descriptors(vxba_loopsearch* h, double* triangle, double* centre, int32_t* corners) {
  if (!h) return VXBA_ERR_ARG;
  const int nd = h->nd;
  if (nd == 0) return VXBA_OK;
  VX_HIP(h, hipSetDevice(h->device));
  const size_t st = h->cur.stride;
  std::vector<double> f((size_t)6 * nd); std::vector<int> c((size_t)3 * nd);
  for (int p = 0; p < 6; p++) VX_HIP(h, hipMemcpyAsync(f.data() + (size_t)p * nd, h->cur.f + p * st, sizeof(double) * nd, hipMemcpyDeviceToHost, h->s));
  for (int p = 0; p < 3; p++) VX_HIP(h, hipMemcpyAsync(c.data() + (size_t)p * nd, h->d_cid + p * st, sizeof(int) * nd, hipMemcpyDeviceToHost, h->s));
  VX_HIP(h, hipStreamSynchronize(h->s));
  for (int i = 0; i < nd; i++)
    for (int k = 0; k < 3; k++) {
      if (triangle) triangle[3 * (size_t)i + k] = f[(size_t)k * nd + i];
      if (centre) centre[3 * (size_t)i + k] = f[(size_t)(3 + k) * nd + i];
      if (corners) corners[3 * (size_t)i + k] = c[(size_t)k * nd + i];
    }
  return VXBA_OK;
}

int vxba_loopsearch_add(vxba_loopsearch* h, int cloud_id) {
  if (!h) return VXBA_ERR_ARG;
  const float* cd = nullptr; int cn = 0;
  if (!vxlr::cloud_of(h->reg, cloud_id, &cd, &cn)) return fail(h, VXBA_ERR_ARG, "loopsearch_add: cloud " + std::to_string(cloud_id) + " is out of range");
  if (h->reg_generation != vxlr::generation_of(h->reg)) {
    if (!h->frames.empty()) return fail(h, VXBA_ERR_STATE, "loopsearch_add: the registration handle was cleared; clear the search handle too");
    h->reg_generation = vxlr::generation_of(h->reg);
  }
  VX_HIP(h, hipSetDevice(h->device));
  const int nd = h->nd, F = (int)h->frames.size();
  // the frame table and what is sized by it
  if ((size_t)F + 1 > h->d_frames.capacity()) {
    const size_t cap = h->d_frames.capacity() ? 2 * h->d_frames.capacity() : 64;
    vxu::Dev<Frame> nf;
    VX_HIP(h, nf.reserve(cap));
    if (F) VX_HIP(h, hipMemcpyAsync(nf, h->d_frames, sizeof(Frame) * F, hipMemcpyDeviceToDevice, h->s));
    VX_HIP(h, hipStreamSynchronize(h->s));
    h->d_frames = std::move(nf);
  }
  VX_HIP(h, h->d_votes.reserve((size_t)F + 1, h->d_frames.capacity())); VX_HIP(h, h->d_cand_of_frame.reserve((size_t)F + 1, h->d_frames.capacity()));
  // the cell table: at most half full
  const size_t want = 2 * (h->tb_used_ub + (size_t)nd);
  if (!h->tb.key || want > (size_t)h->tb.mask + 1) {
    size_t cap = h->tb.key ? (size_t)h->tb.mask + 1 : 1024;
    while (cap < want) cap *= 2;
    Table nt;
    vxu::Dev<char> nt_mem;
    int rc = table_alloc(h, nt_mem, nt, cap);
    if (rc != VXBA_OK) return rc;
    if (h->tb.key) hipLaunchKernelGGL(rehash_kernel, dim3(blocks_for((long long)h->tb.mask + 1)), dim3(256), 0, h->s, h->tb, nt);
    VX_HIP(h, hipStreamSynchronize(h->s));
    h->tb_mem = std::move(nt_mem);
    h->tb = nt;
  }
  vxu::Dev<char> blk;      // gone with every error return below; the database takes it at the end
  VX_HIP(h, blk.reserve((nd ? (size_t)nd : 1) * REC_BYTES));
  Frame fr;
  fr.r = rec_at(blk.get(), nd); fr.cloud = cd; fr.cloud_n = cn; fr.cloud_id = cloud_id;
  if (nd) {
    vxu::Temp temp;
    hipError_t e = vxu::sort_temp<unsigned long long, unsigned int>(temp.bytes, (size_t)nd, 64, h->s);
    if (e == hipSuccess) e = h->work.layout([&](vxu::Arena& a) { temp.p = a.take<char>(temp.bytes); }, h->s);
    if (e != hipSuccess) return fail(h, VXBA_ERR_HIP, "loopsearch_add: no room for the sort");
    hipLaunchKernelGGL(iota_kernel, dim3(blocks_for(nd)), dim3(256), 0, h->s, h->d_pos, nd);      // the sort's values; d_pos is free outside describe
    e = vxu::sort(temp, h->d_cell.get(), h->d_key_s.get(), h->d_pos.get(), h->d_val_s.get(), (size_t)nd, 64, h->s);
    if (e != hipSuccess) return fail(h, VXBA_ERR_HIP, std::string("loopsearch_add: ") + hipGetErrorString(e));
    hipLaunchKernelGGL(add_runs_kernel, dim3(blocks_for(nd)), dim3(256), 0, h->s, (const unsigned long long*)h->d_key_s, (const unsigned int*)h->d_val_s, nd, F, h->tb, fr.r);
    hipLaunchKernelGGL(copy_kernel, dim3(blocks_for(nd)), dim3(256), 0, h->s, h->cur, fr.r, nd);
  }
  hipError_t e = hipMemcpyAsync(h->d_frames + F, &fr, sizeof(Frame), hipMemcpyHostToDevice, h->s);
  if (e == hipSuccess) e = hipStreamSynchronize(h->s);
  if (e == hipSuccess) e = hipGetLastError();
  if (e != hipSuccess) return fail(h, VXBA_ERR_HIP, std::string("loopsearch_add: ") + hipGetErrorString(e));
  h->frames.push_back(fr); h->blocks.push_back(std::move(blk));
  h->tb_used_ub += nd; h->n_db += nd; h->rec_bytes += (int64_t)nd * (int64_t)REC_BYTES;
  return VXBA_OK;
}

int vxba_loopsearch_search(vxba_loopsearch* h, int cloud_cur, const vxba_loopsearch_params* params, int* frame, double* score, double pose[12], int* n_candidates,
                           int64_t* cand_ints, double* cand_doubles) {
  if (!h || !frame) return fail(h, VXBA_ERR_ARG, "loopsearch_search: bad argument");
  vxba_loopsearch_params p;
  if (params) p = *params; else defaults(&p);
  int rc = check_params(h, "loopsearch_search", p);
  if (rc != VXBA_OK) return rc;
  const float* cd = nullptr; int cn = 0;
  if (!vxlr::cloud_of(h->reg, cloud_cur, &cd, &cn)) return fail(h, VXBA_ERR_ARG, "loopsearch_search: cloud " + std::to_string(cloud_cur) + " is out of range");
  if (!h->frames.empty() && h->reg_generation != vxlr::generation_of(h->reg))
    return fail(h, VXBA_ERR_STATE, "loopsearch_search: the registration handle was cleared; clear the search handle too");
  *frame = -1;
  if (score) *score = 0.0;
  if (n_candidates) *n_candidates = 0;
  h->launches = h->syncs = 0; h->n_matches = 0; h->moff.clear();
  const int nd = h->nd, F = (int)h->frames.size(), NC = p.candidate_num;
  if (nd == 0 || F == 0) return VXBA_OK;               // SearchLoop's early return; an empty database has nothing to visit
  VX_HIP(h, hipSetDevice(h->device));
  const size_t nq = (size_t)nd * 27;
  VX_HIP(h, h->d_cnt.reserve(nq + 1)); VX_HIP(h, h->d_off.reserve(nq + 1));
  vxu::Temp temp;
  VX_HIP(h, vxu::scan_temp<int>(temp.bytes, nq + 1, h->s));
  VX_HIP(h, h->work.layout([&](vxu::Arena& a) { temp.p = a.take<char>(temp.bytes); }, h->s));
  const int frame_cur = F;
  hipLaunchKernelGGL(query_kernel<false>, dim3(blocks_for(nq + 1)), dim3(256), 0, h->s, h->cur, nd, h->tb, (const Frame*)h->d_frames, frame_cur, p.skip_near_num, p.rough_dis_threshold,
                     p.similarity_threshold, h->d_cnt, (const int*)h->d_off, h->d_mq, h->d_mf, h->d_mi, h->d_votes);
  VX_HIP(h, vxu::scan(temp, h->d_cnt.get(), h->d_off.get(), nq + 1, h->s));
  h->launches += 2;
  int M = 0;
  VX_HIP(h, hipMemcpyAsync(&M, h->d_off + nq, 4, hipMemcpyDeviceToHost, h->s));
  VX_HIP(h, hipStreamSynchronize(h->s));
  h->syncs += 1;
  const size_t Ms = M > 0 ? (size_t)M : 1;
  VX_HIP(h, h->d_mq.reserve(Ms)); VX_HIP(h, h->d_mf.reserve(Ms)); VX_HIP(h, h->d_mi.reserve(Ms)); VX_HIP(h, h->d_ck.reserve(Ms)); VX_HIP(h, h->d_ck_s.reserve(Ms)); VX_HIP(h, h->d_cv.reserve(Ms)); VX_HIP(h, h->d_cv_s.reserve(Ms));
  VX_HIP(h, vxu::sort_temp<unsigned int, unsigned int>(temp.bytes, Ms, 8, h->s));
  VX_HIP(h, h->work.layout([&](vxu::Arena& a) { temp.p = a.take<char>(temp.bytes); }, h->s));
  VX_HIP(h, hipMemsetAsync(h->d_votes, 0, sizeof(int) * F, h->s));
  VX_HIP(h, hipMemsetAsync(h->d_cand_of_frame, 0xff, sizeof(int) * F, h->s));
  VX_HIP(h, hipMemsetAsync(h->d_useful, 0, sizeof(int) * NC, h->s));
  VX_HIP(h, hipMemsetAsync(h->d_ck, 0xff, sizeof(unsigned int) * Ms, h->s));
  hipLaunchKernelGGL(query_kernel<true>, dim3(blocks_for(nq)), dim3(256), 0, h->s, h->cur, nd, h->tb, (const Frame*)h->d_frames, frame_cur, p.skip_near_num, p.rough_dis_threshold,
                     p.similarity_threshold, h->d_cnt, (const int*)h->d_off, h->d_mq, h->d_mf, h->d_mi, h->d_votes);
  hipLaunchKernelGGL(select_kernel, dim3(1), dim3(256), 0, h->s, h->d_votes, F, NC, h->d_cand_of_frame, h->d_cframe, h->d_cvotes, h->d_coff, h->d_ncand);
  hipLaunchKernelGGL(candkey_kernel, dim3(blocks_for(M)), dim3(256), 0, h->s, (const int*)h->d_mf, M, (const int*)h->d_cand_of_frame, h->d_ck, h->d_cv);
  VX_HIP(h, vxu::sort(temp, h->d_ck.get(), h->d_ck_s.get(), h->d_cv.get(), h->d_cv_s.get(), Ms, 8, h->s));
  hipLaunchKernelGGL(verify_kernel, dim3(HYP, NC), dim3(256), 0, h->s, h->cur, (const Frame*)h->d_frames, (const int*)h->d_mq, (const int*)h->d_mf, (const int*)h->d_mi,
                     (const unsigned int*)h->d_cv_s, (const int*)h->d_cvotes, (const int*)h->d_coff, (const int*)h->d_ncand, h->d_hvote, h->d_hpose);
  hipLaunchKernelGGL(best_kernel, dim3(NC), dim3(64), 0, h->s, (const Frame*)h->d_frames, (const int*)h->d_cframe, (const int*)h->d_cvotes, (const int*)h->d_ncand, (const int*)h->d_hvote,
                     (const double*)h->d_hpose, cd, cn, h->d_tab, h->d_poses, h->d_pairs);
  vxlr::enqueue_score(h->reg, NC, cn, h->d_pairs, h->d_poses, h->d_useful, p.normal_threshold, p.dis_threshold);
  h->launches += 7;
  VX_HIP(h, hipGetLastError());
  int nc = 0;
  std::vector<long long> tab((size_t)CI * NC); std::vector<double> poses((size_t)12 * NC); std::vector<int> useful(NC);
  VX_HIP(h, hipMemcpyAsync(&nc, h->d_ncand, 4, hipMemcpyDeviceToHost, h->s));
  VX_HIP(h, hipMemcpyAsync(tab.data(), h->d_tab, sizeof(long long) * CI * NC, hipMemcpyDeviceToHost, h->s));
  VX_HIP(h, hipMemcpyAsync(poses.data(), h->d_poses, sizeof(double) * 12 * NC, hipMemcpyDeviceToHost, h->s));
  VX_HIP(h, hipMemcpyAsync(useful.data(), h->d_useful, sizeof(int) * NC, hipMemcpyDeviceToHost, h->s));
  VX_HIP(h, hipStreamSynchronize(h->s));
  h->syncs += 1;
  h->n_matches = M;
  double best = 0.0; int bc = -1;
  for (int c = 0; c < nc; c++) {
    long long* row = tab.data() + (size_t)CI * c;
    double sc = -1.0;
    if (row[5] >= 4) { row[6] = useful[c]; sc = cn > 0 ? (double)useful[c] / (double)cn : 0.0; }
    if (sc > best) { best = sc; bc = c; }
    if (cand_ints) for (int k = 0; k < CI; k++) cand_ints[(size_t)CI * c + k] = row[k];
    if (cand_doubles) { cand_doubles[(size_t)CD * c] = sc; std::memcpy(cand_doubles + (size_t)CD * c + 1, poses.data() + (size_t)12 * c, sizeof(double) * 12); }
  }
  if (n_candidates) *n_candidates = nc;
  if (bc >= 0 && best > p.icp_threshold) {
    *frame = (int)tab[(size_t)CI * bc];
    if (score) *score = best;
    if (pose) std::memcpy(pose, poses.data() + (size_t)12 * bc, sizeof(double) * 12);
  }
  return VXBA_OK;
}

int vxba_loopsearch_search_multi(vxba_loopsearch* h, int S, vxba_loopsearch* const* dbs, const int* skip_near_num, int cloud_cur, const vxba_loopsearch_params* params,
                                 int* frame, double* score, double* pose, int* n_candidates, int64_t* cand_ints, double* cand_doubles) {
  if (!h || !frame || !dbs || !skip_near_num || S < 1 || S > VXBA_LOOPSEARCH_MAX_SESSIONS)
    return fail(h, VXBA_ERR_ARG, "loopsearch_search_multi: bad argument (1.." + std::to_string(VXBA_LOOPSEARCH_MAX_SESSIONS) + " sessions)");
  for (int s = 0; s < S; s++)
    if (!dbs[s] || dbs[s]->device != h->device || dbs[s]->reg != h->reg)
      return fail(h, VXBA_ERR_ARG, "loopsearch_search_multi: session " + std::to_string(s) + " is null, on another device or attached to another registration handle");
  vxba_loopsearch_params p;
  if (params) p = *params; else defaults(&p);
  int rc = check_params(h, "loopsearch_search_multi", p);
  if (rc != VXBA_OK) return rc;
  const float* cd = nullptr; int cn = 0;
  if (!vxlr::cloud_of(h->reg, cloud_cur, &cd, &cn)) return fail(h, VXBA_ERR_ARG, "loopsearch_search_multi: cloud " + std::to_string(cloud_cur) + " is out of range");
  for (int s = 0; s < S; s++)
    if (!dbs[s]->frames.empty() && dbs[s]->reg_generation != vxlr::generation_of(h->reg))
      return fail(h, VXBA_ERR_STATE, "loopsearch_search_multi: the registration handle was cleared; clear the search handle of session " + std::to_string(s) + " too");
  const int NC = p.candidate_num, B = S * NC, nd = h->nd, frame_cur = (int)h->frames.size();
  for (int s = 0; s < S; s++) {
    frame[s] = -1;
    if (score) score[s] = 0.0;
    if (n_candidates) n_candidates[s] = 0;
  }
  h->launches = h->syncs = 0; h->n_matches = 0; h->moff.assign((size_t)S + 1, 0);
  // the table of the sessions: what goes up in the one pinned copy
  Sess tab_h[VXBA_LOOPSEARCH_MAX_SESSIONS];
  size_t totalF = 0;
  for (int s = 0; s < S; s++) {
    const vxba_loopsearch* d = dbs[s];
    tab_h[s] = Sess{d->tb, d->d_frames, (int)d->frames.size(), skip_near_num[s], (int)totalF};
    totalF += d->frames.size();
  }
  if (nd == 0 || totalF == 0) return VXBA_OK;           // SearchLoop's early return, in every session
  VX_HIP(h, hipSetDevice(h->device));
  const size_t nq = (size_t)nd * 27, ncnt = (size_t)S * nq + 1;
  if (ncnt > (size_t)std::numeric_limits<int>::max()) return fail(h, VXBA_ERR_UNSUPPORTED, "loopsearch_search_multi: more than 2^31 (session, descriptor, cell) lanes");
  // one block for everything that comes back: the candidate tables, their poses, then useful, the candidate counts and the lists' offsets
  const size_t res_bytes = (size_t)B * (CI * 8 + 12 * 8 + 4) + (size_t)(2 * S + 1) * 4;
  const size_t pin_bytes = res_bytes > sizeof(tab_h) ? res_bytes : sizeof(tab_h);
  if (pin_bytes > h->pin.capacity()) {
    if (h->pin) VX_HIP(h, hipStreamSynchronize(h->s));
    VX_HIP(h, h->pin.reserve(pin_bytes));
  }
  Sess* d_sess = nullptr; int *d_cnt = nullptr, *d_off = nullptr, *d_votes = nullptr, *d_cof = nullptr, *d_cframe = nullptr, *d_cvotes = nullptr, *d_coff = nullptr, *d_hvote = nullptr;
  double* d_hpose = nullptr; char* d_res = nullptr; vxlr::PairDesc* d_pairs = nullptr;
  vxu::Temp temp;
  VX_HIP(h, vxu::scan_temp<int>(temp.bytes, ncnt, h->s));
  VX_HIP(h, h->work.layout([&](vxu::Arena& a) {
    d_sess = a.take<Sess>(VXBA_LOOPSEARCH_MAX_SESSIONS); d_cnt = a.take<int>(ncnt); d_off = a.take<int>(ncnt); d_votes = a.take<int>(totalF); d_cof = a.take<int>(totalF);
    d_cframe = a.take<int>(B); d_cvotes = a.take<int>(B); d_coff = a.take<int>(B); d_hvote = a.take<int>((size_t)B * HYP); d_hpose = a.take<double>((size_t)B * HYP * 12);
    d_res = a.take<char>(res_bytes); d_pairs = a.take<vxlr::PairDesc>(B); temp.p = a.take<char>(temp.bytes);
  }, h->s));
  long long* d_tab = (long long*)d_res; double* d_poses = (double*)(d_tab + (size_t)B * CI);
  int *d_useful = (int*)(d_poses + (size_t)B * 12), *d_ncand = d_useful + B, *d_moff = d_ncand + S;
  std::memcpy(h->pin, tab_h, sizeof(Sess) * S);
  VX_HIP(h, hipMemcpyAsync(d_sess, h->pin, sizeof(Sess) * S, hipMemcpyHostToDevice, h->s));
  hipLaunchKernelGGL(multi_query_kernel<false>, dim3(blocks_for(nq), S), dim3(256), 0, h->s, h->cur, nd, (const Sess*)d_sess, S, frame_cur, p.rough_dis_threshold, p.similarity_threshold,
                     d_cnt, (const int*)d_off, (int*)nullptr, (int*)nullptr, (int*)nullptr, d_votes, d_moff);
  VX_HIP(h, vxu::scan(temp, d_cnt, d_off, ncnt, h->s));
  h->launches += 2;
  int M = 0;
  VX_HIP(h, hipMemcpyAsync(&M, d_off + (ncnt - 1), 4, hipMemcpyDeviceToHost, h->s));
  VX_HIP(h, hipStreamSynchronize(h->s));
  h->syncs += 1;
  const size_t Ms = M > 0 ? (size_t)M : 1;
  unsigned int *d_ck = nullptr, *d_ck_s = nullptr, *d_cv = nullptr, *d_cv_s = nullptr;
  vxu::Temp stemp;
  VX_HIP(h, vxu::sort_temp<unsigned int, unsigned int>(stemp.bytes, Ms, 12, h->s));
  VX_HIP(h, h->mlist.layout([&](vxu::Arena& a) {
    h->m_mq = a.take<int>(Ms); h->m_mf = a.take<int>(Ms); h->m_mi = a.take<int>(Ms);
    d_ck = a.take<unsigned int>(Ms); d_ck_s = a.take<unsigned int>(Ms); d_cv = a.take<unsigned int>(Ms); d_cv_s = a.take<unsigned int>(Ms); stemp.p = a.take<char>(stemp.bytes);
  }, h->s));
  VX_HIP(h, hipMemsetAsync(d_votes, 0, sizeof(int) * totalF, h->s));
  VX_HIP(h, hipMemsetAsync(d_cof, 0xff, sizeof(int) * totalF, h->s));
  VX_HIP(h, hipMemsetAsync(d_useful, 0, sizeof(int) * B, h->s));
  VX_HIP(h, hipMemsetAsync(d_ck, 0xff, sizeof(unsigned int) * Ms, h->s));
  hipLaunchKernelGGL(multi_query_kernel<true>, dim3(blocks_for(nq), S), dim3(256), 0, h->s, h->cur, nd, (const Sess*)d_sess, S, frame_cur, p.rough_dis_threshold, p.similarity_threshold,
                     d_cnt, (const int*)d_off, h->m_mq, h->m_mf, h->m_mi, d_votes, d_moff);
  hipLaunchKernelGGL(multi_select_kernel, dim3(S), dim3(256), 0, h->s, (const Sess*)d_sess, d_votes, NC, d_cof, d_cframe, d_cvotes, d_coff, d_ncand, (const int*)d_moff);
  hipLaunchKernelGGL(multi_candkey_kernel, dim3(blocks_for(M)), dim3(256), 0, h->s, (const int*)h->m_mf, M, S, (const int*)d_moff, (const int*)d_cof, d_ck, d_cv);
  VX_HIP(h, vxu::sort(stemp, d_ck, d_ck_s, d_cv, d_cv_s, Ms, 12, h->s));
  hipLaunchKernelGGL(multi_verify_kernel, dim3(HYP, NC, S), dim3(256), 0, h->s, h->cur, (const Sess*)d_sess, NC, (const int*)h->m_mq, (const int*)h->m_mf, (const int*)h->m_mi,
                     (const unsigned int*)d_cv_s, (const int*)d_cvotes, (const int*)d_coff, (const int*)d_ncand, d_hvote, d_hpose);
  hipLaunchKernelGGL(multi_best_kernel, dim3(NC, S), dim3(64), 0, h->s, (const Sess*)d_sess, NC, (const int*)d_cframe, (const int*)d_cvotes, (const int*)d_ncand, (const int*)d_hvote,
                     (const double*)d_hpose, cd, cn, d_tab, d_poses, d_pairs);
  vxlr::enqueue_score(h->reg, B, cn, d_pairs, d_poses, d_useful, p.normal_threshold, p.dis_threshold);
  h->launches += 7;
  VX_HIP(h, hipGetLastError());
  VX_HIP(h, hipMemcpyAsync(h->pin, d_res, res_bytes, hipMemcpyDeviceToHost, h->s));
  VX_HIP(h, hipStreamSynchronize(h->s));
  h->syncs += 1;
  h->n_matches = M;
  long long* tab = (long long*)h->pin.get(); const double* poses = (const double*)(tab + (size_t)B * CI);
  const int *useful = (const int*)(poses + (size_t)B * 12), *ncand = useful + B, *moff = ncand + S;
  for (int s = 0; s <= S; s++) h->moff[s] = moff[s];
  for (int s = 0; s < S; s++) {                         // per session what the single search does with its table
    double best = 0.0; int bc = -1;
    for (int c = 0; c < ncand[s]; c++) {
      const size_t r = (size_t)s * NC + c;
      long long* row = tab + CI * r;
      double sc = -1.0;
      if (row[5] >= 4) { row[6] = useful[r]; sc = cn > 0 ? (double)useful[r] / (double)cn : 0.0; }
      if (sc > best) { best = sc; bc = c; }
      if (cand_ints) for (int k = 0; k < CI; k++) cand_ints[CI * r + k] = row[k];
      if (cand_doubles) { cand_doubles[CD * r] = sc; std::memcpy(cand_doubles + CD * r + 1, poses + 12 * r, sizeof(double) * 12); }
    }
    if (n_candidates) n_candidates[s] = ncand[s];
    if (bc >= 0 && best > p.icp_threshold) {
      const size_t r = (size_t)s * NC + bc;
      frame[s] = (int)tab[CI * r];
      if (score) score[s] = best;
      if (pose) std::memcpy(pose + 12 * (size_t)s, poses + 12 * r, sizeof(double) * 12);
    }
  }
  return VXBA_OK;
}

int vxba_loopsearch_read_match_offsets(vxba_loopsearch* h, int64_t* out) {
  if (!h || !out) return fail(h, VXBA_ERR_ARG, "loopsearch_read_match_offsets: bad argument");
  if (h->moff.empty()) return fail(h, VXBA_ERR_STATE, "loopsearch_read_match_offsets: the last search was not vxba_loopsearch_search_multi");
  for (size_t s = 0; s < h->moff.size(); s++) out[s] = h->moff[s];
  return VXBA_OK;
}

int vxba_loopsearch_read_matches(vxba_loopsearch* h, int64_t capacity, int32_t* rows, int64_t* n) {
  if (!h || !n || capacity < 0 || (capacity > 0 && !rows)) return fail(h, VXBA_ERR_ARG, "loopsearch_read_matches: bad argument");
  *n = h->n_matches;
  const size_t m = (size_t)(capacity < h->n_matches ? capacity : h->n_matches);
  if (m == 0) return VXBA_OK;
  VX_HIP(h, hipSetDevice(h->device));
  std::vector<int> q(m), f(m), i(m);
  const bool multi = !h->moff.empty();                  // the list of the last search, whichever it was
  VX_HIP(h, hipMemcpyAsync(q.data(), multi ? h->m_mq : h->d_mq, 4 * m, hipMemcpyDeviceToHost, h->s));
  VX_HIP(h, hipMemcpyAsync(f.data(), multi ? h->m_mf : h->d_mf, 4 * m, hipMemcpyDeviceToHost, h->s));
  VX_HIP(h, hipMemcpyAsync(i.data(), multi ? h->m_mi : h->d_mi, 4 * m, hipMemcpyDeviceToHost, h->s));
  VX_HIP(h, hipStreamSynchronize(h->s));
  for (size_t k = 0; k < m; k++) { rows[3 * k] = q[k]; rows[3 * k + 1] = f[k]; rows[3 * k + 2] = i[k]; }
  return VXBA_OK;
}

int vxba_loopsearch_stats(const vxba_loopsearch* h, int64_t out[6]) {
  if (!h || !out) return VXBA_ERR_ARG;
  out[0] = h->launches; out[1] = h->syncs; out[2] = (int64_t)h->frames.size(); out[3] = h->n_db; out[4] = h->rec_bytes;
  out[5] = h->tb.key ? ((int64_t)h->tb.mask + 1) * 20 : 0;
  return VXBA_OK;
}

}  // extern "C"
