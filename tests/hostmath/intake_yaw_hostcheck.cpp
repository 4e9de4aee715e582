// Host build of the yaw-time arithmetic of voxel-slam_amd/csrc/vxba_intake_math.hpp for tests/test_intake_yaw_cpu.py: the text the yaw kernels of
// vxba_intake.hip run, compiled with g++ (-ffp-contract=off, as the device unit), against tests/_intake_yaw_ref.py.  ikh_yaw_walk strings the
// functions together the way the kernels do -- one step per kernel, the resolver pass by pass over 64 "lanes" -- so that the CPU suite checks the
// parallel form itself and not only its pieces.
#include <cstdint>
#include <vector>

#include "../../voxel-slam_amd/csrc/vxba_intake_math.hpp"

extern "C" {

int ikh_yaw_class(long long n, const double* d, int32_t* cls) {
  for (long long i = 0; i < n; i++) cls[i] = vxik::yaw_class(d[i]);
  return 0;
}

int ikh_yaw_constants(int32_t* out) {
  out[0] = vxik::RULE_YAW; out[1] = vxik::YAW_IDENT; out[2] = vxik::YAW_SET; out[3] = vxik::YAW_RESET; out[4] = vxik::YAW_CAND; out[5] = (int32_t)vxik::YAW_COOL;
  return 0;
}

// every composition of two maps against applying them one after the other: out[16 x 2]
int ikh_yaw_compose(int32_t* out) {
  for (uint32_t then = 0; then < 4; then++)
    for (uint32_t first = 0; first < 4; first++)
      for (uint32_t q = 0; q < 2; q++)
        out[(then * 4 + first) * 2 + q] = vxik::yaw_map_apply(vxik::yaw_map_compose(then, first), q) == vxik::yaw_map_apply(then, vxik::yaw_map_apply(first, q));
  return 0;
}

// kept n (0 / 1), time n, yaw n (active points; NaN elsewhere is the caller's), counts 4 = [skipped | active | candidates | events], passes 1: the
// resolver's scan passes
int ikh_yaw_walk(long long n, const float* x, const float* y, const float* z, long long pfn, double blind, double omega_l, int32_t* kept, float* time, double* yaw, int64_t* counts,
                 int64_t* passes) {
  using namespace vxik;
  std::vector<double> r(n > 0 ? n : 1, 0.0);
  std::vector<long long> last(n > 0 ? n : 1, -1);
  std::vector<int> cls(n > 0 ? n : 1, YAW_IDENT);
  std::vector<uint32_t> pos(n > 0 ? n : 1, 0u), sp_idx, sp_cls, sp_state;
  long long first = -1;
  counts[0] = counts[1] = counts[2] = counts[3] = 0;
  for (long long i = 0; i < n; i++) {                       // yaw_decode_kernel and the max-scan
    const int kind = yaw_point(x[i], y[i], z[i], blind, &r[i]);
    if (kind == YAW_SKIPPED) counts[0]++;
    if (kind == YAW_ACTIVE) counts[1]++;
    if (kind >= YAW_BLIND && first < 0) first = i;
    last[i] = kind == YAW_ACTIVE ? i : (i ? last[i - 1] : -1);
  }
  for (long long i = 0; i < n; i++) {                       // yaw_link_kernel, the sum-scan and yaw_compact_kernel
    if (last[i] == i) {
      const long long p = i > 0 ? last[i - 1] : -1;
      cls[i] = yaw_class(r[i] - r[p >= 0 ? p : first]);
    }
    if (cls[i] == YAW_CAND) counts[2]++;
    if (cls[i] != YAW_IDENT) { sp_idx.push_back((uint32_t)i); sp_cls.push_back((uint32_t)cls[i]); }
    pos[i] = (uint32_t)sp_idx.size();
  }
  const long long S = (long long)sp_idx.size();
  sp_state.assign(S > 0 ? S : 1, 0u);
  uint32_t q = 0u, k = 0u;                                  // yaw_resolve_kernel, lane by lane
  long long e = -1;
  *passes = 0;
  for (long long c0 = 0; c0 < S; c0 += 64) {
    int start = 0;
    while (start < 64 && c0 + start < S) {
      (*passes)++;
      uint32_t acc[64], q_after[64];
      bool in[64], allowed[64];
      for (int lane = 0; lane < 64; lane++) {
        const long long s = c0 + lane;
        in[lane] = s < S && lane >= start;
        allowed[lane] = s < S && yaw_cool_allows(e, (long long)sp_idx[s]);
        acc[lane] = in[lane] ? yaw_map((int)sp_cls[s], allowed[lane]) : YAW_MAP_IDENT;
      }
      for (int d = 1; d < 64; d <<= 1) {
        uint32_t below[64];
        for (int lane = 0; lane < 64; lane++) below[lane] = lane >= d ? acc[lane - d] : acc[lane];
        for (int lane = 0; lane < 64; lane++) if (lane >= d) acc[lane] = yaw_map_compose(acc[lane], below[lane]);
      }
      int at = 64;
      for (int lane = 0; lane < 64; lane++) {
        q_after[lane] = yaw_map_apply(acc[lane], q);
        const uint32_t q_before = lane == 0 ? q : q_after[lane - 1];
        if (at == 64 && in[lane] && sp_cls[c0 + lane] == (uint32_t)YAW_CAND && allowed[lane] && q_before == 0u) at = lane;
      }
      for (int lane = 0; lane < 64; lane++)
        if (in[lane] && lane <= at) sp_state[c0 + lane] = yaw_state_pack(k + (lane == at ? 1u : 0u), lane == at, q_after[lane]);
      if (at < 64) { k += 1u; q = 0u; e = (long long)sp_idx[c0 + at]; start = at + 1; }
      else { q = q_after[63]; start = 64; }
    }
  }
  counts[3] = (int64_t)k;
  for (long long i = 0; i < n; i++) {                       // yaw_time_kernel
    kept[i] = 0; time[i] = 0.0f;
    if (last[i] != i) continue;
    const uint32_t st = pos[i] ? sp_state[pos[i] - 1u] : 0u;
    yaw[i] = yaw_value(r[i], st >> 2, cls[i] != YAW_IDENT && (st & 2u), st & 1u);
    float t = yaw_curvature(r[first], yaw[i], omega_l);
    if (i % pfn == 0 && yaw_keep(t)) {
      if ((f32_bits(t) & 0x7FFFFFFFu) == 0u) t = bits_f32(0u);
      kept[i] = 1; time[i] = t;
    }
  }
  return 0;
}

}  // extern "C"
