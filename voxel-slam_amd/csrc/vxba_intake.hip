// Scan intake on the GPU -- self-contained translation unit: the `vxba_intake_*` entry points of include/vxba.h.
//
// What it replaces (VoxelSLAM/src): the handlers of `Features::process` (feature_point.hpp:142-366)
// and `pcl_handler` behind them (voxelslam.hpp:76-103): the bytes of the driver's message in, the decimated, range-filtered, time-sorted and trimmed
// cloud out, resident for vxba_imuekf_process_device.
//
// The message's point bytes go up in ONE copy from a pinned staging block.  Two launches of this unit with rocPRIM's stable radix sort between them:
//
//   intake_decode_kernel   one lane per input point, 256-lane workgroups.  The workgroup's byte range goes to LDS as ALIGNED dwords (the range starts
//                          wherever 256 i point_step falls; the load starts at the dword below), and every field is assembled from two LDS dwords --
//                          no load is ever issued on an unaligned address.  Time rule, decimation on the original index, blind test, the finiteness
//                          deviations and the 0.11 trim are one verdict per point (vxba_intake_math.hpp).  Point i can only survive when
//                          i % point_filter_num == 0, so it owns slot i / point_filter_num of ceil(n / point_filter_num) candidate slots: a number
//                          the host knows.  A slot holds (x, y, z, t), the sort key -- the order-preserving bits of t, or KEY_DROPPED -- and its own
//                          index.  Survivors are counted by one integer atomic per workgroup.
//   rocPRIM                stable sort of the (key 32 bit, slot) pairs: survivors first, by time, ties in slot order = input order.  Nothing in it
//                          depends on scheduling.
//   intake_gather_kernel   one lane per sorted slot: the survivor's point to its place in xyz / toff; lane 0 writes the record, and the two-point
//                          cloud of the fallback (voxelslam.hpp:82-90) when nothing passed decimation and blind.
//
// vxba_intake_push_yaw (the Velodyne branch without a usable time field, :200-252) puts five launches and two rocPRIM scans in the decode kernel's
// place -- yaw_decode, max-scan, yaw_link, sum-scan, yaw_compact, yaw_resolve (one wave), yaw_time; see there -- and shares the sort and the gather.
//
// One host wait per push, for the record.  Launches and waits do not depend on n (one more wait when a buffer has to grow).
#include "vxba_wait.hpp"
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <cstdint>
#include <cstring>
#include <mutex>
#include <string>

#include "../../include/vxba.h"
#include "vxba_dev.hpp"
#include "vxba_intake_math.hpp"
#include "vxba_internal.h"

namespace vxik {

constexpr int REC_LEN = 6;

__global__ __launch_bounds__(256) void intake_decode_kernel(const uint32_t* __restrict__ words, long long total_words, Layout L, long long n, long long pfn, double blind,
                                                            double time_head, float4* __restrict__ dec, uint32_t* __restrict__ key, uint32_t* __restrict__ val,
                                                            unsigned int* __restrict__ counters) {
  extern __shared__ uint32_t lds[];
  const long long i0 = (long long)blockIdx.x * 256;
  const long long np = n - i0 < 256 ? (n - i0 > 0 ? n - i0 : 0) : 256;
  const long long b0 = i0 * (long long)L.point_step, a0 = b0 & ~3LL;
  const uint32_t shift = (uint32_t)(b0 - a0);
  const uint32_t nwords = np > 0 ? (shift + (uint32_t)np * (uint32_t)L.point_step + 3u) / 4u + 1u : 0u;   // one spare dword for the last field's upper half
  for (uint32_t k = threadIdx.x; k < nwords; k += 256) {
    const long long g = a0 / 4 + k;
    lds[k] = g < total_words ? words[g] : 0u;
  }
  __syncthreads();
  const long long i = i0 + threadIdx.x;
  int verdict = DROP_DECIMATED;
  if (i < n) {
    float p[4];
    verdict = decode_point(lds, shift + threadIdx.x * (uint32_t)L.point_step, L, i, pfn, blind, time_head, p);
    if (verdict != DROP_DECIMATED) {
      const long long slot = i / pfn;
      dec[slot] = make_float4(p[0], p[1], p[2], p[3]);
      key[slot] = verdict == KEEP ? time_key(p[3]) : KEY_DROPPED;
      val[slot] = (uint32_t)slot;
    }
  } else if (n == 0 && i == 0) {                   // the sort runs on one slot at least
    key[0] = KEY_DROPPED; val[0] = 0u;
  }
  const int kept = __syncthreads_count(verdict == KEEP);
  const int passed = __syncthreads_count(verdict >= DROP_TRIM);
  if (threadIdx.x == 0) {
    if (kept) atomicAdd(&counters[0], (unsigned int)kept);
    if (passed) atomicAdd(&counters[1], (unsigned int)passed);
  }
}

__global__ __launch_bounds__(256) void intake_gather_kernel(const uint32_t* __restrict__ key_s, const uint32_t* __restrict__ val_s, const float4* __restrict__ dec, long long ms,
                                                            const unsigned int* __restrict__ counters, long long n_points, float* __restrict__ xyz, float* __restrict__ toff,
                                                            double* __restrict__ rec) {
  const long long j = (long long)blockIdx.x * 256 + threadIdx.x;
  if (j < ms && key_s[j] != KEY_DROPPED) {
    const float4 p = dec[val_s[j]];
    xyz[3 * j] = p.x; xyz[3 * j + 1] = p.y; xyz[3 * j + 2] = p.z;
    toff[j] = p.w;
  }
  if (j != 0) return;
  const unsigned int n_out = counters[0], n_pass = counters[1];
  if (n_pass == 0) {                               // voxelslam.hpp:82-90: two points at the origin, times 0 and 0.09
    const float late = 0.09f;
    for (int k = 0; k < 6; k++) xyz[k] = 0.0f;
    toff[0] = 0.0f; toff[1] = late;
    rec[0] = 2.0; rec[1] = 0.0; rec[2] = (double)late; rec[3] = 1.0; rec[4] = (double)n_points; rec[5] = 0.0;
    return;
  }
  rec[0] = (double)n_out;
  rec[1] = n_out ? (double)dec[val_s[0]].w : 0.0;
  rec[2] = n_out ? (double)dec[val_s[n_out - 1]].w : 0.0;
  rec[3] = 0.0; rec[4] = (double)n_points; rec[5] = (double)n_pass;
}

// ---- yaw-derived times (vxba_intake_push_yaw; the arithmetic and the restated walk: vxba_intake_math.hpp) ------------------------------------------
// counters of a yaw push, behind the two the gather reads
constexpr int YC_SKIPPED = 2, YC_ACTIVE = 3, YC_CANDIDATES = 4, YC_EVENTS = 5, YC_FIRST = 6, YC_LEN = 8;

// One lane per input point -- every i, the state runs over all of them.  Fields from LDS as intake_decode_kernel.  own[i] = i for an active point, -1
// for any other (an inclusive max-scan turns it into "the last active point at or before i"), r[i] the angle of a non-skipped one; the first
// non-skipped index by an atomic minimum that a workgroup only issues while it can still lower it.
__global__ __launch_bounds__(256) void yaw_decode_kernel(const uint32_t* __restrict__ words, long long total_words, Layout L, long long n, double blind, double* __restrict__ r,
                                                         int* __restrict__ own, unsigned int* __restrict__ counters) {
  extern __shared__ uint32_t lds[];
  const long long i0 = (long long)blockIdx.x * 256;
  const long long np = n - i0 < 256 ? (n - i0 > 0 ? n - i0 : 0) : 256;
  const long long b0 = i0 * (long long)L.point_step, a0 = b0 & ~3LL;
  const uint32_t shift = (uint32_t)(b0 - a0);
  const uint32_t nwords = np > 0 ? (shift + (uint32_t)np * (uint32_t)L.point_step + 3u) / 4u + 1u : 0u;
  for (uint32_t k = threadIdx.x; k < nwords; k += 256) {
    const long long g = a0 / 4 + k;
    lds[k] = g < total_words ? words[g] : 0u;
  }
  __syncthreads();
  const long long i = i0 + threadIdx.x;
  int kind = -1;
  if (i < n) {
    const uint32_t base = shift + threadIdx.x * (uint32_t)L.point_step;
    const float x = bits_f32(load_u32(lds, base + (uint32_t)L.off_x)), y = bits_f32(load_u32(lds, base + (uint32_t)L.off_y)), z = bits_f32(load_u32(lds, base + (uint32_t)L.off_z));
    double ri = 0.0;
    kind = yaw_point(x, y, z, blind, &ri);
    r[i] = ri;
    own[i] = kind == YAW_ACTIVE ? (int)i : -1;
  }
  const unsigned long long seen = __ballot(kind >= YAW_BLIND);                  // the wave's non-skipped points
  if (seen && (threadIdx.x & 63) == __ffsll((long long)seen) - 1 && (uint32_t)i < __atomic_load_n(&counters[YC_FIRST], __ATOMIC_RELAXED)) atomicMin(&counters[YC_FIRST], (uint32_t)i);
  const int skipped = __syncthreads_count(kind == YAW_SKIPPED);
  const int active = __syncthreads_count(kind == YAW_ACTIVE);
  if (threadIdx.x == 0) {
    if (skipped) atomicAdd(&counters[YC_SKIPPED], (unsigned int)skipped);
    if (active) atomicAdd(&counters[YC_ACTIVE], (unsigned int)active);
  }
}

// One lane per point, behind the max-scan of own[] into last[]: an active point's predecessor is last[i - 1] (the first non-skipped point when there
// is none), d its angle's step from there, cls[i] the class of d, and flag[i] = 1 for a special (any class but the identity): the inclusive sum-scan of
// flag[] is both the compaction and, later, every point's governing special.
__global__ __launch_bounds__(256) void yaw_link_kernel(const double* __restrict__ r, const int* __restrict__ last, long long n, uint8_t* __restrict__ cls, uint32_t* __restrict__ flag,
                                                       unsigned int* __restrict__ counters) {
  const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
  int c = YAW_IDENT;
  if (i < n) {
    if (last[i] == (int)i) {
      const int p = i > 0 ? last[i - 1] : -1;
      const double rp = r[p >= 0 ? (long long)p : (long long)counters[YC_FIRST]];   // an active point exists, so a first non-skipped one does
      c = yaw_class(r[i] - rp);
    }
    cls[i] = (uint8_t)c;
    flag[i] = c != YAW_IDENT ? 1u : 0u;
  }
  const int cand = __syncthreads_count(c == YAW_CAND);
  if (threadIdx.x == 0 && cand) atomicAdd(&counters[YC_CANDIDATES], (unsigned int)cand);
}

// The specials, compacted in index order: special number pos[i] - 1 is point i.
__global__ __launch_bounds__(256) void yaw_compact_kernel(const uint8_t* __restrict__ cls, const uint32_t* __restrict__ pos, long long n, uint32_t* __restrict__ sp_idx,
                                                          uint8_t* __restrict__ sp_cls) {
  const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
  if (i >= n || cls[i] == YAW_IDENT) return;
  sp_idx[pos[i] - 1u] = (uint32_t)i;
  sp_cls[pos[i] - 1u] = cls[i];
}

// ONE wave walks the S specials in chunks of 64.  With the last event's index e known, every special of the chunk is a map on q (a candidate that
// cool allows resets, one it blocks toggles), a 64-wide scan of map compositions gives every lane its q before and after, and the first allowed
// candidate that meets q = 0 is the next event: the lanes up to it are final, (k, e, q) move on, and the rest of the chunk is scanned again under the
// new e.  Passes: at most ceil(S / 64) + events, six shuffle steps each; events lie 1000 indices apart, so at most n / 1000 + 1 of them.
__global__ __launch_bounds__(64) void yaw_resolve_kernel(const uint32_t* __restrict__ sp_idx, const uint8_t* __restrict__ sp_cls, const uint32_t* __restrict__ pos, long long n,
                                                         uint32_t* __restrict__ sp_state, unsigned int* __restrict__ counters) {
  const int lane = threadIdx.x;
  const long long S = n > 0 ? (long long)pos[n - 1] : 0;
  uint32_t q = 0u, k = 0u;
  long long e = -1;
  for (long long c0 = 0; c0 < S; c0 += 64) {
    const long long s = c0 + lane;
    const bool live = s < S;
    const long long idx = live ? (long long)sp_idx[s] : 0;
    const int cls = live ? (int)sp_cls[s] : YAW_IDENT;
    int start = 0;
    while (start < 64 && c0 + start < S) {                                      // wave-uniform
      const bool in = live && lane >= start;
      const bool allowed = yaw_cool_allows(e, idx);
      uint32_t acc = in ? yaw_map(cls, allowed) : YAW_MAP_IDENT;
      for (int d = 1; d < 64; d <<= 1) {
        const uint32_t below = (uint32_t)__shfl_up((int)acc, d);
        if (lane >= d) acc = yaw_map_compose(acc, below);
      }
      const uint32_t q_after = yaw_map_apply(acc, q);
      uint32_t q_before = (uint32_t)__shfl_up((int)q_after, 1);
      if (lane == 0) q_before = q;
      const unsigned long long events = __ballot(in && cls == YAW_CAND && allowed && q_before == 0u);
      const int at = events ? __ffsll((long long)events) - 1 : 64;
      if (in && lane <= at) sp_state[s] = yaw_state_pack(k + (lane == at ? 1u : 0u), lane == at, q_after);
      if (at < 64) {
        k += 1u; q = 0u;
        e = __shfl((int)idx, at);
        start = at + 1;
      } else {
        q = (uint32_t)__shfl((int)q_after, 63);
        start = 64;
      }
    }
  }
  if (lane == 0) counters[YC_EVENTS] = k;
}

// One lane per point that decimation leaves a slot (i % pfn == 0, active or not -- the sort reads every slot): an active point takes (k, q, event)
// from its governing special, number pos[i] - 1 (none: the walk's start), rebuilds yaw_angle and its time, and is kept or dropped (:246).
__global__ __launch_bounds__(256) void yaw_time_kernel(const uint32_t* __restrict__ words, Layout L, long long n, long long pfn, double omega_l, const double* __restrict__ r,
                                                       const int* __restrict__ last, const uint8_t* __restrict__ cls, const uint32_t* __restrict__ pos,
                                                       const uint32_t* __restrict__ sp_state, float4* __restrict__ dec, uint32_t* __restrict__ key, uint32_t* __restrict__ val,
                                                       unsigned int* __restrict__ counters) {
  const long long slot = (long long)blockIdx.x * 256 + threadIdx.x, i = slot * pfn;
  bool kept = false;
  if (i < n) {
    uint32_t kk = KEY_DROPPED;
    if (last[i] == (int)i) {
      const uint32_t rank = pos[i], st = rank ? sp_state[rank - 1u] : 0u;
      const double yaw = yaw_value(r[i], st >> 2, cls[i] != YAW_IDENT && (st & 2u), st & 1u);
      float t = yaw_curvature(r[counters[YC_FIRST]], yaw, omega_l);
      if (yaw_keep(t)) {
        if ((f32_bits(t) & 0x7FFFFFFFu) == 0u) t = bits_f32(0u);                // -0.0 -> +0.0
        // the point's bytes once more, from global memory: any offset, so byte by byte through the aligned dword below and above
        const unsigned long long b = (unsigned long long)i * (unsigned long long)L.point_step;
        const uint32_t* w = words + (b >> 2);
        const uint32_t sh = (uint32_t)(b & 3u);
        dec[slot] = make_float4(bits_f32(load_u32(w, sh + (uint32_t)L.off_x)), bits_f32(load_u32(w, sh + (uint32_t)L.off_y)), bits_f32(load_u32(w, sh + (uint32_t)L.off_z)), t);
        kk = time_key(t);
        kept = true;
      }
    }
    key[slot] = kk; val[slot] = (uint32_t)slot;
  } else if (n == 0 && slot == 0) {                // the sort runs on one slot at least
    key[0] = KEY_DROPPED; val[0] = 0u;
  }
  const int count = __syncthreads_count(kept);
  if (threadIdx.x == 0 && count) { atomicAdd(&counters[0], (unsigned int)count); atomicAdd(&counters[1], (unsigned int)count); }
}

}  // namespace vxik

struct vxba_intake {
  int device = 0;
  vxu::Stream s;
  vxu::Event ev_done;
  vxu::Event ev_prof[4];   // vxba_intake_set_profiling: before the upload, behind the decode, the sort, the gather
  bool profiling = false, prof_valid = false;
  vxu::Pin<char> h_stage;        // pinned: the message's point bytes
  vxu::Dev<char> d_bytes;        // the same on the device, with 8 spare bytes; the two grow together
  vxu::Pin<double> h_rec;        // pinned: the record
  vxu::Arena work;
  float *d_xyz = nullptr, *d_toff = nullptr;
  int64_t n = 0, n_decoded = 0;
  float toff_first = 0.f, toff_last = 0.f;
  int64_t launches = 0, waits = 0;
  vxu::Pin<unsigned int> h_yaw;  // pinned: the counters of a yaw push
  bool last_yaw = false;         // the last push that ran was vxba_intake_push_yaw
  int64_t yaw_info[4] = {0, 0, 0, 0};
  std::string err;
  std::recursive_mutex mtx;
};

namespace {

#define IK_LOCK(h) std::lock_guard<std::recursive_mutex> lk__((h)->mtx)

// a field of `len` bytes at `off` lies inside the point; two fields do not share a byte
bool inside(int32_t off, int32_t len, int32_t step) { return off >= 0 && (int64_t)off + len <= step; }
bool apart(int32_t a, int32_t la, int32_t b, int32_t lb) { return a + la <= b || b + lb <= a; }

const char* layout_fault(const vxba_scan_layout& L) {
  using namespace vxik;
  if (L.point_step < 12 || L.point_step > MAX_STEP) return "point_step outside 12..VXBA_SCAN_MAX_STEP";
  if (L.filter != 0 && L.filter != 1) return "filter is neither 0 nor 1";
  const bool pair = (L.time_rule == RULE_NONE && L.time_type == TIME_NONE) || (L.time_rule == RULE_AS_IS && L.time_type == TIME_F32) ||
                    (L.time_rule == RULE_NANOSECONDS && L.time_type == TIME_U32) || (L.time_rule == RULE_MINUS_HEAD && L.time_type == TIME_F64) ||
                    (L.time_rule == RULE_YAW && (L.time_type == TIME_NONE || L.time_type == TIME_F32));
  if (!pair) return "time_type and time_rule do not belong together";
  if (L.time_rule == RULE_YAW && L.filter != 1) return "filter is not 1 under the yaw rule";
  const int32_t tl = L.time_type == TIME_NONE ? 0 : (L.time_type == TIME_F64 ? 8 : 4);
  if (!inside(L.off_x, 4, L.point_step) || !inside(L.off_y, 4, L.point_step) || !inside(L.off_z, 4, L.point_step) || (tl && !inside(L.off_time, tl, L.point_step)))
    return "a field ends behind point_step";
  if (!apart(L.off_x, 4, L.off_y, 4) || !apart(L.off_x, 4, L.off_z, 4) || !apart(L.off_y, 4, L.off_z, 4) ||
      (tl && (!apart(L.off_time, tl, L.off_x, 4) || !apart(L.off_time, tl, L.off_y, 4) || !apart(L.off_time, tl, L.off_z, 4))))
    return "two fields overlap";
  return nullptr;
}

}  // namespace

// vxba_imuekf_process_device's view of the last push: the resident cloud, toff_first and the event recorded behind the gather
extern "C" int vxba_internal_intake_view(vxba_intake* h, const float** d_xyz, const float** d_toff, long long* n, float* toff_first, void** ev_done, int* device) {
  if (!h) return VXBA_ERR_ARG;
  IK_LOCK(h);
  *d_xyz = h->n > 0 ? h->d_xyz : nullptr; *d_toff = h->n > 0 ? h->d_toff : nullptr; *n = h->n; *toff_first = h->toff_first; *ev_done = (void*)h->ev_done; *device = h->device;
  return VXBA_OK;
}

extern "C" {

int vxba_intake_create(int device, vxba_intake** out) {
  if (!out) return VXBA_ERR_ARG;
  *out = nullptr;
  if (const int rc = vxu::select_device(device)) return rc;
  vxba_intake* h = new vxba_intake();
  h->device = device;
  if (h->s.create() != hipSuccess || h->ev_done.create(hipEventDisableTiming) != hipSuccess || h->h_rec.reserve(8) != hipSuccess || h->h_yaw.reserve(vxik::YC_LEN) != hipSuccess) { delete h; return VXBA_ERR_HIP; }
  *out = h;
  return VXBA_OK;
}

int vxba_intake_destroy(vxba_intake* h) {
  if (!h) return VXBA_ERR_ARG;
  hipSetDevice(h->device);
  if (h->s) hipStreamSynchronize(h->s);
  h->work.release();
  delete h;
  return VXBA_OK;
}

const char* vxba_intake_last_error(const vxba_intake* h) { return h ? h->err.c_str() : "null handle"; }

// vxba_intake_push (omega_l null) and vxba_intake_push_yaw behind their argument checks
static int intake_push(vxba_intake* h, const char* who, const vxba_scan_layout* layout, int64_t n_points, const void* bytes, int point_filter_num, double blind, double time_head,
                       const double* omega_l, double* rec_out) {
  using namespace vxik;
  const std::string me = std::string(who) + ": ";
  const bool yaw = omega_l != nullptr;
  if (!layout || !rec_out || n_points < 0 || n_points >= ((int64_t)1 << 31) || (n_points > 0 && !bytes)) return vxu::fail(h, VXBA_ERR_ARG, me + "bad argument");
  if (point_filter_num < 1) return vxu::fail(h, VXBA_ERR_ARG, me + "point_filter_num < 1");
  if (const char* why = layout_fault(*layout)) return vxu::fail(h, VXBA_ERR_ARG, me + why);
  if (std::isnan(blind) || !std::isfinite(time_head)) return vxu::fail(h, VXBA_ERR_ARG, me + "blind is NaN or time_head is not finite");
  Layout L;
  static_assert(sizeof(Layout) == sizeof(vxba_scan_layout), "vxik::Layout mirrors vxba_scan_layout");
  std::memcpy(&L, layout, sizeof L);
  if (yaw && L.time_rule != RULE_YAW) return vxu::fail(h, VXBA_ERR_ARG, me + "the layout's time rule is not VXBA_SCAN_RULE_YAW");
  if (!yaw && L.time_rule == RULE_YAW) return vxu::fail(h, VXBA_ERR_ARG, me + "a VXBA_SCAN_RULE_YAW layout needs omega_l (vxba_intake_push_yaw)");
  if (yaw && !(std::isfinite(*omega_l) && *omega_l > 0.0)) return vxu::fail(h, VXBA_ERR_ARG, me + "omega_l is not finite or not positive");
  if (L.time_rule == RULE_MINUS_HEAD && n_points == 0) return vxu::fail(h, VXBA_ERR_ARG, me + "an empty message under the minus-head rule (upstream reads points[0])");
  if (L.time_rule == RULE_AS_IS && n_points > 0) {     // feature_point.hpp:176: the branch with a usable time field, decided from the last point
    float t;
    std::memcpy(&t, (const char*)bytes + (size_t)(n_points - 1) * L.point_step + L.off_time, 4);
    if (!((double)t > 0.01 && (double)t < 0.12))
      return vxu::fail(h, VXBA_ERR_UNSUPPORTED, me + "the last point's time is not in (0.01, 0.12): the yaw-derived Velodyne times are out of scope");
  }
  const long long pfn = L.filter ? point_filter_num : 1;
  const long long m = (n_points + pfn - 1) / pfn, ms = std::max<long long>(m, 1), mo = std::max<long long>(m, 2);
  const size_t total = (size_t)n_points * (size_t)L.point_step;
  const size_t ny = yaw ? (size_t)std::max<long long>(n_points, 1) : 0;     // the per-point arrays of the walk

  VX_HIP(h, hipSetDevice(h->device));
  h->launches = 0; h->waits = 0;
  bool grew = false;
  const size_t held = std::min(h->h_stage.capacity(), h->d_bytes.capacity());
  if (total + 8 > held) {
    VX_HIP(h, hipStreamSynchronize(h->s));
    grew = true;
    const size_t cap = (std::max(total + 8, 2 * held) + 255) / 256 * 256;
    VX_HIP(h, h->h_stage.reserve(total + 8, cap));
    VX_HIP(h, h->d_bytes.reserve(total + 8, cap));
  }
  vxu::Temp temp;
  VX_HIP(h, (vxu::sort_temp<uint32_t, uint32_t>(temp.bytes, (size_t)ms, 32, h->s)));
  if (yaw && n_points > 0) {
    size_t t = 0;
    VX_HIP(h, rocprim::inclusive_scan(nullptr, t, (int*)nullptr, (int*)nullptr, (size_t)n_points, rocprim::maximum<int>(), h->s));
    temp.bytes = std::max(temp.bytes, t);
    VX_HIP(h, rocprim::inclusive_scan(nullptr, t, (uint32_t*)nullptr, (uint32_t*)nullptr, (size_t)n_points, rocprim::plus<uint32_t>(), h->s));
    temp.bytes = std::max(temp.bytes, t);
  }
  float4* dec = nullptr; uint32_t *key = nullptr, *key_s = nullptr, *val = nullptr, *val_s = nullptr; unsigned int* counters = nullptr; double* rec = nullptr;
  float *o_xyz = nullptr, *o_toff = nullptr;
  double* y_r = nullptr; int* y_last = nullptr; uint8_t *y_cls = nullptr, *y_spcls = nullptr; uint32_t *y_pos = nullptr, *y_spidx = nullptr, *y_state = nullptr;
  bool synced = false;
  h->n = 0; h->d_xyz = nullptr; h->d_toff = nullptr;        // from here on the previous result is gone
  h->last_yaw = false;
  VX_HIP(h, h->work.layout([&](vxu::Arena& a) {
    o_xyz = a.take<float>(3 * (size_t)mo); o_toff = a.take<float>((size_t)mo); dec = a.take<float4>((size_t)ms);
    key = a.take<uint32_t>((size_t)ms); key_s = a.take<uint32_t>((size_t)ms); val = a.take<uint32_t>((size_t)ms); val_s = a.take<uint32_t>((size_t)ms);
    counters = a.take<unsigned int>(YC_LEN); rec = a.take<double>(REC_LEN); temp.p = a.take<char>(temp.bytes);
    if (yaw) {
      y_r = a.take<double>(ny); y_last = a.take<int>(ny); y_cls = a.take<uint8_t>(ny); y_pos = a.take<uint32_t>(ny);
      y_spidx = a.take<uint32_t>(ny); y_spcls = a.take<uint8_t>(ny); y_state = a.take<uint32_t>(ny);
    }
  }, h->s, &synced));
  if (grew || synced) h->waits += 1;

  if (total) std::memcpy(h->h_stage, bytes, total);
  h->prof_valid = false;
  if (h->profiling) VX_HIP(h, hipEventRecord(h->ev_prof[0], h->s));
  if (total) VX_HIP(h, hipMemcpyAsync(h->d_bytes, h->h_stage, total, hipMemcpyHostToDevice, h->s));
  VX_HIP(h, hipMemsetAsync(counters, 0, YC_LEN * sizeof(unsigned int), h->s));
  const size_t lds = ((size_t)256 * L.point_step + 3) / 4 * 4 + 8;
  const uint32_t* words = (const uint32_t*)h->d_bytes.get();
  if (!yaw) {
    intake_decode_kernel<<<vxu::blocks_for(n_points), 256, lds, h->s>>>(words, (long long)((total + 3) / 4), L, (long long)n_points, pfn, blind, time_head, dec, key, val, counters);
    VX_HIP(h, hipGetLastError());
    h->launches += 1;
  } else {
    const long long n = (long long)n_points;
    VX_HIP(h, hipMemsetAsync(counters + YC_FIRST, 0xFF, sizeof(unsigned int), h->s));      // the first non-skipped index: none yet
    yaw_decode_kernel<<<vxu::blocks_for(n), 256, lds, h->s>>>(words, (long long)((total + 3) / 4), L, n, blind, y_r, y_last, counters);
    VX_HIP(h, hipGetLastError());
    if (n > 0) VX_HIP(h, rocprim::inclusive_scan(temp.p, temp.bytes, y_last, y_last, (size_t)n, rocprim::maximum<int>(), h->s));
    yaw_link_kernel<<<vxu::blocks_for(n), 256, 0, h->s>>>(y_r, y_last, n, y_cls, y_pos, counters);
    VX_HIP(h, hipGetLastError());
    if (n > 0) VX_HIP(h, rocprim::inclusive_scan(temp.p, temp.bytes, y_pos, y_pos, (size_t)n, rocprim::plus<uint32_t>(), h->s));
    yaw_compact_kernel<<<vxu::blocks_for(n), 256, 0, h->s>>>(y_cls, y_pos, n, y_spidx, y_spcls);
    VX_HIP(h, hipGetLastError());
    yaw_resolve_kernel<<<1, 64, 0, h->s>>>(y_spidx, y_spcls, y_pos, n, y_state, counters);
    VX_HIP(h, hipGetLastError());
    yaw_time_kernel<<<vxu::blocks_for(m), 256, 0, h->s>>>(words, L, n, pfn, *omega_l, y_r, y_last, y_cls, y_pos, y_state, dec, key, val, counters);
    VX_HIP(h, hipGetLastError());
    h->launches += 5;
  }
  if (h->profiling) VX_HIP(h, hipEventRecord(h->ev_prof[1], h->s));
  VX_HIP(h, vxu::sort(temp, key, key_s, val, val_s, (size_t)ms, 32, h->s));
  if (h->profiling) VX_HIP(h, hipEventRecord(h->ev_prof[2], h->s));
  intake_gather_kernel<<<vxu::blocks_for(ms), 256, 0, h->s>>>(key_s, val_s, dec, ms, counters, (long long)n_points, o_xyz, o_toff, rec);
  VX_HIP(h, hipGetLastError());
  h->launches += 1;
  VX_HIP(h, hipMemcpyAsync(h->h_rec, rec, REC_LEN * sizeof(double), hipMemcpyDeviceToHost, h->s));
  if (yaw) VX_HIP(h, hipMemcpyAsync(h->h_yaw, counters, YC_LEN * sizeof(unsigned int), hipMemcpyDeviceToHost, h->s));
  VX_HIP(h, hipEventRecord(h->ev_done, h->s));
  if (h->profiling) { VX_HIP(h, hipEventRecord(h->ev_prof[3], h->s)); h->prof_valid = true; }
  VX_HIP(h, vxwait::stream_wait(h->s));
  h->waits += 1;

  std::memcpy(rec_out, h->h_rec, REC_LEN * sizeof(double));
  h->n_decoded = n_points;
  if (yaw) {
    const unsigned int* c = h->h_yaw;
    h->yaw_info[0] = c[YC_SKIPPED]; h->yaw_info[1] = c[YC_ACTIVE]; h->yaw_info[2] = c[YC_CANDIDATES]; h->yaw_info[3] = c[YC_EVENTS];
    h->last_yaw = true;
  }
  if (rec_out[0] == 0.0) return vxu::fail(h, VXBA_ERR_ARG, me + "every surviving point lies behind 0.11 s (upstream pops an empty vector)");
  h->n = (int64_t)rec_out[0]; h->d_xyz = o_xyz; h->d_toff = o_toff;
  h->toff_first = (float)rec_out[1]; h->toff_last = (float)rec_out[2];
  return VXBA_OK;
}

int vxba_intake_push(vxba_intake* h, const vxba_scan_layout* layout, int64_t n_points, const void* bytes, int point_filter_num, double blind, double time_head, double* rec_out) {
  if (!h) return VXBA_ERR_ARG;
  IK_LOCK(h);
  return intake_push(h, "vxba_intake_push", layout, n_points, bytes, point_filter_num, blind, time_head, nullptr, rec_out);
}

int vxba_intake_push_yaw(vxba_intake* h, const vxba_scan_layout* layout, int64_t n_points, const void* bytes, int point_filter_num, double blind, double omega_l, double* rec_out) {
  if (!h) return VXBA_ERR_ARG;
  IK_LOCK(h);
  return intake_push(h, "vxba_intake_push_yaw", layout, n_points, bytes, point_filter_num, blind, 0.0, &omega_l, rec_out);
}

int vxba_intake_yaw_info(const vxba_intake* h, int64_t out[4]) {
  if (!h || !out) return VXBA_ERR_ARG;
  if (!h->last_yaw) return VXBA_ERR_STATE;
  for (int k = 0; k < 4; k++) out[k] = h->yaw_info[k];
  return VXBA_OK;
}

int vxba_intake_read(vxba_intake* h, float* xyz, float* toff) {
  if (!h || !xyz || !toff) return VXBA_ERR_ARG;
  IK_LOCK(h);
  if (h->n == 0) return vxu::fail(h, VXBA_ERR_STATE, "vxba_intake_read: no cloud");
  VX_HIP(h, hipSetDevice(h->device));
  VX_HIP(h, hipMemcpyAsync(xyz, h->d_xyz, (size_t)h->n * 12, hipMemcpyDeviceToHost, h->s));
  VX_HIP(h, hipMemcpyAsync(toff, h->d_toff, (size_t)h->n * 4, hipMemcpyDeviceToHost, h->s));
  VX_HIP(h, hipStreamSynchronize(h->s));
  return VXBA_OK;
}

int vxba_intake_device(vxba_intake* h, const float** d_xyz, const float** d_toff, int64_t* n) {
  if (!h || !d_xyz || !d_toff || !n) return VXBA_ERR_ARG;
  IK_LOCK(h);
  *d_xyz = h->n > 0 ? h->d_xyz : nullptr; *d_toff = h->n > 0 ? h->d_toff : nullptr; *n = h->n;
  return VXBA_OK;
}

int vxba_intake_stats(const vxba_intake* h, int64_t out[4]) {
  if (!h || !out) return VXBA_ERR_ARG;
  out[0] = h->launches; out[1] = h->waits; out[2] = h->n; out[3] = h->n_decoded;
  return VXBA_OK;
}

int vxba_intake_set_profiling(vxba_intake* h, int enable) {
  if (!h) return VXBA_ERR_ARG;
  IK_LOCK(h);
  VX_HIP(h, hipSetDevice(h->device));
  for (vxu::Event& e : h->ev_prof) if (enable) VX_HIP(h, e.create());
  h->profiling = enable != 0;
  h->prof_valid = false;
  return VXBA_OK;
}

int vxba_intake_stage_times(vxba_intake* h, double out_ms[3]) {
  if (!h || !out_ms) return VXBA_ERR_ARG;
  IK_LOCK(h);
  out_ms[0] = out_ms[1] = out_ms[2] = -1.0;
  if (!h->profiling) return vxu::fail(h, VXBA_ERR_STATE, "vxba_intake_stage_times: profiling is off");
  if (!h->prof_valid) return VXBA_OK;
  VX_HIP(h, hipSetDevice(h->device));
  VX_HIP(h, hipStreamSynchronize(h->s));
  float ms = 0.f;
  VX_HIP(h, hipEventElapsedTime(&ms, h->ev_prof[0], h->ev_prof[1])); out_ms[0] = (double)ms;
  VX_HIP(h, hipEventElapsedTime(&ms, h->ev_prof[1], h->ev_prof[2])); out_ms[1] = (double)ms;
  VX_HIP(h, hipEventElapsedTime(&ms, h->ev_prof[0], h->ev_prof[3])); out_ms[2] = (double)ms;
  return VXBA_OK;
}

}  // extern "C"
