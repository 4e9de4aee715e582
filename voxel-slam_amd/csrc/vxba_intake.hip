// Scan intake on the GPU -- self-contained translation unit: the `vxba_intake_*` entry points of include/vxba.h.
//
// What it replaces (VoxelSLAM/src): the handlers of `Features::process` (feature_point.hpp:142-366, all but the yaw-derived Velodyne branch :200-252)
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
                    (L.time_rule == RULE_NANOSECONDS && L.time_type == TIME_U32) || (L.time_rule == RULE_MINUS_HEAD && L.time_type == TIME_F64);
  if (!pair) return "time_type and time_rule do not belong together";
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
  if (h->s.create() != hipSuccess || h->ev_done.create(hipEventDisableTiming) != hipSuccess || h->h_rec.reserve(8) != hipSuccess) { delete h; return VXBA_ERR_HIP; }
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

int vxba_intake_push(vxba_intake* h, const vxba_scan_layout* layout, int64_t n_points, const void* bytes, int point_filter_num, double blind, double time_head, double* rec_out) {
  using namespace vxik;
  if (!h) return VXBA_ERR_ARG;
  IK_LOCK(h);
  if (!layout || !rec_out || n_points < 0 || n_points >= ((int64_t)1 << 31) || (n_points > 0 && !bytes)) return vxu::fail(h, VXBA_ERR_ARG, "vxba_intake_push: bad argument");
  if (point_filter_num < 1) return vxu::fail(h, VXBA_ERR_ARG, "vxba_intake_push: point_filter_num < 1");
  if (const char* why = layout_fault(*layout)) return vxu::fail(h, VXBA_ERR_ARG, std::string("vxba_intake_push: ") + why);
  if (std::isnan(blind) || !std::isfinite(time_head)) return vxu::fail(h, VXBA_ERR_ARG, "vxba_intake_push: blind is NaN or time_head is not finite");
  Layout L;
  static_assert(sizeof(Layout) == sizeof(vxba_scan_layout), "vxik::Layout mirrors vxba_scan_layout");
  std::memcpy(&L, layout, sizeof L);
  if (L.time_rule == RULE_MINUS_HEAD && n_points == 0) return vxu::fail(h, VXBA_ERR_ARG, "vxba_intake_push: an empty message under the minus-head rule (upstream reads points[0])");
  if (L.time_rule == RULE_AS_IS && n_points > 0) {     // feature_point.hpp:176: the branch with a usable time field, decided from the last point
    float t;
    std::memcpy(&t, (const char*)bytes + (size_t)(n_points - 1) * L.point_step + L.off_time, 4);
    if (!((double)t > 0.01 && (double)t < 0.12))
      return vxu::fail(h, VXBA_ERR_UNSUPPORTED, "vxba_intake_push: the last point's time is not in (0.01, 0.12): the yaw-derived Velodyne times are out of scope");
  }
  const long long pfn = L.filter ? point_filter_num : 1;
  const long long m = (n_points + pfn - 1) / pfn, ms = std::max<long long>(m, 1), mo = std::max<long long>(m, 2);
  const size_t total = (size_t)n_points * (size_t)L.point_step;

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
  float4* dec = nullptr; uint32_t *key = nullptr, *key_s = nullptr, *val = nullptr, *val_s = nullptr; unsigned int* counters = nullptr; double* rec = nullptr;
  float *o_xyz = nullptr, *o_toff = nullptr;
  bool synced = false;
  h->n = 0; h->d_xyz = nullptr; h->d_toff = nullptr;        // from here on the previous result is gone
  VX_HIP(h, h->work.layout([&](vxu::Arena& a) {
    o_xyz = a.take<float>(3 * (size_t)mo); o_toff = a.take<float>((size_t)mo); dec = a.take<float4>((size_t)ms);
    key = a.take<uint32_t>((size_t)ms); key_s = a.take<uint32_t>((size_t)ms); val = a.take<uint32_t>((size_t)ms); val_s = a.take<uint32_t>((size_t)ms);
    counters = a.take<unsigned int>(4); rec = a.take<double>(REC_LEN); temp.p = a.take<char>(temp.bytes);
  }, h->s, &synced));
  if (grew || synced) h->waits += 1;

  if (total) std::memcpy(h->h_stage, bytes, total);
  h->prof_valid = false;
  if (h->profiling) VX_HIP(h, hipEventRecord(h->ev_prof[0], h->s));
  if (total) VX_HIP(h, hipMemcpyAsync(h->d_bytes, h->h_stage, total, hipMemcpyHostToDevice, h->s));
  VX_HIP(h, hipMemsetAsync(counters, 0, 4 * sizeof(unsigned int), h->s));
  const size_t lds = ((size_t)256 * L.point_step + 3) / 4 * 4 + 8;
  intake_decode_kernel<<<vxu::blocks_for(n_points), 256, lds, h->s>>>((const uint32_t*)h->d_bytes.get(), (long long)((total + 3) / 4), L, (long long)n_points, pfn, blind, time_head, dec, key,
                                                                      val, counters);
  VX_HIP(h, hipGetLastError());
  if (h->profiling) VX_HIP(h, hipEventRecord(h->ev_prof[1], h->s));
  VX_HIP(h, vxu::sort(temp, key, key_s, val, val_s, (size_t)ms, 32, h->s));
  if (h->profiling) VX_HIP(h, hipEventRecord(h->ev_prof[2], h->s));
  intake_gather_kernel<<<vxu::blocks_for(ms), 256, 0, h->s>>>(key_s, val_s, dec, ms, counters, (long long)n_points, o_xyz, o_toff, rec);
  VX_HIP(h, hipGetLastError());
  h->launches += 2;
  VX_HIP(h, hipMemcpyAsync(h->h_rec, rec, REC_LEN * sizeof(double), hipMemcpyDeviceToHost, h->s));
  VX_HIP(h, hipEventRecord(h->ev_done, h->s));
  if (h->profiling) { VX_HIP(h, hipEventRecord(h->ev_prof[3], h->s)); h->prof_valid = true; }
  VX_HIP(h, vxwait::stream_wait(h->s));
  h->waits += 1;

  std::memcpy(rec_out, h->h_rec, REC_LEN * sizeof(double));
  h->n_decoded = n_points;
  if (rec_out[0] == 0.0) return vxu::fail(h, VXBA_ERR_ARG, "vxba_intake_push: every surviving point lies behind 0.11 s (upstream pops an empty vector)");
  h->n = (int64_t)rec_out[0]; h->d_xyz = o_xyz; h->d_toff = o_toff;
  h->toff_first = (float)rec_out[1]; h->toff_last = (float)rec_out[2];
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
