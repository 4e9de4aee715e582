// Host-side plumbing shared by every unit that owns a handle or a stand-alone entry point (the back end: vxba_downsample, vxba_hba, vxba_pgo,
// vxba_loopreg, vxba_loopsearch, vxba_init, vxba_imuekf, vxba_intake, vxba_keyframe, vxba_session, vxba_corner; the per-scan path: vxba_map, vxba_lio,
// vxba_capi*, vxba_voxelize, vxba_wide): the error path, the device check, the owners of a handle's long-lived memory, stream and events (Dev<T>,
// Pin<T>, MapPin<T>, CohPin<T>, FineDev<T> over vxba_buf.hpp; Stream, Event: behind every handle of both lists but the voxeliser's process-wide pool), the grow-only workspace of a call (Arena, Lease) and rocPRIM's two-pass temp-storage protocol.  Host-only and free of floating-point
// arithmetic: the same in the units built with -ffp-contract=off and in those built without.
#pragma once
#include <hip/hip_runtime.h>

#include <rocprim/device/device_radix_sort.hpp>
#include <rocprim/device/device_run_length_encode.hpp>
#include <rocprim/device/device_scan.hpp>

#include <mutex>
#include <string>
#include <utility>
#include "../../include/vxba.h"
#include "vxba_buf.hpp"
#include "vxba_env.hpp"   // vxu::env_flag, vxu::env_int: the readers of the VXBA_* knobs

namespace vxu {

// the message a handle's *_last_error returns and the code its entry point returns; VX_HIP_RC: below a handle, where there is nowhere to leave a message
template <class H>
int fail(H* h, int rc, const std::string& m) { if (h) h->err = m; return rc; }
#define VX_HIP(h, ...) do { hipError_t e_ = (__VA_ARGS__); if (e_ != hipSuccess) return vxu::fail(h, VXBA_ERR_HIP, std::string(#__VA_ARGS__) + ": " + hipGetErrorString(e_)); } while (0)
#define VX_HIP_RC(...) do { if ((__VA_ARGS__) != hipSuccess) return VXBA_ERR_HIP; } while (0)

// the check at the top of every *_create and stand-alone entry point; `device` is the calling thread's current device afterwards
inline int select_device(int device) {
  int ndev = 0;
  if (hipGetDeviceCount(&ndev) != hipSuccess || device < 0 || device >= ndev) return VXBA_ERR_NODEV;
  return hipSetDevice(device) == hipSuccess ? VXBA_OK : VXBA_ERR_HIP;
}

// the kinds of memory a handle owns (vxba_buf.hpp): Dev<T> on the current device, Pin<T> pinned on the host; MapPin<T> pinned and mapped into the
// device's address space (zero-copy stores; the map's h_cnt, the odometry's h_partials), CohPin<T> mapped and coherent (the factor's result words, which
// the host reads while the kernel still runs), FineDev<T> fine-grained device memory (lirec_vram, the peers' box).  Each keeps exactly the flags its
// users had.  The device alias of a mapped block is fetched right after the reserve that made it and is a plain pointer, reset where the owner is released.
struct DevMem {
  using status = hipError_t;
  static status alloc(void** p, size_t bytes) { return hipMalloc(p, bytes); }
  static status free(void* p) { return hipFree(p); }
};
struct PinMem {
  using status = hipError_t;
  static status alloc(void** p, size_t bytes) { return hipHostMalloc(p, bytes, hipHostMallocDefault); }
  static status free(void* p) { return hipHostFree(p); }
};
struct MapPinMem {
  using status = hipError_t;
  static status alloc(void** p, size_t bytes) { return hipHostMalloc(p, bytes, hipHostMallocMapped); }
  static status free(void* p) { return hipHostFree(p); }
};
struct CohPinMem {
  using status = hipError_t;
  static status alloc(void** p, size_t bytes) { return hipHostMalloc(p, bytes, hipHostMallocMapped | hipHostMallocCoherent); }
  static status free(void* p) { return hipHostFree(p); }
};
struct FineDevMem {
  using status = hipError_t;
  static status alloc(void** p, size_t bytes) { return hipExtMallocWithFlags(p, bytes, hipDeviceMallocFinegrained); }
  static status free(void* p) { return hipFree(p); }
};
template <class T> using Dev = Buf<T, DevMem>;
template <class T> using Pin = Buf<T, PinMem>;
template <class T> using MapPin = Buf<T, MapPinMem>;
template <class T> using CohPin = Buf<T, CohPinMem>;
template <class T> using FineDev = Buf<T, FineDevMem>;

// a handle's own stream (non-blocking) and an event of it, destroyed with the handle; the same rule as for Buf: members and locals only
struct Stream {
  hipStream_t s = nullptr;
  Stream() = default;
  Stream(const Stream&) = delete;
  Stream& operator=(const Stream&) = delete;
  ~Stream() { if (s) hipStreamDestroy(s); }
  hipError_t create() { return s ? hipSuccess : hipStreamCreateWithFlags(&s, hipStreamNonBlocking); }
  operator hipStream_t() const { return s; }
};
struct Event {
  hipEvent_t e = nullptr;
  Event() = default;
  Event(const Event&) = delete;
  Event& operator=(const Event&) = delete;
  ~Event() { if (e) hipEventDestroy(e); }
  hipError_t create(unsigned flags = hipEventDefault) { return e ? hipSuccess : hipEventCreateWithFlags(&e, flags); }
  operator hipEvent_t() const { return e; }
};

// never zero: a launch whose kernel finds nothing to do (n <= 0) is still a valid launch
inline unsigned blocks_for(long long n, int b = 256) { return (unsigned)((n > 0 ? n + b - 1 : b) / b); }

// Grow-only device workspace of one handle or stream (never shared between threads), carved anew by every call that uses it:
//   VX_HIP(h, h->work.layout([&](vxu::Arena& a) { d_x = a.take<double>(3 * n); d_key = a.take<unsigned long long>(n); }, h->s));
// layout() runs the carving twice -- into an Arena without a block, which only counts, then into this one with that much reserved -- so that the
// size asked for and the size carved cannot drift apart.  A later layout() rewinds the block and may free it: pointers of an earlier carving are dead.
class Arena {
 public:
  // a block that grows to bytes + bytes / grow_div (the local map keeps its 3/2); grow_div 0: to bytes and no further
  explicit Arena(unsigned grow_div = 4) : grow_div_(grow_div) {}
  // room for `bytes`, and rewound.  Growing frees the old block, after waiting for `s` (whose kernels may still use it): *synced tells.
  hipError_t reserve(size_t bytes, hipStream_t s, bool* synced = nullptr) {
    const bool grow = bytes > cap_, wait = grow && base_;
    if (synced) *synced = wait;
    used_ = 0;
    if (!grow) return hipSuccess;
    if (wait) { const hipError_t e = hipStreamSynchronize(s); if (e != hipSuccess) return e; hipFree(base_); }
    base_ = nullptr; cap_ = 0;
    const size_t want = bytes + (grow_div_ ? bytes / grow_div_ : 0);
    const hipError_t e = hipMalloc((void**)&base_, want);
    if (e == hipSuccess) cap_ = want;
    return e;
  }
  // the next `count` elements, 256-byte aligned
  template <class T>
  T* take(size_t count) { char* r = base_ ? base_ + used_ : nullptr; used_ += (count * sizeof(T) + 255) / 256 * 256; return (T*)r; }
  // the bytes a carving takes: it runs into an Arena without a block, which only counts
  template <class F>
  static size_t measure(F&& carve) { Arena count; carve(count); return count.used_; }
  template <class F>
  hipError_t layout(F&& carve, hipStream_t s, bool* synced = nullptr) {
    const hipError_t e = reserve(measure(carve), s, synced);
    if (e == hipSuccess) carve(*this);
    return e;
  }
  void rewind() { used_ = 0; }
  void release() { if (base_) hipFree(base_); base_ = nullptr; cap_ = used_ = 0; }
  size_t capacity() const { return cap_; }   // bytes held

 private:
  char* base_ = nullptr;
  size_t cap_ = 0, used_ = 0;
  unsigned grow_div_;
};

// Workspace of the stand-alone (handle-less) entry points: one Arena per device, leased for the duration of a call.  These calls are small batched
// kernels on the null stream, run once per scan (plane fits, cluster builds, plane covariances); a handful of hipMalloc / hipFree pairs each time
// costs ten times the kernel.  Calls on one device take turns; a carving above 1 GiB gets a private block that is freed with the lease.
class Lease {
 public:
  explicit Lease(int device) : slot_(device >= 0 && device < 16 ? &slots()[device] : nullptr) { if (slot_) slot_->mtx.lock(); }
  ~Lease() { own_.release(); if (slot_) slot_->mtx.unlock(); }
  Lease(const Lease&) = delete;
  Lease& operator=(const Lease&) = delete;
  // as Arena::layout, on the null stream; the current device must be the lease's
  template <class F>
  hipError_t layout(F&& carve) {
    const size_t bytes = Arena::measure(carve);
    Arena& a = slot_ && bytes <= ((size_t)1 << 30) ? slot_->arena : own_;
    const hipError_t e = a.reserve(bytes, nullptr);
    if (e == hipSuccess) carve(a);
    return e;
  }

 private:
  struct Slot { std::mutex mtx; Arena arena; };
  static Slot* slots() { static Slot s[16]; return s; }
  Slot* slot_;
  Arena own_{0};   // the private block: exactly what the call needs
};

// rocPRIM: stable radix sort of (key, value) pairs, run-length encode, exclusive prefix sum.  Every call is made twice: with a null temp pointer it
// only reports the temp bytes it wants, with a real one it runs, and it may overwrite the size it was handed.  *_temp() raise `bytes` to what the
// stage wants (start from Temp{}, pass every stage that will run); the stage functions enqueue on `s` with the size handed over by value.  What runs
// between the stages -- kernels, event records, a host wait -- is the caller's.  Config: a rocPRIM radix_sort_config other than the default one.
struct Temp { void* p = nullptr; size_t bytes = 8; };
template <class K, class V, class Config = rocprim::default_config>
hipError_t sort_temp(size_t& bytes, size_t n, unsigned bits, hipStream_t s) {
  size_t t = 0;
  const hipError_t e = rocprim::radix_sort_pairs<Config>(nullptr, t, (K*)nullptr, (K*)nullptr, (V*)nullptr, (V*)nullptr, n, 0, bits, s);
  if (t > bytes) bytes = t;
  return e;
}
template <class Config = rocprim::default_config, class K, class V>
hipError_t sort(Temp t, K* key, K* key_s, V* val, V* val_s, size_t n, unsigned bits, hipStream_t s) { return rocprim::radix_sort_pairs<Config>(t.p, t.bytes, key, key_s, val, val_s, n, 0, bits, s); }
// runs of equal keys in key_s: the distinct keys, their lengths, and the number of runs in *runs_out (device or mapped host memory)
template <class K>
hipError_t encode_temp(size_t& bytes, size_t n, hipStream_t s) {
  size_t t = 0;
  const hipError_t e = rocprim::run_length_encode(nullptr, t, (K*)nullptr, n, (K*)nullptr, (unsigned int*)nullptr, (unsigned int*)nullptr, s);
  if (t > bytes) bytes = t;
  return e;
}
template <class K>
hipError_t encode(Temp t, K* key_s, size_t n, K* ukey, unsigned int* cnt, unsigned int* runs_out, hipStream_t s) { return rocprim::run_length_encode(t.p, t.bytes, key_s, n, ukey, cnt, runs_out, s); }
// out[i] = in[0] + ... + in[i - 1] over `count` elements, in place where out == in: run lengths to offsets, flags to positions
template <class T>
hipError_t scan_temp(size_t& bytes, size_t count, hipStream_t s) {
  size_t t = 0;
  const hipError_t e = rocprim::exclusive_scan(nullptr, t, (T*)nullptr, (T*)nullptr, T(0), count, rocprim::plus<T>(), s);
  if (t > bytes) bytes = t;
  return e;
}
template <class T>
hipError_t scan(Temp t, T* in, T* out, size_t count, hipStream_t s) { return rocprim::exclusive_scan(t.p, t.bytes, in, out, T(0), count, rocprim::plus<T>(), s); }

// The arrays of "sort (voxel key, point index), encode the runs, scan them to a cell table" over n points, and the temp of the three stages: cnt and
// ptr have n + 1 entries (the scan's last output is the total; its temp is sized for that many), Off is the cell table's offset type.
template <class Off>
struct Cells {
  unsigned long long *key = nullptr, *key_s = nullptr, *ukey = nullptr;
  unsigned int *idx = nullptr, *idx_s = nullptr, *cnt = nullptr;
  Off* ptr = nullptr;
  Temp temp;
  hipError_t size(size_t n, unsigned bits, hipStream_t s) {
    hipError_t e = sort_temp<unsigned long long, unsigned int>(temp.bytes, n, bits, s);
    if (e == hipSuccess) e = encode_temp<unsigned long long>(temp.bytes, n, s);
    return e == hipSuccess ? scan_temp<Off>(temp.bytes, n + 1, s) : e;
  }
  void carve(Arena& a, size_t n) {
    key = a.take<unsigned long long>(n); key_s = a.take<unsigned long long>(n); ukey = a.take<unsigned long long>(n);
    idx = a.take<unsigned int>(n); idx_s = a.take<unsigned int>(n); cnt = a.take<unsigned int>(n + 1); ptr = a.take<Off>(n + 1);
    temp.p = a.take<char>(temp.bytes);
  }
};

}  // namespace vxu
