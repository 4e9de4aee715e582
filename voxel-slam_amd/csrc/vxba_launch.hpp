// How the host launchers (vxba_kernels.hip, vxba_wide.hip) pick and start a kernel instantiation: the run-time choice to compile-time tags
// (with_flag, with_variant), the opt-in of an instantiation into more than 64 KB of dynamic LDS (opt_in_lds) and the launch itself, with or
// without dispatch events (launch).  A launcher names its instantiation once, as `constexpr auto kernel = ...<tags>`, and hands that one
// pointer to opt_in_lds and launch: the function that is opted in and the function that runs cannot differ.
#pragma once
#include <hip/hip_ext.h>
#include <hip/hip_runtime.h>

#include <atomic>
#include <type_traits>

namespace vxk {

template <bool B>
using flag_t = std::integral_constant<bool, B>;

// f(flag_t<on>{})
template <class F>
void with_flag(bool on, F&& f) {
  if (on) f(flag_t<true>{});
  else f(flag_t<false>{});
}
// f(DBG, ALT) for the three instantiations a family has of its <DBG, ALT> flags -- ALT: k2's F32, k3's and k23's MIXED -- and no fourth:
// alt wins over dbg (there is no instrumented form of the f32 / mixed kernels), dbg alone, neither
template <class F>
void with_variant(bool dbg, bool alt, F&& f) {
  if (alt) f(flag_t<false>{}, flag_t<true>{});
  else if (dbg) f(flag_t<true>{}, flag_t<false>{});
  else f(flag_t<false>{}, flag_t<false>{});
}

// Dynamic LDS above 64 KB must be opted into per kernel AND per device.  Kernel is the instantiation itself, so every instantiation has its own
// mask: one bit per device, set atomically once the attribute is (host threads of different factors come through here at once).  A device
// beyond the mask's 64 sets the attribute at every call.
template <auto Kernel>
hipError_t opt_in_lds(size_t bytes) {
  static std::atomic<unsigned long long> opted{0ull};
  int dev = 0;
  (void)hipGetDevice(&dev);
  const unsigned long long bit = dev >= 0 && dev < 64 ? 1ull << dev : 0ull;
  if (bit && (opted.load(std::memory_order_relaxed) & bit)) return hipSuccess;
  const hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void*>(Kernel), hipFuncAttributeMaxDynamicSharedMemorySize, (int)bytes);
  if (e == hipSuccess) opted.fetch_or(bit, std::memory_order_relaxed);
  return e;
}

template <class T>
struct as_is { using type = T; };
// The one launch of the launchers: with ev_start (and its ev_stop) the events are tied to the dispatch's own begin / end timestamps, the
// interval rocprofv3 reports for the kernel; without, the plain launch.  The arguments convert to the kernel's parameter types at the call.
template <class... P>
void launch(void (*kernel)(P...), dim3 grid, dim3 block, size_t lds_bytes, hipStream_t s, hipEvent_t ev_start, hipEvent_t ev_stop, typename as_is<P>::type... args) {
  if (ev_start) hipExtLaunchKernelGGL(kernel, grid, block, (uint32_t)lds_bytes, s, ev_start, ev_stop, 0, args...);
  else hipLaunchKernelGGL(kernel, grid, block, lds_bytes, s, args...);
}

}  // namespace vxk
