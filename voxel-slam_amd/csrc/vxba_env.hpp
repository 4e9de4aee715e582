// The two readers of the VXBA_* environment knobs: every getenv of csrc is in this file.  Plain C++ without HIP, so that a host program can
// include it on its own (tests/test_launch_knobs_cpu.py); the units get it through vxba_dev.hpp.  A reader parses at every call.  A knob that
// holds for the process is kept by its call site in a function-local `static const` (initialised once, thread-safely); a knob that gives a
// handle its initial value is read where the handle is created, so that a later handle sees a later value.  DESIGN.md lists every knob.
#pragma once
#include <cstdlib>
#include <cstring>

namespace vxu {

// The knob's first character as a digit where `accept` holds it, else dflt; what follows the first character is not looked at.
//   env_flag(name, 0)        on at '1' only            env_flag(name, 1)   off at '0' only
//   env_flag(name, 0, "12")  1 or 2, else 0            accept == nullptr:  1 where the knob is set at all, the empty string included
inline int env_flag(const char* name, int dflt, const char* accept = "01") {
  const char* e = std::getenv(name);
  if (!accept) return e ? 1 : dflt;
  return e && e[0] && std::strchr(accept, e[0]) ? e[0] - '0' : dflt;
}

// atoll of the knob clamped to [lo, hi] (no digits: 0), dflt as it is where the knob is not set
inline long long env_int(const char* name, long long dflt, long long lo = -0x7fffffffffffffffll - 1, long long hi = 0x7fffffffffffffffll) {
  const char* e = std::getenv(name);
  if (!e) return dflt;
  const long long v = std::atoll(e);
  return v < lo ? lo : (v > hi ? hi : v);
}

}  // namespace vxu
