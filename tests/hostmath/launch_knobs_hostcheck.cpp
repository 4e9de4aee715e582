// The readers of the VXBA_* knobs (voxel-slam_amd/csrc/vxba_env.hpp) on their own, for tests/test_launch_knobs_cpu.py.  Every reader call of the
// library is listed here by the knob it reads, with the arguments of its call site; all of them read the environment variable KNOB instead, which
// the test sets, so that one run prints the whole table for one value:  <knob> <value>.
//   launch_knobs_hostcheck            the table
//   launch_knobs_hostcheck threads    eight threads go through one `static const` reader at once (as the four host threads of a hierarchical pass go
//                                     through a launcher) and through the uncached readers; prints "threads ok <value>" when all of them agree
#include <cstdio>
#include <cstring>
#include <thread>
#include <vector>

#include "../../voxel-slam_amd/csrc/vxba_env.hpp"

static const char* const KNOB = "KNOB";

static int cached_level() { static const int v = vxu::env_flag(KNOB, 0, "12"); return v; }   // the shape of vxk::dbg_level()

int main(int argc, char** argv) {
  if (argc > 1 && !std::strcmp(argv[1], "threads")) {
    int got[8];
    long long raw[8];
    std::vector<std::thread> th;
    for (int i = 0; i < 8; i++) th.emplace_back([&got, &raw, i] { got[i] = cached_level(); raw[i] = vxu::env_int(KNOB, 100, 0) + vxu::env_flag(KNOB, 1); });
    for (auto& t : th) t.join();
    for (int i = 1; i < 8; i++) if (got[i] != got[0] || raw[i] != raw[0]) { std::printf("threads disagree\n"); return 1; }
    std::printf("threads ok %d\n", got[0]);
    return 0;
  }
  const int level = vxu::env_flag(KNOB, 0, "12");
  std::printf("VXBA_DBG %d\n", level == 1);                                                 // k2, k3, finalize, solve launchers
  std::printf("VXBA_DBG.fused %d\n", level != 0);                                           // the fused launch
  std::printf("VXBA_LI_TIMING %d\n", vxu::env_flag(KNOB, 0));
  std::printf("VXBA_VOXELIZE_WAITS %d\n", vxu::env_flag(KNOB, 0));
  std::printf("VXBA_K23_PAIR %d\n", vxu::env_flag(KNOB, 1));
  std::printf("VXBA_VOXELIZE_PARTITION %d\n", vxu::env_flag(KNOB, 1));
  std::printf("VXBA_VOXELIZE_COMPACT_KEY %d\n", vxu::env_flag(KNOB, 1));
  std::printf("VXBA_LIO_DEVICE_EKF %d\n", vxu::env_flag(KNOB, 1));
  std::printf("VXBA_LI_REC_VRAM %d\n", vxu::env_flag(KNOB, 1));
  std::printf("options_from_env %d\n", vxu::env_flag(KNOB, 1));                             // VXBA_FUSED_SOLVE, _SPEC_COLLECTIVE, _WIDE_DEVICE_SOLVE, _FUSED_SWEEPS
  std::printf("VXBA_K2_HEAD_START %lld\n", vxu::env_int(KNOB, 100, 0));
  std::printf("VXBA_K2_VPB %lld\n", vxu::env_int(KNOB, 64));                                // the call site keeps [32, 64], else 64
  std::printf("VXBA_WIDE_NWG %lld\n", vxu::env_int(KNOB, 128, 1));
  std::printf("VXBA_MAP_FIX_COMPACT_AT %lld\n", vxu::env_int(KNOB, 0));                     // the call site takes it where it is positive
  std::printf("VXBA_SPIN_US %lld\n", vxu::env_int(KNOB, 4000, 0));
  std::printf("VXBA_MAP_DEBUG %d\n", vxu::env_flag(KNOB, 0, nullptr));
  return 0;
}
