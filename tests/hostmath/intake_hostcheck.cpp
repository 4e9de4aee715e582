// Host build of voxel-slam_amd/csrc/vxba_intake_math.hpp for tests/test_intake_cpu.py: the text the decode kernel runs, compiled with g++
// (-ffp-contract=off, as the device unit), against tests/_intake_ref.py.
#include <cstdint>
#include <cstring>
#include <vector>

#include "../../voxel-slam_amd/csrc/vxba_intake_math.hpp"

extern "C" {

// Every point of a message through decode_point, from a dword array that starts `shift` (0..3) bytes in front of the message, as a workgroup's LDS
// range does.  out: n x 4 floats (x, y, z, curvature), verdict n, key n (time_key of the curvature).
int ikh_decode(const uint8_t* bytes, long long n, const int32_t* layout, long long point_filter_num, double blind, double time_head, int shift, float* out, int32_t* verdict,
               uint32_t* key) {
  vxik::Layout L;
  std::memcpy(&L, layout, sizeof L);
  const size_t total = (size_t)n * (size_t)L.point_step;
  std::vector<uint32_t> w((shift + total + 3) / 4 + 1, 0xA5A5A5A5u);
  if (total) std::memcpy((uint8_t*)w.data() + shift, bytes, total);
  for (long long i = 0; i < n; i++) {
    float p[4];
    verdict[i] = vxik::decode_point(w.data(), (uint32_t)(shift + i * L.point_step), L, i, point_filter_num, blind, time_head, p);
    std::memcpy(out + 4 * i, p, sizeof p);
    key[i] = vxik::time_key(p[3]);
  }
  return 0;
}

int ikh_constants(int32_t* out) {
  out[0] = vxik::MAX_STEP; out[1] = vxik::KEEP; out[2] = vxik::DROP_DECIMATED; out[3] = vxik::DROP_TRIM; out[4] = (int32_t)sizeof(vxik::Layout);
  return 0;
}

}  // extern "C"
