// Arithmetic of the scan intake (VoxelSLAM/src/feature_point.hpp:142-366 and pcl_handler, voxelslam.hpp:76-103; include/vxba.h: vxba_intake_*), host +
// device: vxba_intake.hip runs it in its decode kernel, tests/hostmath/intake_hostcheck.cpp compiles the same text with g++ for the CPU suite.
//
// Both translation units that include this file are compiled WITHOUT floating-point contraction, so every expression rounds as written.
//
// One point of a driver message, from its bytes to (x, y, z, curvature, verdict):
//   * fields are little-endian and sit at any byte offset; they are assembled from a dword array (LDS in the kernel) that starts at an aligned address
//     `shift` bytes in front of the message, so no load is ever issued on an unaligned address.
//   * the time rules are the reference's lines: as is (float) time (:188); nanoseconds (float) u32 / float(1000000000) (:155, :271) -- the conversion
//     rounds to nearest, the division is correctly rounded; minus head (float)(t - time_head) on doubles (:304, :335); none 0 (:356).
//   * the blind test (:159) is x*x + y*y + z*z in float, left to right, compared as double, strictly.  A NaN fails it, as upstream.
//   * stated deviations: a coordinate or a time that is not finite drops the point (upstream's sort is undefined on a NaN, and nothing downstream
//     accepts an infinite coordinate); -0.0 times become +0.0, so that equal times have equal bits.
//   * the trim of pcl_handler (:96-97) -- (double) curvature > 0.11 off the sorted tail -- is a per-point verdict here: the same set, known before the sort.
#pragma once
#include <cmath>
#include <cstdint>

#if defined(__HIPCC__)
#define VXK_HD __host__ __device__ __forceinline__
#else
#define VXK_HD inline
#endif

namespace vxik {

constexpr int TIME_NONE = 0, TIME_F32 = 1, TIME_U32 = 2, TIME_F64 = 3;                 // vxba_scan_layout.time_type
constexpr int RULE_NONE = 0, RULE_AS_IS = 1, RULE_NANOSECONDS = 2, RULE_MINUS_HEAD = 3;  // vxba_scan_layout.time_rule
constexpr int MAX_STEP = 240;                    // 256 points x MAX_STEP bytes + 8 of LDS per workgroup stays below 64 KB
constexpr double TRIM = 0.11;                    // voxelslam.hpp:96
constexpr uint32_t KEY_DROPPED = 0xFFFFFFFFu;    // sorts behind every time a survivor can carry (<= 0.11)

// verdicts, in the order the tests are made
constexpr int DROP_DECIMATED = 0, DROP_BLIND = 1, DROP_NONFINITE = 2, DROP_TRIM = 3, KEEP = 4;

struct Layout { int32_t point_step, off_x, off_y, off_z, off_time, time_type, time_rule, filter; };   // vxba_scan_layout, member for member

// the 4 bytes at byte offset `o` of a dword array (one spare dword behind the last one that holds data)
VXK_HD uint32_t load_u32(const uint32_t* w, uint32_t o) {
  const uint32_t k = o >> 2, sh = (o & 3u) * 8u;
  const uint64_t two = ((uint64_t)w[k + 1] << 32) | (uint64_t)w[k];
  return (uint32_t)(two >> sh);
}
VXK_HD float bits_f32(uint32_t b) { union { uint32_t u; float f; } c; c.u = b; return c.f; }
VXK_HD uint32_t f32_bits(float f) { union { uint32_t u; float f; } c; c.f = f; return c.u; }
VXK_HD double bits_f64(uint64_t b) { union { uint64_t u; double f; } c; c.u = b; return c.f; }

VXK_HD float div_rn(float a, float b) {
#if defined(__HIP_DEVICE_COMPILE__)
  return __fdiv_rn(a, b);
#else
  return a / b;
#endif
}

// `curvature` of the point whose bytes start at byte offset `base` of w
VXK_HD float point_time(const uint32_t* w, uint32_t base, const Layout& L, double time_head) {
  if (L.time_rule == RULE_AS_IS) return bits_f32(load_u32(w, base + (uint32_t)L.off_time));
  if (L.time_rule == RULE_NANOSECONDS) return div_rn((float)load_u32(w, base + (uint32_t)L.off_time), float(1000000000));
  if (L.time_rule == RULE_MINUS_HEAD) {
    const uint64_t lo = load_u32(w, base + (uint32_t)L.off_time), hi = load_u32(w, base + (uint32_t)L.off_time + 4u);
    return (float)(bits_f64((hi << 32) | lo) - time_head);
  }
  return 0.0f;
}

VXK_HD bool finite32(float v) { return (f32_bits(v) & 0x7F800000u) != 0x7F800000u; }

// Point i of the message: p = (x, y, z, curvature) and the verdict.  point_filter_num >= 1.
VXK_HD int decode_point(const uint32_t* w, uint32_t base, const Layout& L, long long i, long long point_filter_num, double blind, double time_head, float p[4]) {
  const float x = bits_f32(load_u32(w, base + (uint32_t)L.off_x)), y = bits_f32(load_u32(w, base + (uint32_t)L.off_y)), z = bits_f32(load_u32(w, base + (uint32_t)L.off_z));
  float t = point_time(w, base, L, time_head);
  if ((f32_bits(t) & 0x7FFFFFFFu) == 0u) t = bits_f32(0u);   // -0.0 -> +0.0
  p[0] = x; p[1] = y; p[2] = z; p[3] = t;
  if (L.filter) {
    if (i % point_filter_num != 0) return DROP_DECIMATED;
    const float xx = x * x, yy = y * y, zz = z * z;
    const float s = (xx + yy) + zz;
    if (!((double)s > blind)) return DROP_BLIND;
  }
  if (!finite32(x) || !finite32(y) || !finite32(z) || !finite32(t)) return DROP_NONFINITE;
  if ((double)t > TRIM) return DROP_TRIM;
  return KEEP;
}

// sort key of a time: unsigned order = float order (finite values, -0.0 already gone)
VXK_HD uint32_t time_key(float t) {
  const uint32_t b = f32_bits(t);
  return (b & 0x80000000u) ? ~b : (b | 0x80000000u);
}

// ---- yaw-derived times: the Velodyne branch without a usable time field (feature_point.hpp:200-252), include/vxba.h: vxba_intake_push_yaw ----------
// Upstream walks the points once, carrying yaw_last, yaw_bias and cool.  Restated: every non-skipped point has the angle r = (double) atan2f(y, x) *
// 57.2957; an ACTIVE point (not skipped, not blind) j with the previous active point p (the first non-skipped point for the first one) has d = r_j - r_p,
// and the walk's state is q in {0, 1} (whether yaw_last carries the `+= 360` of :237), the wrap count k (yaw_bias = 360 k) and the index e of the
// last wrap event (cool = 1000 - (j - e)).  d falls into one of four classes, and all but one of them are maps on q that need nothing else:
//     d >  180   candidate: q = 1 -> 0.  q = 0: an EVENT (k += 1, e = j, q = 0) when cool allows (no event yet, or j - e >= 1000), else q = 1
//     d == 180   q = 0
//     -180 <= d < 180   q stays
//     d < -180   q = 1
// so between two events the walk is a composition of 2-state maps, and the events are the only serial chain (vxba_intake.hip: yaw_resolve_kernel).
// The float atan2 is the float rounding of the double routine's value (include/vxba.h, FIXED CHOICES): never the device's atan2f.
constexpr int RULE_YAW = 4;
constexpr double YAW_SKIP_X = 0.1, YAW_DEG = 57.2957, YAW_HALF = 180.0, YAW_TURN = 360.0, YAW_LATE = 0.1;   // :216, :219, :230, :232, :246
constexpr long long YAW_COOL = 1000;                                                                       // :232
constexpr int YAW_SKIPPED = 0, YAW_BLIND = 1, YAW_ACTIVE = 2;                  // what a point is to the walk
constexpr int YAW_IDENT = 0, YAW_SET = 1, YAW_RESET = 2, YAW_CAND = 3;         // the class of d
// a map on q as two bits: bit 0 the image of q = 0, bit 1 the image of q = 1
constexpr uint32_t YAW_MAP_IDENT = 2u, YAW_MAP_SET = 3u, YAW_MAP_RESET = 0u, YAW_MAP_TOGGLE = 1u;

// what point (x, y, z) is to the walk, and its angle in *r (left alone for a skipped point).  A non-finite coordinate skips the point (FIXED CHOICES).
VXK_HD int yaw_point(float x, float y, float z, double blind, double* r) {
  if (!finite32(x) || !finite32(y) || !finite32(z)) return YAW_SKIPPED;
  if ((double)std::fabs(x) < YAW_SKIP_X) return YAW_SKIPPED;                    // :216
  const float a = (float)std::atan2((double)y, (double)x);
  *r = (double)a * YAW_DEG;                                                     // :219, the bias taken off later
  const float xx = x * x, yy = y * y, zz = z * z;
  const float s = (xx + yy) + zz;
  return (double)s < blind ? YAW_BLIND : YAW_ACTIVE;                            // :227, strictly: a squared range equal to blind stays
}

VXK_HD int yaw_class(double d) {
  if (d > YAW_HALF) return YAW_CAND;
  if (d == YAW_HALF) return YAW_RESET;
  if (d < -YAW_HALF) return YAW_SET;
  return YAW_IDENT;
}

// cool <= 0 at index j: no event so far (e < 0), or the last one at least YAW_COOL ORIGINAL indices back (skipped points count)
VXK_HD bool yaw_cool_allows(long long e, long long j) { return e < 0 || j - e >= YAW_COOL; }

// the map a special point applies to q; a candidate that cool allows ends in q = 0 either way (an event from q = 0, a plain reset from q = 1)
VXK_HD uint32_t yaw_map(int cls, bool allowed) {
  if (cls == YAW_SET) return YAW_MAP_SET;
  if (cls == YAW_RESET) return YAW_MAP_RESET;
  if (cls == YAW_CAND) return allowed ? YAW_MAP_RESET : YAW_MAP_TOGGLE;
  return YAW_MAP_IDENT;
}
VXK_HD uint32_t yaw_map_apply(uint32_t m, uint32_t q) { return (m >> q) & 1u; }
// first `first`, then `then`
VXK_HD uint32_t yaw_map_compose(uint32_t then, uint32_t first) { return yaw_map_apply(then, first & 1u) | (yaw_map_apply(then, (first >> 1) & 1u) << 1); }

// what a special point leaves behind: (wrap count << 2) | (event here << 1) | q
VXK_HD uint32_t yaw_state_pack(uint32_t k, bool event, uint32_t q) { return (k << 2) | (event ? 2u : 0u) | q; }

// yaw_angle as :219-238 leave it: at an event the bias of before comes off, then 360 (:232) -- two subtractions; anywhere else the current bias
VXK_HD double yaw_value(double r, uint32_t k, bool event, uint32_t q) {
  double yaw;
  if (event) {
    const double before = r - YAW_TURN * (double)(k - 1u);
    yaw = before - YAW_TURN;
  } else {
    yaw = r - YAW_TURN * (double)k;
  }
  if (q) yaw = yaw + YAW_TURN;                                                  // :237
  return yaw;
}

// :240: a double quotient, correctly rounded, assigned to a float
VXK_HD float yaw_curvature(double yaw_first, double yaw, double omega_l) {
  const double turned = yaw_first - yaw;
  return (float)(turned / omega_l);
}

// :246
VXK_HD bool yaw_keep(float curvature) { return curvature >= 0.0f && (double)curvature < YAW_LATE; }

}  // namespace vxik
