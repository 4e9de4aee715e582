// Voxel-grid down-sampling on the GPU: `down_sampling_voxel` (VoxelSLAM/src/tools.hpp:201-238), the filter the reference runs on
// every raw scan before the odometry (voxelslam.cpp:1236, 1577-1583) and on every merged submap of the hierarchical BA (:2447).
// Upstream: an unordered_map from voxel index to a running mean, updated point by point in cloud order, in float.  Here: one key
// per point (upstream's float-typed voxel index), one stable radix sort, run-length encode + scan for the cell table, and one lane
// per occupied voxel that replays the running-mean recurrence over its points in cloud order with unfused float arithmetic -- the
// means are bit-identical to upstream's.  Output order is ascending (x, y, z) voxel index (upstream: hash-map iteration order,
// which is implementation-defined).
#include "vxba_wait.hpp"
#include <hip/hip_runtime.h>

#include <cstdint>
#include <cstring>
#include <mutex>

#include "../../include/vxba.h"
#include "vxba_dev.hpp"
#include "vxba_downsample.h"

namespace vxd {

constexpr long long OFF = 1ll << 20;   // voxel indices in [-2^20, 2^20)

__global__ void ds_key_kernel(const float* __restrict__ xyz, long long n, double voxel_size, unsigned long long* __restrict__ key, unsigned int* __restrict__ idx,
                              int* __restrict__ err) {
#pragma clang fp contract(off)
  const long long q = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  if (q >= n) return;
  unsigned long long k = 0;
  for (int j = 0; j < 3; j++) {
    float loc = (float)((double)xyz[3 * q + j] / voxel_size);   // loc_xyz[j] = p_c.data[j] / voxel_size   (:211)
    if (loc < 0) loc = (float)((double)loc - 1.0);              // loc_xyz[j] -= 1.0                         (:212-213)
    const long long pos = (long long)loc;
    if (pos < -OFF || pos >= OFF) { *err = 1; return; }
    k = (k << 21) | (unsigned long long)(pos + OFF);
  }
  key[q] = k;
  idx[q] = (unsigned int)q;
}

// pp = (pp * curvature + p) / (curvature + 1), curvature += 1   (:227-230), float, unfused, in cloud order
__global__ void ds_mean_kernel(const float* __restrict__ xyz, const unsigned int* __restrict__ idx_sorted, const long long* __restrict__ cell_ptr, long long n_cells,
                               float* __restrict__ out) {
#pragma clang fp contract(off)
  const long long c = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  if (c >= n_cells) return;
  long long q = cell_ptr[c];
  const long long end = cell_ptr[c + 1];
  unsigned int i = idx_sorted[q];
  float x = xyz[3 * (size_t)i], y = xyz[3 * (size_t)i + 1], z = xyz[3 * (size_t)i + 2], cur = 1.0f;
  for (q++; q < end; q++) {
    i = idx_sorted[q];
    const float d = cur + 1.0f;
    x = (x * cur + xyz[3 * (size_t)i]) / d;
    y = (y * cur + xyz[3 * (size_t)i + 1]) / d;
    z = (z * cur + xyz[3 * (size_t)i + 2]) / d;
    cur = d;
  }
  out[3 * c] = x; out[3 * c + 1] = y; out[3 * c + 2] = z;
}

// down_sampling_close (tools.hpp:269-300): the float sum of the voxel's points in cloud order divided by their number, then the first point at the smallest
// double-typed squared distance below 100 from that mean (the voxel's first point if none is)
__global__ void ds_close_kernel(const float* __restrict__ xyz, const unsigned int* __restrict__ idx_sorted, const long long* __restrict__ cell_ptr, long long n_cells,
                                float* __restrict__ out, unsigned int* __restrict__ sel) {
#pragma clang fp contract(off)
  const long long c = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  if (c >= n_cells) return;
  const long long beg = cell_ptr[c], end = cell_ptr[c + 1];
  unsigned int i = idx_sorted[beg];
  float x = xyz[3 * (size_t)i], y = xyz[3 * (size_t)i + 1], z = xyz[3 * (size_t)i + 2];
  for (long long q = beg + 1; q < end; q++) {
    i = idx_sorted[q];
    x += xyz[3 * (size_t)i]; y += xyz[3 * (size_t)i + 1]; z += xyz[3 * (size_t)i + 2];
  }
  const float cnt = (float)(int)(end - beg);
  x /= cnt; y /= cnt; z /= cnt;
  double ndis = 100;
  unsigned int best = idx_sorted[beg];
  for (long long q = beg; q < end; q++) {
    i = idx_sorted[q];
    const double xx = (double)(x - xyz[3 * (size_t)i]), yy = (double)(y - xyz[3 * (size_t)i + 1]), zz = (double)(z - xyz[3 * (size_t)i + 2]);
    const double dis = (xx * xx + yy * yy) + zz * zz;
    if (dis < ndis) { best = i; ndis = dis; }
  }
  out[3 * c] = xyz[3 * (size_t)best]; out[3 * c + 1] = xyz[3 * (size_t)best + 1]; out[3 * c + 2] = xyz[3 * (size_t)best + 2];
  sel[c] = best;
}

__global__ void ds_widen_kernel(const unsigned int* __restrict__ cnt, long long n, long long* __restrict__ out) {
  const long long q = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  if (q < n) out[q] = (long long)cnt[q];
  if (q == n) out[q] = 0;
}

}  // namespace vxd

namespace vxd {

int downsample_device(Scratch& sc, hipStream_t s, const float* d_in, int64_t n, double voxel_size, float* d_out, int64_t* n_out, unsigned int* d_sel) {
  *n_out = 0;
  if (n == 0) return VXBA_OK;
  if (n < 0 || n >= (1ll << 32)) return VXBA_ERR_ARG;
  if (voxel_size < 0.001) {
    if (hipMemcpyAsync(d_out, d_in, (size_t)n * 3 * sizeof(float), hipMemcpyDeviceToDevice, s) != hipSuccess) return VXBA_ERR_HIP;
    *n_out = n;
    return VXBA_OK;
  }
  const unsigned grid = (unsigned)((n + 255) / 256), grid1 = (unsigned)((n + 256) / 256);
  vxu::Cells<long long> c;
  VX_HIP_RC(c.size((size_t)n, 63, s));
  VX_HIP_RC(sc.work.layout([&](vxu::Arena& a) { c.carve(a, (size_t)n); }, s));
  // The two words the host needs -- the range-error flag and the number of occupied voxels -- are written by the kernels that produce them
  // straight into mapped pinned memory (round 6: no memset, no copy-engine round trips; hipHostMalloc'd memory is mapped at the same address).
  if (!sc.pinned) VX_HIP_RC(hipHostMalloc((void**)&sc.pinned, 64, hipHostMallocDefault));
  ((volatile unsigned int*)sc.pinned)[0] = 0;
  ((volatile unsigned int*)sc.pinned)[1] = 0;
  int* d_err = (int*)sc.pinned;
  unsigned int* d_runs = sc.pinned + 1;
  ds_key_kernel<<<grid, 256, 0, s>>>(d_in, n, voxel_size, c.key, c.idx, d_err);
  VX_HIP_RC(hipGetLastError());
  VX_HIP_RC(vxu::sort(c.temp, c.key, c.key_s, c.idx, c.idx_s, (size_t)n, 63, s));
  VX_HIP_RC(vxu::encode(c.temp, c.key_s, (size_t)n, c.ukey, c.cnt, d_runs, s));
  // by polling: a blocking wait parks the thread (~25 us to wake up from); pinned destination: a copy into pageable memory is staged and waited for
  VX_HIP_RC(vxwait::stream_wait(s));
  const int err = (int)((volatile unsigned int*)sc.pinned)[0];
  const unsigned int runs = ((volatile unsigned int*)sc.pinned)[1];
  if (err) return VXBA_ERR_ARG;   // a voxel index outside [-2^20, 2^20)
  ds_widen_kernel<<<grid1, 256, 0, s>>>(c.cnt, (long long)runs, c.ptr);
  VX_HIP_RC(hipGetLastError());
  VX_HIP_RC(vxu::scan(c.temp, c.ptr, c.ptr, (size_t)runs + 1, s));
  if (d_sel) ds_close_kernel<<<(unsigned)((runs + 63) / 64), 64, 0, s>>>(d_in, c.idx_s, c.ptr, (long long)runs, d_out, d_sel);
  else ds_mean_kernel<<<(unsigned)((runs + 63) / 64), 64, 0, s>>>(d_in, c.idx_s, c.ptr, (long long)runs, d_out);
  VX_HIP_RC(hipGetLastError());
  *n_out = (int64_t)runs;
  return VXBA_OK;
}

}  // namespace vxd

static int ds_entry(int device, int64_t n, const float* xyz, double voxel_size, float* out_xyz, int64_t* n_out, int32_t* sel_out) {
  if (n < 0 || !n_out || (n > 0 && (!xyz || !out_xyz)) || n >= (1ll << 32)) return VXBA_ERR_ARG;
  *n_out = 0;
  if (n == 0) return VXBA_OK;
  if (voxel_size < 0.001) {   // upstream returns the cloud untouched (:203, :242)
    std::memcpy(out_xyz, xyz, (size_t)n * 3 * sizeof(float));
    for (int64_t i = 0; sel_out && i < n; i++) sel_out[i] = (int32_t)i;
    *n_out = n;
    return VXBA_OK;
  }
  if (const int rc = vxu::select_device(device)) return rc;
  // one grow-only scratch + in / out buffers per device for this stand-alone entry point (it runs once per scan: a dozen hipMalloc / hipFree
  // pairs per call cost more than the sort); calls are serialised on it.  Static storage, so raw pointers and explicit frees and no vxu::Dev / vxu::Pin
  // (Scratch included): their destructors would run after the HIP runtime has shut down
  static std::mutex mtx;
  static vxd::Scratch scratch[16];
  static float* io[16] = {nullptr};   // in | out | selected indices (n words)
  static size_t io_cap[16] = {0};
  std::lock_guard<std::mutex> lock(mtx);
  const int dv = device < 16 ? device : 15;
  if ((size_t)n > io_cap[dv] || device >= 16) {
    if (io[dv]) { hipDeviceSynchronize(); hipFree(io[dv]); }
    io[dv] = nullptr; io_cap[dv] = 0;
    const size_t want = (size_t)n + (size_t)n / 4;
    if (hipMalloc((void**)&io[dv], (2 * want * 3 + want) * sizeof(float)) != hipSuccess) return VXBA_ERR_HIP;
    io_cap[dv] = want;
  }
  float* d_in = io[dv];
  float* d_out = io[dv] + 3 * io_cap[dv];
  unsigned int* d_sel = sel_out ? (unsigned int*)(io[dv] + 6 * io_cap[dv]) : nullptr;
  if (hipMemcpy(d_in, xyz, (size_t)n * 3 * sizeof(float), hipMemcpyHostToDevice) != hipSuccess) return VXBA_ERR_HIP;
  int64_t kept = 0;
  int rc;
  if (device >= 16) {
    // devices beyond the per-device table share slot 15 for the in / out buffers (re-allocated on every call, above); the sort's scratch must
    // not be shared: it would keep memory owned by the previous such device (round-5 advisor) -- a scratch of the call's own instead
    vxd::Scratch own;
    rc = vxd::downsample_device(own, nullptr, d_in, n, voxel_size, d_out, &kept, d_sel);
    (void)hipDeviceSynchronize();
    own.release();
  } else {
    rc = vxd::downsample_device(scratch[dv], nullptr, d_in, n, voxel_size, d_out, &kept, d_sel);
  }
  if (rc != VXBA_OK) return rc;
  if (hipMemcpy(out_xyz, d_out, (size_t)kept * 3 * sizeof(float), hipMemcpyDeviceToHost) != hipSuccess) return VXBA_ERR_HIP;
  if (sel_out && hipMemcpy(sel_out, d_sel, (size_t)kept * sizeof(int32_t), hipMemcpyDeviceToHost) != hipSuccess) return VXBA_ERR_HIP;
  *n_out = kept;
  return VXBA_OK;
}

extern "C" int vxba_down_sampling_voxel(int device, int64_t n, const float* xyz, double voxel_size, float* out_xyz, int64_t* n_out) {
  return ds_entry(device, n, xyz, voxel_size, out_xyz, n_out, nullptr);
}

extern "C" int vxba_down_sampling_close(int device, int64_t n, const float* xyz, double voxel_size, float* out_xyz, int32_t* sel_out, int64_t* n_out) {
  if (!sel_out || n >= (1ll << 31)) return VXBA_ERR_ARG;
  return ds_entry(device, n, xyz, voxel_size, out_xyz, n_out, sel_out);
}
