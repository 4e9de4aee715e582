// Device-to-device core of the voxel-grid filter (vxba_downsample.hip), for callers inside the library (vxba_hba.hip).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "vxba_dev.hpp"

namespace vxd {

// grow-only temporaries of one caller (one stream): never shared between threads
struct Scratch {
  vxu::Arena work;
  unsigned int* pinned = nullptr;   // two words of pinned host memory: range check and voxel count come down here (polled, not waited for)
  void release() { work.release(); if (pinned) hipHostFree(pinned); pinned = nullptr; }
};
// d_in: n x 3 floats on the device (unchanged), d_out: room for n x 3 floats; *n_out = occupied voxels.  Two small device-to-host copies
// (range check, voxel count) are waited for by polling `s`.  voxel_size < 0.001: the cloud is copied through (tools.hpp:203).
// d_sel != nullptr selects down_sampling_close (tools.hpp:240-302) instead: per voxel the point nearest the voxel's mean, and its index into d_in in
// d_sel (room for n entries) -- so that a caller can carry the point's other fields (its time) along.
int downsample_device(Scratch& sc, hipStream_t s, const float* d_in, int64_t n, double voxel_size, float* d_out, int64_t* n_out, unsigned int* d_sel = nullptr);

}  // namespace vxd
