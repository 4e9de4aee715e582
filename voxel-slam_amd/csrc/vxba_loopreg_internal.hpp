// What the loop search (vxba_loopsearch.hip) uses of the loop-edge registration (vxba_loopreg.hip) below the C ABI: the handle's stream, the
// device rows of its plane clouds, and the score kernel enqueued on pairs that are already on the device.
#pragma once
#include <hip/hip_runtime.h>

struct vxba_loopreg;

namespace vxlr {

struct PairDesc {
  const float* src;
  const float* tar;
  int S, T;
};

hipStream_t stream_of(vxba_loopreg* h);
unsigned long long generation_of(const vxba_loopreg* h);    // counts vxba_loopreg_clear
bool cloud_of(const vxba_loopreg* h, int id, const float** d, int* n);
// associate_kernel<MODE_SCORE> over B pairs whose descriptors, poses (B x 12) and counters (B ints, zeroed by the caller) live on the device; one
// launch on the handle's stream, no synchronisation.  A pair with S == 0 costs nothing.  max_s: the largest S of the batch.
void enqueue_score(vxba_loopreg* h, int B, int max_s, const PairDesc* d_pairs, const double* d_poses, int* d_useful, double normal_thr, double dis_thr);

}  // namespace vxlr
