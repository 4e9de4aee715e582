/* vxba.h -- C ABI of the MI355X-native LiDAR bundle-adjustment factor (libvxba.so).
 *
 * Drop-in boundary for the local-mapping BA hot path of hku-mars/Voxel-SLAM: everything
 * `class LidarFactor` (VoxelSLAM/src/voxel_map.hpp:109-290) does, plus the optimizer shells that
 * own the loop (`Lidar_BA_Optimizer` voxel_map.hpp:293-444, `LI_BA_Optimizer[Gravity]` :446-864 with the
 * `IMU_PRE` factor of preintegration.hpp), plus the batch factor construction of the hierarchical BA
 * (`OctreeGBA`, loop_refine.hpp:273-476), behind plain pointers and sizes.
 * The reference has no FFI; these are the entry points a binding of that class would need
 * (INTEGRATION.md shows the adapter a maintainer would add to voxel_map.hpp).
 *
 * All kernels behind this header are hand-written HIP for gfx950 (CDNA4).  There is NO CPU
 * fallback: every entry point that needs the GPU returns VXBA_ERR_HIP / VXBA_ERR_NODEV if the
 * device or the HIP runtime is unavailable.
 *
 * Packed formats (all f64, caller-owned, host memory unless the name says `_device`):
 *   cluster : 10 f64  [Pxx Pxy Pxz Pyy Pyz Pzz vx vy vz N]        <- PointCluster, tools.hpp:304-365
 *                     (P symmetric; N stored as an exact integer-valued double; N == 0 means
 *                      "frame did not observe this voxel", voxel_map.hpp:178,217,221,258)
 *   pose    : 12 f64  [R column-major (9) | p (3)]                 <- IMUST::R, IMUST::p, tools.hpp:139-140
 *   eig_val :  3 f64  ascending                                     <- LidarFactor::eig_values
 *   eig_vec :  9 f64  column-major, column k = eigenvector k        <- LidarFactor::eig_vectors
 *   Hess    : (6W)x(6W) f64 column-major (Eigen::MatrixXd layout), JacT : 6W f64
 *             per-frame tangent order [dphi(3); dp(3)], R <- R Exp(dphi), p <- p + dp (tools.hpp:154-162)
 */
#ifndef VXBA_H
#define VXBA_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef struct vxba_factor vxba_factor; /* opaque; one per `LidarFactor` instance */

enum {
  VXBA_OK = 0,
  VXBA_ERR_ARG = 1,    /* bad argument (null pointer, range, win_size) */
  VXBA_ERR_HIP = 2,    /* a HIP runtime call failed; see vxba_last_error */
  VXBA_ERR_NODEV = 3,  /* no usable gfx950 device */
  VXBA_ERR_STATE = 4,  /* call not legal in the current state (e.g. empty factor) */
  VXBA_ERR_UNSUPPORTED = 5
};

/* Largest window of the MFMA sweeps and the device-resident LM loop (6W <= 64 columns of the accumulator tile set). */
#define VXBA_MAX_WIN 10
/* Wide windows (VXBA_MAX_WIN < win_size <= VXBA_MAX_WIN_WIDE; the top level of the hierarchical BA optimises ~100 submap poses,
 * voxelslam.cpp:2485-2595): same entry points, sparse-incidence sweeps (pair-major Hessian assembly over an incidence index built
 * once per factor content; deterministic), LM shell on the host.  Not available there: vxba_lm_steps, the LiDAR-inertial shells,
 * mixed precision. */
#define VXBA_MAX_WIN_WIDE 128

/* ---- lifetime -------------------------------------------------------------------------------- */
/* LidarFactor(int _w)                                   voxel_map.hpp:120 */
int vxba_create(int win_size, int device, vxba_factor** out);
int vxba_destroy(vxba_factor* f);
/* LidarFactor::clear()                                  voxel_map.hpp:281-286 */
int vxba_clear(vxba_factor* f);
/* `voxhess.win_size = ...` (voxelslam.cpp:623,1609); only legal on an empty factor */
int vxba_set_win_size(vxba_factor* f, int win_size);
int vxba_win_size(const vxba_factor* f);
/* plvec_voxels.size()                                   voxel_map.hpp:314,344 */
int vxba_size(const vxba_factor* f);
/* Run on a caller-owned hipStream_t instead of the factor's own (non-blocking) stream.  NULL selects the factor's own stream again --
 * so the legacy default stream (handle 0, e.g. torch's default current stream) cannot be chosen: work queued there is NOT ordered with the
 * factor's kernels; share a created stream instead (voxel_slam_amd/dist.py does). */
int vxba_set_stream(vxba_factor* f, void* hip_stream);
int vxba_reserve(vxba_factor* f, int n_voxels);
const char* vxba_last_error(const vxba_factor* f);

/* ---- factor construction --------------------------------------------------------------------- */
/* Batched LidarFactor::push_voxel (voxel_map.hpp:122-130): appends n voxels.
 *   clusters n*W*10 (voxel-major, frames chronological, voxel_map.hpp:1317-1319), fix n*10 (world frame),
 *   coe n (>= 0), eig_val n*3, eig_vec n*9, merged n*10 -- the (lambda, U, pcr_add) cache seeded by the
 *   caller (recut's eigen-decomposition, voxel_map.hpp:1161-1163).  eig_val/eig_vec/merged may be NULL:
 *   the cache is then undefined until vxba_evaluate_only_residual has run. */
int vxba_push_voxels(vxba_factor* f, int n, const double* clusters, const double* fix, const double* coe,
                     const double* eig_val, const double* eig_vec, const double* merged);
/* The same for sparse incidence (the hierarchical BA's top level, loop_refine.hpp:358-405, pushes voxels seen from a handful of
 * ~100 poses): voxel a's observed frames are frame_idx[row_ptr[a] .. row_ptr[a + 1]) (strictly increasing, < win_size), their clusters
 * clusters[e * 10 ..]; unlisted frames are unobserved.  row_ptr has n + 1 entries, row_ptr[0] = 0.  Works for any win_size; the planes
 * are filled on the device, so no dense n x W x 10 array exists on the host or crosses PCIe. */
int vxba_push_voxels_csr(vxba_factor* f, int n, const int64_t* row_ptr, const int32_t* frame_idx, const double* clusters, const double* fix, const double* coe,
                         const double* eig_val, const double* eig_vec, const double* merged);

/* K1 -- per-(voxel, frame) cluster accumulation from raw points, PointCluster::push (tools.hpp:326-331;
 * call sites voxel_map.hpp:988, loop_refine.hpp:383-385).  Appends n_voxels voxels whose body-frame
 * clusters are built on the GPU from points bucketed contiguously per cell:
 *   cell index = frame * n_voxels + voxel;  cell_ptr has W*n_voxels + 1 entries;  xyz_body n_points*3.
 *   fix / coe as in vxba_push_voxels (fix may be NULL = no fix clusters, coe NULL = all ones). */
int vxba_push_points(vxba_factor* f, int n_voxels, int64_t n_points, const double* xyz_body, const int64_t* cell_ptr,
                     const double* fix, const double* coe);

/* Read back the body-frame clusters of voxels [head,end) as n*W*10 (parity checks of K1). */
int vxba_read_clusters(vxba_factor* f, int head, int end, double* clusters);

/* ---- the two sweeps -------------------------------------------------------------------------- */
/* LidarFactor::acc_evaluate2 (voxel_map.hpp:132-241): Hessian / gradient / residual of voxels [head,end)
 * under poses Rp (W*12) using the CACHED (lambda, U, merged) of the last evaluate_only_residual / push.
 * Outputs are overwritten (the reference zeroes them, :134) and the lower block triangle is mirrored (:237-239). */
int vxba_acc_evaluate2(vxba_factor* f, const double* Rp, int head, int end, double* Hess, double* JacT, double* residual);

/* LidarFactor::evaluate_only_residual (voxel_map.hpp:243-279): world merge of the clusters under Rp,
 * 3x3 covariance, symmetric eigen-decomposition; WRITES the (lambda, U, merged) cache of [head,end);
 * residual = sum coe * lambda_0. */
int vxba_evaluate_only_residual(vxba_factor* f, const double* Rp, int head, int end, double* residual);

/* Same sweeps leaving the result in DEVICE memory (for an RCCL all-reduce across voxel shards):
 *   d_out of acc_evaluate2: packed [Hess (6W)^2 col-major | JacT 6W | residual 1] = (6W)^2 + 6W + 1 f64
 *   d_out of evaluate_only_residual: 1 f64.  Asynchronous on the factor's stream. */
int vxba_acc_evaluate2_device(vxba_factor* f, const double* Rp, int head, int end, double* d_out);
int vxba_evaluate_only_residual_device(vxba_factor* f, const double* Rp, int head, int end, double* d_out);
size_t vxba_packed_len(const vxba_factor* f); /* (6W)^2 + 6W + 1 */

/* Public members pcr_adds / eig_values / eig_vectors read by OctoTree::margi (voxel_map.hpp:1211-1222)
 * and motion_init (voxelslam.cpp:651-655).  Any output may be NULL. */
int vxba_read_cache(vxba_factor* f, int head, int end, double* eig_val, double* eig_vec, double* merged);
/* Keep / restore a device-side copy of the cache (a new window re-seeds the cache; used by bench.py). */
int vxba_snapshot_cache(vxba_factor* f);
int vxba_restore_cache(vxba_factor* f);

/* ---- K4: batched plane fit ---------------------------------------------------------------------- */
/* eig(pcr.cov()) for n clusters (OctoTree::recut voxel_map.hpp:1161-1163, margi :1242-1244,
 * OctreeGBA::recut loop_refine.hpp:363-366).  Stand-alone; runs on `device`. */
int vxba_plane_fit(int device, int64_t n, const double* clusters, double* eig_val, double* eig_vec);
/* The same with the reference's plane criteria evaluated on the GPU; flags[a] is a bit set:
 *   1 = enough points       N > min_point                                   (voxel_map.hpp:1155, loop_refine.hpp:360)
 *   2 = plane_judge         lambda0 < min_eigen_value && lambda0/lambda2 < eigen_ratio_thre   (voxel_map.hpp:1015-1019)
 *   4 = factor-worthy       lambda0/lambda1 <= factor_ratio_max (0.12 upstream)   (voxel_map.hpp:1314, loop_refine.hpp:378) */
int vxba_plane_fit_judge(int device, int64_t n, const double* clusters, int min_point, double min_eigen_value, double eigen_ratio_thre,
                         double factor_ratio_max, double* eig_val, double* eig_vec, uint8_t* flags);
/* Stand-alone K1: PointCluster::push over n_cells buckets of points (cell_ptr has n_cells + 1 entries) -> n_cells packed
 * clusters.  Same kernel arithmetic as vxba_push_points (bit-exact with the CPU); use it for world-frame fix clusters
 * (OctoTree::push_fix, voxel_map.hpp:996-1013) or to rebuild clusters from stored points (loop_refine.hpp:382-385). */
int vxba_build_clusters(int device, int64_t n_cells, int64_t n_points, const double* xyz, const int64_t* cell_ptr, double* clusters);

/* ---- the LM shell that owns the loop ------------------------------------------------------------ */
/* Collective hook for voxel-sharded multi-GPU BA: called on the packed device buffer after each sweep's
 * on-device reduction, before the host reads it.  Must sum `count` f64 across ranks in place, stream-ordered
 * on `hip_stream`.  NULL = single GPU. */
typedef int (*vxba_allreduce_fn)(void* ctx, double* d_buf, size_t count, void* hip_stream);
int vxba_set_allreduce(vxba_factor* f, vxba_allreduce_fn fn, void* ctx);
/* Direct RCCL collective (no per-sweep host callback): creates an RCCL communicator for this factor's shard group and
 * all-reduces the exchange buffers with ncclAllReduce on the factor's stream after every sweep.
 *   librccl_path : the librccl.so to dlopen -- pass the one the process already uses (e.g. torch/lib/librccl.so) so that
 *                  there is ONE RCCL instance in the process;
 *   unique_id    : 128 bytes from vxba_rccl_unique_id() on rank 0, distributed out of band (e.g. torch.distributed.broadcast).
 * Collective: every rank of the group must call it.  Takes precedence over vxba_set_allreduce. */
int vxba_rccl_unique_id(const char* librccl_path, void* unique_id_out_128);
int vxba_rccl_attach(vxba_factor* f, const char* librccl_path, int nranks, int rank, const void* unique_id_128);
/* One-shot all-reduce over the peers' mailboxes (point-to-point xGMI reads instead of a ring collective): at W <= 10 the exchange
 * buffer is 29 KB and a ring is pure latency.  Every rank: vxba_peer_export -> 64-byte IPC handle of its mailbox; gather all handles
 * (rank order) by any means; vxba_peer_attach.  From then on the sharded LM loop of vxba_damping_iter / vxba_lm_steps / the LI shells
 * sums its exchange buffer through the mailboxes (fixed rank order: bit-identical results on all ranks); RCCL / the hook stay the
 * fallback when this is not attached.  Needs peer access between the GPUs (one node) and HSA_ENABLE_IPC_MODE_LEGACY=0 in the
 * environment.  vxba_peer_status reports a peer that never arrived (the kernel's bounded wait gave up). */
#define VXBA_PEER_HANDLE_BYTES 64
#define VXBA_PEER_MAX 16
int vxba_peer_export(vxba_factor* f, void* handle_out);
int vxba_peer_attach(vxba_factor* f, int nranks, int rank, const void* handles /* nranks x VXBA_PEER_HANDLE_BYTES */);
int vxba_peer_detach(vxba_factor* f);
int vxba_peer_status(vxba_factor* f, int* status);
/* collective: one all-reduce of a known pattern through the mailboxes; *ok = 1 when every element came back as the exact sum */
int vxba_peer_selftest(vxba_factor* f, int* ok);
/* The id exchange through a caller-supplied broadcast (MPI_Bcast, a socket ...): bcast(ctx, buf, nbytes, root) returns 0 after
 * root's bytes are in every rank's buf.  librccl_path NULL: the RCCL the process already uses, else /opt/rocm/lib/librccl.so. */
typedef int (*vxba_bcast_fn)(void* ctx, void* buf, size_t nbytes, int root);
int vxba_rccl_attach_bcast(vxba_factor* f, const char* librccl_path, int nranks, int rank, vxba_bcast_fn bcast, void* ctx);
int vxba_rccl_detach(vxba_factor* f);

/* Let the caller own the exchange buffers the sweeps reduce into (e.g. a torch tensor, so torch.distributed /
 * RCCL can all-reduce it): d_packed holds vxba_packed_len() f64, d_scalar 1 f64.  NULL restores the internal ones.
 * If d_scalar == d_packed + vxba_packed_len() (one allocation of vxba_packed_len() + 1 doubles; the internal buffers are laid
 * out like that) the device-resident LM loop reduces both with ONE collective per iteration of count vxba_packed_len() + 1
 * (speculative form: the next Hessian sweep runs at the trial poses and is discarded if the step is rejected). */
int vxba_use_external_buffers(vxba_factor* f, double* d_packed, double* d_scalar);

/* One LM trace row: [residual1 residual2 u v q q1 accepted recomputed_hess] */
#define VXBA_TRACE_COLS 8

/* Lidar_BA_Optimizer::damping_iter (voxel_map.hpp:367-442).  Rp (W*12) in/out.  hess_out (6W)^2 col-major =
 * `*hess`, exported BEFORE the gauge fix (:391).  resis_out[2] = residual before / after (:394-395,440).
 * trace_out max_iter*VXBA_TRACE_COLS (may be NULL).  *is_converge as the reference's return value. */
int vxba_damping_iter(vxba_factor* f, double* Rp, int max_iter, double* hess_out, double* resis_out, double* trace_out,
                      int* n_trace, int* is_converge);

/* The same LM shell over caller-supplied sweeps (host-only code, needs no GPU): hess_fn must fill `packed`
 * (vxba_packed_len doubles: Hess col-major | JacT | residual) for poses Rp, resid_fn the residual -- e.g. a local voxel
 * shard's sweep followed by an all-reduce.  Used to drive voxel-sharded BA from torch.distributed and to test the
 * N > 1 logic with gloo on CPUs.  Semantics identical to vxba_damping_iter (voxel_map.hpp:367-442). */
typedef int (*vxba_hess_fn)(void* ctx, const double* Rp, double* packed);
typedef int (*vxba_resid_fn)(void* ctx, const double* Rp, double* residual);
int vxba_damping_iter_generic(int win_size, double* Rp, int max_iter, vxba_hess_fn hess_fn, vxba_resid_fn resid_fn, void* ctx,
                              double* hess_out, double* resis_out, double* trace_out, int* n_trace, int* is_converge);

/* Benchmark driver: exactly n_steps LM iterations of damping_iter WITHOUT the early break; every `steps_per_solve`
 * steps a new solve starts from Rp_init with u = 0.01, v = 2 and the snapshot cache restored (a new window).
 * A rejected step behaves like the reference (no Hessian recompute on the next iteration); stats_out[3] (may be NULL)
 * receives {iterations run, accepted steps, rejected steps}.
 * Rp_out (W*12) receives the final poses. */
int vxba_lm_steps(vxba_factor* f, const double* Rp_init, int n_steps, int steps_per_solve, double* Rp_out,
                  double* last_resis, int64_t* stats_out);

/* ---- batch factor construction: points of a window -> voxel hash -> octree subdivision -> plane test -> factor -------- */
/* OctreeGBA::cut_voxel + subdivide + recut (loop_refine.hpp:273-476), the per-round re-voxelisation of the hierarchical BA
 * (voxelslam.cpp:2374-2379), as sorts and segmented sums on the GPU.  A voxel becomes a factor at the coarsest octree layer
 * where it has more than min_points points (10 upstream), passes plane_judge (lambda0 < min_eigen_value and
 * lambda0/lambda2 < eigen_ratio[layer], the already inverted GBA/eigen_value_array), is seen from >= 2 frames and has
 * lambda0/lambda1 <= factor_ratio_max (0.12); non-planes are subdivided while layer < max_layer (<= 3). */
typedef struct vxba_voxelize_params {
  double voxel_size;
  int max_layer;
  int min_points;
  double min_eigen_value;
  double eigen_ratio[4];
  double factor_ratio_max;
  /* OctoTree's variant of the same construction -- the map build of motion_init (cut_voxel for every scan of the window, then one
   * recut + tras_opt, voxelslam.cpp:606-625; OctoTree::recut voxel_map.hpp:1148-1194, tras_opt :1308-1333): the point-count floor
   * depends on the layer (min_point[layer], voxelslam.cpp:812) and a single observing frame is enough. */
  int min_points_layer[4]; /* > 0: overrides min_points for that layer */
  int min_frames;          /* a factor needs at least this many observing frames: 2 for OctreeGBA (loop_refine.hpp:371-376), 0 for OctoTree */
  /* Voxel-sharded windows (one process per GPU; the reference shards the voxel list over threads, voxel_map.hpp:318-321, and builds per-thread
   * factors in OctreeGBA_multi_recut, loop_refine.hpp:483-537).  shard_count > 1: every rank passes the SAME points and keeps the root voxels
   * that hash to its shard_index -- filtered on the device right after the voxel keys are computed, so the sorts and the octree only see the
   * shard.  Whole root voxels stay together: the union of the ranks' factor voxels is the unsharded set, each voxel bit for bit.  0 / 1: off. */
  int shard_index;
  int shard_count;
} vxba_voxelize_params;
/* xyz_local: n_points x 3 body-frame points, frame by frame in cloud order; frame_ptr: win_size + 1 offsets; Rp: win_size*12.
 * Appends the factor voxels to f (coe = 1, no fix cluster, cache seeded with (lambda, U, world cluster) as recut's push_voxel
 * does) and returns their number in *n_pushed.  node_ids (optional, ids_capacity entries) receives one id per pushed voxel,
 * [x:16 | y:16 | z:16 | octant path:9 | 0:4 | layer:3] with the voxel coordinates offset by 32768, in push order (by layer,
 * ascending id inside a layer).  Voxel coordinates must stay within +-32768. */
int vxba_voxelize_push(vxba_factor* f, int64_t n_points, const double* xyz_local, const int64_t* frame_ptr, const double* Rp,
                       const vxba_voxelize_params* params, int64_t* n_pushed, uint64_t* node_ids, int64_t ids_capacity);
/* The same with the points already in device memory (n_points x 3 f64 on the factor's device; frame_ptr, Rp and params stay host
 * arrays): nothing but a few counters crosses PCIe.  The buffer must stay valid and unchanged until the call returns. */
int vxba_voxelize_push_device(vxba_factor* f, int64_t n_points, const double* d_xyz_local, const int64_t* frame_ptr, const double* Rp,
                              const vxba_voxelize_params* params, int64_t* n_pushed, uint64_t* node_ids, int64_t ids_capacity);

/* ---- inertial half of the LiDAR-inertial BA (host code; runs while the GPU sweeps) ------------------- */
/* Flat formats, every matrix column-major:
 *   state (VXBA_STATE_LEN f64) = the IMUST fields the BA touches (tools.hpp:135-199): [R 9 | p 3 | v 3 | bg 3 | ba 3 | g 3]
 *   imu   (VXBA_IMU_LEN f64)   = IMU_PRE (preintegration.hpp:11-30): [R_delta 9 | p_delta 3 | v_delta 3 | bg 3 | ba 3 |
 *       R_bg 9 | p_bg 9 | p_ba 9 | v_bg 9 | v_ba 9 | dtime | dbg 3 | dba 3 | dbg_buf 3 | dba_buf 3 | cov 15x15]
 * Tangent order per frame: [dphi dp dv dbg dba] (15), LiDAR block = the first 6. */
#define VXBA_STATE_LEN 24
#define VXBA_IMU_LEN 304
#define VXBA_LI_DIM 15

/* IMU_PRE::IMU_PRE(bg, ba) (preintegration.hpp:32-48); bg / ba may be NULL (zero). */
int vxba_imu_init(double* imu, const double* bg, const double* ba);
/* IMU_PRE::add_imu (preintegration.hpp:75-135): one mid-point, bias-corrected sample (what push_imu :50-73 feeds it).
 * noise_meas / noise_walk: the reference's 6x6 `noiseMeas` / `noiseWalk` (preintegration.hpp:9, voxelslam.cpp:828-833). */
int vxba_imu_add(double* imu, const double* gyr, const double* acc, double dt, const double* noise_meas, const double* noise_walk);
/* IMU_PRE::give_evaluate (preintegration.hpp:137-212): *residual = r^T cov^-1 r; with jac_enable also jtj (30x30) and gg (30). */
int vxba_imu_evaluate(const double* imu, const double* st1, const double* st2, int jac_enable, double* jtj, double* gg, double* residual);
/* IMU_PRE::give_evaluate_g (preintegration.hpp:214-294): as above with three more Jacobian columns for the gravity
 * vector -- jtj 33x33, gg 33. */
int vxba_imu_evaluate_g(const double* imu, const double* st1, const double* st2, int jac_enable, double* jtj, double* gg, double* residual);
/* IMU_PRE::update_state (preintegration.hpp:296-303). */
int vxba_imu_update_state(double* imu, const double* dxi15);
/* LI_BA_Optimizer::hess_plus (voxel_map.hpp:455-463): scatter-add the (6W) LiDAR system into the (15W) one. */
int vxba_hess_plus(int win_size, double* Hess15, double* JacT15, const double* Hess6, const double* JacT6);

/* LI_BA_Optimizer::divide_thread (voxel_map.hpp:465-523): Hess (15W)^2 col-major and JacT (15W) of the joint system
 * (imu_coef * IMU blocks + scattered LiDAR blocks), *residual = imu_coef/2 * sum r^T cov^-1 r + LiDAR residual.
 * states W*VXBA_STATE_LEN, imus (W-1)*VXBA_IMU_LEN.  The Hessian sweep runs on the GPU, the IMU blocks on the host
 * meanwhile. */
int vxba_li_evaluate(vxba_factor* f, const double* states, const double* imus, double imu_coef, double* Hess, double* JacT,
                     double* residual);
/* LI_BA_Optimizer::only_residual (voxel_map.hpp:525-560). */
int vxba_li_only_residual(vxba_factor* f, const double* states, const double* imus, double imu_coef, double* residual);
/* LI_BA_OptimizerGravity's members of the same names (voxel_map.hpp:663-773): hess_plus into a (15W+3)^2 system, divide_thread (Hess (15W+3)^2
 * column-major, JacT 15W+3: the three gravity unknowns at the tail, IMU factors through give_evaluate_g); only_residual is vxba_li_only_residual
 * (give_evaluate_g without Jacobian is give_evaluate without Jacobian, preintegration.hpp:214-294). */
int vxba_hess_plus_gravity(int win_size, double* Hess15g, double* JacT15g, const double* Hess6, const double* JacT6);
int vxba_li_evaluate_gravity(vxba_factor* f, const double* states, const double* imus, double imu_coef, double* Hess, double* JacT, double* residual);
/* LI_BA_Optimizer::damping_iter (voxel_map.hpp:562-653; three iterations upstream).  states and imus are in/out (the
 * factors' dbg / dba and their _buf copies move with every step and roll back on a rejected one, :608-609, 639-643).
 * hess_out (15W)^2 = `*hess`, exported before the gauge fix (:588).  trace_out max_iter*VXBA_TRACE_COLS, may be NULL. */
int vxba_li_damping_iter(vxba_factor* f, double* states, double* imus, double imu_coef, int max_iter, double* hess_out,
                         double* trace_out, int* n_trace);

/* LI_BA_OptimizerGravity::damping_iter (voxel_map.hpp:775-862; max_iter = 5 at its call site voxelslam.cpp:1644): the
 * gravity vector (states[21..23] of every frame, kept equal) joins the unknowns at the tail of the system; hess_out is
 * (15W+3)^2; only frame 0's pose is gauge-fixed.  resis_out[2] = residual before / after. */
int vxba_li_damping_iter_gravity(vxba_factor* f, double* states, double* imus, double imu_coef, int max_iter, double* hess_out,
                                 double* resis_out, double* trace_out, int* n_trace);

/* ---- the incremental local map, resident on the GPU -------------------------------------------------------
 * `surf_map` / `surf_map_slide` of OctoTree nodes with their sliding windows (voxel_map.hpp:896-1639), driven the way the
 * local-mapping thread drives them (voxelslam.cpp:1592-1700).  Each entry point replaces one call of that thread; the tree, the
 * window clusters, the stored scan points, the fix clusters and the plane records never leave the device, and tras_opt writes the
 * factor's planes in place -- a scan cycle moves the scan up and the poses down.  Parameters are the reference's globals
 * (voxel_map.hpp:83-89, voxelslam.cpp:795-812). */
typedef struct vxba_map vxba_map;
typedef struct vxba_lio vxba_lio;   /* the odometry handle, declared below */
typedef struct vxba_map_params {
  double voxel_size;                 /* voxel_size */
  int max_layer;                     /* max_layer (0..2) */
  double min_point[4];               /* min_point[layer]: a leaf is tested for planarity when N > min_point[layer] */
  double min_eigen_value;            /* plane_judge: lambda0 < min_eigen_value && lambda0 / lambda2 < plane_eigen_value_thre[layer] */
  double plane_eigen_value_thre[4];
  int max_points;                    /* fix cluster cap (voxel_map.hpp:86) */
  int win_size;                      /* <= 16 */
  int thread_num;                    /* only for upstream's `if(g_size < thd_num) return;` early returns (voxel_map.hpp:1603, voxelslam.cpp:1406, 1337) */
} vxba_map_params;
int vxba_map_create(const vxba_map_params* params, int device, vxba_map** out);
int vxba_map_destroy(vxba_map* m);
const char* vxba_map_last_error(const vxba_map* m);
/* cut_voxel_multi(surf_map, pvec, ord, surf_map_slide, win_size, pwld, sws) (voxel_map.hpp:1545-1639, call site voxelslam.cpp:1609):
 * scan `ord` of the window (= win_count - 1): n body-frame points (n x 3), their covariances as pvec_update left them (n x 9
 * column-major), their world coordinates (n x 3).  The _device variant takes device pointers (e.g. the arrays vxba_lio_pvec_update
 * keeps resident). */
int vxba_map_cut_voxel(vxba_map* m, int ord, int64_t n, const double* pnt_body, const double* var_world, const double* pwld);
int vxba_map_cut_voxel_device(vxba_map* m, int ord, int64_t n, const double* d_pnt_body, const double* d_var_world, const double* d_pwld);
/* The same on the scan resident in an odometry handle after vxba_lio_pvec_update (body points, world points and world covariances
 * are taken from the device: nothing crosses PCIe). */
int vxba_map_cut_voxel_lio(vxba_map* m, int ord, vxba_lio* lio);
/* cut_voxel(surf_map, pvec, win_size, jour) (voxel_map.hpp:1641-1671 -> OctoTree::allocate_fix :1048-1072 -> push_fix_novar :1007-1013), the form
 * keyframe_loading (voxelslam.cpp:1189-1228, call site :1608) and loop closing (:1167, :2149) use: n world-frame points (n x 3) enter the map as FIXED
 * points.  var: their n x 9 column-major variances, or NULL = all zero (what keyframe_loading stores, :1210); it is only stored, for the fix_divide of
 * a later split.  A root voxel this call creates is stamped with `jour` (what vxba_map_release ages it by), has no window and is not in the slide map;
 * an existing root is not re-stamped.  pcr_fix / pcr_add continue their running sums in input order (bit-identical to sequential push()), cov_add is
 * not touched, max_points does not cap the stored points (only vxba_map_margi caps).  The _device variant takes device pointers. */
int vxba_map_cut_voxel_fix(vxba_map* m, int64_t n, const double* pnt_world, const double* var, double jour);
int vxba_map_cut_voxel_fix_device(vxba_map* m, int64_t n, const double* d_pnt_world, const double* d_var, double jour);
/* The teardown of loop_update (voxelslam.cpp:1105-1112) / system_reset: no roots, no nodes, empty slide map, empty fix-point pool, empty voxel table,
 * ring back to mp[i] = i, resident scans forgotten.  Allocations are kept; the handle behaves like a new one. */
int vxba_map_clear(vxba_map* m);
/* New plane thresholds (min_eigen_value, plane_eigen_value_thre[4] of vxba_map_params) for a map that holds nothing: the switch between the two phases of
 * Initialization::motion_init, whose every round rebuilds the map from nothing.  VXBA_ERR_STATE on a map that is not empty (vxba_map_clear first). */
int vxba_map_set_plane_thresholds(vxba_map* m, double min_eigen_value, const double plane_eigen_value_thre[4]);
/* The map's part of loop_update (voxelslam.cpp:1101-1186) in one call: vxba_map_clear -> vxba_map_cut_voxel_fix(.., jour) of n_clouds world-frame
 * clouds in the order given (cloud c = points cloud_ptr[c] .. cloud_ptr[c + 1] of pnt_world / var, var may be NULL: map_loop's keyframes, then the
 * buffered scans of :1161-1168; jour is 0 upstream) -> for i < win_count the single-thread cut_voxel (voxel_map.hpp:1504-1540; no
 * `if(g_size < thd_num) return;`) of window scan i under the corrected pose Rp[i], world points computed on the device -> recut of EVERY root
 * (:1179-1180; no early return, no tras_opt: the next vxba_map_recut fills the factor).  The window's scans: scan_ptr == NULL re-cuts the scans the ring
 * slots already hold where they lie (slot i after the ring reset is the old slot mp[i]; nothing crosses PCIe); otherwise scan i = points scan_ptr[i] ..
 * scan_ptr[i + 1] of pnt_body (x 3) / var_world (x 9 column-major), host arrays.  lio (may be NULL): the odometry handle whose plane map mirrors this
 * map is cleared too, so that the next vxba_map_export_planes rebuilds what `match` walks.  Velocity, gravity, x_curr and the path stay with the caller. */
int vxba_map_loop_update(vxba_map* m, int n_clouds, const int64_t* cloud_ptr, const double* pnt_world, const double* var, double jour, int win_count, const double* Rp,
                         const int64_t* scan_ptr, const double* pnt_body, const double* var_world, vxba_lio* lio);
/* vxba_map_loop_update in its scan_ptr == NULL form (the window's scans are re-cut where the ring slots hold them) with the clouds read from DEVICE memory:
 * d_pnt_world cloud_ptr[n_clouds] x 3 and d_var x 9 column-major (may be NULL: zeros) as vxba_kfarchive_map_loop hands them out, cloud_ptr on the host.
 * Only read during the call.  The result is byte-identical to the host route on the same numbers; the refusals are the same and leave the map as it was. */
int vxba_map_loop_update_device(vxba_map* m, int n_clouds, const int64_t* cloud_ptr, const double* d_pnt_world, const double* d_var, double jour, int win_count, const double* Rp,
                                vxba_lio* lio);
/* The resident scan of window position i (ring slot mp[i]) in device memory: *n points, body points n x 3 float64, `var` n x 9 float64 column-major as
 * pvec_update left them -- what vxba_keyframe_push_scan_device takes, so that ScanPose(x_buf[0], pvec_buf[0]) (voxelslam.cpp:1656) after vxba_map_margi and
 * before the slot is reused moves device to device.  Read-only; valid until the next call that writes that slot: vxba_map_cut_voxel* into it,
 * vxba_map_loop_update*, vxba_map_clear.  Every call that writes a slot has waited for the device before it returned, so the arrays are complete and this
 * accessor does not wait.  VXBA_ERR_STATE: the slot holds no scan (never cut, cut with n = 0, or forgotten by a clear). */
int vxba_map_scan_device(vxba_map* m, int i, int64_t* n, const double** d_pnt_body, const double** d_var_world);
/* multi_recut (voxelslam.cpp:1396-1453, OctoTree::recut voxel_map.hpp:1148-1194) followed by tras_opt (:1308-1333) straight into
 * `factor` (cleared by the caller, as voxhess.clear(); same win_size).  Rp: win_count poses.  Factor voxels are ordered by node id;
 * *n_pushed (optional) receives their number. */
int vxba_map_recut(vxba_map* m, int win_count, const double* Rp, vxba_factor* factor, int64_t* n_pushed);
/* multi_margi (voxelslam.cpp:1321-1394, OctoTree::margi voxel_map.hpp:1196-1305, mgsize = 1) with the optimised poses; reads the
 * cache the optimiser left in `factor` (pcr_adds / eig_values / eig_vectors) on the device. */
int vxba_map_margi(vxba_map* m, int win_count, const double* Rp, vxba_factor* factor);
/* Brings the odometry's plane map (vxba_lio, what `match` walks, voxel_map.hpp:1335-1392) up to date with the tree, on the device: the
 * plane records of every leaf -- and "no plane" for the empty octants of subdivided nodes -- under all roots that were in the slide map
 * since the last export.  Same voxel_size / max_layer / device.  Call after recut / margi, before the next scan is matched. */
int vxba_map_export_planes(vxba_map* m, vxba_lio* lio, int64_t* n_exported);
/* The ring of window slots moves on by mgsize (voxelslam.cpp:1683-1687). */
int vxba_map_slide(vxba_map* m, int mgsize);
/* out = [roots, roots in the slide map, leaves, mp[0]] */
int vxba_map_counts(vxba_map* m, int64_t out[4]);
/* The pool that holds the marginalised (fix) points of all leaves: out = [cursor, capacity, compactions so far], in points (96 bytes each).
 * The pool is a bump allocator -- a leaf that outgrows its region gets a new one, the old one is abandoned -- that is COMPACTED (live regions
 * moved to the front of a fresh pool, inside vxba_map_recut / vxba_map_margi) whenever the cursor passes max(4M points, 3 x what was live at
 * the last compaction), so a long mapping session holds a bounded multiple of its live points (the reference frees point_fix vectors instead). */
int vxba_map_fix_pool(vxba_map* m, int64_t out[3]);
/* The caller's journey odometer (`jour += spat`, voxelslam.cpp:1677).  The next vxba_map_margi stamps it on every root voxel of the slide
 * map, as multi_margi does (`iter->second->jour = jour`, voxelslam.cpp:1349). */
int vxba_map_set_journey(vxba_map* m, double jour);
/* The release branch of the local-mapping loop (voxelslam.cpp:1503-1523; OctoTree::tras_ptr voxel_map.hpp:1394-1405): every root voxel with
 * int(jour_now - root.jour) >= min_age (700 upstream) leaves the map with its whole subtree.  The node pool is compacted (survivors keep their
 * relative order, so id-ordered steps see the order they would have seen), child / root references and the voxel table are rebuilt, the
 * fix-point pool is compacted behind it, and the arrays are re-sized to what is left: device memory follows the map down.  Roots that are in
 * the slide map are kept whatever their stamp (upstream would delete them under the window's feet).  lio (may be NULL): the odometry handle
 * whose plane map mirrors this map -- the released roots are cleared there too.  Outputs may be NULL. */
int vxba_map_release(vxba_map* m, double jour_now, int min_age, vxba_lio* lio, int64_t* n_roots_released, int64_t* n_nodes_released);
/* Device memory held by the map, bytes: [0] node pool, [1] fix-point pool, [2] resident scans of the window, [3] voxel table + scratch, [4] total. */
int vxba_map_device_bytes(vxba_map* m, int64_t out[5]);
/* Every leaf (octo_state == 0), unordered.  ids: [x:16 | y:16 | z:16 | octant path:9 | 0:4 | layer:3] (as vxba_voxelize_push);
 * ints n x 8 = [layer, isexist, is_plane, has window, opt_state, last_num, stored fix points, root in slide map]; dbl n x (156 + 11 W) =
 * [pcr_add 10 | pcr_fix 10 | eig_value 3 | eig_vector 9 | plane centre 3 | normal 3 | radius | plane_var 36 | cov_add 81 | window
 * clusters W x 10 in window order | stored points per window slot W], matrices column-major.  *n_out = number of leaves (fills up to
 * `capacity`; pass NULL arrays to query the count). */
int vxba_map_leaves(vxba_map* m, int64_t capacity, uint64_t* ids, int32_t* ints, double* dbl, int64_t* n_out);
/* The points the leaf with id `node_id` (as vxba_map_leaves reports it) keeps for a later subdivision; read-only.  which = -1: its fix points (world
 * frame) in the order of its region of the fix pool; which = i in [0, win_size): the points of the window's i-th scan (body frame) in the order of the
 * leaf's range of that scan's permutation (none when the leaf has no window).  out: up to `capacity` rows of 12 = [x y z | variance 3x3 column-major];
 * *n_out = the number the leaf holds, also when it exceeds capacity.  VXBA_ERR_ARG when no leaf has that id. */
int vxba_map_leaf_points(vxba_map* m, uint64_t node_id, int which, int64_t capacity, double* out, int64_t* n_out);

/* ---- execution options (per handle; none of them changes results beyond rounding) -----------------------------------------
 * Every switch that used to be an environment variable is a setter.  The environment variables of the same name
 * (VXBA_FUSED_SOLVE, VXBA_SPEC_COLLECTIVE, VXBA_WIDE_DEVICE_SOLVE, VXBA_K2_VPB, VXBA_LIO_DEVICE_EKF) still give the
 * INITIAL value of a new handle -- for A/B scripts -- and nothing reads them after vxba_create / vxba_lio_create. */
#define VXBA_OPT_FUSED_SOLVE 0        /* 1 (default): the 6W damped solve runs as workgroup 0 of the residual-sweep launch; 0: own launch */
#define VXBA_OPT_SPEC_COLLECTIVE 1    /* 1 (default): sharded LM loop with ONE all-reduce per iteration (speculative Hessian sweep at the trial poses) */
#define VXBA_OPT_WIDE_DEVICE_SOLVE 2  /* 1 (default): the damped step of a wide window (W > 10) by the library's blocked Cholesky on the device (host pivoted
                                         LDL^T when a pivot is not positive); 0: always the host LDL^T */
#define VXBA_OPT_LI_DEVICE_LOOP 3     /* reserved: the device-resident 15W loop of rounds 1-3 (IMU factor kernels + a one-wave block-Thomas solve, ~265 us per
                                         iteration against ~66 for the default shell) was removed in round 4; only 0 is accepted */
#define VXBA_OPT_K2_VOXELS_PER_BLOCK 4 /* 64 (default) or 32..63: voxels per residual-sweep workgroup (tuning experiment) */
#define VXBA_OPT_DEBUG_SOLVE_TIMEOUT 5 /* test hook, 0 (default): with 1 the voxel workgroups of a fused launch give up waiting for the in-launch solve at
                                         once, which exercises the transparent non-fused retry of vxba_damping_iter; with 2 vxba_li_damping_iter treats the
                                         first in-launch pose step of a call as undelivered, which exercises its host-solve fallback */
#define VXBA_OPT_LI_STRUCTURED_SOLVE 6 /* 1 (default): the host shells of LI_BA_Optimizer[Gravity] solve the damped 15W(+3) system by a band Cholesky of
                                         the velocity/bias part + Schur complement onto the poses (3x fewer flops); 0: dense pivoted LDL^T */
#define VXBA_OPT_LI_QUEUED_SWEEPS 7    /* 1 (default): the host shells of LI_BA_Optimizer[Gravity] queue an iteration's residual sweep (and the speculative Hessian sweep
                                       * behind it) BEFORE the host has finished the damped solve; the sweep's first workgroup waits for the trial poses in mapped host
                                       * memory while the others already hold their cluster rows.  0: every sweep is launched when its poses exist. */
#define VXBA_OPT_LI_DEVICE_POSE_SOLVE 8 /* 1 (default): LI_BA_Optimizer's host shell (queued sweeps, structured solve) eliminates velocities and biases on the host WHILE
                                       * the Hessian sweep runs and lets the device solve the reduced 6W-dimensional pose system inside the residual-sweep launch
                                       * (the LiDAR-only loop's four-wave solve): no kernel ever waits for the host, the LiDAR Hessian never crosses PCIe on the
                                       * critical path.  Steps after a rejection, the gravity variant and a non-positive band pivot take the host solve.  0: host solve. */
#define VXBA_OPT_FUSED_SWEEPS 9         /* 1 (default): inside one solve of the device-resident 6W loop (vxba_damping_iter, vxba_lm_steps; no collective attached)
                                       * the residual sweep at the trial poses and the Hessian sweep that linearises at the same poses one iteration later are
                                       * ONE launch behind the in-launch solve (Lidar_BA_Optimizer::damping_iter, voxel_map.hpp:386-439: only_residual, then
                                       * divide_thread of the next iteration), and the reduction behind it takes the accept / reject decision; a rejected step
                                       * then costs a Hessian sweep the reference does not run -- so a factor whose LAST call rejected more than a third of its steps runs its next
                                       * call as the three-launch iteration (break-even by the round-6 kernel times: 18 % rejected steps at 50k voxels, 32 % at 400k; results do not depend on the form).
                                       * 2: fused whatever the history -- and ALSO on a factor with a collective attached (one process per GPU only: the launch takes whole CUs and waits inside
                                       * itself, which two process ranks sharing one device do not survive; worth 7-9 % of a step from ~100k voxels per rank, nothing at 50k).  0: the three-launch iteration of rounds 1-5.  Needs
                                       * VXBA_OPT_FUSED_SOLVE = 1.  (The number belonged to a round-4 experiment that was removed in round 5.) */
#define VXBA_OPT_COUNT 10
#define VXBA_STAT_FUSED_FALLBACKS 100 /* read-only (vxba_get_option): times vxba_damping_iter re-ran a call with the solve as its own launch after the
                                         voxel workgroups of a fused launch had timed out waiting for it */
#define VXBA_STAT_LI_LAST_CALL_US 101 /* read-only (vxba_get_option): wall time of the last vxba_li_damping_iter[_gravity] call, microseconds,
                                         * measured inside the library (what a C caller sees; the Python mirror adds its array handling) */
#define VXBA_STAT_LI_DEVICE_FALLBACKS 102 /* read-only (vxba_get_option): times vxba_li_damping_iter found the in-launch pose step non-finite / undelivered when its
                                         * launch had ended, discarded that launch's residual sweep and took the host solve (the reference's pivoted LDL^T) instead */
#define VXBA_STAT_REJECT_HEAVY 103     /* read-only (vxba_get_option): 1 when the factor's last device-resident LM call rejected more than a third of its steps
                                       * (VXBA_OPT_FUSED_SWEEPS = 1 then runs the next call as the three-launch iteration) */
int vxba_set_option(vxba_factor* f, int option, int value);
int vxba_get_option(const vxba_factor* f, int option, int* value);

/* Arithmetic of the Hessian sweep (BASELINE.json configs[2], the mixed-precision tolerance study).  F64 (default): fp64
 * throughout, like the reference.  MIXED: the rank-3 rows of every voxel ("Jacobian") are rounded to f32 and multiplied on the
 * f32 matrix cores, summed in f32 inside one wave (<= 72 voxels) and accumulated in f64 across waves, workgroups and GPUs;
 * gradient, block-diagonal terms, residuals, eigen-decompositions and the solve stay fp64.  The gradient is exact, so the LM
 * fixed point is unchanged; only the step direction carries ~1e-7 relative error. */
#define VXBA_PRECISION_F64 0
#define VXBA_PRECISION_MIXED 1
/* MIXED, and the residual sweep reads the clusters from an f32 copy ("clusters also emitted as f32", configs[2]): per (voxel, frame)
 * [C sym6 | c | n] with c the cluster's mean and C its second moments ABOUT that mean -- raw body-frame moments do not survive f32, the
 * re-centred ones do (round-off ~1e-7 m^2 against a plane thickness of ~1e-2 m^2).  Half the bytes of that sweep's dominant stream.
 * The copy is kept beside the f64 rows (the Hessian sweep and every read-back use those) and refreshed when voxels were appended.
 * Eigenvalues / residuals move by ~1e-6 relative, and with them the LM fixed point by tens of nanometres (measured; the per-row errors average out). */
#define VXBA_PRECISION_MIXED_F32_CLUSTERS 2
int vxba_set_precision(vxba_factor* f, int mode);

/* ---- odometry: point-to-plane state estimation against the voxel plane map ---------------- */
/* Replaces `lio_state_estimation` (voxelslam.cpp:855-958): per EKF iteration every scan point is transformed with the
 * current pose, matched to the plane of the octree leaf it falls into (`match`, voxel_map.hpp:1335-1392, 1674-1698) and
 * the matched points' information is summed into HTH (6x6), HTz (6) and nnt (3x3).  The map walk (float-typed voxel index,
 * `wld > voxel_center` descent, float-typed distance tests, the per-point node cache `octos[i]` + `inside` :1471-1480) is
 * reproduced exactly, on a flattened map held in GPU memory.  The 15-dimensional EKF algebra between the sweeps runs on
 * the host.  No CPU fallback.
 *   state : VXBA_STATE_LEN f64 as above [R 9 col-major | p 3 | v 3 | bg 3 | ba 3 | g 3]      <- IMUST, tools.hpp:135-199
 *   cov   : 15x15 f64 col-major, tangent order [dphi dp dv dbg dba]                          <- IMUST::cov
 *   sweep : VXBA_LIO_SWEEP_LEN f64 = [HTH 36 col-major | HTz 6 | nnt 9 col-major | match_num] */
typedef struct vxba_lio vxba_lio; /* opaque: one plane map (`surf_map`) + the current scan (`pptr`) */
#define VXBA_LIO_SWEEP_LEN 52
#define VXBA_LIO_MAX_ITER 4 /* num_max_iter, voxelslam.cpp:859 */

/* voxel_size / max_layer: the reference's globals (voxel_map.hpp:86-88; max_layer <= 3 here). */
int vxba_lio_create(double voxel_size, int max_layer, int device, vxba_lio** out);
/* VXBA_LIO_OPT_DEVICE_EKF: 1 (default) = the 15x15 EKF update between sweeps runs as a kernel, whole state estimation enqueued
 * up front; 0 = the algebra on the host between sweeps. */
#define VXBA_LIO_OPT_DEVICE_EKF 0
int vxba_lio_set_option(vxba_lio* h, int option, int value);
int vxba_lio_destroy(vxba_lio* h);
const char* vxba_lio_last_error(const vxba_lio* h);

/* The plane map, flattened: one entry per octree leaf (OctoTree with octo_state == 0) that the walk can reach.
 *   loc n*3       root voxel, the VOXEL_LOC key of `surf_map` (tools.hpp:24-35); |index| < 2^20
 *   layer n       depth of the leaf, 0 = the root voxel itself
 *   path n        `leafnum` taken at each level on the way down (voxel_map.hpp:1371), 3 bits per level, first level lowest
 *   is_plane n    Plane::is_plane; 0 removes the leaf's plane (NULL = all ones)
 *   center, normal n*3, plane_var n*36 col-major, radius n  <- struct Plane (voxel_map.hpp:66-80; radius is a float there)
 * Upsert: a leaf seen before has its plane replaced.  When the host tree splits a leaf, remove it (is_plane = 0) in an
 * earlier call than the one that adds its children.  Plane records are reclaimed by vxba_lio_map_clear only. */
int vxba_lio_map_update(vxba_lio* h, int64_t n, const int64_t* loc, const int32_t* layer, const int32_t* path, const int32_t* is_plane,
                        const double* center, const double* normal, const double* plane_var, const double* radius);
int vxba_lio_map_clear(vxba_lio* h);
int vxba_lio_map_size(const vxba_lio* h, int64_t* n_roots, int64_t* n_planes);

/* The scan.  _raw = var_init (voxelslam.hpp:187-201): sensor-frame float points -> calcBodyVar (:164-185; dept_err / beam_err are
 * narrowed to float as there) -> extrinsic ext = [R 9 col-major | p 3] (NULL = identity).  _set takes ready pointVar arrays
 * (pnt n*3, var n*9 col-major; voxel_map.hpp:14-19).  _read returns what the sweeps use. */
int vxba_lio_scan_raw(vxba_lio* h, int64_t n, const float* xyz, const double* ext, double dept_err, double beam_err);
/* _raw for a cloud that lies in device memory on the handle's device (vxba_imuekf_filtered_device): a device-to-device copy on this handle's stream.
 * Behind a producer of this library it is ordered through the producer's event, not through a host wait; any other producer must have finished. */
int vxba_lio_scan_raw_device(vxba_lio* h, int64_t n, const float* d_xyz, const double* ext, double dept_err, double beam_err);
int vxba_lio_scan_set(vxba_lio* h, int64_t n, const double* pnt, const double* var);
int64_t vxba_lio_scan_size(const vxba_lio* h);
int vxba_lio_scan_read(vxba_lio* h, double* pnt, double* var);

/* One pass of the loop body voxelslam.cpp:873-919 under (state, cov).  reset_cache != 0 forgets the per-point node cache first
 * (the reference starts every lio_state_estimation call with an empty one).  plane_of_point (index of the matched leaf's plane
 * record = order of first insertion, -1 = no match) and sigma_of_point may both be NULL. */
int vxba_lio_sweep(vxba_lio* h, const double* state, const double* cov, int reset_cache, double* sweep, int32_t* plane_of_point,
                   double* sigma_of_point);
/* lio_state_estimation: state and cov in/out (x_curr).  info[4] = [ok (nnt's smallest eigenvalue >= 14, :951-957), iterations,
 * match_num of the last sweep, that eigenvalue]; sweeps_out VXBA_LIO_MAX_ITER * VXBA_LIO_SWEEP_LEN.  Both may be NULL. */
int vxba_lio_state_estimation(vxba_lio* h, double* state, double* cov, double* info, double* sweeps_out);
/* pvec_update (voxelslam.hpp:203-215): world points (n*3) and world covariances (n*9 col-major) of the scan under (state, cov).
 * Both also stay on the device for vxba_lio_leaf_stats until the scan is replaced; var may be NULL (not downloaded: the host tree
 * needs the world points to bucket them into leaves, the 72 bytes of covariance per point only feed cov_add). */
int vxba_lio_pvec_update(vxba_lio* h, const double* state, const double* cov, double* pwld, double* var);
/* What cut_voxel adds to the leaves this scan touches (OctoTree::push, voxel_map.hpp:969-993: pcr_add.push(pw), cov_add += Bf_var),
 * from the resident result of the last vxba_lio_pvec_update.  The host tree's bucketing comes in as indices: leaf c owns the scan
 * points order[cell_ptr[c] .. cell_ptr[c+1]) in push order.  Out: clusters n_cells x 10 (the PointCluster of the new points,
 * bit-identical to sequential push) and cov_add n_cells x 81 col-major -- increments the caller adds to its nodes.
 * VXBA_ERR_STATE without a preceding pvec_update of the current scan. */
int vxba_lio_leaf_stats(vxba_lio* h, int64_t n_cells, const int64_t* cell_ptr, const int32_t* order, double* clusters, double* cov_add);

/* The map-side producers of those plane records (f2's arithmetic; the host tree decides which leaves exist):
 * cov_add of OctoTree::push (voxel_map.hpp:990-992) = sum over a cell's points of Bf_var (:91-106), n_cells x 81 col-major 9x9, from
 * world points (n*3), their world covariances (n*9 col-major, e.g. vxba_lio_pvec_update's) and bucket offsets (n_cells + 1);
 * OctoTree::plane_update (:1118-1146) batched: world cluster (10), its eigen-decomposition (vxba_plane_fit) and cov_add ->
 * center / normal n*3, plane_var n*36 col-major, radius n (rounded to float as upstream). */
int vxba_cov_add_build(int device, int64_t n_cells, int64_t n_points, const double* xyz_world, const double* var, const int64_t* cell_ptr, double* cov_add);
int vxba_plane_update(int device, int64_t n, const double* clusters, const double* eig_val, const double* eig_vec, const double* cov_add, double* center,
                      double* normal, double* plane_var, double* radius);

/* down_sampling_voxel (tools.hpp:201-238): the voxel-grid filter upstream runs on every raw scan before the odometry
 * (voxelslam.cpp:1236, 1577-1583) and on every merged submap of the hierarchical BA (:2447).  One point per occupied voxel = the
 * running mean of its points in cloud order, in float and unfused like upstream (bit-identical means); voxel index = upstream's
 * float quotient / "-1 if negative" / truncation, |index| < 2^20.  xyz n*3 float, out_xyz capacity n*3; output ordered by ascending
 * (x, y, z) voxel index (upstream: unordered_map iteration order).  voxel_size < 0.001 copies the cloud through, like upstream. */
int vxba_down_sampling_voxel(int device, int64_t n, const float* xyz, double voxel_size, float* out_xyz, int64_t* n_out);
/* down_sampling_close (tools.hpp:240-302), the filter of the raw copy initialization() keeps for motion_init: one point per occupied voxel = the voxel's point
 * nearest the voxel's mean (float sum in cloud order / count; double squared distances; the first of equals; nothing beyond a squared distance of 100).
 * sel_out (capacity n): the index into xyz of every output point, so the caller can carry its time along.  Same voxel index and output order as above. */
int vxba_down_sampling_close(int device, int64_t n, const float* xyz, double voxel_size, float* out_xyz, int32_t* sel_out, int64_t* n_out);

/* ---- initialisation: scan-to-cloud odometry ---------------------------------------------------------------------------------
 * Replaces `lio_state_estimation_kdtree` (voxelslam.cpp:960-1098), the odometry of the first win_size scans, when no plane map exists yet:
 * each scan is aligned against a growing world point cloud (`pl_tree`, float xyz, device resident here) -- five nearest neighbours per
 * point, a plane through them, the iterated EKF of the regular odometry with K_1 = (H_T_H + cov^-1 / 1000)^-1 -- and then appended; the
 * cloud is voxel-filtered at 0.5 (vxba_down_sampling_voxel: ascending voxel index).
 * The search is exact brute force in float32: squared distance ((dx dx + dy dy) + dz dz) without contraction, candidates ordered by
 * (distance, index) ascending, so equal distances go to the lower index.  The plane is the least-squares solution of A x = -1 (A = the five
 * points in that order, widened to f64) by column-pivoted Householder QR; a point is rejected if any |x . A_i + 1| > 0.1.  Five collinear or
 * coincident points (rank-deficient A): pivots <= 3 * 2^-52 * the first pivot end the factorisation and the remaining components of x are
 * zero -- finite and deterministic, but outside what is pinned to the reference.  No CPU fallback. */
typedef struct vxba_initodom vxba_initodom; /* opaque: the world cloud (`pl_tree`) + the current scan */
#define VXBA_INITODOM_NMATCH 5
#define VXBA_INITODOM_INFO_LEN 8
int vxba_initodom_create(int device, vxba_initodom** out);
int vxba_initodom_destroy(vxba_initodom* h);
const char* vxba_initodom_last_error(const vxba_initodom* h);
/* `pl_tree->clear()` of system_reset */
int vxba_initodom_clear(vxba_initodom* h);
/* The resident cloud: size, and read-back into xyz (size x 3 float). */
int64_t vxba_initodom_cloud_size(const vxba_initodom* h);
int vxba_initodom_cloud(vxba_initodom* h, float* xyz);
/* The search alone, for inspection: n float queries (n x 3) against the resident cloud -> idx n x 5 (ascending by (distance, index); -1 where
 * the cloud holds fewer than five points) and sqd n x 5 (the float32 squared distances; +inf beside -1). */
int vxba_initodom_search(vxba_initodom* h, int64_t n, const float* qry, int32_t* idx, float* sqd);
/* One scan: pnt_body n x 3 f64 (the pointVar points of var_init), state VXBA_STATE_LEN and cov 15x15 col-major in/out (x_curr).
 * A cloud of fewer than 100 points: the scan under `state`, rounded to float, is appended -- no filter, state and cov untouched.
 * Otherwise up to VXBA_LIO_MAX_ITER iterations (searching again after a converged step, and at iteration 2 if none has converged; finished
 * after two converged steps or iteration 3, with cov = (I - G) cov), then the scan under the final state is appended and the cloud filtered.
 * Everything is enqueued up front; the host waits once (once more per buffer that has to grow), for the filter's voxel count -- the filter's last
 * kernels are still in flight when the call returns; every later call on the handle is ordered behind them on the handle's stream.
 *   info (may be NULL) VXBA_INITODOM_INFO_LEN = [seeded (1: the first branch ran), iterations, valid of the last iteration, rematch_num,
 *        refind flag of iterations 0..3]
 *   sweeps_out (may be NULL) VXBA_LIO_MAX_ITER * VXBA_LIO_SWEEP_LEN: per iteration [HTH | HTz | 9 zeros | valid] in the layout of vxba_lio_sweep
 * A state or scan point that is not finite: VXBA_ERR_ARG, nothing launched.  A point beyond 2^20 filter voxels of the origin: VXBA_ERR_ARG, and the
 * cloud is cleared. */
int vxba_initodom_step(vxba_initodom* h, int64_t n, const double* pnt_body, double* state, double* cov, double* info, double* sweeps_out);
/* Per point of the last step's scan, as the search of `iteration` left it: nn n x 5 cloud indices (into the cloud the step started from),
 * ok n (1 = passed the gate), plane n x 4 (n, d).  VXBA_ERR_STATE if the last step did not search in that iteration. */
int vxba_initodom_inspect(vxba_initodom* h, int iteration, int32_t* nn, int32_t* ok, double* plane);
/* out[4] = [own kernel launches of the last step (rocPRIM's inside the filter not counted), host waits of the last step, cloud size, scan size] */
int vxba_initodom_stats(const vxba_initodom* h, int64_t out[4]);

/* ---- initialisation: pieces of Initialization::motion_init (voxelslam.cpp:488-713) ---------------------------------------------------
 * The IMU pose table of motion_blur (:495-521): K raw messages (stamps K, gyr / acc K x 3) integrated BACKWARD from xc (VXBA_STATE_LEN; its biases
 * replaced by those of bias_from, VXBA_STATE_LEN) with mid-point rates minus the bias, the accelerometer times `scale` (imupre_scale_gravity) and
 * dt = head - tail < 0; one entry of VXBA_INIT_POSE_LEN per head, messages K-2 .. 0: [offt = head stamp - beg_time | R 9 col-major | p 3 | v 3 | rate 3 |
 * acc_imu 3], the state AFTER the step.  Host code. */
#define VXBA_INIT_POSE_LEN 22
int vxba_init_pose_table(int K, const double* stamps, const double* gyr, const double* acc, double beg_time, const double* xc, const double* bias_from, double scale,
                         double* table);
/* motion_blur's de-skew of one raw scan (xyz n x 3 float, toff n float seconds, ascending: the reference's `curvature`) on the GPU, one lane per output
 * point: P = xc.R^T (R_i (ext.R P_i + ext.p) + T_ei).  The output is upstream's sequence exactly: descending time; points with toff <= the earliest
 * table offset are dropped; and the scan's FIRST point, once the walk has reached it, is emitted again under every earlier head it is later than (the
 * inner loop breaks at pl.begin() without leaving the outer one).  So *n_out may be smaller or larger than n: capacity n + K always suffices
 * (VXBA_ERR_ARG with *n_out set if not).  src_out (may be NULL): the scan index of every output point.  point_notime != 0: the extrinsic only, input
 * order, the IMU arguments ignored.  ext = [R 9 col-major | p 3]. */
int vxba_init_deskew(int device, int64_t n, const float* xyz, const float* toff, int K, const double* stamps, const double* gyr, const double* acc, double beg_time,
                     const double* xc, const double* bias_from, const double* ext, double scale, int point_notime, int64_t capacity, double* out, int32_t* src_out,
                     int64_t* n_out);
/* Sum of n n^T over the plane normals in the factor's cache (eig_vectors[k].col(0) after an evaluation), 3 x 3 column-major: motion_init's degeneracy
 * test takes its smallest eigenvalue.  One workgroup, fixed reduction tree, read where the cache lies. */
int vxba_init_normal_scatter(vxba_factor* f, double* nnt9);
/* IMU_PRE::push_imu (preintegration.hpp:50-73) over vxba_imu_add: for each pair of consecutive messages the mid-point sample, the accelerometer times
 * `scale`, minus the factor's biases, dt from the stamps.  Host code. */
int vxba_imu_push(double* imu, int K, const double* stamps, const double* gyr, const double* acc, double scale, const double* noise_meas, const double* noise_walk);
/* Initialization::motion_init (voxelslam.cpp:563-713): up to VXBA_INIT_MAX_ROUNDS rounds of { vxba_map_clear; per scan i: de-skew with x_buf[i] carrying the
 * biases of x_buf[max(i-1,0)], world points (converged rounds: calcBodyVar on the de-skewed point, then pvec_update with the frame's covariance; otherwise
 * identity variances), vxba_map_cut_voxel_device(ord = i); vxba_map_recut into the cleared factor -- stop below 10 voxels; vxba_li_damping_iter_gravity(.., 3);
 * new IMU factors from x_buf[i-1]'s biases and scan i's messages (vxba_imu_push) }, the convergence rule (|r0 - r1| / r0 < 0.05, then 0.01, from round 2 on:
 * normals' scatter, is_degrade = lambda0 < 15; the first time align_gravity and the caller's plane thresholds, the second time stop), and the final
 * checks (flag 0 if degenerate or |g| outside [9.6, 10.0]).  First-phase rounds run with min_eigen_value 0.02 and every plane_eigen_value_thre 1/4.
 *   m        the map (created with thread_num = 1 and the same win_size); f the factor of that win_size; both on one device
 *   scans    scan i = points scan_ptr[i] .. scan_ptr[i+1] of xyz (x 3 float) / toff (seconds after beg_times[i], ascending; NULL with point_notime)
 *   IMU      messages imu_ptr[i] .. imu_ptr[i+1] of stamps / gyr (x 3) / acc (x 3) belong to scan i
 *   states   win_size x VXBA_STATE_LEN in/out (x_curr is the last); covs win_size x 225 column-major; ext = [R 9 col-major | p 3]
 *   imus     (win_size - 1) x VXBA_IMU_LEN in/out; hess_out (15 W + 3)^2 of the last solve
 *   report   VXBA_INIT_MAX_ROUNDS x VXBA_INIT_REPORT_LEN, row per round: [factor voxels | resis 2 | g 3 after the solve | |r0 - r1| / r0 | 1 = the caller's
 *            thresholds and real variances were active | LM iterations | 1 = the solve ran | the convergence threshold in force | 1 = the rule fired]
 *   traces   (may be NULL) VXBA_INIT_MAX_ROUNDS x 3 x VXBA_TRACE_COLS; *n_rounds rounds were begun; eigvalue[3] of the last scatter (zero if none)
 *   *flag    converge_flag after the final checks.  With 0 the map and the factor are empty, as upstream leaves surf_map; the map's thresholds are the
 *            caller's again either way. */
#define VXBA_INIT_MAX_ROUNDS 10
#define VXBA_INIT_REPORT_LEN 12
typedef struct vxba_init_motion_params {
  double imupre_scale_gravity, dept_err, beam_err, imu_coef;
  double noise_meas[36], noise_walk[36];     /* column-major 6 x 6 */
  double min_eigen_value;                    /* the caller's plane thresholds (second phase) */
  double plane_eigen_value_thre[4];
  int point_notime;
} vxba_init_motion_params;
int vxba_init_motion(vxba_map* m, vxba_factor* f, int win_size, const int64_t* scan_ptr, const float* xyz, const float* toff, const double* beg_times,
                     const int64_t* imu_ptr, const double* stamps, const double* gyr, const double* acc, double* states, const double* covs, const double* ext,
                     const vxba_init_motion_params* prm, double* imus, double* hess_out, double* report, double* traces, int* n_rounds, double* eigvalue, int* flag);
/* Wall time of the calling thread's last vxba_init_motion by stage, microseconds, summed over its rounds: [de-skew | map build (variances, cut, recut) |
 * LM (vxba_li_damping_iter_gravity) | re-preintegration]. */
int vxba_init_motion_times(double out_us[4]);

/* ---- raw scan + raw IMU in: IMUEKF propagation and de-skew ----------------------------------------------------------------------------
 * Replaces `IMUEKF::process` (ekf_imu.hpp:41-214), the first link of both `initialization()` (voxelslam.cpp:1237) and the steady-state odometry
 * (:1571), and the voxel filter with its fallback behind it (:1574-1581).  The state machine, IMU_init and the forward propagation with its
 * covariance run on the host in f64; the scan is de-skewed by ONE kernel launch (one lane per point, the pose table in LDS, the head found by binary
 * search, one sin / cos pair per point, output to a second buffer) and stays in device memory for the filter and the odometry.
 *   state : VXBA_STATE_LEN f64 [R 9 col-major | p | v | bg | ba | g];  cov : 15 x 15 col-major in the order rot, p, v, bg, ba
 *
 * Reference semantics that are kept as they are:
 *   IMU_init       the first message sets the means and init_num = 1; EVERY message then does init_num++, so the divisors run 2, 3, ... and init_num
 *                  ends one above the message count.  The means are upstream's recurrence mean += (x - mean) / init_num evaluated in its order,
 *                  not a sum divided once.  init_num persists over calls; init_flag = init_num > 30, i.e. from the 30th message on.
 *   propagation    the working list is last_imu followed by the K messages.  A pair is skipped when tail.stamp < last_pcl_end_time;
 *                  cur_time = max(head.stamp, last_pcl_end_time), dt = tail.stamp - cur_time, offt = cur_time - beg_time.  Mid-point rate minus bg,
 *                  mid-point acc x scale_gravity minus ba; acc_imu = R acc + g with the OLD R; the pose entry is stored BEFORE the step.
 *                  F_x blocks: (0,0) = Exp(rate, -dt), (0,9) = -I dt, (3,6) = I dt, (6,0) = -R hat(acc) dt, (6,12) = -R dt; cov_w diagonals x dt^2 with
 *                  R diag(cov_acc) R^T dt^2 at (6,6); cov = F cov F^T + cov_w; then p, v, then R = R Exp(rate, dt).
 *                  Tail: note = +-1, dt = note (end_time - last stamp), v, R, p from the LAST surviving pair's rate and acc_imu.  With note = -1 (the
 *                  scan ends before the last message) upstream steps p back with - acc_imu dt^2 / 2 where the parabola has +: kept.
 *   de-skew        (toff non-decreasing)  point j > 0 belongs to the latest head with t_i < (double)toff_j -- strictly.  Points with toff <= t_0 are
 *                  left untouched, bit for bit.  P = L^T (xc.R^T (R_i (L P_i + l) + T_ei) - l), R_i = R Exp(rate, dt), T_ei = p + v dt + a dt^2 / 2 - xc.p
 *                  with the PROPAGATED xc, rounded to float.  Point 0: upstream's inner loop breaks at begin() without leaving the outer one, so point
 *                  0 is compensated once under EVERY head earlier than it, latest first, each application on the float result of the one before.
 *                  point_notime: the cloud passes through unchanged.
 *   refusals       each VXBA_ERR_ARG, nothing launched, the handle, state and cov untouched: n = 0 (upstream dereferences end() - 1); K < 1; any input
 *                  that is not finite; last_pcl_end_time - beg_time > 0.01 (upstream exits); no surviving pair (upstream reads uninitialised
 *                  vectors); toff not non-decreasing (upstream sorts in pcl_handler), tested on the host before the upload; IMU stamps that
 *                  decrease, among themselves or behind last_imu (the binary search needs the heads in time order; upstream's queue delivers them so).
 *                  More than VXBA_IMUEKF_MAX_HEADS surviving pairs: VXBA_ERR_UNSUPPORTED.  A handle that is not initialised does not look at the scan.
 * No CPU fallback. */
typedef struct vxba_imuekf vxba_imuekf; /* opaque: init_flag, init_num, the means, scale_gravity, last_pcl_end_time, last_imu, the device buffers */
#define VXBA_IMUEKF_INFO_LEN 8
#define VXBA_IMUEKF_MAX_HEADS 64
#define VXBA_IMUEKF_MSG_LEN 7               /* one IMU message: [stamp | gyr 3 | acc 3] */
typedef struct vxba_imuekf_params {
  double cov_acc[3], cov_gyr[3], cov_bias_gyr[3], cov_bias_acc[3];
  double ext[12];                           /* Lid_rot_to_IMU 9 col-major | Lid_offset_to_IMU 3 */
  int acc_in_g;                             /* upstream's `imu_topic == "/livox/imu"`: an accelerometer that may report in g */
  int point_notime;
} vxba_imuekf_params;
/* noise 0.1 / 0.1 / 1e-4 / 1e-4, identity extrinsic, acc_in_g = 1, point_notime = 0 */
void vxba_imuekf_default_params(vxba_imuekf_params* p);
/* params == NULL: the defaults.  min_init_num is 30. */
int vxba_imuekf_create(int device, const vxba_imuekf_params* params, vxba_imuekf** out);
int vxba_imuekf_destroy(vxba_imuekf* h);
const char* vxba_imuekf_last_error(const vxba_imuekf* h);
/* process().  xyz n x 3 float (LiDAR frame), toff n float (upstream's `curvature`: seconds after beg_time); stamps K / gyr K x 3 / acc K x 3 f64.
 * Not initialised: IMU_init, scale_gravity = 9.8 when |mean_acc| < 2 && acc_in_g, state.g = -mean_acc * scale_gravity, init_flag = init_num > 30,
 * last_pcl_end_time = end_time, last_imu = the last message; ready = 0, nothing launched, the scan is not looked at.
 * Initialised: motion_blur; state and cov in/out; ready = 1.  The call does not wait for the device.
 *   imus_out (may be NULL) (K + 1) x VXBA_IMUEKF_MSG_LEN: the list as upstream leaves it for IMU_PRE::push_imu -- last_imu in front re-stamped to the
 *            PREVIOUS last_pcl_end_time, the K messages, the last one re-stamped to end_time (the handle's last_imu keeps the original stamp);
 *            *K_out (may be NULL) = K + 1, or 0 while not ready
 *   info (may be NULL) VXBA_IMUEKF_INFO_LEN = [ready | heads M | points compensated | applications to point 0 | xc.t | scale_gravity | init_num | 0] */
int vxba_imuekf_process(vxba_imuekf* h, int64_t n, const float* xyz, const float* toff, int K, const double* stamps, const double* gyr, const double* acc, double beg_time,
                        double end_time, double* state, double* cov, double* imus_out, int* K_out, double* info);
/* The de-skewed cloud of the last ready process, n x 3 float, input order. */
int vxba_imuekf_read_scan(vxba_imuekf* h, float* xyz_out);
/* The M heads of the last ready process x VXBA_INIT_POSE_LEN: [offt | R | p | v | rate | acc_imu], the state BEFORE each step, as
 * imu_poses.emplace_back stores it.  table: room for VXBA_IMUEKF_MAX_HEADS rows. */
int vxba_imuekf_pose_table(const vxba_imuekf* h, double* table);
/* system_reset's share (voxelslam.cpp:1302-1305): mean_acc = 0, init_num = 0, IMU_init over the K messages, g_out = -mean_acc * scale.  init_flag is
 * left as it is. */
int vxba_imuekf_reinit(vxba_imuekf* h, int K, const double* stamps, const double* gyr, const double* acc, double scale, double* g_out);
/* A new handle's state (the device buffers are kept). */
int vxba_imuekf_clear(vxba_imuekf* h);
/* voxelslam.cpp:1574-1581 on the resident de-skewed cloud: the voxel filter (vxba_down_sampling_voxel's, device to device) at down_size; fewer than
 * min_points (upstream 500) out: again from the full cloud at down_size / 2.  One host wait per pass.  vxba_imuekf_filter_passes: 1 or 2 for the last
 * filter. */
int vxba_imuekf_filter(vxba_imuekf* h, double down_size, int64_t min_points, int64_t* n_out);
int vxba_imuekf_filter_passes(const vxba_imuekf* h);
/* The filtered cloud: read back (n_out x 3 float), or handed on in device memory -- valid until the handle's next process, filter or destroy; a
 * consumer inside this library (vxba_lio_scan_raw_device) orders itself behind the filter through the handle's event. */
int vxba_imuekf_filtered(vxba_imuekf* h, float* xyz_out);
int vxba_imuekf_filtered_device(vxba_imuekf* h, const float** d_xyz, int64_t* n);
/* out[4] = [own kernel launches of the last process + filter (rocPRIM's inside the filter not counted), host waits of the same (one per filter
 * pass; one more when the buffers had to grow or the previous upload was still in flight), n, n filtered] */
int vxba_imuekf_stats(const vxba_imuekf* h, int64_t out[4]);
/* Measurement: with profiling on, events are recorded on the handle's stream around the de-skew (upload + kernel) and around the filter (all passes).
 * vxba_imuekf_stage_times waits for the stream and returns out_ms[2] = [de-skew | filter] of the last process / filter, -1 where none ran. */
int vxba_imuekf_set_profiling(vxba_imuekf* h, int enable);
int vxba_imuekf_stage_times(vxba_imuekf* h, double out_ms[2]);

/* ---- driver messages in: scan decoding, filters and time sort ------------------------------------------------------------------------------
 * Replaces the handlers of `Features::process` (feature_point.hpp:142-366) and `pcl_handler` behind them (voxelslam.hpp:76-103): the point bytes of
 * the driver's message in, the decimated, range-filtered, time-sorted and trimmed cloud out -- resident xyz n x 3 float and toff n float, what
 * vxba_imuekf_process takes from the host, handed to vxba_imuekf_process_device without leaving the device.  Intensity is not carried: nothing
 * downstream reads it.  `sync_packages` (voxelslam.hpp:105-161) is host bookkeeping and lives in the Python front (front.PackageSync).
 *
 *   layout         point_step and the byte offsets of x, y, z (float32) and of the time field carry NO alignment assumption (Livox CustomPoint: 19
 *                  bytes, offset_time u32 at 0, x y z at 4 8 12; a common Velodyne layout: time f32 at 18, step 22).  Little-endian only.  The kernel
 *                  loads a workgroup's byte range as aligned dwords into LDS and assembles every field from there.
 *   time rules     the time is written as `curvature` (toff):
 *                    VXBA_SCAN_RULE_AS_IS        (float) time of an f32 field: the Velodyne branch with a time field, :179-197
 *                    VXBA_SCAN_RULE_NANOSECONDS  (float) u32 / float(1000000000): the conversion rounds to nearest, the division is correctly
 *                                                rounded.  Livox :155, Ouster :271
 *                    VXBA_SCAN_RULE_MINUS_HEAD   (float)(t - time_head), both doubles.  Hesai :304, Robosense :335; time_head is point 0's timestamp
 *                    VXBA_SCAN_RULE_NONE         0.  TartanAir :350-366, with filter = 0: every point is taken, no decimation and no blind test
 *   filter         point i is kept when i % point_filter_num == 0 on the ORIGINAL index and x*x + y*y + z*z > blind: the sum in float, left to
 *                  right, no contraction, compared as double, strictly.  A NaN coordinate fails the test and is dropped, as upstream.
 *   trim           pcl_handler pops the sorted tail while (double) curvature > 0.11 (:96); here those points are dropped before the sort -- the same set.
 *   fallback       (:82-90) when nothing survives decimation and blind -- n_points = 0 included -- the cloud is two points at the origin, times 0, 0.09.
 *   FIXED CHOICES where upstream leaves the result open:
 *     tie order    upstream's std::sort is not stable and multi-ring sensors tie constantly.  Here: by time, ties in INPUT order (a stable radix sort
 *                  of (time bits, slot) pairs; the result does not depend on scheduling).
 *     non-finite   a time that is not finite drops the point (upstream's sort is undefined on a NaN); so does an infinite coordinate, and a NaN one
 *                  under filter = 0 (upstream passes them on; nothing downstream accepts them).  Such points do not count as survivors.
 *     -0.0 times   become +0.0.
 *     all trimmed  survivors exist but all lie behind 0.11: upstream pops an empty vector.  Here VXBA_ERR_ARG AFTER the run, the record written with
 *                  n_out = 0, and the handle holds no cloud.
 *   refusals       each VXBA_ERR_ARG, nothing launched, the previous cloud still readable: point_filter_num < 1; point_step below 12, above
 *                  VXBA_SCAN_MAX_STEP or smaller than a field's end; fields that overlap; time_type and time_rule that do not belong together;
 *                  n_points == 0 under MINUS_HEAD (upstream reads points[0]); n_points >= 2^31; blind NaN.
 *   plain push     under AS_IS a message whose LAST point's time is not in (0.01, 0.12) -- upstream's test, :176 -- is VXBA_ERR_UNSUPPORTED from
 *                  vxba_intake_push, decided on the host, nothing launched: such a message belongs to vxba_intake_push_yaw (below).  Big-endian
 *                  messages are not accepted.
 *   YAW TIMES      VXBA_SCAN_RULE_YAW + vxba_intake_push_yaw: the Velodyne branch without a usable time field (:200-252), every point's time derived
 *                  from its yaw angle.  The rule pairs with VXBA_SCAN_TIME_NONE (no time field) or VXBA_SCAN_TIME_F32 (a field that is present and
 *                  ignored); filter must be 1.  Upstream's loop, restated -- x, y, z floats, i the original index, every operation unfused:
 *                    skip      fabs(x) < 0.1 (float against the double): the point takes no part; its index still counts for `cool`
 *                    angle     r_i = (double) atan2f(y, x) * 57.2957
 *                    first     the first non-skipped point f sets yaw_first = r_f, blind or not
 *                    active    not skipped and not ((x*x + y*y) + z*z in float) < blind as doubles, STRICTLY: a squared range equal to blind stays
 *                    step      d_j = r_j - r_p for an active j, p the previous active point (f for the first one)
 *                    state     q in {0, 1}, the wrap count k, the index e of the last wrap event; "cool allows": no event yet, or j - e >= 1000
 *                                d_j >  180 (candidate)   q_p = 0: cool allows -> EVENT k += 1, e = j, q = 0; else q = 1.     q_p = 1: q = 0
 *                                d_j == 180               q = 0
 *                                -180 <= d_j < 180        q = q_p
 *                                d_j < -180               q = 1
 *                              (the q = 1 of a blocked candidate adds 360 the "wrong" way: upstream's behaviour, kept)
 *                    yaw       at an event (r_j - 360 (k - 1)) - 360, two subtractions; otherwise r_j - 360 k; then + 360 when q_j = 1
 *                    time      curvature = (float)((yaw_first - yaw_j) / omega_l), the double division correctly rounded
 *                    keep      curvature >= 0, (double) curvature < 0.1 and i % point_filter_num == 0
 *                  then as every other rule: -0.0, the stable sort, the gather, the two-point fallback when nothing is kept, the record (n after
 *                  filter = the points kept).  FIXED CHOICES of this route:
 *                    atan2      the float atan2 is the correctly rounded float of the exact value.  The device takes the float rounding of a DOUBLE
 *                               atan2, which differs from that only where the exact value lies within the double routine's error of a float rounding
 *                               tie; the device's float atan2f, whose last bit is unspecified, is not used.  Equal to upstream wherever upstream's libm
 *                               rounds atan2f correctly.
 *                    decisions  the tests on 180 and -180 are made on d_j = r_j - r_p, rounded once.  Upstream evaluates (r_j - bias) - yaw_last,
 *                               which can round differently at magnitudes near 540; the two agree unless upstream's own difference lies within 2^-40
 *                               degrees of the threshold.
 *                    non-finite a point with a coordinate that is not finite is skipped like |x| < 0.1 (upstream lets a NaN poison yaw_first and
 *                               every later time).
 *                  Refusals of vxba_intake_push_yaw, each VXBA_ERR_ARG, nothing launched, the previous cloud still readable: a layout that is not
 *                  RULE_YAW; omega_l not finite or <= 0; and those above on point_step, overlap, point_filter_num, blind and n_points.
 *                  vxba_intake_push with a RULE_YAW layout is VXBA_ERR_ARG: omega_l is missing.
 * One host wait per push, for the record; launches and waits do not depend on n_points (one more wait when a buffer has to grow).  No CPU fallback. */
typedef struct vxba_intake vxba_intake; /* opaque: the pinned staging block, the device buffers, the last cloud */
#define VXBA_SCAN_TIME_NONE 0
#define VXBA_SCAN_TIME_F32 1
#define VXBA_SCAN_TIME_U32 2
#define VXBA_SCAN_TIME_F64 3
#define VXBA_SCAN_RULE_NONE 0
#define VXBA_SCAN_RULE_AS_IS 1
#define VXBA_SCAN_RULE_NANOSECONDS 2
#define VXBA_SCAN_RULE_MINUS_HEAD 3
#define VXBA_SCAN_RULE_YAW 4
#define VXBA_SCAN_MAX_STEP 240
#define VXBA_INTAKE_REC_LEN 6
typedef struct { int32_t point_step, off_x, off_y, off_z, off_time, time_type, time_rule, filter; } vxba_scan_layout;
int vxba_intake_create(int device, vxba_intake** out);
int vxba_intake_destroy(vxba_intake* h);
const char* vxba_intake_last_error(const vxba_intake* h);
/* bytes: n_points x layout->point_step.  time_head: MINUS_HEAD only.  rec_out VXBA_INTAKE_REC_LEN doubles =
 * [n_out | toff_first | toff_last | fallback used | n decoded | n after filter (decimation, blind, finiteness; before the trim)]. */
int vxba_intake_push(vxba_intake* h, const vxba_scan_layout* layout, int64_t n_points, const void* bytes, int point_filter_num, double blind, double time_head,
                     double* rec_out);
/* The same for a VXBA_SCAN_RULE_YAW layout (YAW TIMES above): omega_l is the sensor's turn rate in degrees per second (upstream 3610).  The same record,
 * fallback and resident cloud; six launches of this unit, two rocPRIM scans and the sort, one host wait, none depending on n_points. */
int vxba_intake_push_yaw(vxba_intake* h, const vxba_scan_layout* layout, int64_t n_points, const void* bytes, int point_filter_num, double blind, double omega_l,
                         double* rec_out);
/* out[4] = [points skipped by |x| < 0.1 or a non-finite coordinate | active points (not skipped, not blind) | wrap candidates (d > 180) | wrap events]
 * of the last push when that was a yaw push; VXBA_ERR_STATE otherwise. */
int vxba_intake_yaw_info(const vxba_intake* h, int64_t out[4]);
/* The last cloud: read back (n_out x 3 float, n_out float), or in device memory -- valid until the handle's next push or destroy; a consumer inside
 * this library (vxba_imuekf_process_device) orders itself behind the push through the handle's event.  VXBA_ERR_STATE / n = 0 without a cloud. */
int vxba_intake_read(vxba_intake* h, float* xyz, float* toff);
int vxba_intake_device(vxba_intake* h, const float** d_xyz, const float** d_toff, int64_t* n);
/* out[4] = [own kernel launches of the last push (rocPRIM's not counted), host waits of the same, n_out, n decoded] */
int vxba_intake_stats(const vxba_intake* h, int64_t out[4]);
/* Measurement, as vxba_imuekf_set_profiling: out_ms[3] = [upload + decode / filter | sort | the whole push on the device] of the last push. */
int vxba_intake_set_profiling(vxba_intake* h, int enable);
int vxba_intake_stage_times(vxba_intake* h, double out_ms[3]);
/* vxba_imuekf_process with the scan taken from an intake's resident cloud, device to device behind its event: only the pose table goes up.  The host
 * checks of the scan are replaced by what the intake guarantees (finite, non-decreasing, n >= 1); an intake without a cloud is the empty scan.
 * info[3] comes from the intake's toff_first; info[2], the points compensated, is -1 on this route (counting them would take a host wait).  The
 * de-skewed cloud, state, cov and imus_out are byte-identical to vxba_imuekf_process on the same arrays. */
int vxba_imuekf_process_device(vxba_imuekf* h, vxba_intake* intake, int K, const double* stamps, const double* gyr, const double* acc, double beg_time, double end_time,
                               double* state, double* cov, double* imus_out, int* K_out, double* info);

/* ---- hierarchical global BA: one bottom-up pass over a session of keyframes (BASELINE configs[4]) ----------------------------
 * thd_globalmapping's loop (voxelslam.cpp:2485-2595): windows of `wdsize` keyframes with stride `mgsize`, each refined by one round of
 * HBA_add_edge (:2320-2482 -- OctreeGBA::cut_voxel + OctreeGBA_multi_recut, Lidar_BA_Optimizer::damping_iter with 4 iterations, Hessian ->
 * pose-graph edge weights :2405-2427) and merged into a voxel-filtered submap anchored at its first keyframe (:2430-2450); then ONE
 * HBA_add_edge over all S submap poses (S <= VXBA_MAX_WIN_WIDE; vxba_hba_num_windows) with up to `top_max_iter` re-voxelisation
 * rounds.  The keyframe clouds live in device memory from vxba_hba_add_keyframes on; a pass moves only poses, Hessians and counts
 * across PCIe.  What consumes the edges (GTSAM's ISAM2 in the reference, :2231-2317): the pose-graph optimiser below, vxba_pgo_*. */
typedef struct vxba_hba vxba_hba;
int vxba_hba_create(int device, vxba_hba** out);
int vxba_hba_destroy(vxba_hba* h);
const char* vxba_hba_last_error(const vxba_hba* h);
/* Appends n_keyframes clouds (PointType xyz as float, keyframe coordinates): cloud_ptr n_keyframes + 1 offsets in points (cloud_ptr[0] = 0). */
int vxba_hba_add_keyframes(vxba_hba* h, int64_t n_keyframes, const int64_t* cloud_ptr, const float* xyz);
int vxba_hba_num_keyframes(const vxba_hba* h);
int vxba_hba_threads_used(const vxba_hba* h); /* host threads / streams the last vxba_hba_pass ran its bottom level on */
int vxba_hba_clear(vxba_hba* h); /* forget the keyframes (the device buffers are kept) */
/* Windows of a bottom-up pass over K keyframes (thd_globalmapping, voxelslam.cpp:2498-2575): S_full = (K - wdsize) / mgsize + 1 full windows of
 * wdsize keyframes at stride mgsize (0 when K < wdsize) and, with tail != 0, the CLOSING window of upstream's total_ba iteration (:2519-2523: it skips
 * the "fewer than wdsize keyframes" test) over the keyframes left behind the last pop, [S_full mgsize, K) -- wdsize - mgsize .. wdsize - 1 of them
 * in a long session, all K of a session shorter than one window.  A closing window of one keyframe is not refined (its cloud is the submap).
 * vxba_hba_window: first keyframe and keyframe count of window w. */
int vxba_hba_num_windows(int n_keyframes, int wdsize, int mgsize, int tail);
int vxba_hba_window(int n_keyframes, int wdsize, int mgsize, int tail, int w, int* first, int* count);
/* One whole pass on one device.  poses: K x 12 ([R column-major 9 | p 3], as everywhere).  n_threads: 1 .. 8 host threads / streams for the
 * bottom level; <= 0: the library picks -- 4 (measured best on one MI355X), fewer under a small cgroup CPU quota (the threads poll while their
 * streams run).  tail: see above (upstream: 1).
 * Out, S = vxba_hba_num_windows(..): submap_poses S x 12 (refined anchors), submap_sizes S (points per voxel-filtered submap; may be NULL); the edges
 * of both levels in order -- bottom level window by window, then the top level: edge_ij 2 ints (keyframe indices i < j), edge_data 18 doubles
 * [R_i^T R_j row-major 9 | R_i^T (p_j - p_i) 3 | v6 = 1 / |hess(6i+k, 6j+k)| 6] per edge, at most edge_capacity of them (the counts are exact even
 * when the arrays were too small or NULL: VXBA_ERR_ARG then); top_rounds 5 doubles per top-level round [factor voxels, residual before, after,
 * is_converge, fine parameters used] (top_max_iter x 5, may be NULL). */
int vxba_hba_pass(vxba_hba* h, const double* poses, const vxba_voxelize_params* coarse, const vxba_voxelize_params* fine, int wdsize, int mgsize, int tail,
                  int top_max_iter, int n_threads, double* submap_poses, int64_t* submap_sizes, int64_t edge_capacity, int32_t* edge_ij, double* edge_data,
                  int64_t* n_edges1, int64_t* n_edges2, double* top_rounds, int* n_top_rounds);
/* The same pass in its two halves, for one rank of N (one process per GPU; vxba_hba_pass is vxba_hba_bottom(0, 1) + vxba_hba_top on one device):
 *   vxba_hba_bottom          the windows w_first, w_first + w_stride, .. (rank r of N: r, N -- independent HBA_add_edge problems, no exchange): fills
 *                            THEIR rows of submap_poses / submap_sizes, leaves their submaps in device memory, returns their edges with the window
 *                            each came from (edge_window, may be NULL);
 *   vxba_hba_export_submaps  those submaps packed back to back (window order, float xyz) into the caller's DEVICE buffer -- what the rank hands to
 *                            the all-gather (ncclAllGather / torch.distributed over RCCL, device to device);
 *   vxba_hba_import_submaps  a peer's packed submaps (sizes: S entries, the selection's are read) into place;
 *   vxba_hba_top_factor      the factor of the top level (session-owned): attach the rank's collective to it (vxba_rccl_attach / vxba_peer_attach /
 *                            vxba_set_allreduce) when the top level is voxel-sharded;
 *   vxba_hba_top             ONE HBA_add_edge over all submap poses (voxelslam.cpp:2553-2560); coarse / fine may carry the rank's voxel shard
 *                            (shard_index / shard_count: every rank voxelises the same submaps and keeps the root voxels that hash to it; the packed
 *                            [Hess | JacT | residual] is summed by the attached collective, one all-reduce per sweep).  Needs every submap present. */
int vxba_hba_bottom(vxba_hba* h, const double* poses, const vxba_voxelize_params* coarse, const vxba_voxelize_params* fine, int wdsize, int mgsize, int tail,
                    int w_first, int w_stride, int n_threads, double* submap_poses, int64_t* submap_sizes, int64_t edge_capacity, int32_t* edge_ij,
                    double* edge_data, int32_t* edge_window, int64_t* n_edges);
int vxba_hba_export_submaps(vxba_hba* h, int w_first, int w_stride, float* d_out, int64_t capacity_points, int64_t* n_points);
int vxba_hba_import_submaps(vxba_hba* h, int w_first, int w_stride, const int64_t* sizes, const float* d_in);
int vxba_hba_top_factor(vxba_hba* h, vxba_factor** out);
int vxba_hba_top(vxba_hba* h, const double* poses, const vxba_voxelize_params* coarse, const vxba_voxelize_params* fine, int top_max_iter, double* submap_poses,
                 int64_t edge_capacity, int32_t* edge_ij, double* edge_data, int64_t* n_edges, double* top_rounds, int* n_top_rounds);

/* ---- pose-graph optimisation: the top-down half of the global BA ------------------------------------------------------------
 * What topDownProcess (voxelslam.cpp:2231-2317) and the loop-closure graph (build_graph :1741-1802, solved :2090-2097) hand to GTSAM's
 * ISAM2: poses on SE(3) under between and prior factors with diagonal variances.  Nodes are pose records [R column-major 9 | p 3].
 *   between (i, j, Z = (Zr, zt), v6):  e = [Log(Zr^T R_i^T R_j) ; Zr^T (R_i^T (p_j - p_i) - zt)]
 *   prior   (i, Z, v6):                e = [Log(Zr^T R_i)       ; Zr^T (p_i - zt)]
 *   cost = 1/2 sum over factors, k of e_k^2 / v6_k -- rotation entries first, then translation: the order of hess(6i+k, ..) and of v6.
 * This is BetweenFactor<Pose3> / PriorFactor<Pose3> with noiseModel::Diagonal::Variances under GTSAM's default Pose3 chart (translation
 * as is, not through the SE(3) logarithm).  GTSAM's rotation chart is a build option (Cayley or Log; they agree to second order in the
 * residual angle); Log is used here, accurate from 1e-9 rad up; residual angles near pi are out of scope.  GTSAM is not part of this
 * project's test environment: parity with ISAM2 cannot be pinned here; the optimiser is pinned to the mathematics above (tests/_pgo_ref.py).
 * The minimiser: Levenberg-Marquardt with the damping rule of the LiDAR optimisers (gain ratio; accept: u *= max(1/3, 1 - (2 rho - 1)^3),
 * v = 2; reject: u *= v, v *= 2; a trial cost that is not a number is a rejected step), update R <- R Exp(dphi), p <- p + dp, inner solve
 * (H + u diag H) dx = -g by conjugate gradients preconditioned with the inverted 6 x 6 diagonal blocks.  Deterministic: no floating-point
 * atomics, every sum in a fixed order.  The number of kernel launches and host synchronisations of one vxba_pgo_optimize is a constant
 * times max_iter, whatever the CG iteration count (vxba_pgo_stats). */
typedef struct vxba_pgo vxba_pgo;
typedef struct vxba_pgo_options {
  int max_iter;         /* linearisations at most; <= 0: 6 (the reference's ISAM2 calls: one update + five with relinearizeSkip = 1) */
  int cg_max_iter;      /* CG iteration cap per solve; <= 0: max(200, 2 x 6 x nodes) */
  double cg_tol;        /* relative tolerance on the preconditioned residual sqrt(r.z / r0.z0); <= 0: 1e-8 */
  double rel_cost_tol;  /* stop when |cost change| / cost falls below it; < 0: 1e-6 (as the other optimisers); 0: never */
  double u0;            /* initial damping; <= 0: VXBA_PGO_DEFAULT_U0 */
  double v0;            /* initial rejection factor; <= 0: 2 */
} vxba_pgo_options;
/* 1e-6, not the LiDAR optimisers' 0.01: the damping is relative to diag H, and the weak modes of a pose graph (a chain bending as a whole)
 * have curvature ~1 / nodes^2 of it -- damped at 1e-2 they move by a fraction of a per cent per step. */
#define VXBA_PGO_DEFAULT_U0 1e-6
/* One report row per outer iteration: [cost before, cost after (at the trial poses), accepted (1 / 0), u of this solve, CG iterations,
 * 1 if the cap ended the solve, decrease predicted by the quadratic model, relative preconditioned residual at the end of the solve]. */
#define VXBA_PGO_REPORT_LEN 8
int vxba_pgo_create(int device, vxba_pgo** out);
int vxba_pgo_destroy(vxba_pgo* h);
const char* vxba_pgo_last_error(const vxba_pgo* h);
int vxba_pgo_clear(vxba_pgo* h); /* forget nodes and factors (the device buffers are kept) */
int vxba_pgo_num_nodes(const vxba_pgo* h);
int64_t vxba_pgo_num_factors(const vxba_pgo* h);
/* The nodes: n x 12.  Before any factor; later calls replace the values of the same n nodes.  A pose that is not finite: VXBA_ERR_ARG. */
int vxba_pgo_set_poses(vxba_pgo* h, int n, const double* poses);
int vxba_pgo_read_poses(vxba_pgo* h, double* poses);
/* n between factors.  edge_ij 2 ints and edge_data 18 doubles per edge, EXACTLY the records vxba_hba_pass writes: [Zr row-major 9 | zt 3 |
 * v6 6]; factor k joins node node_offset_i + edge_ij[2k] to node node_offset_j + edge_ij[2k + 1] (the reference's stepsizes: several sessions
 * in one graph).  i > j and repeated pairs are fine.  i == j, an index out of range, a value that is not finite or a v6 <= 0: VXBA_ERR_ARG,
 * and none of the n is added. */
int vxba_pgo_add_edges(vxba_pgo* h, int64_t n, int node_offset_i, int node_offset_j, const int32_t* edge_ij, const double* edge_data);
/* n prior factors: node n ints, pose12 n x 12 pose records, v6 n x 6 (the reference: the first pose, variances 1e-9, voxelslam.cpp:1777-1782). */
int vxba_pgo_add_priors(vxba_pgo* h, int64_t n, const int32_t* node, const double* pose12, const double* v6);
/* Cost at the current poses; residuals (may be NULL): 6 per factor in the order the factors were added. */
int vxba_pgo_cost(vxba_pgo* h, double* cost, double* residuals);
/* Optimise the current poses in place.  options may be NULL (all defaults).  poses_out n x 12 (may be NULL: vxba_pgo_read_poses), report
 * report_capacity >= max_iter rows of VXBA_PGO_REPORT_LEN (may be NULL), n_outer the rows written.  A node without any factor keeps its
 * pose bit for bit.  A connected component that has between factors but no prior is gauge-free: VXBA_ERR_ARG naming one of its nodes,
 * nothing launched. */
int vxba_pgo_optimize(vxba_pgo* h, const vxba_pgo_options* options, double* poses_out, double* report, int report_capacity, int* n_outer);
/* [kernel launches, host synchronisations] of the last vxba_pgo_optimize, [nodes, factors] of the graph. */
int vxba_pgo_stats(const vxba_pgo* h, int64_t out[4]);

/* ---- loop-edge registration: plane clouds, the verify score, normal-gated ICP ---------------------------------------------------
 * What stands between place recognition and lp_edges.push in the reference: a keyframe cloud -> one (centre, normal) per voxel that
 * holds a plane (STDescManager::init_voxel_map / BTCOctoTree::init_plane / get_plane, BTC.cpp:96-139, 279-338), the share of source
 * planes that find a compatible target plane under a hypothesis (plane_geometric_verify, BTC.cpp:1422-1479), and icp_normal
 * (loop_refine.hpp:47-145).  The descriptors, the hash database and the voting that produce candidates and hypotheses: vxba_loopsearch_* below.
 * A plane cloud is n x 6 float32 (x, y, z, nx, ny, nz): the reference's PointXYZINormal fields.  A pose record [R column-major 9 | t 3]
 * maps source-frame coordinates into the target frame (loop_transform); with source = the current keyframe j and target = keyframe i it
 * is the (rot, tra) of the between factor (i, j) that vxba_pgo_add_edges takes.
 * Association, per source plane:  p = R p_s + t and n = R n_s in float64 from the float32 fields; q = float32(p); the nearest target
 * centre is the one of smallest float32 squared distance (dx dx + dy dy) + dz dz (no contraction), ties to the LOWEST index -- exact, by
 * brute force over LDS tiles -- then the gate, in float64, with gates = (a, b, c, d):
 *   (|n - n_t| < a or |n + n_t| < b) and |n_t . (p - p_t)| < c and |p - p_t| < d
 * Deterministic: no floating-point atomics, every sum down a fixed tree; a pair's result does not depend on the batch around it. */
typedef struct vxba_loopreg vxba_loopreg;
typedef struct vxba_planecloud_params {
  double voxel_size;            /* <= 0: 1.0  (BTC.h:30) */
  int voxel_init_num;           /* a voxel needs N > voxel_init_num points; < 0: 10  (BTC.h:31) */
  double plane_detection_thre;  /* a voxel is a plane iff lambda_min < it; <= 0: 0.01  (BTC.cpp:10) */
} vxba_planecloud_params;
typedef struct vxba_icp_options {
  int max_iter;       /* <= 0: 20 */
  double gates0[4];   /* the gates until the first small step; gates0[0] <= 0: (0.2, 0.2, 0.5, 3) */
  double gates1[4];   /* the gates after it; gates1[0] <= 0: (0.1, 0.1, 0.1, 1) */
  double step_tol;    /* a step is small when |dphi| and |dt| are both below it; <= 0: 1e-3 */
  double icp_eigval;  /* accept needs the smallest eigenvalue of sum n_t n_t^T above it; <= 0: 14 (voxelslam.cpp:1812) */
} vxba_icp_options;
/* One report row per pair: [accept (1 / 0), is_converge, iterations run, match_num, eig0 <= eig1 <= eig2 of sum n_t n_t^T, resi] -- the
 * last four of the last iteration run. */
#define VXBA_ICP_REPORT_LEN 8
int vxba_loopreg_create(int device, vxba_loopreg** out);
int vxba_loopreg_destroy(vxba_loopreg* h);
const char* vxba_loopreg_last_error(const vxba_loopreg* h);
int vxba_loopreg_clear(vxba_loopreg* h); /* forget every cloud; ids start at 0 again */
int vxba_loopreg_num_clouds(const vxba_loopreg* h);
int64_t vxba_loopreg_cloud_size(const vxba_loopreg* h, int id); /* rows of cloud id; -1 for an id out of range */
int vxba_loopreg_read_cloud(vxba_loopreg* h, int id, float* xyzn);
/* A plane cloud as it is: n x 6 (n may be 0).  A value that is not finite: VXBA_ERR_ARG.  *id receives the cloud's id (ids count up from 0). */
int vxba_loopreg_add_cloud(vxba_loopreg* h, int64_t n, const float* xyzn, int* id);
/* The plane cloud of a keyframe: xyz n_points x 3 in the keyframe's frame.  Voxel coordinate per axis exactly as BTC.cpp:287-295 (divide by
 * voxel_size, subtract 1.0 where negative, truncate); per voxel with N > voxel_init_num: c = sum p / N, cov = sum p p^T / N - c c^T (sums in
 * input order), a plane iff lambda_min < plane_detection_thre; the row is (c, eigenvector of lambda_min) rounded to float32.  Where the
 * reference leaves the order (unordered_map) and the eigenvector's sign open: rows ascend by voxel coordinate, lexicographic in (x, y, z),
 * and the normal's component of largest magnitude (the first of equals) is positive -- the gate tests n - n_t and n + n_t alike, and a
 * flipped n_t flips Jacobian row and residual together, so nothing downstream sees either choice.  params may be NULL (all defaults).
 * A point that is not finite or lies beyond 2^20 voxels of the origin: VXBA_ERR_ARG, no cloud added. */
int vxba_loopreg_add_keyframe(vxba_loopreg* h, int64_t n_points, const double* xyz, const vxba_planecloud_params* params, int* id, int64_t* n_planes);
/* Inspection of one hypothesis under one gate vector: per source row the nearest target index (-1 when the target is empty) and the gate's verdict. */
int vxba_loopreg_associate(vxba_loopreg* h, int src, int tar, const double pose[12], const double gates[4], int32_t* nn, uint8_t* matched);
/* The verify score of B hypotheses: src_tar B x 2 cloud ids, poses B x 12.  Gates (normal_thr, normal_thr, dis_thr, none)
 * (BTC.cpp:1468-1475); useful (may be NULL) the count, score = useful / source rows (0 for an empty source). */
int vxba_loopreg_score(vxba_loopreg* h, int B, const int32_t* src_tar, const double* poses, double normal_thr, double dis_thr, double* score, int64_t* useful);
/* icp_normal on B pairs at once; poses_inout B x 12 holds the hypotheses on entry and the refined poses on return.  Per iteration and pair,
 * over the gated rows:  rr = n_t . (p - p_t), jac = [hat(p_s) R^T n_t ; n_t], Hess += jac jac^T, JacT += jac rr, resi += rr^2 / 2,
 * mat_norm += n_t n_t^T;  Hess dx = -JacT;  R <- R Exp(dx[0:3]), t <- t + dx[3:6].  The first time both step norms are below step_tol the
 * gates change to gates1 and is_converge is set, the next time the pair stops; max_iter iterations at most.
 * accept = (smallest eigenvalue of the last mat_norm > icp_eigval) and is_converge.
 * Where the reference is undefined -- fewer than 6 gated rows (it solves a singular system and carries NaN on), or a step that is not
 * finite -- the pair stops there: accept 0 (the reference's answer too), is_converge 0, the pose the last finite one, a finite report.
 * The loop stays on the device: 2 max_iter launches and a constant number of host synchronisations, whatever B, the cloud sizes and the
 * iteration counts (vxba_loopreg_stats); the workgroups of a finished pair return at once.  options may be NULL (all defaults), report
 * (may be NULL) B x VXBA_ICP_REPORT_LEN.  A cloud id out of range or a pose that is not finite: VXBA_ERR_ARG, nothing launched. */
int vxba_loopreg_icp(vxba_loopreg* h, int B, const int32_t* src_tar, double* poses_inout, const vxba_icp_options* options, double* report);
/* [kernel launches, host synchronisations, clouds held, pairs] of the last associate / score / icp call. */
int vxba_loopreg_stats(const vxba_loopreg* h, int64_t out[4]);

/* ---- loop search: triangle descriptors, database, vote, verify -------------------------------------- */
/* The head of the loop-closure chain: from a keyframe's corners to the candidates and guesses vxba_loopreg_icp takes -- the reference's
 * STDescManager::generate_std, AddSTDescs, candidate_selector, candidate_verify / triangle_solver and SearchLoop (BTC.cpp:979-1420, 205-277)
 * on a device-resident database.  The corners come from vxba_corner_extract below (the projection images of BTC.cpp:340-977) or from the caller:
 * a corner is a location (3 float64) and an occupancy word (bit k = cell k of its column occupied; the reference's occupy_array_).
 *
 * describe:  locations rounded to float32; every corner's K = min(descriptor_near_num, n) nearest corners (itself included) by float32 squared
 * distance (dx dx + dy dy) + dz dz, ties to the lowest index; for corner i and 1 <= m < n < K the triangle (i, m-th, n-th): sides from float32
 * differences squared and summed in float64; rejected when a side lies outside [min_len, max_len]; sides sorted by the reference's three swaps;
 * rejected when |c - (a + b)| < 0.2; key ((int64)(float)(1000 a), ... b, ... c), the first triangle of a key in (i, m, n) order survives.
 * Vertex A is shared by a and b, B by a and c, C by b and c; centre = (A + B + C) / 3 of the float32-rounded corners; triangle = (a, b, c) *
 * (1 / std_side_resolution); a descriptor keeps the float64 locations and the occupancy words of A, B, C.  Fewer than 3 corners: no descriptor.
 * add:  the current set becomes frame num_frames, filed under cell (int)(triangle + 0.5) per axis, in order.
 * search:  per descriptor i and neighbour offset o (27, x outermost): cell (int)(triangle + inc), visited if |triangle - (cell + 0.5)| < 1.5;
 * an entry j matches when num_frames - frame_j > skip_near_num and |triangle - triangle_j| < |triangle| rough_dis_threshold and the mean over
 * A, B, C of 2 |b1 & b2| / (|b1| + |b2|) exceeds similarity_threshold.  The match list is ordered by (i, o, position in the cell).  Candidates:
 * frames by (votes descending, frame ascending) while votes >= 5, candidate_num at most.  Per candidate with M pairs: skip_len = M / 50 + 1,
 * hypothesis h from pair h skip_len (h < M / skip_len): the proper rotation maximising tr(R src ref^T) and t = c_ref - R c_src; its vote counts
 * the pairs whose A, B, C all land within 3.0; the best is the first maximum; max vote >= 4: score = the verify score of cloud_cur against the
 * frame's cloud (vxba_loopreg_score's arithmetic, gates normal_threshold / dis_threshold), else -1.  Result: the first candidate of strictly
 * greatest score, if that score exceeds max(icp_threshold, 0); else frame -1.
 * Deterministic: integer atomics only (votes); the match list is written in its order, never in arrival order. */
typedef struct vxba_loopsearch vxba_loopsearch;
typedef struct vxba_loopsearch_params {      /* BTC.cpp:22-34 */
  int descriptor_near_num;      /* 15; 3..32 */
  double descriptor_min_len;    /* 2 */
  double descriptor_max_len;    /* 50 */
  double std_side_resolution;   /* 0.2 */
  int skip_near_num;            /* 30; may be negative (voxelslam.cpp:401) */
  int candidate_num;            /* 20; 1..64 */
  double rough_dis_threshold;   /* 0.01 */
  double similarity_threshold;  /* 0.7 */
  double icp_threshold;         /* 0.15 */
  double normal_threshold;      /* 0.2 */
  double dis_threshold;         /* 0.5 */
} vxba_loopsearch_params;
#define VXBA_LOOPSEARCH_MAX_CORNERS 2048
#define VXBA_LOOPSEARCH_MAX_HYPOTHESES 50
#define VXBA_LOOPSEARCH_CAND_INTS 7      /* frame, votes, pairs, hypotheses tried, best hypothesis, max vote, useful */
#define VXBA_LOOPSEARCH_CAND_DOUBLES 13  /* score, pose[12] of the best hypothesis */
/* Attaches to the registration handle whose plane clouds the score reads and whose stream it shares.  vxba_loopreg_clear on that handle kills
 * the clouds the frames are bound to: every later search returns VXBA_ERR_STATE until vxba_loopsearch_clear.  Destroy the search handle before
 * the registration handle. */
int vxba_loopsearch_create(int device, vxba_loopreg* clouds, vxba_loopsearch** out);
int vxba_loopsearch_destroy(vxba_loopsearch* h);
const char* vxba_loopsearch_last_error(const vxba_loopsearch* h);
int vxba_loopsearch_clear(vxba_loopsearch* h); /* forget the database and the current set; frames count from 0 again */
int vxba_loopsearch_num_frames(const vxba_loopsearch* h);
/* which >= 0: descriptors of that frame (-1 when out of range); -1: of the whole database; -2: of the current set */
int64_t vxba_loopsearch_num_descriptors(const vxba_loopsearch* h, int which);
void vxba_loopsearch_default_params(vxba_loopsearch_params* p);
/* The current keyframe's descriptors, built on the device: locations n x 3, occupancy n words.  params NULL: defaults (no sentinel inside the
 * struct means "default": skip_near_num is meaningful when negative).  VXBA_ERR_ARG, nothing launched, current set and database untouched: a
 * location that is not finite, n > VXBA_LOOPSEARCH_MAX_CORNERS, descriptor_near_num outside 3..32, descriptor_min_len / std_side_resolution
 * < 2 (the truncations above need positive cells), descriptor_max_len outside (min_len, 2000], candidate_num outside 1..64.  An occupancy is one
 * 64-bit word per corner (the reference's columns hold 50 cells); a longer one cannot be passed, and the Python mirror turns it away as VXBA_ERR_ARG. */
int vxba_loopsearch_describe(vxba_loopsearch* h, int64_t n, const double* locations, const uint64_t* occupancy, const vxba_loopsearch_params* params, int64_t* n_descriptors);
/* Inspection of the current set: triangle nd x 3, centre nd x 3, the corner indices of A, B, C nd x 3 (any may be NULL). */
int vxba_loopsearch_read_descriptors(vxba_loopsearch* h, double* triangle, double* centre, int32_t* corners);
/* The current set against the database.  cloud_cur: the current keyframe's plane cloud in the registration handle.  frame: the matched frame
 * or -1; score and pose (maps current-frame coordinates into the matched frame: vxba_loopreg_icp's hypothesis) are set when frame >= 0.
 * n_candidates and the table (candidate_num rows of VXBA_LOOPSEARCH_CAND_INTS / _DOUBLES; any of the three may be NULL) describe every
 * candidate verified.  The number of launches and host synchronisations does not depend on the database, the matches or the candidates.
 * A cloud id out of range or bad params (as describe): VXBA_ERR_ARG, nothing launched. */
int vxba_loopsearch_search(vxba_loopsearch* h, int cloud_cur, const vxba_loopsearch_params* params, int* frame, double* score, double pose[12],
                           int* n_candidates, int64_t* cand_ints, double* cand_doubles);
/* The ordered match list of the last search: rows (query descriptor, frame, index within the frame), at most capacity of them written;
 * *n the length of the list. */
int vxba_loopsearch_read_matches(vxba_loopsearch* h, int64_t capacity, int32_t* rows, int64_t* n);
/* The current set becomes the next frame, bound to plane cloud cloud_id of the registration handle; work and device bytes proportional to
 * the set (the cell table doubles now and then).  The current set stays current.  A cloud id out of range: VXBA_ERR_ARG, nothing changed. */
int vxba_loopsearch_add(vxba_loopsearch* h, int cloud_id);
/* [launches, host synchronisations] of the last search (a library sort or scan counts as one launch), frames, descriptors in the database,
 * device bytes of the frames' records, device bytes of the cell table. */
int vxba_loopsearch_stats(const vxba_loopsearch* h, int64_t out[6]);

/* ---- loop search over several sessions ------------------------------------------------------------------
 * The reference keeps one STDescManager per session (loaded by previous_map_read or opened by system_reset) and searches all of them for
 * every keyframe (voxelslam.cpp:1987-1989).  Here that loop is ONE search: cur holds the current set (vxba_loopsearch_describe), dbs[s] are
 * the sessions' handles -- all attached to cur's registration handle; cur may be among them -- and skip_near_num[s] takes the place of
 * params->skip_near_num for session s (the reference sets it per manager, voxelslam.cpp:401, 1869).  The query's frame number is
 * vxba_loopsearch_num_frames(cur) in every session (BTC.cpp:195 stamps the descriptors with the current manager's frame id, :1184-1186 compare
 * it with the searched manager's entries): entry j of session s is eligible when num_frames(cur) - frame_j > skip_near_num[s].  Everything else
 * is vxba_loopsearch_search's arithmetic, applied per session.
 *   Row s of every output -- frame[s], score[s], pose + 12 s, n_candidates[s], the candidate_num table rows from s candidate_num on -- is, integers
 *   equal and doubles bit for bit, what vxba_loopsearch_search returns on dbs[s] holding the same current set with
 *   skip_near_num = skip_near_num[s] - (num_frames(cur) - num_frames(dbs[s])).  score, pose, n_candidates and the tables may be NULL.
 *   The launches and host synchronisations (vxba_loopsearch_stats(cur)) are those of one single search, whatever S, the databases, the matches
 *   and the candidates; the sessions' table goes to the device in one pinned copy and every result comes back in one.
 *   vxba_loopsearch_read_matches(cur, ...) afterwards returns the lists of the sessions one after the other, session 0 first, each in the
 *   single search's order; the frame column holds vote offset of the session + frame, the vote offset being the number of frames of the
 *   sessions before it in dbs.  vxba_loopsearch_read_match_offsets: out[s] = where session s's list starts, out[S] = the length (S + 1 values;
 *   VXBA_ERR_STATE when the handle's last search was a single one).
 *   An empty current set, or S databases without a frame: every frame -1, score 0, n_candidates 0, nothing launched.
 *   VXBA_ERR_ARG, nothing launched, no handle touched: S outside 1..VXBA_LOOPSEARCH_MAX_SESSIONS, a NULL handle, a handle on another device or
 *   attached to another registration handle than cur's, cloud_cur out of range, bad params (as describe).  VXBA_ERR_STATE: a session that holds
 *   frames from before a vxba_loopreg_clear.
 * What the host policy on top of this (voxel_slam_amd/multisession.py, thd_loop_closure :1856-2129) keeps of the reference's quirks: a session's
 * first contact with another (no edge between the two yet) is pushed and optimised whatever its drift; relc_counts are incremented for every
 * session on every keyframe, found or not; a drift over a zero journey divides by zero as IEEE says (inf or NaN, the test then fails as the
 * reference's does); the running graph keeps the chain measured at push time while build_graph re-derives it from the current poses. */
#define VXBA_LOOPSEARCH_MAX_SESSIONS 16
int vxba_loopsearch_search_multi(vxba_loopsearch* cur, int S, vxba_loopsearch* const* dbs, const int* skip_near_num, int cloud_cur,
                                 const vxba_loopsearch_params* params, int* frame, double* score, double* pose, int* n_candidates, int64_t* cand_ints,
                                 double* cand_doubles);
int vxba_loopsearch_read_match_offsets(vxba_loopsearch* cur, int64_t* out);

/* ---- keyframes: marginalised scans -> the clouds of the loop chain and of the hierarchical BA ----------------------------------
 * The front half of thd_loop_closure (voxelslam.cpp:1898-1977): the ScanPose buffer (bl_local), the keyframe rule (:1928-1942), the merge of
 * win_size scans into the NEWEST pose's frame (:1944-1955) and down_sampling_pvec(voxel_size / 10) (:1965, voxel_map.hpp:24-65).  The handle keeps
 * the buffered scans on the device -- body points n x 3 float64 and the diagonal of every point's covariance, the only part of `var` that is ever
 * read.  A push applies the rule:
 *   x_key = xc when buf_base == 0; buf_base++; nothing further while fewer than win_size scans are buffered;
 *   ang = |Log(x_key.R^T xc.R)| * 57.3, len = |xc.p - x_key.p|;
 *   ang < ang_deg and len < len and buf_base > win_size: the OLDEST buffered scan is dropped, no keyframe;
 *   otherwise jour += len, x_key = xc and a keyframe is emitted with id = buf_base - 1 and pose xc; all win_size buffered scans are consumed.
 * A keyframe, N = the buffered scans' points, oldest scan first, point order kept:
 *   q = delta_R pnt + delta_p with delta_R = xc.R^T bl.R, delta_p = xc.R^T (bl.p - xc.p) in float64 (computed for the newest scan as well),
 *   every inner product (a0 b0 + a1 b1) + a2 b2, the translation added last; the covariances are carried over UNROTATED, as upstream does;
 *   full  N x 3 float32: q rounded (`plbtc`, :1967-1974) -- what vxba_loopreg_add_keyframe_device takes;
 *   down  n_down x 6 float32 (x, y, z, var00, var11, var22: the fields PointType carries, voxel_map.hpp:58-61): per occupied voxel of edge
 *         voxel_size / 10 the running mean m = (m c + v) / (c + 1) of its points in input order, in float64, unfused, bit-identical to
 *         upstream's; voxel index per axis: float l = q / vs; if (l < 0) l -= 1.0; (int64_t)l, |index| < 2^20.  Rows ascend by voxel index,
 *         lexicographic in (x, y, z) (upstream: unordered_map iteration order).  Its xyz columns are what vxba_hba_add_keyframes_device takes.
 * An emitting push enqueues a fixed number of launches and waits for the device once, whatever N (vxba_keyframe_stats).
 * VXBA_ERR_ARG -- the push undone: buffer, buf_base, x_key, jour and the scan list as before, the previous keyframe still readable -- for a body
 * coordinate that is not finite (any push) and for a merged coordinate that is not finite or whose voxel index is not inside (-2^20, 2^20)
 * (an emitting push; it concerns every buffered scan). */
typedef struct vxba_keyframe vxba_keyframe;
typedef struct vxba_keyframe_params {
  int win_size;       /* scans per keyframe; <= 0: 10 (at most 64) */
  double voxel_size;  /* the map's voxel size; the filter runs at voxel_size / 10; <= 0: 1.0 */
  double ang_deg;     /* <= 0: 5    (:1934) */
  double len;         /* <= 0: 0.1  (:1934) */
} vxba_keyframe_params;
int vxba_keyframe_create(int device, const vxba_keyframe_params* params /* may be NULL */, vxba_keyframe** out);
int vxba_keyframe_destroy(vxba_keyframe* h);
const char* vxba_keyframe_last_error(const vxba_keyframe* h);
/* The reset_flag branch (:1856-1887): empty buffer, buf_base 0, jour 0, no scan poses, no keyframe to read.  Device buffers are kept. */
int vxba_keyframe_clear(vxba_keyframe* h);
/* One ScanPose: pose [R column-major 9 | t 3], v6 (its pose variances, kept for the odometry chain), n body points n x 3 and their covariances
 * n x 9 column-major (NULL: zeros); n may be 0.  *emitted: 1 when this push made a keyframe. */
int vxba_keyframe_push_scan(vxba_keyframe* h, const double pose[12], const double v6[6], int64_t n, const double* pnt_body, const double* var, int* emitted);
/* The same with pnt_body and var in device memory (pose and v6 on the host); the result is byte-identical. */
int vxba_keyframe_push_scan_device(vxba_keyframe* h, const double pose[12], const double v6[6], int64_t n, const double* d_pnt_body, const double* d_var, int* emitted);
/* The last keyframe (any output may be NULL); VXBA_ERR_STATE before the first one. */
int vxba_keyframe_info(const vxba_keyframe* h, int64_t* id, double pose[12], double* jour, int64_t* n_full, int64_t* n_down);
int vxba_keyframe_read(vxba_keyframe* h, float* full_xyz /* n_full x 3 */, float* down_xyzv /* n_down x 6 */);
/* Device addresses of the two clouds (NULL for an empty one): valid until the next emitting push. */
int vxba_keyframe_device(const vxba_keyframe* h, const float** d_full, const float** d_down);
/* The xyz columns of `down` packed n_down x 3 (the layout vxba_hba_add_keyframes_device takes); same lifetime. */
int vxba_keyframe_device_down_xyz(const vxba_keyframe* h, const float** d_down_xyz);
/* Every ScanPose pushed since clear -- dropped ones included, like upstream's scanPoses: what the odometry chain of the pose graph is built
 * from (:1909-1921). */
int64_t vxba_keyframe_num_scans(const vxba_keyframe* h);
int vxba_keyframe_num_buffered(const vxba_keyframe* h); /* scans waiting in the buffer (bl_local.size()): 0 .. win_size - 1 between pushes */
int vxba_keyframe_scan_poses(const vxba_keyframe* h, int64_t first, int64_t count, double* poses /* count x 12 */, double* v6 /* count x 6 */);
/* [launches (a library sort, encode or scan counts as one), host waits, bytes device -> host, bytes host -> device] of the last push. */
int vxba_keyframe_stats(const vxba_keyframe* h, int64_t out[4]);
/* Measurement: with enable != 0 an emitting push records events between its stages (no extra wait); the times [ms] of the last one:
 * [assembly, sort + run-length encode + scan, filter].  VXBA_ERR_STATE when the last emitting push was not profiled or held no points. */
int vxba_keyframe_set_profiling(vxba_keyframe* h, int enable);
int vxba_keyframe_stage_times(vxba_keyframe* h, double ms[3]);

/* Device-pointer variants of two keyframe consumers, byte-identical to the host routes: the cloud of vxba_loopreg_add_keyframe as float32 in
 * device memory (widened exactly to float64), and the clouds of vxba_hba_add_keyframes in device memory (cloud_ptr stays on the host). */
int vxba_loopreg_add_keyframe_device(vxba_loopreg* h, int64_t n_points, const float* d_xyz, const vxba_planecloud_params* params, int* id, int64_t* n_planes);
int vxba_hba_add_keyframes_device(vxba_hba* h, int64_t n_keyframes, const int64_t* cloud_ptr, const float* d_xyz);

/* ---- corners: a keyframe's cloud -> the corner set of the loop search ---------------------------------------------------------------
 * STDescManager::GenerateSTDescs without its last step (generate_std = vxba_loopsearch_describe): init_voxel_map / init_plane, get_project_plane,
 * merge_plane, binary_extractor, extract_binary, non_maxi_suppression (BTC.cpp:90-139, 156-186, 279-321, 340-977).  All float64, every inner
 * product (a0 b0 + a1 b1) + a2 b2, nothing fused.  Where the reference leaves a choice open it is fixed here:
 * 1 plane records: voxel index per axis as vxba_loopreg_add_keyframe (divide by voxel_size, subtract 1.0 where negative, truncate, |index| < 2^20);
 *   per voxel with N > voxel_init_num the sums of p and p p^T in input order, c = sum / N, cov = sum pp^T / N - c c^T, a symmetric eigen-solve; a
 *   plane iff lambda_min < plane_detection_thre.  Record (VXBA_CORNER_REC doubles): [c 3 | cov xx xy xz yy yz zz | N | normal 3 | d = -n.c |
 *   radius = sqrt(lambda_max) | lambda_min].  Rows ascend by voxel coordinate, lexicographic in (x, y, z) (the reference: unordered_map order).  The
 *   normal's component of largest magnitude (the first of equals) is positive.  The sign MATTERS here, unlike in the registration: a flipped
 *   normal flips y_axis and re-anchors the image at its other edge, so other cells, other corners.
 * 2 get_project_plane over that list: the pair test (|n_a - n_b| or |n_a + n_b| < plane_merge_normal_thre, |n_a.c_b + d_a| and |n_b.c_a + d_b| <
 *   plane_merge_dis_thre) and the reference's SEQUENTIAL labelling -- outer index from the last row down to 1, inner from 0 to outer - 1; both
 *   unlabelled: a fresh id; one unlabelled: it takes the other's; both labelled: nothing -- which is not connected components.  Groups in
 *   ascending first row fold every other member (ascending) by the reference's update of (cov, c, N) and are solved once at the end (the same
 *   sign rule); unlabelled rows are dropped.
 * 3 a STABLE sort by N descending, merge_plane (a list of one passes through; else the same labelling, unlabelled rows kept at their position,
 *   groups at their first member's), the same sort again.  An empty list: the fallback plane, normal (0, 0, 1) through the cloud's first point.
 * 4 the gate of binary_extractor: last = 0; a plane is used when |n - last| < 0.3 or |n + last| > 0.3, then last = n; proj_plane_num at most.
 * 5 extract_binary per used plane: x_axis from (1, 1, -(A+B)/C) with its two fall-backs, y_axis = n x x_axis; dis = |((xA + yB) + zC) + D|, kept
 *   iff proj_dis_min <= dis <= proj_dis_max; project_x along Y_AXIS and project_y along x_axis of the foot point; min_x = min(10, min px),
 *   max_x = max(-10, max px), likewise y; five or fewer kept points: no corner from this plane; per cell, in input order: count, sum px, sum py,
 *   bit (int)((dis - dis_min) / high_inc) -- a bit index that reaches cut_num = (int)((dis_max - dis_min) / high_inc), i.e. dis = dis_max, counts
 *   for the cell and sets NO bit (the reference writes out of bounds).  Per 5 x 5 segment, x outermost: the first cell of strictly greatest
 *   summary; kept when summary >= summary_min_thre, with the touch filter any of bits 0..3, not on the image border, and not a line (:860-890,
 *   an empty cell reads 0).  Location = py x_axis + px y_axis + centre, px = sum px / count.  Order (plane, segment x, segment y).
 * 6 non_maxi_suppression over all candidates: locations rounded to float32; j near i when (dx dx + dy dy) + dz dz < float32(radius^2), strict;
 *   i is dropped when a near j != i has summary_j >= summary_i (equal neighbours drop each other).
 * 7 useful_corner_num > count: everything in order; else a stable sort by summary descending and the first useful_corner_num.
 * Launches and host waits depend on the entry point only, never on n, the planes, the cells or the candidates (vxba_corner_stats).  The
 * labelling, the folds of the groups and the final cut run on the host from the downloaded bit matrix / candidate list.  Bounds: at most
 * VXBA_CORNER_MAX_PLANES plane voxels (VXBA_ERR_ARG), at most VXBA_CORNER_MAX_CANDIDATES candidates ahead of the suppression
 * (VXBA_ERR_UNSUPPORTED), n <= 2^28.
 * VXBA_ERR_ARG -- the previous result still readable, and nothing launched on the host routes: a coordinate that is not finite or a voxel index
 * outside (-2^20, 2^20) (the device route finds it in its first kernel); cut_num outside 4..64; a resolution, increment, voxel size or radius
 * <= 0; proj_dis_max <= proj_dis_min; proj_plane_num outside 1..8; useful_corner_num outside 1..VXBA_LOOPSEARCH_MAX_CORNERS; an image axis of
 * 2^24 cells or more (found after the projection).  n == 0: VXBA_OK and zero corners. */
typedef struct vxba_corner vxba_corner;
typedef struct vxba_corner_params {      /* read_parameters, BTC.cpp:7-20, 25 | 39-52, 57: normal | high-fly */
  int useful_corner_num;              /* 100 | 200 */
  double plane_merge_normal_thre;     /* 0.1 | 0.3 */
  double plane_merge_dis_thre;        /* 0.3 | 0.6 */
  double plane_detection_thre;        /* 0.01 | 0.05 */
  double voxel_size;                  /* 1 | 2 */
  int voxel_init_num;                 /* 10 | 10 */
  int proj_plane_num;                 /* 2 | 1 */
  double proj_image_resolution;       /* 0.5 | 0.5 */
  double proj_image_high_inc;         /* 0.1 | 0.2 */
  double proj_dis_min;                /* 0 | 0 */
  double proj_dis_max;                /* 5 | 10 */
  double summary_min_thre;            /* 10 | 6 */
  int line_filter_enable;             /* 1 | 0 */
  int touch_filter_enable;            /* 0 | 0 */
  double non_max_suppression_radius;  /* 2 | 3 */
} vxba_corner_params;
#define VXBA_CORNER_REC 16
#define VXBA_CORNER_MAX_PLANES 16384
#define VXBA_CORNER_MAX_CANDIDATES 65536
#define VXBA_CORNER_CAND_INTS 6      /* plane (position among the used), cell x, cell y, count, summary, kept by the suppression */
#define VXBA_CORNER_STAGES 6         /* plane records | pair tests | pair tests of the merged list | projection, bounds, keys | sort, encode, scan | cells .. suppression */
/* No sentinel inside the struct means "default"; params NULL: the normal preset. */
void vxba_corner_default_params(vxba_corner_params* p, int is_high_fly);
int vxba_corner_create(int device, vxba_corner** out);
int vxba_corner_destroy(vxba_corner* h);
const char* vxba_corner_last_error(const vxba_corner* h);
/* xyz n x 3 float64 on the host. */
int vxba_corner_extract(vxba_corner* h, int64_t n, const double* xyz, const vxba_corner_params* params, int64_t* n_corners);
/* The keyframe's `full` cloud, n x 3 float32 in device memory, widened exactly: byte-identical to the host route on the same values. */
int vxba_corner_extract_device(vxba_corner* h, int64_t n, const float* d_xyz, const vxba_corner_params* params, int64_t* n_corners);
/* Stages 4-7 on a caller's plane list (m x 3 centres, m x 3 normals, 1 <= m <= VXBA_CORNER_MAX_PLANES, used as they are). */
int vxba_corner_extract_with_planes(vxba_corner* h, int64_t n, const double* xyz, int64_t m, const double* centres, const double* normals, const vxba_corner_params* params,
                                    int64_t* n_corners);
/* The corners of the last extract: locations n x 3, occupancy n words, summary n (any may be NULL). */
int vxba_corner_read(vxba_corner* h, double* locations, uint64_t* occupancy, int32_t* summary);
/* Inspection of the last extract, every output may be NULL (call once for the count).  planes: the records of stage 1 and their labels of
 * stage 2.  projection_planes: the final sorted list of stage 3 (of a fallback or a caller's plane only centre and normal are set) and per row
 * its position among the used planes or -1.  candidates: VXBA_CORNER_CAND_INTS ints, the occupancy word and the location per candidate of stage 5. */
int vxba_corner_planes(vxba_corner* h, int64_t* n_planes, double* records, int32_t* labels);
int vxba_corner_projection_planes(vxba_corner* h, int64_t* n_planes, double* records, int32_t* used);
int vxba_corner_candidates(vxba_corner* h, int64_t* n_candidates, int32_t* ints, uint64_t* occupancy, double* locations);
/* [launches (a library sort, encode or scan counts as one), host waits, bytes device -> host, bytes host -> device, occupied cells of all
 * images, candidates] of the last extract. */
int vxba_corner_stats(const vxba_corner* h, int64_t out[6]);
/* Measurement: events around the stages of an extract (no extra wait); [ms] per stage of the last profiled extract or extract_device. */
int vxba_corner_set_profiling(vxba_corner* h, int enable);
int vxba_corner_stage_times(vxba_corner* h, double ms[VXBA_CORNER_STAGES]);

/* ---- saved sessions: scans and poses of an earlier run -> keyframes, descriptor clouds, the global map ----------------------------------
 * The per-point half of previous_map_read (voxelslam.cpp:307-448) and pub_globalmap (:108-150); the files are read on the host
 * (voxel_slam_amd/sessionio.py).  All pose algebra is the keyframe builder's (delta_R = xc.R^T xj.R, delta_p = xc.R^T (xj.p - xc.p), every inner product
 * (a0 b0 + a1 b1) + a2 b2, the translation added last, nothing fused); every point is float32 between the stages, as PointXYZI / PointType are.
 * Kept as upstream writes it:
 *   - keyframe g is scans [g win_size, (g + 1) win_size); trailing scans that do not fill a group are dropped; its id is the index of the group's
 *     last scan and its pose x0 that scan's pose (:341-346, :368-371); the group's last scan is multiplied by its own xc.R^T xc.R too;
 *   - the filter is down_sampling_voxel(voxel_size / 10) on the merged FLOAT points, the division in double (:362): keyframe k's cloud is bit for
 *     bit what vxba_down_sampling_voxel returns on keyframe k's merged cloud alone, rows ascending by (x, y, z) voxel index; below 0.001 the
 *     merged cloud is returned untouched (tools.hpp:203);
 *   - descriptor windows start at i = 0, mgsize, ... while i + acsize < K -- STRICT: a session of exactly acsize keyframes yields none (:377);
 *     window w merges keyframes [i, i + acsize) into the frame of keyframe i + acsize - 1 under the x0 poses and is stamped with that keyframe's id;
 *   - after an optimisation x0[k] = poses[ids[k]] (kf->x0 = scanPoses[kf->id]->x, :2171-2174): vxba_session_set_scan_poses.
 * vxba_session_build_keyframes enqueues a fixed number of launches whatever the number of points and keyframes and waits for the device once --
 * plus once more when the handle's workspace has to grow over a block it already holds (a larger session loaded into a used handle):
 * vxba_session_stats then reports 2 host waits.
 * VXBA_ERR_ARG with the handle as it was -- scans, keyframes and their clouds still readable -- for offsets that decrease, a pose that is not
 * finite, and (at build time) a merged point that is not finite or whose voxel index lies outside [-2^20, 2^20), which is what
 * vxba_down_sampling_voxel refuses. */
typedef struct vxba_session vxba_session;
int vxba_session_create(int device, vxba_session** out);
int vxba_session_destroy(vxba_session* h);
const char* vxba_session_last_error(const vxba_session* h);
int vxba_session_clear(vxba_session* h); /* no scans, no keyframes; device buffers are kept */
/* Every saved scan, once: scan_ptr n_scans + 1 host offsets (points) into xyz (host, float32, body frame), poses n_scans x 12.  Replaces what
 * the handle held; its keyframes are gone. */
int vxba_session_load_scans(vxba_session* h, int64_t n_scans, const int64_t* scan_ptr, const float* xyz, const double* poses);
int64_t vxba_session_num_scans(const vxba_session* h);
int vxba_session_build_keyframes(vxba_session* h, int win_size, double voxel_size, int64_t* n_keyframes);
int64_t vxba_session_num_keyframes(const vxba_session* h);
/* kf_ptr: K + 1 offsets (points) into the packed clouds; ids: the scan index per keyframe; poses: x0, K x 12.  Any of them may be NULL. */
int vxba_session_keyframes(const vxba_session* h, int64_t* kf_ptr, int64_t* ids, double* poses);
int vxba_session_read_keyframes(vxba_session* h, float* xyz /* kf_ptr[K] x 3 */);
/* The packed clouds in device memory (NULL when they hold no point), valid until the next build: with kf_ptr exactly what
 * vxba_hba_add_keyframes_device takes. */
int vxba_session_device(const vxba_session* h, const float** d_xyz);
int vxba_session_set_scan_poses(vxba_session* h, const double* poses /* n_scans x 12 */);
int vxba_session_num_windows(int64_t n_keyframes, int acsize, int mgsize);
/* One launch into a buffer the handle owns: *d_xyz (n x 3 float32, NULL when n = 0) stays valid until the next call; the device has finished when
 * the call returns.  What vxba_corner_extract_device and vxba_loopreg_add_keyframe_device take. */
int vxba_session_window_cloud(vxba_session* h, int w, int acsize, int mgsize, int64_t* n, const float** d_xyz, int64_t* frame_id);
int vxba_session_read_window(vxba_session* h, float* xyz /* n x 3 of the last window_cloud */);
/* [launches (a library sort or scan counts as one), host waits] of the last build_keyframes / window_cloud, points loaded, keyframes. */
int vxba_session_stats(const vxba_session* h, int64_t out[4]);
/* Measurement: with enable != 0 a build records events between its stages (no extra wait); the times [ms] of the last one: [merge, the two sorts
 * + run heads + scan + tables, running means].  VXBA_ERR_STATE when the last build was not profiled, held no point or ran without the filter. */
int vxba_session_set_profiling(vxba_session* h, int enable);
int vxba_session_stage_times(vxba_session* h, double ms[3]);
/* pub_globalmap over n_sets sets of keyframe clouds, in the order given.  Set s: d_xyz[s] packed float32 clouds in device memory, cloud_ptr[s]
 * n_keyframes[s] + 1 host offsets (points) into it, poses[s] n_keyframes[s] x 12 on the host, intensity[s] the session id written into every
 * point.  psize = the sum of all clouds, jump = psize / (10 interval_size) + 1; keyframe k contributes its points 0, jump, 2 jump, ... each as
 * float(R double(v) + p).  THE ONE DEVIATION: psize and jump are 64-bit; upstream's `uint psize` wraps beyond 4.29e9 points.  out_xyzi: host,
 * *n_out x 4 float32.  chunk_ptr (NULL, or room for the number of keyframes + 2) records upstream's flush rule: after a keyframe, when more than
 * interval_size points are pending, a chunk ends (:141-146); the last chunk ends at *n_out and may be empty, like upstream's last publish.
 * One launch: one lane per output point, the owning keyframe by binary search.  capacity < the number of output points: VXBA_ERR_ARG with the
 * exact count in *n_out and nothing written. */
int vxba_globalmap(int device, int n_sets, const float* const* d_xyz, const int64_t* const* cloud_ptr, const int64_t* n_keyframes, const double* const* poses,
                   const float* intensity, int64_t interval_size, float* out_xyzi, int64_t capacity, int64_t* n_out, int64_t* chunk_ptr, int64_t* n_chunks);
/* The running session's keyframes as a set of vxba_globalmap: the device clouds and the host offsets of a vxba_hba handle, read-only, valid until
 * its next add_keyframes / clear. */
int vxba_hba_device_clouds(const vxba_hba* h, const float** d_xyz, const int64_t** cloud_ptr, int64_t* n_keyframes);

/* ---- loop hand-back: the running session's keyframes on the device, back into the local map ------------------------------------------------
 * The reference's `keyframes` vector of the running session and the three places that turn its clouds into world-frame FIXED points of the local
 * map: keyframe_loading (voxelslam.cpp:1189-1228), the map_loop build behind an optimisation (:2103, :2114-2119, :2131-2167) and the buffered
 * scans of loop_update (:1161-1168).  A keyframe is its `down` cloud as vxba_keyframe_device hands it out -- n x 6 float32: x, y, z, var00, var11,
 * var22 (the variances down_sampling_pvec leaves in the `normal` fields) -- its id (the index of its ScanPose), its pose x0, its journey and its
 * `exist` flag.  The clouds live in one packed store on the device that grows geometrically; offsets, ids, x0, jour and exist live on the host.
 * One kernel serves all three consumers, ONE launch and one host wait per call whatever the number of keyframes and points (vxba_kfarchive_stats):
 *   q = x0.R double(v) + x0.p in float64, every inner product (a0 b0 + a1 b1) + a2 b2, the translation added last, nothing fused;
 *   var = diag(double(var00), double(var11), double(var22)) and zero elsewhere for map_loop, NULL for load_near.
 * Quirks kept as upstream writes them:
 *   - the variances are NOT rotated although the frame changes (:2145-2146, and :1164-1166 for a buffered scan's full 3 x 3);
 *   - map_loop with cumulative != 0: `pvec_tem` is never cleared (:2131), so cloud c holds the points of keyframes first .. first + c and the first
 *     keyframe enters the map init_num times; cumulative == 0 gives one cloud per keyframe;
 *   - the radius search reads a float32 SNAPSHOT of the positions taken when the history was armed (`pl_kdmap`, :2154-2163) while the transform
 *     reads the current x0: a vxba_kfarchive_set_poses after arming moves the clouds and not the search;
 *   - a keyframe within the radius whose flag is clear is skipped and does not end the walk (:1201-1226); one keyframe per call.
 * Fixed here where the reference leaves it open (FLANN's radiusSearch, sorted): distances are float32 between float(p_curr) and the snapshot,
 * (dx dx + dy dy) + dz dz, unfused; candidates have d2 < float(radius radius); ascending d2, ties broken by the LOWEST index.  The boundary
 * d2 == r2 (strict < here) is UNVERIFIED against PCL.
 * VXBA_ERR_ARG leaves the archive exactly as it was: a pose (add, set_poses, a buffered scan) or a query that is not finite, an index out of range,
 * init_num above 64, more than 1024 buffered scans, more than 2^30 - 1 points in one keyframe or one call's output.  The points themselves are not
 * inspected: what the keyframe builder emitted is finite. */
typedef struct vxba_kfarchive vxba_kfarchive;
int vxba_kfarchive_create(int device, vxba_kfarchive** out);
int vxba_kfarchive_destroy(vxba_kfarchive* h);
const char* vxba_kfarchive_last_error(const vxba_kfarchive* h);
/* The reset_flag branch / system_reset: no keyframes, no history.  Device buffers are kept. */
int vxba_kfarchive_clear(vxba_kfarchive* h);
/* A new keyframe at the end: exist = 0 (Keyframe's constructor), n may be 0.  down_xyzv n x 6 float32 on the host; the _device variant copies device
 * to device without host staging (the source is the caller's again when the call returns).  Both give byte-identical stores. */
int vxba_kfarchive_add(vxba_kfarchive* h, int64_t id, const double pose[12], double jour, int64_t n, const float* down_xyzv);
int vxba_kfarchive_add_device(vxba_kfarchive* h, int64_t id, const double pose[12], double jour, int64_t n, const float* d_down_xyzv);
int64_t vxba_kfarchive_num(const vxba_kfarchive* h);
int vxba_kfarchive_info(const vxba_kfarchive* h, int64_t k, int64_t* id, double pose[12], double* jour, int64_t* n, int* exist); /* outputs may be NULL */
int vxba_kfarchive_read(vxba_kfarchive* h, int64_t k, float* out /* n x 6 */);
/* The packed store (NULL while it holds no point) and the K + 1 host offsets (points) into it: read-only, valid until the next add / clear / destroy. */
int vxba_kfarchive_device(const vxba_kfarchive* h, const float** d_xyzv, const int64_t** cloud_ptr);
/* kf->x0 = scanPoses[kf->id]->x (:2114-2119): x0 K x 12, row k the new pose of keyframe k -- the caller indexes its scan poses by id. */
int vxba_kfarchive_set_poses(vxba_kfarchive* h, const double* x0);
/* :2103, :2132-2167 (init_num <= 0: 5).  The last init_num keyframes get exist = 0.  K > init_num: keyframes [0, K - init_num) get exist = 1, their
 * positions are snapshotted as float32 and history_kfsize = K - init_num; otherwise history_kfsize = 0 (and every call of load_near does nothing). */
int vxba_kfarchive_arm_history(vxba_kfarchive* h, int init_num);
int64_t vxba_kfarchive_history_size(const vxba_kfarchive* h);
/* keyframe_loading (:1191-1226; radius <= 0: 10).  Nothing happens while history_kfsize <= 0.  The first candidate (order above) whose exist is set
 * is loaded: it gets exist = 0, history_kfsize--, *k_loaded its index, *n its points and *d_pnt_world their world coordinates n x 3 float64 in
 * device memory (NULL when n = 0) -- pass them to vxba_map_cut_voxel_fix_device with d_var = NULL (zero variances, :1210).  Nothing qualifies:
 * *k_loaded = -1, *n = 0.  The device has finished when the call returns; the pointer stays valid until the next load_near / map_loop*. */
int vxba_kfarchive_load_near(vxba_kfarchive* h, const double p_curr[3], double radius, int* k_loaded, int64_t* n, const double** d_pnt_world);
/* The map_loop build (:2131-2150; init_num <= 0: 5): keyframes max(0, K - init_num) .. K - 1 in world coordinates as *n_clouds clouds, cloud c =
 * points cloud_ptr[c] .. cloud_ptr[c + 1] (cloud_ptr: room for init_num + 1) of *d_pnt_world (x 3) / *d_var (x 9, all nine written) -- what
 * vxba_map_loop_update_device takes.  Same completion and lifetime as load_near.  No keyframe or no point: *n_clouds as counted, NULL pointers. */
int vxba_kfarchive_map_loop(vxba_kfarchive* h, int init_num, int cumulative, int64_t* cloud_ptr, int* n_clouds, const double** d_pnt_world, const double** d_var);
/* The same followed by loop_update's buffered scans (`buf_lba2loop`, :1161-1168) as n_pending further clouds, one per scan, in the SAME launch:
 * scan i = pending_n[i] body points d_pending_pnt[i] (n x 3 float64, device) under pending_poses[i] (already updated by dx), its variances
 * d_pending_var[i] (n x 9 float64, device; the array or an entry may be NULL: zeros) carried over unrotated.  cloud_ptr: room for init_num + n_pending + 1. */
int vxba_kfarchive_map_loop_scans(vxba_kfarchive* h, int init_num, int cumulative, int n_pending, const double* pending_poses, const int64_t* pending_n,
                                  const double* const* d_pending_pnt, const double* const* d_pending_var, int64_t* cloud_ptr, int* n_clouds, const double** d_pnt_world,
                                  const double** d_var);
/* [launches, host waits, bytes device -> host, bytes host -> device] of the last add* / load_near / map_loop*. */
int vxba_kfarchive_stats(const vxba_kfarchive* h, int64_t out[4]);

/* ---- measurement --------------------------------------------------------------------------------- */
/* The cluster-build kernel inside the voxeliser (vxba_voxelize_push*, vxba_hba_pass) -- the dominant kernel of a hierarchical-BA pass.
 * enable != 0: start a fresh measurement (every launch bracketed by events bound to its dispatch, one stream synchronisation per layer:
 * not for timed runs); enable == 0: stop and return the sums -- duration [ms], launches, algorithmic bytes (24 B per point + 8 B per
 * cell offset read, 80 B per cluster written). */
int vxba_voxelize_profile(int enable, double* ms_sum, long long* launches, double* algorithmic_bytes);
/* Bit mask of kernels to bracket with hipEvents on the launch stream: 1 = Hessian sweep (K3), 2 = residual sweep (K2),
 * 4 = K3 cross-block reduction, 8 = cluster build (K1), 16 = the all-reduce of a sharded factor, 32 = the fused solve + residual + Hessian
 * launch (VXBA_OPT_FUSED_SWEEPS); 0 = off. */
int vxba_set_profiling(vxba_factor* f, int mask);
/* Sum of kernel durations [ms] and launch counts since the last reset: index 0 = Hessian sweep (K3),
 * 1 = residual sweep (K2), 2 = K3 cross-block reduction, 3 = cluster build (K1). */
int vxba_get_kernel_times(vxba_factor* f, double ms_sum[4], int64_t calls[4], int reset);
/* Voxel-sharded factors (vxba_peer_*, vxba_rccl_*, vxba_set_allreduce): with bit 16 of the profiling mask set every all-reduce of the
 * packed [Hess | JacT | residual] buffer (the exchange step of the reference's thread fan-in, voxel_map.hpp:323-332, across GPUs) is
 * bracketed with hipEvents on the factor's stream; sum [ms] and count since the last reset.  The interval includes the wait for the
 * slowest peer. */
int vxba_get_collective_time(vxba_factor* f, double* ms_sum, int64_t* calls, int reset);
/* The fused launch of VXBA_OPT_FUSED_SWEEPS (in-launch solve, then evaluate_only_residual and acc_evaluate2 at the trial poses, voxel_map.hpp:132-279)
 * bracketed while bit 32 of the profiling mask was set: sum of launch durations [ms] and count since the last reset. */
int vxba_get_fused_time(vxba_factor* f, double* ms_sum, int64_t* calls, int reset);
/* Algorithmic bytes of one full sweep over the current factor: 0 = K3, 1 = K2. */
int vxba_algorithmic_bytes(const vxba_factor* f, double bytes[2]);
int vxba_nnz(vxba_factor* f, int64_t* nnz);
/* Device memory the factor holds right now, in bytes: [0] the factor itself (cluster storage -- frame-major planes, or the compressed
 * rows of a window wider than VXBA_MAX_WIN -- per-voxel planes, batch-major copy, the f32 cluster copy of VXBA_PRECISION_MIXED_F32_CLUSTERS, cache snapshot), [1] sweep work space (block
 * partials, packed system; for wide windows the pair index, the row buffer and the dense solver), [2] grow-only staging / scratch
 * left behind by the push calls, [3] the sum. */
int vxba_device_bytes(const vxba_factor* f, int64_t bytes[4]);

/* Debug: D(16x16, row-major) = A(16x4) B(4x16) through one v_mfma_f64_16x16x4_f64 with the lane maps the Hessian
 * kernel relies on (unit-tested on the GPU so a wrong operand layout is caught in isolation). */
int vxba_debug_mfma_probe(int device, const double* A16x4, const double* B4x16, double* D16x16);
/* test access to the structured solve of the LiDAR-inertial system (host code, no GPU needed): A is m x m (full symmetric storage),
 * m = lead_y + 15 nframes + tail_x, laid out [lead velocity/bias unknowns | nframes x (rot 3, pos 3, v 3, bg 3, ba 3) | tail]; solves A x = b.
 * Returns VXBA_ERR_STATE when the banded part is not positive definite (the library then falls back to the dense pivoted LDL^T). */
int vxba_debug_band_schur(int m, const double* A, const double* b, int nframes, int lead_y, int tail_x, double* x);

/* Test access to the damped LM solves, one system at a time.  All three are synchronous, allocate and free their own buffers and can be
 * called any number of times in one process; none of them touches a factor.
 *
 * vxba_debug_lm_solve: the four-wave blocked LDL^T of windows up to VXBA_MAX_WIN (1 <= W <= 10) in a launch of its own.  Hwork: (6W)^2 doubles,
 * column-major with stride 6W, the gauge-fixed Hessian as the LM state keeps it; Jwork: 6W; Rp: 12W current poses (may be NULL with li_rec);
 * c: control slot 0 / 1; done: the slot's "loop left" flag.  The LM state is built on the host from these and copied to the device; every
 * other byte of it holds the quiet NaN VXBA_DEBUG_NAN_BITS, so a read of a field the solve has no business with shows in the result, and
 * with done != 0 the outputs come back as that sentinel.  li_rec == NULL: the production stand-alone kernel.  li_rec != NULL: the
 * LiDAR-inertial form (reduced pose system) -- li_rec = [u | current poses 12W | e 6W | E (6W)^2 column-major], li_out (may be NULL) =
 * [dx 6W | trial poses 12W | li_seq]; u and the poses are then taken from li_rec.  Production keeps li_rec / li_out in mapped host
 * memory; this entry keeps both in ordinary device memory.  Outputs: dxi (6W), the slot's trial poses (12W), its q1. */
#define VXBA_DEBUG_NAN_BITS 0x7FF8DEB65017E000ull
int vxba_debug_lm_solve(int device, int W, const double* Hwork, const double* Jwork, double u, const double* Rp, int c, int done, const double* li_rec,
                        unsigned li_seq, double* dxi_out, double* Rp_trial_out, double* q1_out, double* li_out);
/* vxba_debug_wide_solve: one step of the wide windows' persistent blocked Cholesky.  n = 6W, a multiple of 6 in [66, 768]; packed: n^2 + n + 1
 * doubles (Hessian column-major | JacT | residual), not gauge-fixed -- the kernel fixes frame 0 itself.  flags bit 0: the device-wide barriers
 * give up at once (as VXBA_OPT_DEBUG_SOLVE_TIMEOUT = 1 does).  *info_out: 0 solved, > 0 a non-positive pivot (1 + its index), -1 a barrier gave
 * up; with *info_out != 0 no other output is written.  VXBA_ERR_STATE: info 0 and yet no result (a NaN in the solution). */
int vxba_debug_wide_solve(int device, int n, const double* packed, double u, int flags, double* dxi_out, double* q1_out, double* residual1_out, int* info_out);
/* vxba_debug_host_damped_step: the host's damped step (gauge fix, pivoted LDL^T, trial poses, q1) that every device solve falls back to.
 * Host code, no GPU needed.  1 <= W <= 128; Hess (6W)^2 column-major and JacT 6W are not modified. */
int vxba_debug_host_damped_step(int W, const double* Hess, const double* JacT, double u, const double* Rp, double* Rp_trial_out, double* dxi_out, double* q1_out);

/* Debug: per-wave s_memtime stamps written by the instrumented kernel instantiations (env VXBA_DBG=1 /
 * VXBA_K3_SGB=5); 8 slots per wave. */
int vxba_debug_stamps(int clear, unsigned long long* out, size_t n);
int vxba_debug_partials(vxba_factor* f, double* out, size_t n);   /* development: workgroup partials of the last Hessian sweep */

#ifdef __cplusplus
}
#endif
#endif /* VXBA_H */
