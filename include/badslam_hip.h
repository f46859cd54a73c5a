/*
 * badslam_hip.h -- C ABI of the MI355X-native BAD SLAM bundle-adjustment hot path.
 *
 * Every entry point here replaces one free function of the reference's operator
 * boundary, applications/badslam/src/badslam/kernels.h (cited per function as
 * "BS/kernels.h:<line>"), or one host loop of DirectBA
 * (BS/direct_ba_alternating.cc, BS/direct_ba_pcg.cc).  Signatures use only plain
 * pointers, sizes and the POD mirrors below, so the reference's C++ host code (or
 * any FFI) can bind them without seeing HIP or torch types.
 *
 * Conventions (mirroring the reference):
 *   - first argument after the context is the HIP stream (`void*` == hipStream_t),
 *     BS/kernels.h passes cudaStream_t first everywhere;
 *   - all image / surfel memory is owned by the caller and lives in device memory;
 *   - small results written through host pointers are valid on return (the function
 *     synchronises the stream, as BS/kernel_opt_pose.cc:96 does);
 *   - the calls on one context are issued on one stream, or the caller orders them
 *     (events, synchronisation): a context keeps device state between calls (keyframe
 *     table, derived images, surfel work orders, scratch) that a later call re-uses on
 *     the strength of stream order alone;
 *   - return value: 0 on success, negative bslam_status on error.  The reference
 *     aborts via CHECK()/LOG(FATAL) (BS/kernel_opt_pose.cc:58-61); we return the
 *     code and keep the message in bslam_last_error().
 */
#ifndef BADSLAM_HIP_H_
#define BADSLAM_HIP_H_

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* ------------------------------------------------------------------------- */
/* Constants (BS/kernels.cuh:38-93)                                           */
/* ------------------------------------------------------------------------- */

enum {
  BSLAM_INVALID_DEPTH_BIT = 1 << 15,   /* kInvalidDepthBit   BS/kernels.cuh:38 */
  BSLAM_UNKNOWN_DEPTH = 65535,         /* kUnknownDepth      BS/kernels.cuh:41 */
  BSLAM_SURFEL_ACTIVE_FLAG = 1,        /* kSurfelActiveFlag  BS/kernels.cuh:44 */

  /* surfel SoA rows (BS/kernels.cuh:69-93) */
  BSLAM_SURFEL_X = 0,
  BSLAM_SURFEL_Y = 1,
  BSLAM_SURFEL_Z = 2,
  BSLAM_SURFEL_NORMAL = 3,          /* u32: 3 x signed 10 bit */
  BSLAM_SURFEL_RADIUS_SQUARED = 4,
  BSLAM_SURFEL_COLOR = 5,           /* uchar4 rgb0 */
  BSLAM_SURFEL_DESCRIPTOR1 = 6,
  BSLAM_SURFEL_DESCRIPTOR2 = 7,
  BSLAM_SURFEL_ACCUM0 = 8,          /* rows 8..16: scratch, no cross-call guarantees */
  BSLAM_SURFEL_DATA_ATTRIBUTE_COUNT = 8,
  BSLAM_SURFEL_ATTRIBUTE_COUNT = 17
};

/* Keyframe::Activation (BS/keyframe.h:54-67) */
enum {
  BSLAM_KF_ACTIVE = 0,
  BSLAM_KF_COVISIBLE_ACTIVE = 1,
  BSLAM_KF_INACTIVE = 2
};

typedef enum bslam_status {
  BSLAM_OK = 0,
  BSLAM_ERR_INVALID_ARGUMENT = -1,  /* a reference CHECK() would have fired */
  BSLAM_ERR_HIP = -2,               /* a HIP runtime call failed */
  BSLAM_ERR_NO_DEVICE = -3,         /* no gfx950 device visible */
  BSLAM_ERR_OUT_OF_MEMORY = -4,
  BSLAM_ERR_INTERNAL = -5           /* a device-side loop ran into its iteration cap: a bug in the library, never the caller's input */
} bslam_status;

/* ------------------------------------------------------------------------- */
/* POD mirrors of the reference's kernel argument types                       */
/* ------------------------------------------------------------------------- */

/* = vis::CUDABuffer_<T> (libvis/src/libvis/cuda/cuda_buffer.cuh:115-118):
 * element (y, x) lives at (T*)((char*)address + y * pitch) + x. */
typedef struct bslam_buffer2d {
  void* address;
  int32_t height;
  int32_t width;
  size_t pitch; /* bytes */
} bslam_buffer2d;

/* = vis::CUDAMatrix3x4 (BS/cuda_matrix.cuh:140-142): three float4 rows. */
typedef struct bslam_mat3x4 {
  float m[12]; /* row-major: m[4*r + c] */
} bslam_mat3x4;

/* = vis::CUDAMatrix3x3 (BS/cuda_matrix.cuh:76-78): three float3 rows. */
typedef struct bslam_mat3x3 {
  float m[9]; /* row-major */
} bslam_mat3x3;

/* = vis::PinholeCamera4f parameters (libvis/src/libvis/camera.h:1740-1743):
 * fx, fy, cx, cy in the pixel-CORNER convention, plus the image size. */
typedef struct bslam_camera4f {
  float fx, fy, cx, cy;
  int32_t width, height;
} bslam_camera4f;

/* A raw sensor camera with radial-tangential distortion (the reference's RadtanCamera9d as
 * BS/input_structure.cc:391-403 fills it; forward model RadtanDistortion5::Project, LV/camera.h:615-631).
 * fx, fy, cx, cy in the pixel-CENTRE convention, as sensor SDKs report them: the centre of pixel (x, y) has the
 * coordinates (x, y), and a normalised distorted point (dx, dy) lands on (fx * dx + cx, fy * dy + cy).
 * bslam_camera4f stays pixel-CORNER (centre of pixel (x, y) at (x + 0.5, y + 0.5)); the half pixel is added where a
 * radtan camera becomes a bslam_camera4f (DecideUndistortedCamera, host/rectification.hpp: cx_corner = cx_centre +
 * 0.5 - first column) and nowhere else: the rectification kernels take target pixel centres at (x + 0.5, y + 0.5) of
 * the bslam_camera4f and source positions in the radtan camera's own pixel-centre coordinates. */
typedef struct bslam_radtan_camera {
  int32_t width, height;
  float fx, fy, cx, cy;
  float k1, k2, k3; /* radial */
  float p1, p2;     /* tangential (r1, r2 of RadtanDistortion5) */
} bslam_radtan_camera;

/* = vis::DepthParameters (BS/surfel_projection.cuh:129-149). */
typedef struct bslam_depth_params {
  bslam_buffer2d cfactor_buffer; /* float image, ceil(h/cell) x ceil(w/cell) */
  float a;
  float raw_to_float_depth;
  float baseline_fx;
  int32_t sparse_surfel_cell_size;
} bslam_depth_params;

/* The per-keyframe buffers DirectBA hands to the kernels
 * (BS/keyframe.h:160-173,227-231).  `color` is the uchar4 buffer whose .w holds
 * the luma (BS/cuda_image_processing.cu:173-174); MI355X has no texture unit, so
 * the buffer replaces the reference's cudaTextureObject_t and the bilinear /
 * clamp semantics of BS/keyframe.cc:67-73 are computed in the kernel. */
typedef struct bslam_keyframe_view {
  bslam_buffer2d depth;    /* u16 */
  bslam_buffer2d normals;  /* u16 */
  bslam_buffer2d radius;   /* u16 (IEEE half bits) */
  bslam_buffer2d color;    /* uchar4 */
  bslam_mat3x4 frame_T_global;
  bslam_mat3x3 global_R_frame;
  int32_t activation;      /* BSLAM_KF_* */
  int32_t id;
} bslam_keyframe_view;

/* Pose of one keyframe as Sophus::SE3f stores it (unit quaternion xyzw +
 * translation; libvis/third_party/sophus/sophus/se3.hpp). */
typedef struct bslam_se3f {
  float q[4]; /* x, y, z, w */
  float t[3];
} bslam_se3f;

/* How the colour image is sampled where the reference uses tex2D() with
 * cudaFilterModeLinear (BS/cost_function.cuh:140-156). */
enum {
  BSLAM_TEX_FIXED_POINT_1_8 = 0, /* NVIDIA texture unit semantics: 8 fractional weight bits */
  BSLAM_TEX_EXACT_FLOAT = 1      /* exact fp32 bilinear weights */
};

/* Opaque context: owns the scratch the reference keeps in
 * PoseEstimationHelperBuffers / IntrinsicsOptimizationHelperBuffers
 * (BS/kernels.h:46-89) plus the per-launch partial-sum slabs. */
typedef struct bslam_context bslam_context;

/* ------------------------------------------------------------------------- */
/* Library / context                                                          */
/* ------------------------------------------------------------------------- */

/* Version of this ABI; bump on any signature change. */
int bslam_abi_version(void);

/* Last error message of the calling thread ("" if none). */
const char* bslam_last_error(void);

/* Creates a context on HIP device `device`.  Fails with BSLAM_ERR_NO_DEVICE when
 * no GPU is visible: there is no CPU fallback. */
int bslam_create(int device, bslam_context** out_ctx);
int bslam_destroy(bslam_context* ctx);

/* Texture filtering mode (BSLAM_TEX_*), default BSLAM_TEX_FIXED_POINT_1_8. */
int bslam_set_texture_mode(bslam_context* ctx, int mode);

/* The library derives one record per keyframe pixel (calibrated depth, pixel normal, raw depth)
 * from the caller's depth / normal / cfactor images.  By default the records are rebuilt on every
 * call, because the caller owns those images and may rewrite them in place between calls (the
 * reference's tests do, BS/test/test_geometry_optimization_geometric_residual.cc:124-139).
 * enable = 1: the caller promises to call bslam_invalidate_keyframe_cache() after changing the
 * CONTENT of any keyframe depth / normal image or of the cfactor image in place; records are then
 * re-used while buffer addresses, pitches, a, raw_to_float_depth and the cell size are unchanged.
 * The library's own writers of the cfactor image, bslam_optimize_intrinsics (with depth intrinsics)
 * and bslam_update_cfactors_from_pcg_delta, drop the records themselves. */
int bslam_set_keyframe_cache(bslam_context* ctx, int enable);
int bslam_invalidate_keyframe_cache(bslam_context* ctx);

/* Work order of the surfel kernels (default on): surfels are visited along a Morton curve, the work
 * slots of that order dealt round-robin over the XCDs (every XCD gets an even share of every part of
 * the scene; up to round 3 each XCD took one contiguous eighth, and a launch lasted as long as the
 * busiest eighth).  Calls with at least 4 keyframes order the individual surfels by the Morton code of
 * their positions (device radix sort, cached per surfel buffer) and read a sorted copy of the surfel
 * rows, so that a wave's 64 surfels project onto a few cache lines in every keyframe; shorter
 * keyframe lists (the per-keyframe entry points) order 256-column granules by their centroids.
 * Results do not depend on it except for the summation order of the per-keyframe sums; 0 restores
 * index order (A/B measurements, bit-for-bit comparisons between entry points). */
int bslam_set_xcd_schedule(bslam_context* ctx, int enable);

/* Block-level frustum culling (default on).  With the per-surfel work order the surfels of a workgroup are a compact blob; a
 * workgroup skips every keyframe into whose image no point of its surfels' bounding box can project (decided once per
 * workgroup and keyframe, exactly conservatively -- no pair that passes the reference's projection test
 * (ProjectSurfelToImage, BS/util.cuh:86-99) is ever skipped -- so every output is bit-identical with and without it).  The
 * reference spends a thread on every (surfel, keyframe) pair (BS/kernel_opt_pose.cu:263-275).  0 = visit every pair. */
int bslam_set_culling(bslam_context* ctx, int enable);
/* Batched pose loop (bslam_estimate_frame_poses_batched) on keyframe lists of at least `min_keyframes` keyframes: every
 * Gauss-Newton iteration walks a device-side list of the keyframes that are still unconverged instead of the whole keyframe
 * table, so the number of workgroups of an iteration follows the work that is left (on a sequence most keyframes converge in
 * two or three iterations and a few run to the cap of 30, BS/direct_ba_alternating.cc:130).  Results are bit-identical either
 * way.  Default 64; 0 = never (every iteration launches workgroups for every keyframe, converged or not). */
int bslam_set_pose_keyframe_list(bslam_context* ctx, int min_keyframes);
/* (work slot, keyframe) pairs the pose kernel's launches tested / skipped since the last call (HOST out; counted while
 * bslam_profile_enable is on; synchronises the device and resets the counters). */
int bslam_debug_cull_stats(bslam_context* ctx, uint64_t* tested, uint64_t* culled);

/* Kernel timing for the roofline line of bench.py (the role of the reference's cudaEvent
 * pairs, BS/direct_ba.h:513-532): while enabled, every launch of the dominant kernel of a
 * call (the surfel x keyframe pass) is bracketed by HIP events on the launch stream.
 * bslam_profile_read synchronises those events and returns launches and summed ms since
 * the last enable/read. */
int bslam_profile_enable(bslam_context* ctx, int enable);
enum { BSLAM_PROF_POSE_ACCUMULATE = 0, BSLAM_PROF_GEOMETRY = 1, BSLAM_PROF_PCG_INIT = 2, BSLAM_PROF_PCG_STEP1 = 3, BSLAM_PROF_ACTIVATION = 4,
       BSLAM_PROF_EXCHANGE = 5,      /* the K x 32 all-reduce of a batched Gauss-Newton iteration (surfel-sharded runs) */
       BSLAM_PROF_POSE_REDUCE = 6,   /* row sums + 6x6 solve of a batched Gauss-Newton iteration (single-GPU path) */
       BSLAM_PROF_BA_COST = 7 };     /* the objective pass of bslam_compute_ba_cost and its row sums */
int bslam_profile_read(bslam_context* ctx, int kernel, int32_t* launches, float* total_ms);
/* Work counters accumulated since bslam_profile_enable(ctx, 1) by the counting variants of the kernels (8 values, HOST out):
 * [0] (surfel, keyframe) pairs the activation pass actually visited (it stops at a surfel's first associated active keyframe,
 * BS/kernel_surfel_activation.cu:64-79), [1] surfels it set active, [2..7] reserved.  Synchronises the device. */
int bslam_profile_read_counters(bslam_context* ctx, uint64_t* counters8);

/* ------------------------------------------------------------------------- */
/* Pose optimisation                                                          */
/* ------------------------------------------------------------------------- */

/* Replaces AccumulatePoseEstimationCoeffsCUDA (BS/kernels.h:156-174,
 * BS/kernel_opt_pose.cc:39-97): Gauss-Newton coefficients H (21, row-major upper
 * triangle) and b (6) of one keyframe's pose over all surfels.  `residual_count`
 * / `residual_sum` are filled when `debug` != 0 (quirk Q1 of the reference is
 * kept: with descriptor residuals only the first one is counted,
 * BS/kernel_opt_pose.cu:373-381).  H, b, residual_* are HOST pointers, valid on
 * return.  Sums are combined in a fixed order (deterministic), unlike the
 * reference's atomicAdd (BS/gauss_newton.cuh:71,89). */
int bslam_accumulate_pose_estimation_coeffs(
    bslam_context* ctx, void* stream,
    int use_depth_residuals, int use_descriptor_residuals,
    const bslam_camera4f* color_camera, const bslam_camera4f* depth_camera,
    const bslam_depth_params* depth_params,
    const bslam_buffer2d* depth_buffer, const bslam_buffer2d* normals_buffer,
    const bslam_buffer2d* color_buffer,
    const bslam_mat3x4* frame_T_global_estimate,
    uint32_t surfels_size, const bslam_buffer2d* surfels,
    int debug, uint32_t* residual_count, float* residual_sum,
    float* H, float* b);

/* Replaces the keyframe loop around DirectBA::EstimateFramePose in
 * BS/direct_ba_alternating.cc:543-577 (and EstimateFramePose itself, :42-283):
 * all keyframes with activation != BSLAM_KF_INACTIVE advance in lock-step, one
 * launch per Gauss-Newton iteration over (surfels x keyframes); the 6x6 solve
 * (double LDLT, :206), the update global_T_frame * exp(-x) (:214) and the
 * convergence test (BS/convergence_analysis.h:45-52) run on the device, so there
 * is one host sync per iteration instead of one per keyframe and iteration.
 * Surfels are frozen during this phase in the reference too, so per-keyframe
 * results are those of the sequential loop up to summation order.
 *   poses[K]            in/out, global_T_frame per keyframe
 *   iterations_done[K]  out (may be NULL)
 *   converged[K]        out (may be NULL)
 * `allreduce` (may be NULL) is called once per iteration on the device buffer
 * holding K x 32 floats of partial coefficients when surfels are sharded over
 * several GPUs. */
typedef int (*bslam_allreduce_fn)(void* user, void* device_buffer, size_t float_count, void* stream);

int bslam_estimate_frame_poses_batched(
    bslam_context* ctx, void* stream,
    int use_depth_residuals, int use_descriptor_residuals,
    const bslam_camera4f* color_camera, const bslam_camera4f* depth_camera,
    const bslam_depth_params* depth_params,
    int keyframe_count, const bslam_keyframe_view* keyframes,
    uint32_t surfels_size, const bslam_buffer2d* surfels,
    int max_iterations,
    bslam_se3f* poses, int32_t* iterations_done, int32_t* converged,
    bslam_allreduce_fn allreduce, void* allreduce_user);

/* Objective of the surfel model: for every keyframe of the list, whatever its activation field, and every non-deleted
 * surfel (only those with bit 0 of active_surfels set when it is non-null):
 *   cost[k][0] = sum of Tukey depth terms        counts[k][0] = depth-associated pairs
 *   cost[k][1] = sum of kDescWeight * (Huber(r1) + Huber(r2))   counts[k][1] = pairs with valid descriptor residuals
 * HOST outputs, valid on return (counts may be null).  Sums over surfel shards through the call's hook, else the context's
 * hook / RCCL communicator, as bslam_estimate_frame_poses_batched does; the counts then travel as floats and are exact while a
 * keyframe's total stays below 2^24 -- a call in which one reaches it returns BSLAM_ERR_INVALID_ARGUMENT on every rank.
 * keyframe_count == 0 or surfels_size == 0 is valid (zeros).  Not the reference's quirk Q1 (both descriptor residuals).
 * The library's own extension: the reference has no such entry point. */
int bslam_compute_ba_cost(
    bslam_context* ctx, void* stream,
    int use_depth_residuals, int use_descriptor_residuals,
    const bslam_camera4f* color_camera, const bslam_camera4f* depth_camera,
    const bslam_depth_params* depth_params,
    int keyframe_count, const bslam_keyframe_view* keyframes,
    uint32_t surfels_size, const bslam_buffer2d* surfels, const bslam_buffer2d* active_surfels,
    float* cost, uint32_t* counts,
    bslam_allreduce_fn allreduce, void* allreduce_user);

/* Probe of the objective's value-only descriptor path (test aid): for every surfel that associates with `keyframe` and whose
 * pixel lies in the colour image, writes 4 floats to DEVICE out: r1, r2 as the pose kernels form them (with gradients) and
 * r1, r2 as bslam_compute_ba_cost forms them (values only); zeros for the other surfels.  The two pairs are the same bits. */
int bslam_debug_ba_cost_descriptor_residuals(
    bslam_context* ctx, void* stream,
    const bslam_camera4f* color_camera, const bslam_camera4f* depth_camera,
    const bslam_depth_params* depth_params, const bslam_keyframe_view* keyframe,
    uint32_t surfels_size, const bslam_buffer2d* surfels, float* out);

/* One batched accumulation without the solve: H/b for all K keyframes at the
 * given frame_T_global (kf.frame_T_global), written to HOST Hb[K][27] (21 H then
 * 6 b) and counts[K] (number of depth-associated surfels).  Parity probe for the
 * batched kernel and the unit the benchmark times. */
int bslam_accumulate_pose_coeffs_batched(
    bslam_context* ctx, void* stream,
    int use_depth_residuals, int use_descriptor_residuals,
    const bslam_camera4f* color_camera, const bslam_camera4f* depth_camera,
    const bslam_depth_params* depth_params,
    int keyframe_count, const bslam_keyframe_view* keyframes,
    uint32_t surfels_size, const bslam_buffer2d* surfels,
    float* Hb, uint32_t* counts);

/* ------------------------------------------------------------------------- */
/* Surfel activation / geometry                                               */
/* ------------------------------------------------------------------------- */

/* Replaces UpdateSurfelActivationCUDA (BS/kernels.h:262-269,
 * BS/kernel_surfel_activation.cc:39-67): clears bit 0 of active_surfels[0..S) and
 * sets it for every surfel associated with a pixel of an ACTIVE keyframe. */
int bslam_update_surfel_activation(
    bslam_context* ctx, void* stream,
    const bslam_camera4f* depth_camera, const bslam_depth_params* depth_params,
    int keyframe_count, const bslam_keyframe_view* keyframes,
    uint32_t surfels_size, const bslam_buffer2d* surfels,
    const bslam_buffer2d* active_surfels);

/* Replaces UpdateSurfelNormalsCUDA (BS/kernels.h:225-232,
 * BS/kernel_opt_geometry.cc:39-78). */
int bslam_update_surfel_normals(
    bslam_context* ctx, void* stream,
    const bslam_camera4f* depth_camera, const bslam_depth_params* depth_params,
    int keyframe_count, const bslam_keyframe_view* keyframes,
    uint32_t surfels_size, const bslam_buffer2d* surfels,
    const bslam_buffer2d* active_surfels);

/* Replaces OptimizeGeometryIterationCUDA (BS/kernels.h:234-244,
 * BS/kernel_opt_geometry.cc:80-201): normal update, then the position step
 * (geometry-only) or the joint position+descriptor step.  Accumulators stay in
 * registers across keyframes (keyframe order = list order, as the reference's
 * serialised launches), scratch rows 8-16 are not touched. */
int bslam_optimize_geometry_iteration(
    bslam_context* ctx, void* stream,
    int use_depth_residuals, int use_descriptor_residuals,
    const bslam_camera4f* color_camera, const bslam_camera4f* depth_camera,
    const bslam_depth_params* depth_params,
    int keyframe_count, const bslam_keyframe_view* keyframes,
    uint32_t surfels_size, const bslam_buffer2d* surfels,
    const bslam_buffer2d* active_surfels);

/* Replaces OptimizeIntrinsicsCUDA (BS/kernels.h:246-260, BS/kernel_opt_intrinsics.cc:38-283): one
 * Gauss-Newton step on the depth intrinsics (1/fx, 1/fy, -cx/fx, -cy/fy, a, then the per-cell
 * cfactors through the Schur complement, prior 100 a^2) and / or the colour intrinsics.
 * depth_params->cfactor_buffer (device) is updated in place; *a is in/out (the value in
 * depth_params->a is ignored in favour of *a); the out cameras are HOST structs.  The cfactor buffer may be wider or taller
 * than the cell grid of the depth camera: its top-left grid is the image, nothing outside it is read or written. */
int bslam_optimize_intrinsics(
    bslam_context* ctx, void* stream,
    int optimize_depth_intrinsics, int optimize_color_intrinsics,
    int keyframe_count, const bslam_keyframe_view* keyframes,
    const bslam_camera4f* color_camera, const bslam_camera4f* depth_camera,
    const bslam_depth_params* depth_params,
    uint32_t surfels_size, const bslam_buffer2d* surfels,
    bslam_camera4f* out_color_camera, bslam_camera4f* out_depth_camera, float* a);

/* HOST arrays that bslam_debug_optimize_intrinsics fills; a null member is skipped.  cells = the cell grid of the depth
 * camera, ((width - 1) / cell + 1) * ((height - 1) / cell + 1); cell (x, y) has index x + y * ((width - 1) / cell + 1).
 * The 40 sums are A[15] (upper triangle, row by row), b1[5], colour H[10], colour b[4], 6 zeros.  The cell members and x1
 * are written only with optimize_depth_intrinsics, x only with optimize_color_intrinsics. */
typedef struct bslam_intrinsics_tap {
  float* sums;          /* [40]        accumulated over every (keyframe, surfel) pair, before the Schur correction */
  float* cells;         /* [7][cells]  B[5], D, b2 as rounded from the cell sums, at that same point */
  uint32_t* obs;        /* [cells]     observation counts */
  double* schur_sums;   /* [40]        the sums after the Schur correction of A and b1 (before the prior on a): float64, as the
                                       solves read them */
  float* schur_cells;   /* [6][cells]  D^-1 B[5] and D^-1 b2 (NaN: the cell has no usable D) */
  float* x1;            /* [5]         solution of the depth system */
  float* x;             /* [4]         solution of the colour system */
} bslam_intrinsics_tap;

/* bslam_optimize_intrinsics with a tap on its intermediate values (test aid; the same code path, tap == NULL is the product
 * call).  Every copy into the tap waits for the stream.  A call that returns before any device work (surfels_size == 0)
 * writes nothing. */
int bslam_debug_optimize_intrinsics(
    bslam_context* ctx, void* stream,
    int optimize_depth_intrinsics, int optimize_color_intrinsics,
    int keyframe_count, const bslam_keyframe_view* keyframes,
    const bslam_camera4f* color_camera, const bslam_camera4f* depth_camera,
    const bslam_depth_params* depth_params,
    uint32_t surfels_size, const bslam_buffer2d* surfels,
    bslam_camera4f* out_color_camera, bslam_camera4f* out_depth_camera, float* a,
    const bslam_intrinsics_tap* tap);

/* Per-surfel association probe (test / debugging aid; the reference has no such
 * export, the tests need it to check the bit-exact parity target of
 * SURVEY.md 8(a5)): for one keyframe writes out_pixel[i] = py * width + px of the
 * associated pixel, or 0xffffffff when surfel i is not associated.  DEVICE ptr. */
int bslam_debug_association(
    bslam_context* ctx, void* stream,
    const bslam_camera4f* depth_camera, const bslam_depth_params* depth_params,
    const bslam_keyframe_view* keyframe,
    uint32_t surfels_size, const bslam_buffer2d* surfels,
    uint32_t* out_pixel);

/* Tuning knob of bslam_optimize_geometry_iteration: long keyframe lists are walked in (equally long) launches of at most
 * `keyframes_per_launch` keyframes, with the per-surfel sums carried in library scratch (results are bit-identical to a
 * single launch).  -1 = the library's default (one launch); 0 = always one launch. */
int bslam_set_geometry_keyframe_chunk(bslam_context* ctx, int keyframes_per_launch);

/* Replaces AssignColorsCUDA (BS/kernels.h:301-308, BS/kernel_assign_colors.cc:40-80, .cu:42-125): every surfel's
 * colour row becomes the mean of the bilinearly filtered uchar4 colours of the pixels it is associated with over ALL
 * listed keyframes (activation is ignored, as in the reference); surfels without an observation keep their colour.
 * The reference's scratch rows 8..12 are not written (sums live in registers). */
int bslam_assign_colors(
    bslam_context* ctx, void* stream,
    const bslam_camera4f* color_camera, const bslam_camera4f* depth_camera, const bslam_depth_params* depth_params,
    int keyframe_count, const bslam_keyframe_view* keyframes,
    uint32_t surfels_size, const bslam_buffer2d* surfels);

/* Decodes all 65536 u16 image-space normal codes (BS/util.cuh:120-130) with the kernels' own routine into
 * HOST out_xyz[65536 * 3]; lets the tests compare the device's correctly rounded z = -sqrt(1 - x^2 - y^2) with the
 * CPU's bit for bit over the whole domain. */
int bslam_debug_decode_normals(bslam_context* ctx, void* stream, float* out_xyz);

/* Census for the roofline accounting of SURVEY.md 8(d): number of (surfel, keyframe) pairs
 * that pass the z > 0 and image-bounds tests (pairs that do not stop after 12 bytes), and
 * number of associated pairs.  HOST outputs, valid on return. */
int bslam_debug_count_pairs(
    bslam_context* ctx, void* stream,
    const bslam_camera4f* depth_camera, const bslam_depth_params* depth_params,
    int keyframe_count, const bslam_keyframe_view* keyframes,
    uint32_t surfels_size, const bslam_buffer2d* surfels,
    uint64_t* in_bounds_pairs, uint64_t* associated_pairs);

/* Per-surfel residual probe for one keyframe (test / debugging aid): writes 8 floats
 * per surfel to DEVICE out: [depth raw residual, depth weight, descriptor r1, w1, r2,
 * w2, flags (bit0 associated, bit1 descriptor residuals valid), 0].  This is how the
 * tests check "residuals within 1e-4 relative" surfel by surfel. */
int bslam_debug_pose_residuals(
    bslam_context* ctx, void* stream,
    int use_depth_residuals, int use_descriptor_residuals,
    const bslam_camera4f* color_camera, const bslam_camera4f* depth_camera,
    const bslam_depth_params* depth_params, const bslam_keyframe_view* keyframe,
    uint32_t surfels_size, const bslam_buffer2d* surfels, float* out);

/* Point-wise probe of the device residual / Jacobian formulas (test aid): evaluates, for `count` points, the functions of
 * csrc/device_math.hpp that every kernel calls.  HOST in / out, valid on return.  Floats per point (in -> out):
 *   kind 0 depth / pose          [inv_stddev, n_local(3), lu(3), ls(3)]                        -> [raw residual, J(6)]
 *   kind 1 depth / position      [inv_stddev]                                                   -> [j]
 *   kind 2 depth / intrinsics    [inv_stddev, calibrated depth, px, py, nx, ny, n_global(3), frame_T_global row 0 (3), row 1 (3),
 *                                 n_local(3), cfactor, a, raw_inv_depth]                        -> [corrected_inv_depth, dj(6)]
 *   kind 3 descriptor / pose     [tl, tr, bl, br, tx, ty, fx, fy, ls(3)]                        -> [bilinear value, gx fx, gy fy, J(6)]
 *   kind 4 descriptor / position [tl, tr, bl, br, tx, ty, fx, fy, rn(3), ls(3)]                -> [j]
 *   kind 5 descriptor / colour intrinsics [tl, tr, bl, br, tx, ty, nx, ny]                      -> [j(4)]
 *   kind 6 = kind 0 in the pose kernel's fused-multiply-add form
 *   kind 7 arithmetic check  [x] -> [the kernels' correctly rounded reciprocal of x (rcp_rn_midrange), 1.0f / x]
 *   kind 8 arithmetic check  [x] -> [the hardware reciprocal seed (v_rcp_f32), one Newton step from it, two Newton steps]
 * (tl .. br = the 2x2 texel footprint in [0, 1], tx, ty = fractional offsets of the sample).  tests/test_gpu_jacobians.py holds
 * these to the values of the reference's symbolic derivation (applications/badslam/scripts/jacobians_derivation.py). */
int bslam_debug_jacobians(bslam_context* ctx, void* stream, int kind, int count, const float* in, float* out);
/* Test probe of the wave reduction every per-keyframe sum goes through (wave_column_sums_lds, csrc/device_math.hpp): one wave,
 * lane l holds in[32 l .. 32 l + 32) (HOST, 64 x 32 floats); out[c] (HOST, 32 floats, in / out) receives the total of column c
 * over the 64 lanes from the lane that owns the column -- 0 for an owned column >= live_columns; columns no lane owns in the
 * configuration keep the value they had.  (live_columns, columns_per_round) must be one of the kernels' configurations:
 * (27 | 28, 4 | 8), (6, 4), (12, 4). */
int bslam_debug_wave_column_sums(bslam_context* ctx, void* stream, int live_columns, int columns_per_round, const float* in, float* out);
/* Test probe of the photometric pose kernel's descriptor normal equations: for `count` points (HOST in / out, valid on return)
 *   [ls(3), gx1, gy1, r1, gx2, gy2, r2]  (9 floats: surfel position in the frame, the two residuals with their gradients times fx, fy)
 *   -> [H upper triangle (21) and b (6) of the pair through the rank-two form (accumulate_h_b_desc_pair, weights from the
 *       wave-uniform Huber path), the same 27 numbers through two descriptor Jacobian rows and two rank-one updates,
 *       w1, w2 of the wave-uniform Huber path, w1, w2 of the per-lane form]  (58 floats).
 * A wave evaluates 64 consecutive points, so the Huber path taken depends on the residuals of a point's group of 64. */
int bslam_debug_desc_pair(bslam_context* ctx, void* stream, int count, const float* in, float* out);
/* Test probe of the luma quad table (csrc/device_math.hpp: KfDev::quads).  `images` (HOST) holds image_count tightly packed images
 * of width x height pixels with `channels` bytes each: 4 = keyframe colour (luma in byte 3, table built by the kernel of the
 * keyframe calls), 1 = u8 image (table built by the kernels of the odometry calls: the single-pair one for image_count = 1, the
 * batched one otherwise; image_count <= BSLAM_MAX_PAIR_BATCH).  For each of `count` positions [image index, x, y] (HOST,
 * pixel-corner coordinates, any finite value) out (HOST, 6 floats per position, valid on return) receives the bilinear sample
 * and its gradient in byte units, [val, gx, gy], twice: through the table as the kernels sample it, and from four byte loads of
 * the image with clamp addressing and the differences formed per sample in integers.  `entries` (HOST, image_count x (height + 1)
 * x (width + 1) x 4 uint16, valid on return) receives the raw table: fp16 bit patterns {tl, tr - tl, bl - tl,
 * (br - bl) - (tr - tl)} of base texel (i, j) at [image][j + 1][i + 1]. */
int bslam_debug_quad_samples(bslam_context* ctx, void* stream, int image_count, int width, int height, int channels, const uint8_t* images,
                             int count, const float* positions, int tex_mode, float* out, uint16_t* entries);

/* ------------------------------------------------------------------------- */
/* Surfel lifecycle                                          */
/* ------------------------------------------------------------------------- */
/* The reference resolves cell ownership with atomicCAS races; these entry points fix the outcome to
 * "lowest surfel index first" / "raster order first" (one of the outcomes the reference can produce), so
 * results are deterministic.  The supporting-surfel cell buffers (BS/direct_ba.cc:135) are library scratch. */

/* Replaces DetermineSupportingSurfelsAndMergeSurfelsCUDA (BS/kernels.h:105-117): merged surfels get
 * x = NaN (0x7fffffff); *surfel_count is decreased by their number (valid on return). */
int bslam_determine_supporting_surfels_and_merge(
    bslam_context* ctx, void* stream, float merge_dist_factor,
    const bslam_camera4f* depth_camera, const bslam_depth_params* depth_params,
    const bslam_keyframe_view* keyframe, uint32_t surfels_size, const bslam_buffer2d* surfels,
    uint32_t* surfel_count);

/* Replaces DetermineSupportingSurfelsCUDA + CreateSurfelsForKeyframeCUDA, i.e. the body of
 * DirectBA::CreateSurfelsForKeyframe (BS/direct_ba.cc:340-405, BS/kernels.h:94-145).
 * global_T_frame: the keyframe's pose as 3x4; covis_T_frame[i] = covis frame_T_global * global_T_frame
 * (computed by the caller, BS/direct_ba.cc:365-370; only read when filter_new_surfels).
 * Appends at column surfels_size; *new_surfel_count is valid on return.  If the new surfels do not fit,
 * nothing is created and BSLAM_ERR_OUT_OF_MEMORY is returned (the reference logs an error). */
int bslam_create_surfels_for_keyframe(
    bslam_context* ctx, void* stream, int filter_new_surfels, int min_observation_count,
    const bslam_camera4f* color_camera, const bslam_camera4f* depth_camera,
    const bslam_depth_params* depth_params,
    const bslam_keyframe_view* keyframe, const bslam_mat3x4* global_T_frame,
    int covis_count, const bslam_keyframe_view* covis_keyframes, const bslam_mat3x4* covis_T_frame,
    uint32_t surfels_size, const bslam_buffer2d* surfels, uint32_t* new_surfel_count);

/* Replaces DeleteSurfelsAndUpdateRadiiCUDA (BS/kernels.h:271-280): surfels observed by fewer than
 * min_observation_count keyframes, or with more free-space violations than observations, get x = NaN;
 * the others get radius^2 = min over their observations. */
int bslam_delete_surfels_and_update_radii(
    bslam_context* ctx, void* stream, int min_observation_count,
    const bslam_camera4f* depth_camera, const bslam_depth_params* depth_params,
    int keyframe_count, const bslam_keyframe_view* keyframes,
    uint32_t* surfel_count, uint32_t surfels_size, const bslam_buffer2d* surfels);

/* Replaces CompactSurfelsCUDA (BS/kernels.h:292-299): the last valid surfels move into the free spots, in the
 * reference's order; rows 0-7 (and active_surfels, may be NULL) move, *surfels_size becomes surfel_count. */
int bslam_compact_surfels(
    bslam_context* ctx, void* stream, uint32_t surfel_count, uint32_t* surfels_size,
    const bslam_buffer2d* surfels, const bslam_buffer2d* active_surfels);

/* ------------------------------------------------------------------------- */
/* Keyframe preprocessing producers                          */
/* ------------------------------------------------------------------------- */
/* These write the u16 / half / uchar4 keyframe images the bundle adjuster reads.  Buffers are device
 * memory; input and output of one call must not alias. */

/* Input conditioning of the raw frame (BadSlam::PreprocessFrame, BS/bad_slam.cc:645-685; host code in the
 * reference).  Like the other producers: launched on `stream` without synchronisation, results ordered on it.
 * Input and output must not share a byte ([address, address + height * pitch) of each): invalid argument. */

/* One iteration of MedianFilterAndDensifyDepthMap (BS/preprocessing.cc:40-85): per pixel the median of the
 * non-zero values of its 3x3 window, clipped at the border; a window with fewer than 2 of them leaves the pixel
 * as it is.  With an even count: the lower middle value if it is strictly nearer to the fp32 mean than the
 * upper one, else the upper one.  u16 images of one size. */
int bslam_median_filter_and_densify_depth(bslam_context* ctx, void* stream,
                                          const bslam_buffer2d* input_depth, const bslam_buffer2d* output_depth);

/* Image<u16>::DownscaleUsingMedianWhileExcluding(0, ...) (LV/image.h:1003-1053) by a pyramid level L = 1 ... 3,
 * inferred from the shapes (input = output * 2^L in both dimensions): per 2^L x 2^L block the median of its
 * non-zero values by the rule above, 0 for a block of zeros. */
int bslam_downscale_depth_median(bslam_context* ctx, void* stream,
                                 const bslam_buffer2d* input_depth, const bslam_buffer2d* output_depth);

/* L = 1 ... 3 (inferred as above) successive Image<Vec3u8>::DownscaleToHalfSize steps (LV/image.h:929-948,
 * ImagePyramid LV/image_cache.h:212-231) in one launch; a step is a/4 + b/4 + c/4 + d/4 per channel, each
 * quotient truncated.  Both images have 3 bytes per pixel (width = pixels, as in bslam_compute_brightness). */
int bslam_downscale_rgb(bslam_context* ctx, void* stream,
                        const bslam_buffer2d* input_rgb, const bslam_buffer2d* output_rgb);

/* Sensor rectification (host code in the reference: BS/undistortion.cc, BS/input_structure.cc:196-298): a raw frame
 * of a distorted colour camera and a distorted depth camera beside it becomes the ideal pinhole frame of one
 * viewpoint that everything above expects.  Launched on `stream` without synchronisation, like the calls above. */

/* CreateUndistortionMap (BS/undistortion.cc:122-140) in fp32: for every pixel of `target`, the position in the
 * `source` image (its pixel-centre coordinates) that the ray through the target pixel's centre lands on, clamped to
 * [0, width - 1 - FLT_EPSILON] x [0, height - 1 - FLT_EPSILON] (in fp32 that is width - 1, height - 1).  `map` has the
 * size of `target` and 8 bytes per pixel (float x, float y).  The source must be at least 2 x 2. */
int bslam_build_undistortion_map(bslam_context* ctx, void* stream, const bslam_radtan_camera* source,
                                 const bslam_camera4f* target, const bslam_buffer2d* map);

/* UndistortImage (BS/undistortion.cc:142-156): output pixel = bilinear interpolation of input_rgb at the map position,
 * each channel (u8)(value + 0.5f).  3 bytes per pixel; map and output have one size; the input is at least 2 x 2 and
 * must not overlap the output.  Map positions are taken as clamped by bslam_build_undistortion_map; the texel index is
 * limited to width - 2 / height - 2, so a position on the last column / row reads inside the image. */
int bslam_undistort_rgb(bslam_context* ctx, void* stream, const bslam_buffer2d* input_rgb, const bslam_buffer2d* map,
                        const bslam_buffer2d* output_rgb);

/* ReprojectDepthImage (BS/input_structure.cc:196-298) as a rasteriser: the raw u16 depth image (0 = no measurement)
 * becomes a triangle mesh -- vertex of raw pixel (x, y) = depth * input_depth_to_metres * (ux, uy, 1) with (ux, uy)
 * from unprojection_map (8 bytes per pixel, size of input_depth; MakeUnprojectionMap of host/rectification.hpp), two
 * triangles per 2 x 2 pixel block, none where one of the four depths is 0 or two of them differ by
 * depth_difference_threshold (metres, > 0) or more -- which is transformed by target_T_depth (null = identity),
 * projected with `target` and drawn into output_depth (u16, size of `target`) with a z-buffer that keeps the nearest
 * surface: (u16)(output_metres_to_depth * z + 0.5f), 0 where nothing was drawn or the value exceeds 65535.
 * Deviations from the GL path: a triangle with a vertex at z < 0.05 or z > 50 is dropped, not clipped; a pixel is
 * covered when its centre lies in the closed triangle (no top-left rule); z is interpolated perspective-correctly.
 * The result does not depend on the order in which triangles arrive.  Input, map and output must not overlap. */
int bslam_reproject_depth(bslam_context* ctx, void* stream, const bslam_buffer2d* input_depth, float input_depth_to_metres,
                          const bslam_buffer2d* unprojection_map, const bslam_mat3x4* target_T_depth,
                          const bslam_camera4f* target, float depth_difference_threshold, float output_metres_to_depth,
                          const bslam_buffer2d* output_depth);

/* Views of the surfel model from a pose (in place of the reference's on-screen view, BS/render_window.cc and
 * BS/kernel_update_visualization.cu, which draws screen-aligned splats of a fixed pixel size): every surfel is an
 * oriented disc of radius radius_scale * sqrt(radius_squared) around its position, perpendicular to its normal.  A
 * pixel shows the disc that the ray through its centre hits nearest to the camera; among discs hit at bit-equal depths,
 * the one with the lower surfel index.  The result does not depend on the order in which surfels arrive: two calls give
 * identical bits.  All arithmetic is fp32 in a fixed expression order (csrc/render_kernels.hpp, DESIGN.md 8 "Model
 * views").  Not drawn: surfels with NaN x, with a scaled squared radius that is not > 0, whose bounding ball does not lie
 * in [min_depth, max_depth] (centre z - radius >= min_depth and centre z <= max_depth: dropped, not clipped), and those
 * seen from behind or with a zero normal.
 *   camera_T_global  pose of the view; camera: pixel-corner pinhole camera, 1 ... 2^31 - 1 pixels, fx, fy > 0
 *   surfels          the surfel rows up to BSLAM_SURFEL_COLOR at least; surfels_size = 0 gives empty views
 *   0 < min_depth <= max_depth (metres);  radius_scale > 0;  metres_to_depth > 0
 * Outputs, each of the camera's size and optional (null = not written), at least one given; they must not overlap each
 * other or the surfel rows, and their rows must be aligned to their element (2 / 4 / 4 / 4 bytes):
 *   out_depth   u16     (u16)(metres_to_depth * z + 0.5f), 0 where nothing was drawn or the value exceeds 65535 -- with
 *                       metres_to_depth = 1 / raw_to_float_depth the units of a keyframe's depth image
 *   out_index   u32     the surfel's column, 0xFFFFFFFF where nothing was drawn
 *   out_color   uchar4  the surfel's BSLAM_SURFEL_COLOR entry, 0 where nothing was drawn
 *   out_normal  12 B    three floats: the surfel's unit normal in the camera frame, 0 where nothing was drawn
 * Launched on `stream` without synchronisation.  In a surfel-sharded run a rank renders the surfels it was given, i.e.
 * its own shard; nothing is exchanged (merging shards would be a minimum of the keys across the ranks). */
int bslam_render_surfels(bslam_context* ctx, void* stream, const bslam_mat3x4* camera_T_global, const bslam_camera4f* camera,
                         uint32_t surfels_size, const bslam_buffer2d* surfels, float min_depth, float max_depth,
                         float radius_scale, float metres_to_depth, const bslam_buffer2d* out_depth,
                         const bslam_buffer2d* out_index, const bslam_buffer2d* out_color, const bslam_buffer2d* out_normal);

/* Volumetric fusion (the reference ends at the surfel point cloud, BS/io.cc:694, and leaves meshing to other tools): the
 * calibrated depth of every keyframe is averaged into a truncated signed distance volume, from scratch -- bundle
 * adjustment moves all poses, so there is no incremental mode.  Sample (x, y, z) of the volume, 0 <= x < nx and alike,
 * lies at  origin + (float(i) + 0.5f) * voxel_size  per axis (a multiply, then an add).  All arithmetic is fp32 in a
 * fixed expression order (csrc/fusion_kernels.hpp, DESIGN.md 8 "Volumetric fusion"); two calls give identical bits. */
typedef struct bslam_volume {
  float origin[3];
  float voxel_size;
  int32_t nx, ny, nz;
} bslam_volume;

/* Per sample, the keyframes in list order (`activation` is not looked at, as in bslam_assign_colors):
 *   the centre is projected exactly like a surfel (same transform, reciprocal, rounding and bounds test); outside the
 *   depth image or behind the camera: no observation
 *   d = calibrated depth of that pixel (the derived records; bslam_set_keyframe_cache applies); d == 0: no observation
 *   sdf = d - local.z;  sdf < -truncation: no observation (occluded);  else  S += fminf(sdf, truncation), n += 1
 *   colour, only when `color` is given and sdf <= truncation: the uchar4 pixel nearest to the projection of the centre
 *   with color_camera (truncated coordinates), if inside the colour image: r, g, b added to integer sums, nc += 1
 * Outputs, 2-D buffers of nz * ny rows of nx 4-byte elements, row = z * ny + y, rows 4 byte aligned, pitches may exceed
 * the content and padding is never written; every sample of every given output is written:
 *   tsdf   f32     n ? S / float(n) : truncation       (metres, not normalised)
 *   count  u32     n
 *   color  uchar4  nc ? {(sum + nc / 2) / nc per channel, 255} : {0, 0, 0, 0};  may be null (color_camera too, then)
 * Refused: null arguments, voxel_size or truncation not finite and > 0, a dimension < 2, nx * ny * nz > 2^30, pitches
 * too small or misaligned, outputs that overlap, and what the keyframe list checks of the other calls refuse.
 * keyframe_count == 0 is legal: count 0, tsdf = truncation everywhere.
 * A workgroup owns a brick of 8 x 8 x 4 samples and skips the keyframes whose frustum its box cannot reach
 * (bslam_set_culling; counted in bslam_debug_cull_stats as (brick, keyframe) pairs while profiling is on); the outputs
 * are the same bits either way.  Launched on `stream` without synchronisation.  Keyframes are replicated in a
 * surfel-sharded run: every rank computes the same volume, nothing is exchanged. */
int bslam_fuse_keyframes(bslam_context* ctx, void* stream, const bslam_camera4f* color_camera, const bslam_camera4f* depth_camera,
                         const bslam_depth_params* depth_params, int keyframe_count, const bslam_keyframe_view* keyframes,
                         const bslam_volume* volume, float truncation, const bslam_buffer2d* tsdf,
                         const bslam_buffer2d* count, const bslam_buffer2d* color);

/* Triangle mesh of a fused volume by naive surface nets.  A sample is observed iff count >= min_count (>= 1) and inside
 * iff tsdf < 0.  Cell (x, y, z), 0 <= x < nx - 1 and alike, has the samples (x + dx, y + dy, z + dz) as corners, is active
 * iff all eight are observed and not all on one side, and has the linear index (z (ny - 1) + y)(nx - 1) + x.
 * Vertices: one per active cell, id = the cell's rank among the active cells in linear order.  Over the cell's edges
 * a -> b = a + axis whose ends lie on different sides (the four x-edges at (dy, dz) = (0,0), (1,0), (0,1), (1,1), then the
 * y-edges at (dx, dz) and the z-edges at (dx, dy) in the same pattern):  t = Da / (Da - Db), the corner offset of a with t
 * in place of the axis component is added to a running sum;  mean = sum / float(edges);
 *   position = origin + ((float(x) + 0.5f) + mean.x) * voxel_size                              per component
 *   normal   = g / sqrtf((g.x g.x + g.y g.y) + g.z g.z) with g.axis = the sum of Db - Da over the four edges of the
 *              axis in the order above; 0 where the root is 0.  Points towards free space.
 *   colour   = {(sum + k / 2) / k per channel, 255} over the k corners whose colour sample has alpha 255; 0 for k = 0
 * Faces: an active cell owns the grid edges from its minimum corner a along +x, +y, +z.  Such an edge gives a quad iff
 * the sides of its ends differ and the four cells around it are active; for +x these are q0 .. q3 = (x, y-1, z-1),
 * (x, y, z-1), (x, y, z), (x, y-1, z), for +y and +z the same with (z, x) and (x, y) in the places of (y, z).  Triangles
 * (q0, q1, q2), (q0, q2, q3) if a is inside, else of the reversed quad (q3, q2, q1, q0): counter-clockwise seen from free
 * space.  Faces are ordered by (linear cell index, axis).
 * Device outputs: positions float[3 V], normals float[3 V] (may be null), colors uchar4[V] (may be null; written only
 * when a colour volume is given), indices uint32[3 T]; *vertex_count = V and *triangle_count = T on the host.  When
 * positions or indices is null, or V > vertex_capacity or T > triangle_capacity, only the counts are returned and
 * nothing is written: call once for the counts and once with buffers.  Synchronises `stream`. */
int bslam_extract_mesh(bslam_context* ctx, void* stream, const bslam_volume* volume, const bslam_buffer2d* tsdf,
                       const bslam_buffer2d* count, const bslam_buffer2d* color, uint32_t min_count, uint32_t vertex_capacity,
                       uint32_t triangle_capacity, float* positions, float* normals, void* colors, uint32_t* indices,
                       uint32_t* vertex_count, uint32_t* triangle_count);

/* Mesh components: an indexed triangle mesh as a graph (DESIGN.md 8 "Mesh components", csrc/mesh_kernels.hpp).  The input has
 * V vertices, T triangles and indices uint32[3 T]; it may come from bslam_extract_mesh or from anywhere else.
 * Components:
 *   Vertices a and b are joined iff some triangle contains both.  Degenerate triangles such as (a, a, b) and (a, a, a) are
 *   legal, duplicated triangles too.
 *   A component is a class of the transitive closure of "joined".  A vertex in no triangle is a component of its own.
 *   label[v] is the smallest vertex id in v's component.
 *   size[v] is the number of vertices in v's component, stored per vertex, not per component.
 *   component_count is the number of v with label[v] == v.
 *   All three are integers and do not depend on the order of execution: two runs give identical bits.
 * bslam_mesh_components: indices, labels uint32[V] and sizes uint32[V] are device arrays, 4 byte aligned, that do not overlap;
 * *component_count is written on the host.  V == 0 and T == 0 are legal (an array of no elements may be null).  A triangle
 * with an index >= V is never dereferenced: the call returns BSLAM_ERR_INVALID_ARGUMENT, labels and sizes are then
 * unspecified, and nothing outside the given buffers is touched.  Refused without a launch: a null context or
 * component_count, null or misaligned arrays, labels or sizes that overlap each other or the indices.  A union-find over
 * parent[v] <= v: a fixed number of launches whatever the graph's diameter (one union launch); every loop is capped, and
 * BSLAM_ERR_INTERNAL reports a cap that was reached (it cannot be).  While profiling is on, bslam_debug_cull_stats counts the
 * hooks (compare-and-swaps) attempted and, as "culled", those that failed and were retried.  Synchronises `stream`.
 * Filter:
 *   Given size (as bslam_mesh_components wrote it) and min_vertices (>= 1), vertex v is kept iff size[v] >= min_vertices.
 *   A triangle is kept iff its first vertex is kept; its three vertices share a label, so they are all kept or all dropped.
 *   Kept vertices and kept triangles keep their relative order.  The new vertex id is the rank among the kept vertices.
 *   Positions, normals and colours are copied with their bits unchanged; indices are remapped.
 *   V' and T' are returned on the host; output entries at and beyond V' / T' are not written.
 * bslam_filter_mesh: positions float[3 V], normals float[3 V] (may be null), colors uchar4[V] (may be null), indices
 * uint32[3 T], sizes uint32[V] and the outputs of the same shapes (room for V vertices and T triangles) are device arrays.
 * Refused without a launch: null required arguments, an out_normals / out_colors that does not match the presence of its
 * input, min_vertices == 0, misaligned (4 byte) pointers, and an output that overlaps an input or another output -- compaction
 * in place races.  An index >= V: as above.  Synchronises `stream`.  Every rank of a surfel-sharded run holds the same mesh. */
int bslam_mesh_components(bslam_context* ctx, void* stream, uint32_t vertex_count, uint32_t triangle_count, const uint32_t* indices,
                          uint32_t* labels, uint32_t* sizes, uint32_t* component_count);
int bslam_filter_mesh(bslam_context* ctx, void* stream, uint32_t vertex_count, uint32_t triangle_count, const float* positions,
                      const float* normals, const void* colors, const uint32_t* indices, const uint32_t* sizes, uint32_t min_vertices,
                      float* out_positions, float* out_normals, void* out_colors, uint32_t* out_indices, uint32_t* out_vertex_count,
                      uint32_t* out_triangle_count);

/* Mesh simplification: vertex clustering on a uniform grid (DESIGN.md 8 "Mesh simplification", csrc/simplify_kernels.hpp).  All
 * vertices of a grid cell become one vertex, triangles are remapped and those that collapse are dropped.  With T == 0 it is
 * voxel-grid down-sampling of a point cloud.  Nothing is contracted implicitly.
 * Cell:
 *   inv = 1.0f / cell_size, once, in fp32;  c_a = floorf((x_a - origin_a) * inv) per axis, the subtraction and the multiplication
 *   separate fp32 operations (the cell of "Surface evaluation").  A vertex is valid iff its three coordinates are finite and
 *   0 <= c_a < 2^21 on every axis.  -0.0f and values exactly on a cell face follow from the formula; there is no epsilon.
 * Clusters:
 *   Vertices with equal (c_x, c_y, c_z) form a cluster, referenced by a triangle or not; clusters are numbered 0 .. C - 1 in
 *   ascending (c_z, c_y, c_x) order; vertex_cluster[v] is the cluster of vertex v.
 * Representative of a cluster of n members; every sum runs over the members in ascending vertex id:
 *   position.a = (float)(sum_a / (double)n), sum_a a double sum that starts from the first member (a cluster of one keeps its
 *     bits, the sign of a zero included);
 *   normal.a = (float)(s_a / sqrt(ss)), s_a a double sum, ss = (s_x * s_x + s_y * s_y) + s_z * s_z in double; (0, 0, 0) when ss is
 *     not > 0 or a member's normal is not finite;
 *   colour, per channel, alpha included: (S + n / 2) / n in integers, S a 64-bit sum (the rounding of the fusion colours).
 * Triangles:
 *   Triangle t becomes (cluster[i0], cluster[i1], cluster[i2]) in that order and is kept iff the three are pairwise distinct;
 *   kept triangles keep their relative order.  Duplicate triangles are not removed.
 * bslam_simplify_mesh: positions float[3 V], normals float[3 V] (may be null), colors uchar4[V] (may be null), indices uint32[3 T]
 * and the outputs of the same shapes (room for V vertices and T triangles; out_normals and out_colors exactly when their inputs
 * are given) and vertex_cluster uint32[V] (may be null) are device arrays; origin float[3] is a host array.  *out_vertex_count = C
 * and *out_triangle_count are returned on the host; nothing at or beyond them is written.  V == 0 is legal with T == 0, and T == 0
 * is a point cloud.  Refused without a launch: null required arguments, an origin that is not finite, a cell_size that is not
 * finite and > 0 or whose reciprocal is not, an out_normals / out_colors that does not match its input, more than 2^32 - 256
 * vertices or triangles, misaligned (4 byte) pointers, an output that overlaps an input or another output.  Refused behind the
 * launches, by a device error bit, with BSLAM_ERR_INVALID_ARGUMENT and unspecified output contents: an index >= V (never
 * dereferenced; the message of the mesh component calls) and an invalid vertex ("a vertex is not finite or lies outside the grid";
 * no attribute is gathered through it).  A key pass, a stable radix sort of (cell key, vertex id), head flags and their scan, a
 * cluster pass with one lane per cluster walking its members, and a keep-flag / scan / scatter triangle pass; one read-back.
 * Scratch lives in a context slab of its own that the first call reserves.  Synchronises `stream`.  Every rank of a
 * surfel-sharded run holds the same mesh and computes the same result; nothing is exchanged. */
int bslam_simplify_mesh(bslam_context* ctx, void* stream, uint32_t vertex_count, uint32_t triangle_count, const float* positions,
                        const float* normals, const void* colors, const uint32_t* indices, const float* origin, float cell_size,
                        float* out_positions, float* out_normals, void* out_colors, uint32_t* out_indices, uint32_t* vertex_cluster,
                        uint32_t* out_vertex_count, uint32_t* out_triangle_count);
/* The device time in milliseconds of the five stages of the last bslam_simplify_mesh on `ctx` that ran its launches while
 * bslam_profile_enable was on (HOST out): {key pass, sort, head flags and their scan, cluster pass, triangle pass}, taken from
 * events on the call's stream.  Zeros before such a call.  For tools/bench_simplify_mesh.py. */
int bslam_simplify_stage_times(bslam_context* ctx, float* stage_ms5);

/* Mesh decimation: quadric-error edge collapse in data-parallel rounds (DESIGN.md 8 "Mesh decimation", csrc/decimate_kernels.hpp).
 * Every operation that decides anything is float64, `+ - * /` separately in the written order, nothing contracted; fp32 inputs
 * are widened first.  cross(u, v) = (u.y v.z - u.z v.y, u.z v.x - u.x v.z, u.x v.y - u.y v.x), dot(a, b) = (a.x b.x + a.y b.y) + a.z b.z.
 * Input: triangles that repeat an index are dropped first; the others are the live triangles, in their order.  A vertex without a
 *   triangle is kept and never moves.  A vertex is live until it is merged away; live = V at the start.
 * Plane quadric K(n, a) of a normal n and a point a:  d = -dot(n, a);  the ten products (xx, xy, xz, xd, yy, yz, yd, zz, zd, dd) =
 *   (n.x n.x, n.x n.y, n.x n.z, n.x d, n.y n.y, n.y n.z, n.y d, n.z n.z, n.z d, d d).  Quadrics add entry by entry.
 * 1. Triangle t = (i0, i1, i2) with positions a, b, c:  n_t = cross(b - a, c - a), not normalised;  Q_t = K(n_t, a): the form is
 *   (2 area distance)^2, the squared-volume measure of Lindstrom and Turk, without a root or a division.
 * 2. Edge k of t runs from corner k to corner (k + 1) mod 3, a -> b.  It is a boundary edge iff no other input triangle uses the
 *   undirected edge.  Then e = b - a, ee = (e.x e.x + e.y e.y) + e.z e.z, and if ee > 0 every entry p of K(cross(e, n_t), a) becomes
 *   (p * (double)boundary_weight) / ee; that quadric is added to both ends.
 * 3. Q[v] starts from +0.0, adds Q_t over the triangles at v in ascending t, then the boundary quadrics of the boundary edges at v in
 *   ascending (t, k).  Computed once; a collapse sets Q[lo] = Q[lo] + Q[hi].
 * 4. A round.  The unique undirected edges (lo < hi) of the live triangles in ascending (lo, hi) have rank 0, 1, ...; c is the
 *   number of live triangles on the edge; N(v) the vertices that share a live triangle with v; v is boundary iff an edge at v has
 *   c = 1.  An edge is a candidate iff c <= 2, |N(lo) & N(hi)| + [lo and hi boundary] = c + [c = 1] (the link condition with a virtual
 *   vertex beyond the boundary), no common neighbour is a non-boundary vertex in exactly three live triangles, and the cost and
 *   flip tests hold.  Q = Q[lo] + Q[hi]; the places are p0 = p_lo, p1 = p_hi, p2 = per axis (float)((p_lo + p_hi) * 0.5);
 *   cost(p) = (sq + 2 cr) + (2 li + dd) with sq = ((xx x) x + (yy y) y) + (zz z) z, cr = ((xy x) y + (xz x) z) + (yz y) z,
 *   li = (xd x + yd y) + zd z.  The place is 0, replaced by 1 iff cost(p1) < cost(p0), then by 2 iff cost(p2) < the cost so far.
 *   cost32 = (float)(cost > 0 ? cost : 0); the cost must not be NaN, cost32 must be finite and <= max_cost.  Flip test: every live
 *   triangle that holds exactly one of lo and hi, with normal n and, that corner moved to the place, normal n', has dot(n, n') > 0.
 * 5. key = bits(cost32) << 32 | (rank * 0x9E3779B1 mod 2^32), unique since the constant is odd.  m1[v] = the least key of the
 *   candidates at v, m2[v] = the least m1 over v and N(v).  A candidate is selected iff key = m2[lo] = m2[hi]; selected edges have
 *   pairwise non-adjacent ends.  If more are selected than live - target_vertices, the first that many in ascending key collapse.
 * 6. Collapse: lo takes the place and Q; with place 1 the normal and colour of hi, with place 2 the normal (float)(s / sqrt(ss)) per
 *   axis, s the double sum of the two and ss = (s.x s.x + s.y s.y) + s.z s.z, or (0, 0, 0) when ss is not > 0 or a component is not
 *   finite, and the colour (a + b + 1) / 2 per channel in integers.  hi is merged into lo; triangles are remapped and dropped where
 *   two corners meet; live decreases by one.  Rounds repeat while live > target_vertices and fewer than max_rounds (0: no limit) have
 *   run; a round that selects nothing is the last.  *out_rounds counts the rounds evaluated, that last one included.
 * 7. Output: the live vertices in ascending id with their positions, normals and colours; the live triangles in their order;
 *   vertex_map[v] = the new id of the vertex v was merged into, through every merge.  target_vertices >= V returns the input bit for
 *   bit, less the dropped triangles.
 * bslam_decimate_mesh: the arrays are those of bslam_simplify_mesh (device; room for V vertices and T triangles; vertex_map may be
 * null); the three counts are returned on the host; nothing at or beyond the counts is written.  Refused without a launch: null
 * required arguments, a boundary_weight that is not finite and >= 0, a max_cost that is NaN or < 0 (+inf is legal), an out_normals /
 * out_colors that does not match its input, more than 2^32 - 256 vertices or triangle corners, misaligned (4 byte) pointers, an
 * output that overlaps an input or another output.  Refused behind the first launches, with BSLAM_ERR_INVALID_ARGUMENT and no output
 * written: an index >= V (never dereferenced) and "a vertex is not finite".  Per round: two stable radix sorts over the key bits in
 * use -- (edge, slot) and (vertex, slot) -- head flags and their scan, an evaluation pass with one lane per edge that walks the fans
 * of its ends, integer atomic minima for m1, a fan walk for m2, one read-back of the selected count and the error word, the
 * collapses, and the keep-flag / scan / scatter of the triangles.  No floating-point atomics.  Scratch lives in a context slab of its
 * own that the first call reserves.  Synchronises `stream`.  Every rank of a surfel-sharded run computes the same result. */
int bslam_decimate_mesh(bslam_context* ctx, void* stream, uint32_t vertex_count, uint32_t triangle_count, const float* positions,
                        const float* normals, const void* colors, const uint32_t* indices, uint32_t target_vertices, float boundary_weight,
                        float max_cost, uint32_t max_rounds, float* out_positions, float* out_normals, void* out_colors,
                        uint32_t* out_indices, uint32_t* vertex_map, uint32_t* out_vertex_count, uint32_t* out_triangle_count,
                        uint32_t* out_rounds);
/* The device time in milliseconds, summed over the rounds, of the seven stages of the last bslam_decimate_mesh on `ctx` that ran
 * while bslam_profile_enable was on (HOST out): {keys, the two sorts, head flags with their scan and in round 1 the quadrics,
 * evaluation, m2 and selection, cut and collapses, triangle compaction}.  For tools/bench_decimate_mesh.py. */
int bslam_decimate_stage_times(bslam_context* ctx, float* stage_ms7);
/* The collapses of every round of the last bslam_decimate_mesh on `ctx`: *rounds entries, of which the first `capacity` are copied
 * to collapses (HOST out; may be null with capacity 0). */
int bslam_decimate_round_collapses(bslam_context* ctx, uint32_t* collapses, uint32_t capacity, uint32_t* rounds);

/* Mesh smoothing: the Taubin lambda|mu filter over the one-ring, and vertex normals recomputed from the geometry (DESIGN.md 8 "Mesh
 * smoothing", csrc/smooth_kernels.hpp).  Everything that decides a bit is float64, `+ - * /` separately in the written order,
 * nothing contracted; fp32 inputs are widened first and a result is narrowed to fp32 once.  cross and dot are those of "Mesh
 * decimation".
 * 1. Live triangles: a triangle that repeats an index is ignored everywhere; the others are live.
 * 2. Neighbours: N(v) is the set of distinct vertices that share a live triangle with v, in ascending id; c(v, u) the number of live
 *   triangles that hold both.  v is a boundary vertex iff some u has c(v, u) = 1.  An edge with three or more uses is interior.
 * 3. Stencil S(v) by boundary_mode:  0 (fixed): empty for a boundary vertex, N(v) for every other;  1 (rim): {u in N(v) : c(v, u) = 1}
 *   for a boundary vertex -- the rim is smoothed along itself, the VCG convention --, N(v) for every other;  2 (free): N(v) for every
 *   vertex.  A vertex with an empty stencil keeps its position bits through every step: isolated vertices, fixed boundaries, a mesh
 *   without triangles.
 * 4. One step with factor f, a Jacobi step over the previous positions:  per axis s starts from the first member of S(v) and adds the
 *   others in ascending id;  m = s / (double)|S(v)|;  p' = (float)(p + f * (m - p)) with f the fp32 parameter widened.
 * 5. An iteration is a step with lambda, then a step with mu unless mu == 0 (plain Laplacian smoothing).  The stencils are built once
 *   per call.  iterations == 0 returns the positions bit for bit.
 * 6. Normals, written only if out_normals is given, from the final positions:  g(v) starts from +0.0 and adds, over the live triangles
 *   at v in ascending t, cross(b - a, c - a) with a, b, c the corners in index order -- not normalised, so area weighted;
 *   ss = (g.x g.x + g.y g.y) + g.z g.z;  the normal is (float)(g / sqrt(ss)) per axis.  Triangles of bslam_extract_mesh are
 *   counter-clockwise seen from free space, so these normals point the way its own do.  When ss is not > 0 or v has no live
 *   triangle, the normal is the input normal if `normals` is given, else (0, 0, 0).
 * 7. Vertex count, triangle count and indices do not change; colours are no argument.
 * bslam_smooth_mesh: positions float[3 V], normals float[3 V] (may be null), indices uint32[3 T], out_positions float[3 V] and
 * out_normals float[3 V] (may be null, whether or not normals is given) are device arrays, 4 byte aligned.  V == 0 is legal with
 * T == 0, and T == 0 is a point cloud: positions are copied, normals are the input's or zero.  Refused without a launch: null
 * required arguments, a lambda that is not finite or outside (0, 1], a mu that is not finite or outside [-1, 0], boundary_mode > 2,
 * iterations > 65535, more than 2^32 - 256 vertices or 6 T adjacency entries, misaligned pointers, an output that overlaps an input
 * or the other output.  Refused behind the first launches, by a device error bit, with BSLAM_ERR_INVALID_ARGUMENT and no output
 * written: an index >= V (never dereferenced; the message of the mesh component calls) and "a vertex is not finite".  Once per call: a
 * key pass (six directed pairs v << bits | u and three corners per live triangle), the stable radix sort of decimation over (pair,
 * slot) and, for normals, over (vertex, slot), head flags and their scan, and a pass that writes the neighbour list of every vertex
 * -- ascending in u by construction; the run length of a pair is c(v, u) -- then one read-back of the error word.  Per step one launch
 * with one lane per vertex; iterations x (1 or 2) launches between the input, two working buffers and the output.  No
 * floating-point atomics.  Scratch lives in a context slab of its own that the first call reserves.  Synchronises `stream`.  Every
 * rank of a surfel-sharded run computes the same result. */
int bslam_smooth_mesh(bslam_context* ctx, void* stream, uint32_t vertex_count, uint32_t triangle_count, const float* positions,
                      const float* normals, const uint32_t* indices, uint32_t iterations, float lambda, float mu, uint32_t boundary_mode,
                      float* out_positions, float* out_normals);
/* The device time in milliseconds of the five stages of the last bslam_smooth_mesh on `ctx` that ran while bslam_profile_enable was
 * on (HOST out): {keys, sort(s), adjacency, steps, normals}, from events on the call's stream; the read-back between adjacency and
 * steps is in none of them.  Zeros before such a call.  For tools/bench_smooth_mesh.py. */
int bslam_smooth_stage_times(bslam_context* ctx, float* stage_ms5);

/* Mesh repair: welding and removal of what a mesh should not hold, the census of its edges and boundary loops, and the closing of
 * small holes (DESIGN.md 8 "Mesh repair", csrc/repair_kernels.hpp).  Everything is integer but the centroid of a hole, so nothing
 * depends on the order of execution: two calls give identical bits.  A slot is 3 t + k: corner k of triangle t, and the directed
 * half-edge from corner k to corner (k + 1) % 3 (the slot of "Mesh decimation").
 * Clean; weld, remove_duplicates and remove_unreferenced are 0 or 1:
 *   Representative.  With weld, two vertices are the same iff their three coordinates are equal as floats (-0.0f equals +0.0f; the bits
 *   are compared otherwise); the representative rep(v) of v is the smallest vertex id among the vertices that are the same as v.  Its
 *   position, normal and colour are the output's: nothing is averaged.  Without weld rep(v) = v.
 *   Triangles.  Triangle t is looked at as (rep(i0), rep(i1), rep(i2)).  It is degenerate iff two of the three are equal, and is
 *   dropped.  With remove_duplicates, two triangles that are not degenerate and have the same set of three representatives -- whatever
 *   their orientation or rotation -- are duplicates: the one with the smallest triangle id stays, the others are dropped.  The
 *   surviving triangles keep their corner order and their relative order.
 *   Vertices.  Vertex v is kept iff rep(v) = v and (remove_unreferenced is 0, or T == 0 -- a point cloud keeps its points --, or a
 *   surviving triangle names it).  Kept vertices keep their relative order and the bits of their attributes, so a clean mesh comes back
 *   identical and the operation is idempotent.  With all three flags 0 the result is the input less its degenerate triangles.
 *   vertex_map[v] = the new id of rep(v), triangle_map[t] = the new id of t; 0xffffffff where that was dropped.
 *   counts4 = {V - the number of representatives, representatives that were not kept, degenerate triangles, duplicate triangles}.
 * bslam_clean_mesh: the arrays are those of bslam_simplify_mesh (device; room for V vertices and T triangles; out_normals and
 * out_colors exactly when their inputs are given), vertex_map uint32[V] and triangle_map uint32[T] may be null; the two counts and
 * counts4 are returned on the host; nothing at or beyond the counts is written.  V == 0 is legal with T == 0.  Refused without a
 * launch: null required arguments, a flag other than 0 or 1, an out_normals / out_colors that does not match its input, more than
 * 2^32 - 256 vertices or triangles, misaligned (4 byte) pointers, an output that overlaps an input or another output.  Refused behind
 * the launches that precede the scatter, by a device error bit, with BSLAM_ERR_INVALID_ARGUMENT and no output written: an index >= V
 * (never dereferenced) and "a vertex is not finite" (checked with and without weld).  Weld: the stable radix sort twice, by the bits
 * of z over 32 bits and then by y << 32 | x over 64, so the head of a run of equal keys is its smallest id; head flags, their scan,
 * and two passes that hand the head to its run.  Duplicates: the same two-pass sort over the sorted triple (lo, mid, hi), by hi over
 * `bits` bits and then by lo << bits | mid over 2 bits, bits = those of a vertex id.  Then flags, two scans, one read-back, one scatter.
 * Topology, of the indices alone; a triangle that repeats an index is refused ("a triangle repeats an index": clean first):
 *   Edges.  The undirected edge of a slot is the pair of its two ends; edge_uses[slot] = the number of slots with that edge.  An edge
 *   with 1 use is a boundary edge, with 2 an interior edge, with 3 or more a non-manifold edge.  An interior edge whose two slots run
 *   in the same direction is inconsistently oriented.  euler = referenced vertices - unique edges + T.
 *   Loops.  A boundary slot is the slot of a boundary edge.  A vertex is passable iff exactly one boundary slot starts at it and
 *   exactly one ends at it; any other vertex touched by a boundary slot is blocked.  next(h) is the boundary slot that starts where h
 *   ends, defined iff that vertex is passable.  A loop is a cycle of next; its id is its smallest slot.  loop_of_slot[h] is that id
 *   for the slots on a loop and 0xffffffff for every other slot: those of other edges, and boundary slots whose walk meets a blocked
 *   vertex (open_boundary_slots counts the latter).  loops, longest_loop (in edges) and loop_edges (their sum over the loops).
 * bslam_mesh_topology: indices uint32[3 T], edge_uses uint32[3 T] and loop_of_slot uint32[3 T] (either may be null) are device arrays;
 * *report is written on the host.  V == 0 is legal with T == 0.  Refused without a launch: null ctx or report, more than 2^32 - 256
 * vertices or slots, misaligned pointers, an output that overlaps the indices or the other output.  An index >= V and a repeated
 * index are reported behind the key pass, before anything is decoded or written: *report and both outputs stay untouched.  One
 * stable sort of (edge, slot), head flags and their scan, the run starts, a census pass, a scan of the boundary flags, a read-back of the number B of
 * boundary slots, then ceil(log2 B) + 1 rounds of pointer jumping between two buffers (label = min(label, label[next]), open |=
 * open[next], next = next[next]) whatever the loops look like, an integer count per label, and one read-back.
 * Hole filling, 3 <= max_hole_edges <= 4096:
 *   The topology of the input; every loop of n <= max_hole_edges edges is filled, in ascending loop id.  Its slots are visited from
 *   its smallest slot h0 along next.  The new vertex: position, per axis, (float)(s / (double)n) with s the double sum of the origins
 *   of the slots in that order, the first added to 0.0;  colour, if present, (S + n / 2) / n per channel in integers, alpha included
 *   (the rounding of bslam_fuse_keyframes);  normal, if present, (float)(g / sqrt(gg)) per axis with g the double sum of the origins'
 *   normals in that order and gg = (g.x g.x + g.y g.y) + g.z g.z, or (0, 0, 0) unless gg is finite and > 0.  Slot h = (a -> b) gives
 *   the triangle (b, a, new vertex): counter-clockwise, consistent with the triangle across the boundary edge.
 *   Output: the input, unchanged; then the new vertices in loop order; then the new triangles by (loop, place in the walk).
 *   hole_of_triangle[i] = the ordinal of the loop of appended triangle i.  Larger loops and everything on a blocked vertex stay open.
 * bslam_fill_mesh_holes: inputs as bslam_clean_mesh; out_positions float[3 vertex_capacity], out_normals, out_colors (exactly when
 * their inputs are given), out_indices uint32[3 triangle_capacity], hole_of_triangle uint32[triangle_capacity - T] (may be null).
 * *out_vertex_count = V + *filled_holes and *out_triangle_count on the host.  When out_positions or out_indices is null, or a count
 * exceeds its capacity, only the counts are returned and nothing is written: call once for the counts and once with buffers
 * (bslam_extract_mesh).  Refusals as bslam_clean_mesh and bslam_mesh_topology, and max_hole_edges outside [3, 4096].  One lane per
 * loop walks it.
 * All three: scratch lives in a context slab of its own that the first of these calls reserves; they synchronise `stream`.  Every
 * rank of a surfel-sharded run holds the same mesh and computes the same result. */
typedef struct bslam_mesh_report {
  uint32_t referenced_vertices, unique_edges, boundary_edges, interior_edges, nonmanifold_edges, inconsistent_edges;
  uint32_t blocked_vertices, loops, longest_loop, loop_edges, open_boundary_slots, reserved;
  int64_t euler;
} bslam_mesh_report;
int bslam_clean_mesh(bslam_context* ctx, void* stream, uint32_t vertex_count, uint32_t triangle_count, const float* positions,
                     const float* normals, const void* colors, const uint32_t* indices, int weld, int remove_duplicates,
                     int remove_unreferenced, float* out_positions, float* out_normals, void* out_colors, uint32_t* out_indices,
                     uint32_t* vertex_map, uint32_t* triangle_map, uint32_t* out_vertex_count, uint32_t* out_triangle_count,
                     uint32_t* counts4);
int bslam_mesh_topology(bslam_context* ctx, void* stream, uint32_t vertex_count, uint32_t triangle_count, const uint32_t* indices,
                        bslam_mesh_report* report, uint32_t* edge_uses, uint32_t* loop_of_slot);
int bslam_fill_mesh_holes(bslam_context* ctx, void* stream, uint32_t vertex_count, uint32_t triangle_count, const float* positions,
                          const float* normals, const void* colors, const uint32_t* indices, uint32_t max_hole_edges,
                          uint32_t vertex_capacity, uint32_t triangle_capacity, float* out_positions, float* out_normals,
                          void* out_colors, uint32_t* out_indices, uint32_t* hole_of_triangle, uint32_t* out_vertex_count,
                          uint32_t* out_triangle_count, uint32_t* filled_holes);
/* The device time in milliseconds of the stages of the last of the three calls above on `ctx` that ran while bslam_profile_enable
 * was on (HOST out), each between a pair of events on the call's stream, zero where a stage did not run.  bslam_clean_mesh: {vertex
 * keys, weld sorts, representatives, triangle keys, triangle sorts, duplicates, flags and scans, scatter}.  bslam_mesh_topology: {keys,
 * sort, census, loops, 0, 0, 0, 0}.  bslam_fill_mesh_holes: those four, then {scans of the holes, copy and fans, 0, 0}.  For
 * tools/bench_mesh_repair.py. */
int bslam_repair_stage_times(bslam_context* ctx, float* stage_ms8);

/* Mesh orientation: one winding per connected piece, and a rule for which side is out (DESIGN.md 8 "Mesh orientation",
 * csrc/orient_kernels.hpp).  Slots and edges are those of "Mesh repair"; the same triangles are refused (an index >= V, a repeated
 * index, a position that is not finite).
 *   Seams.  A seam is an edge with exactly two uses.  It disagrees iff its two slots start at the same vertex (the test that
 *   inconsistent_edges of bslam_mesh_topology counts), else it agrees.
 *   Patches.  Two triangles are joined iff they share a seam; edges with one use or with three or more join nothing.  A patch is a
 *   connected component of the triangles under joins; its id is its smallest triangle id.  A patch is closed iff every slot of every
 *   triangle of it lies on a seam.
 *   flip0.  A patch is orientable iff bits f[t] exist with f[a] ^ f[b] = disagrees(seam) for every seam (a, b) of it; flip0 is the one
 *   such assignment with flip0[patch id] = 0.  A patch that is not orientable (a Moebius band) is returned unchanged and counted.
 *   Side.  flipped[t] = flip0[t] ^ invert[patch of t] in an orientable patch and 0 in any other.  A flipped triangle (a, b, c) is
 *   written as (a, c, b); triangle order and vertices do not change.  invert by `mode`:
 *     0, majority: invert = 1 iff more triangles of the patch have flip0 = 1 than flip0 = 0 (a tie: 0).  The fewest triangles change.
 *     1, normals: a triangle (i0, i1, i2), with i1 and i2 exchanged where flip0 = 1, votes by the sign of
 *       (cr.x n.x + cr.y n.y) + cr.z n.z,  cr = cross(p1 - p0, p2 - p0),  n = (n0 + n1) + n2  per component,
 *       all in float64 from the fp32 inputs, cross(u, v) = (u.y v.z - u.z v.y, u.z v.x - u.x v.z, u.x v.y - u.y v.x), nothing contracted;
 *       a NaN votes for neither side.  invert = 1 iff the negative votes outnumber the positive ones; equal counts, zero included,
 *       fall back to majority.
 *     2, volume: c = the componentwise minimum of all V positions, D = the largest of the three extents max - min, both taken as
 *       float64; e = the frexp exponent of D (D = m 2^e, 0.5 <= m < 1), k = 58 - 3 e - bit_length(T).  A triangle, exchanged as above,
 *       adds q = llrint(ldexp((a.x cr.x + a.y cr.y) + a.z cr.z, k)), a = p0 - c, cr = cross(p1 - c, p2 - c), rounded to nearest even;
 *       |q| < 6 * 2^(58 - bit_length(T)), so the int64 sum over a patch is exact (|sum| < 2^61) and has no order.  invert = 1 iff it is
 *       negative.  A patch that is not closed, a sum of zero and D = 0 fall back to majority.
 *   Report.  patches = orientable_patches + nonorientable_patches; closed_patches of either kind; seams and those that disagree in the
 *   input and in the output (the latter lie in the patches that are not orientable); flipped_triangles; inverted_patches and
 *   fallback_patches count orientable patches only (fallback_patches is 0 in mode 0).
 * bslam_orient_mesh: positions float[3 V], normals float[3 V] (read in mode 1 alone, may be null otherwise), indices and out_indices
 * uint32[3 T], flipped uint8[T] and patch_of_triangle uint32[T] (either may be null) are device arrays; *report is written on the
 * host.  V == 0 is legal with T == 0, and T == 0 gives a report of zeros.  Refused without a launch: null ctx or report, a mode other
 * than 0, 1, 2, mode 1 without normals, more than 2^32 - 256 vertices or slots, a null array that has elements, misaligned (4 byte,
 * flipped included) pointers, an output that overlaps an input or another output -- out_indices == indices too: the call is not in
 * place.  Refused behind the key pass by a device error bit, before anything is written: the three refusals named above.  The census's
 * key pass, stable sort, head flags, scan and run starts; then one launch with a lane per sorted slot that joins the two triangles of
 * every seam in a lock-free union-find over uint32[T] words parent << 1 | parity (the smaller root wins; a hook is a compare-and-swap
 * of the losing root's word; path halving stores (grandparent, p1 ^ p2) as one word); a second launch over the seams that marks a patch
 * whose two triangles meet their root with the wrong parity; a launch per triangle that writes patch and flip0 and adds the counts and
 * the votes at the root, summed within the wave first; one over the roots that decides; one that writes.  Patch ids, flip0 of
 * orientable patches and the orientable flag do not depend on which thread won which swap.  Scratch is the slab of "Mesh repair"; the
 * call synchronises `stream`.  While profiling is on, bslam_repair_stage_times gives {position check, bounds and keys, sort, runs,
 * union-find, conflict pass, patches and votes, decision and indices, 0}. */
typedef struct bslam_orient_report {
  uint32_t patches, orientable_patches, nonorientable_patches, closed_patches, seams, disagreeing_seams_before, disagreeing_seams_after;
  uint32_t flipped_triangles, inverted_patches, fallback_patches;
} bslam_orient_report;
int bslam_orient_mesh(bslam_context* ctx, void* stream, uint32_t vertex_count, uint32_t triangle_count, const float* positions,
                      const float* normals, const uint32_t* indices, int mode, uint32_t* out_indices, uint8_t* flipped,
                      uint32_t* patch_of_triangle, bslam_orient_report* report);

/* Surface evaluation: the distance from each of N points to the nearest triangle of an indexed mesh, bounded by a search radius
 * (DESIGN.md 8 "Surface evaluation", csrc/distance_kernels.hpp).  All arithmetic is fp32 and nothing is contracted implicitly;
 * `/` and sqrtf are correctly rounded; dot(a, b) = fmaf(a.z, b.z, fmaf(a.y, b.y, a.x * b.x)) and cross has unfused components
 * (csrc/device_math.hpp).  Point p, triangle t with vertices a, b, c = positions[indices[3 t + 0 .. 2]], R = max_distance.
 * Box:
 *   lo, hi = the component-wise minimum and maximum of a, b, c.  t is a candidate for p iff all nine coordinates of the triangle
 *   are finite and on every axis p.a >= lo.a - R && p.a <= hi.a + R (the two sums rounded to fp32, float comparisons).  A point
 *   with a NaN or infinite coordinate has no candidate.
 * Segment, seg(p, a, b):
 *   e = b - a, w = p - a, ee = dot(e, e), we = dot(w, e);  t = ee > 0 ? we / ee : 0, then t = t < 0 ? 0 : (t > 1 ? 1 : t);
 *   q.k = fmaf(-t, e.k, w.k);  the value is dot(q, q).
 * Face, face(p, a, b, c):
 *   u = b - a, v = c - a, w = p - a, n = cross(u, v), nn = dot(n, n).  There is a face term iff nn > 0 and
 *   dot(cross(u, w), n) >= 0 and dot(cross(c - b, p - b), n) >= 0 and dot(cross(a - c, p - c), n) >= 0;  then
 *   d = dot(w, n) / sqrtf(nn) and the value is d * d.
 * Pair:
 *   d2(p, t) = the minimum of seg(p, a, b), seg(p, b, c), seg(p, c, a) and the face term if there is one; a NaN is no value.
 *   Degenerate triangles need no special case: (i, i, i) measures the distance to a point (a point cloud), (i, i, j) to a
 *   segment.  Duplicated triangles are legal.
 * Result:
 *   best = the smallest d2 over the candidates of p, triangle = the smallest t that attains it.  The point hits iff
 *   best <= fl(R * R) (formed on the host).  On a hit distance = sqrtf(best); else distance = +INFINITY and triangle =
 *   0xffffffff.  Nothing depends on the order of execution: two calls give identical bits.
 * bslam_point_mesh_distance: points float[3 N], positions float[3 V], indices uint32[3 T], out_distance float[N] and
 * out_triangle uint32[N] (may be null) are device arrays, non-null where not empty, 4 byte aligned, no output overlapping
 * anything.  Refused without a launch: a null context or out_distance, a max_distance or cell_size that is not finite and > 0,
 * max_grid_entries == 0, more than 2^32 - 256 points or triangles.  An index >= V is never dereferenced:
 * BSLAM_ERR_INVALID_ARGUMENT, outputs untouched.  N == 0 and T == 0 are legal; with T == 0 every point misses.
 * Grid: a uniform grid of cell_size holds each valid triangle in every cell its dilated box [lo - R, hi + R] touches, and a
 * point reads only its own cell.  origin.a = the minimum of the computed lo.a - R; the cell of x is
 * floorf((x - origin.a) * fl(1 / cell_size)), monotone in x, so a point that passes the box predicate lies in a cell the
 * triangle is registered in: the grid is exactly conservative, and it changes no result.  *grid_cells and *grid_entries (host,
 * may be null) receive the number of cells and of (triangle, cell) entries.  If the entries exceed max_grid_entries (or
 * 2^32 - 1), or the cells BSLAM_POINT_MESH_MAX_CELLS (2^26: the scans' 32-bit totals stay safe and the per-cell words at
 * 1 GiB; *grid_cells then holds the number asked for, saturated), the call stops behind the count pass: outputs untouched,
 * BSLAM_ERR_INVALID_ARGUMENT, both
 * numbers in bslam_last_error -- use a larger cell_size.  Scratch lives in a context slab that grows on demand.  While profiling
 * is on, bslam_debug_cull_stats counts the pairs the grid offered and, as "culled", those the box predicate rejected.
 * Synchronises `stream`.  Every rank of a surfel-sharded run holds the same mesh. */
#define BSLAM_POINT_MESH_MAX_CELLS (1ull << 26)
int bslam_point_mesh_distance(bslam_context* ctx, void* stream, uint32_t point_count, const float* points, uint32_t vertex_count,
                              const float* positions, uint32_t triangle_count, const uint32_t* indices, float max_distance,
                              float cell_size, uint64_t max_grid_entries, float* out_distance, uint32_t* out_triangle,
                              uint64_t* grid_cells, uint64_t* grid_entries);

/* Nearest triangle: the distance from each of N points to the nearest triangle of an indexed mesh with any search radius,
 * including none (DESIGN.md 8 "Nearest triangle", csrc/bvh_kernels.hpp): a bounding-volume hierarchy over the triangles in place
 * of the grid, at a cost that does not depend on the radius.  Arithmetic, dot, cross, `/` and sqrtf are those of "Surface
 * evaluation".  Point p, triangle t with vertices a, b, c = positions[indices[3 t + 0 .. 2]], R = max_distance.
 * Validity:
 *   An index >= vertex_count is never dereferenced: BSLAM_ERR_INVALID_ARGUMENT, outputs untouched.  A triangle with a coordinate
 *   that is not finite is not part of the mesh for this call.  A point with a coordinate that is not finite is a miss.
 * Box:
 *   box(t) = (lo, hi), the component-wise fp32 minimum and maximum of a, b, c.
 * Box distance:
 *   on each axis e.a = max(lo.a - p.a, p.a - hi.a, 0) (two fp32 subtractions);  b2(p, box) = fmaf(e.z, e.z, fmaf(e.y, e.y, e.x * e.x)),
 *   the nesting of dot.
 * Pair:
 *   d2(p, t) = max(pair(p, t), b2(p, box(t))), where pair is d2 of "Surface evaluation": three segments and the face term, a NaN
 *   is no value (+infinity when nothing is a value).
 * Result:
 *   best = the smallest d2 over the valid triangles, triangle = the smallest t that attains it.  The point hits iff best is finite
 *   and best <= fl(R * R); R = +INFINITY is legal and means no radius.  On a hit distance = sqrtf(best); else distance =
 *   +INFINITY and triangle = 0xffffffff.
 * Why the clamp by b2: the true distance to a triangle is never below the distance to its box, so the clamp only raises values
 *   that rounding made too small -- and it makes pruning exact.  fp32 subtraction, max, the product of two non-negative numbers
 *   and fmaf with non-negative addends are monotone under round-to-nearest; so for boxes A inside B, b2(p, B) <= b2(p, A) as
 *   floats; so b2(p, box of a node) <= b2(p, box(t)) <= d2(p, t) for every triangle t below the node.  The traversal skips a
 *   subtree if and only if b2(p, box of its node) > min(best so far, fl(R * R)), and enters it on equality, where a lower index
 *   may tie: nothing that could be the result is ever skipped.  The result therefore depends on the rule alone -- not on the
 *   shape of the tree, the width of the Morton code, the order of the traversal or the order in which atomics arrive -- and two
 *   calls give identical bits.  Where no clamp is active at a minimum (the usual case) the result equals that of
 *   bslam_point_mesh_distance at the same R bit for bit.
 * bslam_nearest_triangle: arrays, alignment, overlap rules and the caps of 2^32 - 256 points or triangles as in
 * bslam_point_mesh_distance.  Refused without a launch: a null context or out_distance, a max_distance that is not > 0 (a NaN
 * included).  Refused behind the census: more than 2^31 valid triangles (a child reference keeps one bit for the leaf flag).
 * N == 0 and T == 0 are legal; with T == 0, or without a valid triangle, every point misses.  *leaves (host, may be null)
 * receives the number of valid triangles, the leaves of the tree, and *height (host, may be null) the number of edges from the
 * root to the deepest leaf, at most 62 (30 key bits + 32 index bits: the bound the traversal stack is sized from); 0 for a
 * single leaf.  Scratch and the tree live in a context slab that grows on demand and is released by bslam_destroy.  While
 * profiling is on, bslam_debug_cull_stats counts the nodes the query fetched as `tested` and the triangles it evaluated as
 * tested - culled (modulo 2^64).  Synchronises `stream`.
 * bslam_debug_nearest_triangle_tree copies the tree of the last bslam_nearest_triangle call of the context to the host, for tests:
 * *leaves = L, its leaves (0: there is none, nothing else is written).  If L > leaf_capacity nothing else is written either.
 * Node 0 .. L - 2 are the internal nodes and node 0 is the root; node L - 1 + j is leaf j (with L == 1 node 0 is that leaf).
 * parent uint32[2 L - 1] (0xffffffff for the root), children uint32[2 (L - 1)] (the two children of internal node i at 2 i and
 * 2 i + 1), boxes float[6 (2 L - 1)] (lo.xyz, hi.xyz per node) and leaf_triangle uint32[L] are host arrays.  Children and the
 * boxes of all nodes but the root are read from the nodes as the query fetches them.  Synchronises the device. */
int bslam_nearest_triangle(bslam_context* ctx, void* stream, uint32_t point_count, const float* points, uint32_t vertex_count,
                           const float* positions, uint32_t triangle_count, const uint32_t* indices, float max_distance,
                           float* out_distance, uint32_t* out_triangle, uint32_t* leaves, uint32_t* height);
int bslam_debug_nearest_triangle_tree(bslam_context* ctx, uint32_t leaf_capacity, uint32_t* parent, uint32_t* children, float* boxes,
                                      uint32_t* leaf_triangle, uint32_t* leaves);

/* Mesh rays: what a ray hits on an indexed mesh -- the closest hit, or whether there is any -- and from how many views a point is
 * seen (DESIGN.md 8 "Mesh rays", csrc/ray_kernels.hpp), over the tree of "Nearest triangle".  Every value is fp32 in the order
 * written; nothing is contracted; `/` and sqrtf are correctly rounded; dot is that of "Surface evaluation".  The result is a
 * function of this rule alone, not of the tree's shape, the traversal order or the width of the Morton code: a brute-force
 * restatement over all N x T pairs reproduces every bit.
 * Ray:
 *   origin o, direction d (not normalised: t is in units of d), interval [t_min, t_max].  A ray misses everything if one of its
 *   six components is not finite, if d == (0, 0, 0), if a bound is a NaN or if t_min > t_max; infinite bounds are legal.
 *   Triangles are valid as in "Nearest triangle" (nine finite coordinates) and an index >= vertex_count is handled as there.
 * Per ray:
 *   kz = the axis of the largest |d.a| (of equals the first of x, y, z), kx = kz + 1, ky = kz + 2 (mod 3), swapped if d[kz] < 0;
 *   Sx = d[kx] / d[kz], Sy = d[ky] / d[kz], Sz = 1 / d[kz];  inv.a = 1 / d.a on each axis.
 * Triangle test (Woop, Benthin, Wald 2013), vertices a, b, c:
 *   A = a - o;  Ax = A[kx] - Sx * A[kz], Ay = A[ky] - Sy * A[kz], Az = Sz * A[kz];  B and C alike.
 *   U = Cx * By - Cy * Bx,  V = Ax * Cy - Ay * Cx,  W = Bx * Ay - By * Ax: differences of two rounded products, so each changes
 *   its sign exactly when its edge is taken the other way round.  If U, V or W is exactly 0, all three are formed again in float64
 *   from the same six fp32 numbers (the products are then exact, the difference has the exact sign); the signs are read from
 *   those and U, V, W are their roundings to fp32.  (A nonzero fp32 value already has the exact sign: rounding is monotone.)
 *   The test accepts iff not (one of U, V, W is < 0 and one is > 0), and det = (U + V) + W is not 0, and
 *   t_tri = ((U * Az + V * Bz) + W * Cz) / det is no NaN.  u = V / det, v = W / det: the hit point is (1 - u - v) a + u b + v c.
 *   Both faces hit; front = det > 0: the ray meets the side from which a, b, c run counter-clockwise, the front of
 *   bslam_render_mesh.  Two triangles that share an edge or a vertex evaluate the shared edge function from bit-identical
 *   numbers, so no ray passes between them.
 * Slab:
 *   slab(ray, box) = (enter, exit).  On an axis with d.a == 0 the interval is (-inf, +inf) if lo.a <= o.a <= hi.a, else empty
 *   (+inf, -inf): no 0 x inf is ever formed there, and an origin exactly on a box plane is inside.  On any other axis
 *   t0 = (lo.a - o.a) * inv.a, t1 = (hi.a - o.a) * inv.a, and the interval is (min(t0, t1), max(t0, t1)) -- or (-inf, +inf) if
 *   one of the two is a NaN, which only 0 x inf can give (d.a subnormal, the origin on the plane).  enter = the largest of the
 *   three lower ends moved BSLAM_RAY_PAD_ULPS representable floats down, exit = the smallest of the upper ends moved as many up
 *   (-0 counts as +0; an infinity is never passed).  The slab is empty iff enter > exit.  It is monotone under inclusion of boxes
 *   as floats: for A inside B, enter(B) <= enter(A) and exit(A) <= exit(B).
 * Pair:
 *   hit(ray, t) iff the test accepts, slab(ray, box(t)) is not empty, and t_hit = min(max(t_tri, enter), exit) is finite and
 *   t_min <= t_hit <= t_max.  The slab is part of the value: the clamp makes pruning exact as b2 does in "Nearest triangle", and
 *   the padding keeps the slab from rejecting what the test accepts (axis-aligned triangles have boxes of zero thickness).
 * Closest hit: the smallest t_hit, among bit-equal ones the lowest triangle.  Any hit: whether some valid triangle hits; no
 *   triangle is returned, because which one is found first depends on the tree.
 * Why pruning is exact: a subtree is skipped iff the slab of its node's box is empty, or enter > min(best so far, t_max), or
 *   exit < t_min, and is entered on equality.  By monotonicity [enter, exit] of every triangle below lies inside the node's, and
 *   t_hit lies inside the triangle's: nothing that could be the result, or tie with it, is ever skipped.
 * bslam_mesh_rays: origins and directions float[3 N], t_range float[2 N] = (t_min, t_max) per ray or null for [0, +inf],
 * positions, indices as in bslam_nearest_triangle -- all device arrays, 4 byte aligned (the two byte arrays too), no output
 * overlapping anything, at most 2^32 - 256 rays or triangles.  mode BSLAM_RAYS_CLOSEST needs out_t float[N]; out_triangle
 * uint32[N], out_uv float[2 N] and out_front uint8[N] may be null; out_hit must be null.  A miss gives t = +INFINITY, triangle
 * 0xffffffff, uv = 0, front = 0.  mode BSLAM_RAYS_ANY needs out_hit uint8[N] (1 or 0) and every other output null.  N == 0 and
 * T == 0 are legal.  Both calls build the tree as bslam_nearest_triangle does and leave it for
 * bslam_debug_nearest_triangle_tree; *leaves and *height (host, may be null) as there.  While profiling is on,
 * bslam_debug_cull_stats counts the nodes fetched as `tested` and the triangles evaluated as tested - culled.  Both synchronise
 * `stream`.
 * bslam_mesh_visibility: for N points (device float[3 N]; normals device float[3 N] or null) and K views (HOST arrays:
 * camera_T_global[K] and centres float[3 K], the translation of each global_T_camera -- the kernel derives nothing in between),
 * point p is seen from view k iff
 *   L = camera_T_global[k] . p in the row expression of bslam_render_mesh, ((m0 x + m1 y) + m2 z) + m3, has
 *   min_depth <= L.z <= max_depth, and px = fx * (L.x / L.z) + cx, py alike, have 0 <= px < width and 0 <= py < height;
 *   and, if normals are given, dot(n, d) < 0 for d = p - centres[k];
 *   and the ray o = centres[k], d, [0, 1 - margin / sqrtf(dot(d, d))] has no hit.  An interval that is empty, or a ray that is
 *   not valid, hits nothing.
 * out_count uint32[N] = the number of views that see p, out_first uint32[N] (may be null) = the lowest of them, 0xffffffff for
 * none.  Refused without a launch: depth bounds or a margin that are not finite, min_depth > max_depth, margin < 0, a camera
 * outside the limits of bslam_render_surfels, more than BSLAM_MESH_VISIBILITY_MAX_VIEWS views.  With K == 0 all counts are 0. */
#define BSLAM_RAY_PAD_ULPS 4
#define BSLAM_RAYS_CLOSEST 0
#define BSLAM_RAYS_ANY 1
#define BSLAM_MESH_VISIBILITY_MAX_VIEWS 65536u
int bslam_mesh_rays(bslam_context* ctx, void* stream, uint32_t ray_count, const float* origins, const float* directions,
                    const float* t_range, uint32_t vertex_count, const float* positions, uint32_t triangle_count,
                    const uint32_t* indices, int mode, float* out_t, uint32_t* out_triangle, float* out_uv, uint8_t* out_front,
                    uint8_t* out_hit, uint32_t* leaves, uint32_t* height);
int bslam_mesh_visibility(bslam_context* ctx, void* stream, uint32_t point_count, const float* points, const float* normals,
                          uint32_t vertex_count, const float* positions, uint32_t triangle_count, const uint32_t* indices,
                          uint32_t view_count, const bslam_mat3x4* camera_T_global, const float* centres,
                          const bslam_camera4f* camera, float min_depth, float max_depth, float margin, uint32_t* out_count,
                          uint32_t* out_first, uint32_t* leaves, uint32_t* height);

/* Surface sampling: points drawn uniformly by area from an indexed mesh, so that what is measured at them does not depend on how
 * the mesh happens to be tessellated (DESIGN.md 8 "Surface sampling", csrc/sampling_kernels.hpp).  Integers are uint32 with
 * wrap-around; floats are fp32, nothing is contracted implicitly, and dot, cross, `/` and sqrtf are those of "Surface evaluation"
 * above.  Triangle t with vertices a, b, c = positions[indices[3 t + 0 .. 2]], `density` in samples per square unit, `seed`.
 * Hash:
 *   mix(x):  x ^= x >> 16;  x *= 0x7feb352d;  x ^= x >> 15;  x *= 0x846ca68b;  x ^= x >> 16.
 *   h(s, t, j) = mix(mix((seed + s * 0x9e3779b9) ^ mix(t)) + j);  u24(h) = h >> 8.  s selects a stream: 0 rounds the count, 1 and 2
 *   are the two coordinates of a sample.  (h(0, 0, 0) is 0 at seed 0: there triangle 0 rounds its count up.)
 * Count:
 *   u = b - a, v = c - a, n = cross(u, v), nn = dot(n, n).  If one of the nine coordinates is not finite, or !(nn > 0), the count
 *   is 0: degenerate triangles, and so a whole point cloud, yield nothing.  Otherwise area = 0.5f * sqrtf(nn), x = area * density,
 *   k = floorf(x) and count = k + (float(u24(h(0, t, 0))) * 2^-24 < x - k ? 1 : 0); an x that is not finite or is >= 2^32 counts
 *   as 2^32.  The expected count is area * density for every triangle, however small.
 * Order:
 *   sample i = offset(t) + j for 0 <= j < count(t), offset the exclusive prefix sum of the counts: the samples are ordered by
 *   (triangle, j).  N is the 64-bit total.
 * Sample (t, j):
 *   i1 = u24(h(1, t, j)), i2 = u24(h(2, t, j));  if i1 + i2 > 2^24 then i1 = 2^24 - i1 and i2 = 2^24 - i2 (the reflection of the
 *   unit square's upper half onto the lower, exact in integers and uniform on the triangle);  w1 = float(i1) * 2^-24, w2 alike,
 *   both exact;  p.k = fmaf(w2, v.k, fmaf(w1, u.k, a.k));  normal.k = n.k / sqrtf(nn);  triangle = t.
 *   A sample depends on (seed, t, j) and its triangle alone: two calls give identical bits, and duplicated triangles get
 *   different samples.
 * bslam_sample_mesh: positions float[3 V], indices uint32[3 T], out_points float[3 N], out_normals float[3 N] (may be null) and
 * out_triangles uint32[N] (may be null) are device arrays with room for `capacity` samples; *sample_count (host) receives N
 * whenever the arguments have passed and no index was bad.  When out_points is null or N > capacity, only the count is returned
 * and nothing is written: call once for the count and once with buffers, as with bslam_extract_mesh.  Nothing is written at or
 * beyond N.  Refused without a launch: a null context or sample_count, positions or indices null where not empty, a density
 * that is not finite and > 0, more than 2^32 - 256 triangles, misaligned (4 byte) pointers, outputs that overlap anything.
 * Refused behind the count pass, outputs untouched: an index >= V (never dereferenced; BSLAM_ERR_INVALID_ARGUMENT), and
 * N > 2^32 - 256 (BSLAM_ERR_INVALID_ARGUMENT, bslam_last_error names N: use a lower density; *sample_count holds N).  T == 0 and
 * V == 0 are legal: N = 0.  Three passes: the counts with the index check and their 64-bit total (one read-back), the scan over
 * the counts, and the samples, one per lane, each finding its triangle by a search over the scanned counts that is bounded by
 * ceil(log2(T + 1)) steps.  Scratch lives in a context slab of its own that the first call reserves.  Synchronises `stream`.
 * Every rank of a surfel-sharded run holds the same mesh and computes the same samples; nothing is exchanged. */
int bslam_sample_mesh(bslam_context* ctx, void* stream, uint32_t vertex_count, const float* positions, uint32_t triangle_count,
                      const uint32_t* indices, float density, uint32_t seed, uint64_t capacity, float* out_points, float* out_normals,
                      uint32_t* out_triangles, uint64_t* sample_count);

/* Surface registration: one step of an iterative closest point alignment of N points to a mesh -- the correspondences of the
 * transformed points and their normal equations (DESIGN.md 8 "Surface registration", csrc/registration_kernels.hpp).  The
 * arithmetic is fp32, nothing is contracted implicitly, and dot, cross, `/`, sqrtf, seg, face and the pair are those of "Surface
 * evaluation" above.
 * bslam_registration_prepare builds the triangle side of bslam_point_mesh_distance once -- bounds, entry count with the same
 * budget refusals and messages, records, cell scan and lists, the same grid with boxes dilated by R0 = max_distance -- and keeps
 * it in a context slab of its own.  The records hold copies of the vertices: the caller's arrays may be freed when the call
 * returns (it synchronises `stream`).  The prepared mesh stays valid until the next prepare that gets past its refusals, or
 * bslam_destroy; bslam_point_mesh_distance calls in between neither disturb it nor are disturbed.  T == 0 is legal: every point
 * of a step misses.
 * bslam_registration_step, with M = target_T_source (row-major 3 x 4, host), R = max_distance of the call:
 * Transform:
 *   p'.a = fmaf(M[a][2], p.z, fmaf(M[a][1], p.y, fmaf(M[a][0], p.x, M[a][3])));  the points themselves are never written.
 * Correspondence:
 *   the rule of bslam_point_mesh_distance for p', with the box predicate at the prepared R0 and the hit test best <= fl(R * R):
 *   the nearest triangle, the lowest index on ties.  With the identity and R == R0 distance and triangle equal
 *   bslam_point_mesh_distance bit for bit.  out_distance float[N] and out_triangle uint32[N] (device, each may be null) receive
 *   them at the point's index.
 * Offset vector v of a hit, from the winning triangle alone:
 *   its terms in the order seg ab, seg bc, seg ca, face; a later term replaces an earlier one only when it is strictly smaller.
 *   For a segment v = the q of the rule; for the face s = d / sqrtf(nn), v.k = s * n.k.
 * Rows:
 *   row(m, r, w) with c = cross(p', m), J = (m.x, m.y, m.z, c.x, c.y, c.z) adds (w * J_i) * J_j for i <= j (21 values, upper
 *   triangle, row-major), (w * J_i) * r (6 values) and r * r.
 *   BSLAM_REGISTRATION_PLANE: a hit whose triangle has nn > 0 contributes row(nh, d, w) with nh.k = n.k / sqrtf(nn),
 *     d = dot(p' - a, n) / sqrtf(nn); every other hit counts as degenerate and contributes nothing.
 *   BSLAM_REGISTRATION_POINT: every hit contributes row(e_x, v.x, w), row(e_y, v.y, w), row(e_z, v.z, w) with one weight.
 *   Huber: a = |d| (PLANE) or sqrtf(dot(v, v)) (POINT);  w = a <= k ? 1 : k / a;  rho = a <= k ? (0.5f * a) * a :
 *     k * (a - 0.5f * k), added once per pair.  huber_k = +INFINITY is legal.
 * Outputs (host): out_sums[0..20] = H, [21..26] = b, [27] = the sum of rho, [28] = the sum of r * r, [29..31] = 0;
 *   out_counts = {points, hits, pairs used, degenerate hits}, exact.  The update is left-multiplicative: delta = (translation,
 *   rotation) solves H delta = -b, M <- Exp(delta) * M; the host does that in double.
 * The sums are formed in a fixed order over the points in their original order -- per wave of 64 consecutive points by a shuffle
 * tree, then over the waves' rows by pose_reduce_kernel's two stages -- so two calls give identical bits.
 * Refused without a launch, outputs untouched: a null context, points (N > 0), matrix, out_sums or out_counts; no prepared mesh;
 * a matrix entry that is not finite; R not finite and > 0, or R > R0; huber_k not > 0 (a NaN included); an unknown mode; more
 * than 2^32 - 256 points; arrays that are misaligned or outputs that overlap.  N == 0 is legal: sums and counts zero.
 * Synchronises `stream`.  Every rank of a surfel-sharded run holds the same points and mesh and computes the same result;
 * nothing is exchanged. */
#define BSLAM_REGISTRATION_PLANE 0
#define BSLAM_REGISTRATION_POINT 1
int bslam_registration_prepare(bslam_context* ctx, void* stream, uint32_t vertex_count, const float* positions, uint32_t triangle_count,
                               const uint32_t* indices, float max_distance, float cell_size, uint64_t max_grid_entries,
                               uint64_t* grid_cells, uint64_t* grid_entries);
int bslam_registration_step(bslam_context* ctx, void* stream, uint32_t point_count, const float* points, const float* target_T_source,
                            float max_distance, int mode, float huber_k, float* out_distance, uint32_t* out_triangle,
                            float* out_sums, uint64_t* out_counts);

/* Surface views: a per-pixel ray-cast of a fused volume (depth, colour and normal from a pose, without the holes of the disc
 * view where surfels are sparse).  All arithmetic is fp32 in a fixed expression order with explicit fused multiply-adds
 * (csrc/raycast_kernels.hpp, DESIGN.md 8 "Surface views"); two calls give identical bits.  With G = global_T_camera,
 * inv_voxel = fl(1 / voxel_size) and lerp(a, b, w) = fmaf(w, b - a, a):
 *   pixel (i, j):  dx = ((float(i) + 0.5f) - cx) / fx, dy alike (the expressions of bslam_render_surfels)
 *   sample k:      t = fmaf(float(k), step, min_depth) for k = 0 .. N - 1, N = the number of k with t <= max_depth;
 *                  P.a = fmaf(G[a][2], t, fmaf(G[a][1], dy * t, fmaf(G[a][0], dx * t, G[a][3])));
 *                  g.a = (P.a - origin.a) * inv_voxel - 0.5f;  c.a = floorf(g.a);  f.a = g.a - c.a
 *   in range iff g.a >= 0 and c.a <= n.a - 2 on all axes (as floats).  Cell c is valid iff its 8 corner samples have
 *   count >= min_count; a sample is valid iff it is in range and its cell is valid.  Its value F is the trilinear interpolation
 *   of the corners D[dz][dy][dx] as seven nested lerps: the four x-edges (dy, dz) = (0,0), (1,0), (0,1), (1,1) with f.x, the
 *   two pairs (0,0)-(1,0), (0,1)-(1,1) with f.y, then f.z.
 *   The ray ends at the first k whose sample is valid with F_k < 0.  It is a hit iff k >= 1, sample k - 1 is valid and
 *   F_{k-1} >= 0:  t* = t_{k-1} + step * (F_{k-1} / (F_{k-1} - F_k)).  Otherwise, and when no k ends the ray, the pixel is
 *   empty: surfaces seen from behind, entered from unobserved space or beginning inside are not drawn.
 * Outputs as bslam_render_surfels has them (each optional, at least one; empty pixels are 0):
 *   out_depth   u16     v = metres_to_depth * t* + 0.5f;  v < 65536 ? (u16)v : 0
 *   out_normal  12 B    the gradient of the interpolant in the cell of P(t*) if that cell is valid, else in the cell of sample
 *                       k (differences of the face lerps; towards free space), rotated into the camera frame and divided by
 *                       its sqrtf length; 0 for a zero gradient
 *   out_color   uchar4  in that same cell, over the corners whose colour sample has alpha 255, in corner order, with the
 *                       trilinear weights w = (wx * wy) * wz:  {u8(sum(w * ch) / sum(w) + 0.5f) per channel, 255}; 0 when
 *                       sum(w) is not > 0 or `color` is null
 * The march needs a prepared aux buffer of the caller's: bslam_volume_views_aux_bytes gives its size (8 byte aligned device
 * memory), bslam_prepare_volume_views fills it for one (tsdf, count, min_count) -- a validity bit per cell and a flag per
 * block of 8 x 8 x 8 cells that is set iff the block holds a valid cell with a corner < 0 -- and bslam_raycast_volume reads
 * it; the library caches nothing about it, so prepare again when the volume or min_count changes.  A sample in an unflagged
 * block cannot end a ray (nested lerps with weights in [0, 1) over corners none of which is < 0 are never < 0) and is passed
 * after one test; bslam_set_culling switches that test, with identical output bits, and while profiling is on
 * bslam_debug_cull_stats counts the in-range samples that reached the test and those it skipped.
 * Refused: null arguments, no output, step / depths / metres_to_depth / voxel_size not finite and > 0, min_depth >=
 * max_depth, N > 65536, min_count < 1, outputs that are misaligned or overlap each other, the volume or the aux buffer, an
 * aux buffer that is misaligned or too small, and what bslam_extract_mesh refuses of a volume.
 * Launched on `stream` without synchronisation.  Every rank of a surfel-sharded run holds the same volume. */
int bslam_volume_views_aux_bytes(const bslam_volume* volume, size_t* bytes);
int bslam_prepare_volume_views(bslam_context* ctx, void* stream, const bslam_volume* volume, const bslam_buffer2d* tsdf,
                               const bslam_buffer2d* count, uint32_t min_count, void* aux, size_t aux_bytes);
int bslam_raycast_volume(bslam_context* ctx, void* stream, const bslam_volume* volume, const bslam_buffer2d* tsdf,
                         const bslam_buffer2d* color /* may be null */, const void* aux, const bslam_mat3x4* global_T_camera,
                         const bslam_camera4f* camera, float min_depth, float max_depth, float step, float metres_to_depth,
                         const bslam_buffer2d* out_depth, const bslam_buffer2d* out_color, const bslam_buffer2d* out_normal);

/* Views of an indexed triangle mesh from a pose (DESIGN.md 8 "Mesh views", csrc/render_mesh_kernels.hpp): depth, triangle id,
 * colour and normal of the nearest surface per pixel, with the conventions and outputs of bslam_render_surfels.  The mesh has V
 * vertices and T triangles in device arrays laid out as bslam_extract_mesh writes them -- positions float[3 V], normals
 * float[3 V] (may be null), colors uchar4[V] (may be null), indices uint32[3 T] -- and may come from anywhere.  All arithmetic
 * is fp32 in a fixed expression order; the result does not depend on the order in which triangles arrive: two calls give
 * identical bits.
 * Vertex v:  L = ((m0 x + m1 y) + m2 z) + m3 per row of camera_T_global;  px = fx * (L.x / L.z) + cx, py alike.
 * Triangle t = (a, b, c) draws nothing when two of its indices are equal; when one of its nine camera-frame coordinates is not
 * finite; when one of its three L.z lies outside [min_depth, max_depth] (dropped, not clipped); when its pixel-space area in its
 * own winding,  A = (b.px - a.px) * (c.py - a.py) - (b.py - a.py) * (c.px - a.px),  is 0; and, with cull_backfaces = 1, when
 * not A < 0.  A < 0 is front-facing: counter-clockwise seen from the camera (x right, y down, z forward), which is how
 * bslam_extract_mesh winds its triangles seen from free space.
 * Coverage: the rule of bslam_reproject_depth with the three vertices (v0, v1, v2) taken in ascending vertex id, every edge
 * evaluated from the lower id to the higher, so that two triangles that share an edge get bit-identical edge values and no
 * pixel centre falls between them.  At a pixel centre:  w0 = edge(v1 -> v2), w1 = -edge(v0 -> v2), w2 = edge(v0 -> v1); covered
 * iff all three are >= 0 or all <= 0 and s = (w0 + w1) + w2 is not 0;  b_k = (w_k / s) / z_k;  z = 1 / ((b0 + b1) + b2); drawn
 * iff z > 0.  The pixel keeps the smallest key (float_bits(z) << 32) | t: the nearest surface, and among bit-equal depths the
 * lower triangle id.
 * Outputs, each of the camera's size and optional (null = not written), at least one given, rows aligned to 2 / 4 / 4 / 4 bytes:
 *   out_depth   u16     (u16)(metres_to_depth * z + 0.5f), 0 where nothing was drawn or the value exceeds 65535
 *   out_index   u32     the triangle id, 0xFFFFFFFF where nothing was drawn
 *   out_color   uchar4  needs colors: per channel u8(fminf(z * ((b0 * c0 + b1 * c1) + b2 * c2) + 0.5f, 255.0f)) with c_k the
 *                       channel of v_k as float (perspective-correct), alpha 255; 0 where nothing was drawn
 *   out_normal  12 B    three floats, a unit vector in the camera frame, 0 where nothing was drawn or its length is 0: with
 *                       normals, z * ((b0 * n0 + b1 * n1) + b2 * n2) per component, rotated by camera_T_global and divided by
 *                       its length; without, the face normal (the cross product of the camera-frame edges b - a and c - a),
 *                       negated where it points away from the camera
 * triangle_count == 0 or vertex_count == 0 gives empty views.  An index >= vertex_count is never dereferenced: as in
 * bslam_mesh_components the call returns BSLAM_ERR_INVALID_ARGUMENT, the outputs are then unspecified, and nothing outside the
 * given buffers is touched.  Refused without a launch: null required arguments, no output at all, out_color without colors,
 * min_depth, max_depth or metres_to_depth not finite and > 0, min_depth > max_depth, cull_backfaces other than 0 or 1, a camera
 * outside the limits of bslam_render_surfels, misaligned (4 byte) arrays or image rows, outputs that overlap each other or an
 * input.  Not done: clipping at the near plane, several views per call, anti-aliasing.
 * Synchronises `stream`: the error word of the index test is read back.  The key image and the queue of large triangles live in the
 * context's scratch and are released by bslam_destroy.  Every rank of a surfel-sharded run renders the mesh it was given;
 * nothing is exchanged. */
int bslam_render_mesh(bslam_context* ctx, void* stream, const bslam_mat3x4* camera_T_global, const bslam_camera4f* camera,
                      uint32_t vertex_count, const float* positions, const float* normals /* may be null */,
                      const void* colors /* uchar4[V], may be null */, uint32_t triangle_count, const uint32_t* indices,
                      float min_depth, float max_depth, int cull_backfaces, float metres_to_depth,
                      const bslam_buffer2d* out_depth, const bslam_buffer2d* out_index, const bslam_buffer2d* out_color,
                      const bslam_buffer2d* out_normal);
/* How bslam_render_mesh works, for measurements (tools/bench_render_mesh.py); the views are the same bits for every setting.
 *   small_box                a triangle whose box holds at most this many pixel centres is drawn by its own lane, a larger one
 *                            by its whole wave (default 64; 0: no triangle by its lane alone)
 *   wave_box                 a box of more centres than this is queued and drawn by eight workgroups in a launch behind the draw
 *                            pass (default 256; 0: every box above small_box; INT_MAX: none, and that launch is left out)
 *   project_once             0 (default): the draw pass projects the three vertices of every triangle itself;  1: a vertex pass
 *                            projects every vertex once into scratch, 12 bytes per vertex, which the draw pass reads
 *   resolve_reads_projected  0 (default): the resolve pass projects the winner's vertices again;  1 (needs project_once): it
 *                            reads those records */
int bslam_set_render_mesh_tuning(bslam_context* ctx, int small_box, int wave_box, int project_once, int resolve_reads_projected);

/* Place recognition (in place of the FAST + BRIEF + DBoW2 half of vis::LoopDetector::AddImage, BS/loop_detector.cc:98-127,
 * 160-167): one Harris corner with an unoriented 256-bit BRIEF descriptor per cell of 16 x 16 pixels of a keyframe.  All
 * arithmetic is integer (csrc/place_kernels.hpp, DESIGN.md 8 "Place recognition"); two calls give identical bits.
 *   color   uchar4 image; byte 3 is the intensity L that bslam_compute_brightness writes.  Rows 4 byte aligned.
 *   depth   u16 image of the same size (at most 65535 x 65535).  Rows 2 byte aligned.
 *   cells = (height / 16) * (width / 16), row-major; partial cells at the right and bottom are ignored
 *   score = 16 (A B - C C) - (A + B)^2 in int64 with A, B, C the 5 x 5 sums of gx^2, gy^2, gx gy of the Sobel gradients
 *   A pixel is eligible iff it lies 16 pixels inside the image, its depth is neither 0 nor has bit 15 set, and
 *   score > score_threshold.  The feature of a cell is its eligible pixel of highest score (ties: lowest y, then x).
 *   out_xy[cells]       x | y << 16, or 0xFFFFFFFF for a cell without a feature
 *   out_desc[cells][8]  bit i (word i / 32, bit i % 32) = S(p + a_i) < S(p + b_i), S the 5 x 5 box sum of L and (a_i, b_i)
 *                       pair i of bslam_place_pattern; all zero for a cell without a feature
 * The outputs are device arrays, 4 byte aligned, that overlap neither each other nor the images.  Launched on `stream`
 * without synchronisation (the first call of a context uploads the point pairs synchronously). */
int bslam_extract_keyframe_features(bslam_context* ctx, void* stream, const bslam_buffer2d* color, const bslam_buffer2d* depth,
                                    int64_t score_threshold, uint32_t* out_xy, uint32_t* out_desc);

/* The 256 point pairs of the descriptor as pairs[256][4] = (ax, ay, bx, by), each in -13 ... 13 (HOST array, no GPU
 * needed).  Generator: s = 0x0BAD51A4; a draw is s = s * 1664525 + 1013904223 mod 2^32 -> ((s >> 16) % 27) - 13; four
 * draws per pair; a pair with a == b is drawn again. */
int bslam_place_pattern(int8_t* pairs);

/* Matches the features of one keyframe against n_db database keyframes by Hamming distance with a ratio test.
 *   query_xy[cells], query_desc[cells][8]   as bslam_extract_keyframe_features writes them
 *   database   n_db keyframes of 9 * cells words each: xy[cells] followed by desc[cells][8] (so a keyframe's slot is
 *              what the extraction writes with out_xy = slot, out_desc = slot + cells)
 *   For a non-empty query slot q and database keyframe k: best = the smallest distance over k's non-empty slots (ties:
 *   the lowest slot), second = the smallest over the remaining slots (257 if none; a duplicate of the best descriptor
 *   gives second == best).  Accepted iff best <= max_distance and 4 best < 3 second.
 *   out_match[n_db][cells]  int32: the matched slot, or -1 (empty query slot, k without features, rejected)
 *   out_count[n_db]         uint32: accepted matches of keyframe k
 * cells in 1 ... 2^24, n_db in 0 ... 65535 (0: nothing is launched, nothing is read), max_distance in 0 ... 256.  All
 * arrays are device memory, 4 byte aligned; the outputs overlap neither each other nor the inputs.  Launched on `stream`
 * without synchronisation. */
int bslam_match_features(bslam_context* ctx, void* stream, const uint32_t* query_xy, const uint32_t* query_desc, int cells,
                         const uint32_t* database, int n_db, int max_distance, int32_t* out_match, uint32_t* out_count);

/* The five producers below take pitched images of one size (pitch >= width * element size; u16 rows need 2 byte, colour
 * rows 4 byte alignment) and write nothing outside width x height.  The bilateral filter, the normals and the radii read a
 * pixel's neighbours, so none of their images may be another one of the same call: such a call is refused. */
/* Replaces ComputeBrightnessCUDA (BS/cuda_image_processing.cuh, kernel BS/cuda_image_processing.cu:165-194):
 * rgb_buffer has 3 bytes per pixel, color_buffer 4 (r, g, b, luma). */
int bslam_compute_brightness(bslam_context* ctx, void* stream,
                             const bslam_buffer2d* rgb_buffer, const bslam_buffer2d* color_buffer);

/* Replaces BilateralFilteringAndDepthCutoffCUDA (BS/cuda_depth_processing.cu:42-132); the exponential is
 * evaluated with the library's deterministic exp (the reference uses -use_fast_math). */
int bslam_bilateral_filter_and_depth_cutoff(
    bslam_context* ctx, void* stream, float sigma_xy, float sigma_value, float radius_factor,
    uint16_t max_depth, float raw_to_float_depth,
    const bslam_buffer2d* input_depth, const bslam_buffer2d* output_depth);

/* Replaces ComputeNormalsCUDA (BS/cuda_depth_processing.cu:134-276). */
int bslam_compute_normals(
    bslam_context* ctx, void* stream, const bslam_camera4f* depth_camera,
    const bslam_depth_params* depth_params, const bslam_buffer2d* input_depth,
    const bslam_buffer2d* output_depth, const bslam_buffer2d* normals_buffer);

/* Replaces ComputePointRadiiAndRemoveIsolatedPixelsCUDA (BS/cuda_depth_processing.cu:278-380). */
int bslam_compute_point_radii_and_remove_isolated_pixels(
    bslam_context* ctx, void* stream, const bslam_camera4f* depth_camera, float raw_to_float_depth,
    const bslam_buffer2d* depth_buffer, const bslam_buffer2d* radius_buffer,
    const bslam_buffer2d* out_depth);

/* Replaces ComputeMinMaxDepthCUDA (BS/cuda_depth_processing.cu:382-465); results valid on return. */
int bslam_compute_min_max_depth(
    bslam_context* ctx, void* stream, const bslam_buffer2d* depth_buffer, float raw_to_float_depth,
    float* min_depth, float* max_depth);

/* ------------------------------------------------------------------------- */
/* Pairwise frame tracking / odometry                        */
/* ------------------------------------------------------------------------- */
/* The image-pair variants of the pose kernels and the pyramid construction used by TrackFramePairwise
 * (BS/pairwise_frame_tracking.cc:256-678; the coarse-to-fine loop itself is host code, see
 * badslam_amd/host/pairwise_frame_tracking.hpp).  Depth pyramids are f32 (0 = invalid), colour pyramids u8
 * single channel ("textures" of the reference are plain u8 images here), normals u16.  GradientXY variant
 * (use_gradmag = false, BS/bad_slam.cc:831). */

/* Replaces ComputeBrightnessCUDA(texture overload) (BS/cuda_image_processing.cu:196-222): luma of a uchar4 image. */
int bslam_compute_brightness_from_color(bslam_context* ctx, void* stream,
                                        const bslam_buffer2d* color_buffer, const bslam_buffer2d* intensity_buffer);
/* Replaces CUDABuffer_<u8>::SetToReadModeNormalized (LV/cuda/cuda_buffer.cu:82-102). */
int bslam_set_to_read_mode_normalized(bslam_context* ctx, void* stream,
                                      const bslam_buffer2d* input_u8, const bslam_buffer2d* output_u8);
/* Replaces CalibrateDepthCUDA (BS/kernel_downsample.cu:292-330). */
int bslam_calibrate_depth(bslam_context* ctx, void* stream, const bslam_depth_params* depth_params,
                          const bslam_buffer2d* depth_buffer, const bslam_buffer2d* out_depth);
/* Replaces CalibrateDepthAndTransformColorToDepthCUDA (BS/kernel_downsample.cu:236-290). */
int bslam_calibrate_depth_and_transform_color_to_depth(
    bslam_context* ctx, void* stream, const bslam_camera4f* color_camera, const bslam_camera4f* depth_camera,
    const bslam_depth_params* depth_params, const bslam_buffer2d* depth_buffer, const bslam_buffer2d* color_u8,
    const bslam_buffer2d* out_depth, const bslam_buffer2d* out_color);
/* Replaces DownsampleImagesCUDA (BS/kernel_downsample.cu:105-234).  downsampled_color may have another size than
 * downsampled_depth (the colour camera of another pyramid level): it then halves color_u8 on its own. */
int bslam_downsample_images(
    bslam_context* ctx, void* stream, const bslam_buffer2d* depth_buffer, const bslam_buffer2d* normals_buffer,
    const bslam_buffer2d* color_u8, const bslam_buffer2d* downsampled_depth,
    const bslam_buffer2d* downsampled_normals, const bslam_buffer2d* downsampled_color);
/* Replaces AccumulatePoseEstimationCoeffsFromImagesCUDA (BS/kernels.h:181-203, BS/kernel_opt_pose.cc:99-192): the
 * "downsampled" images are the tracked frame's pyramid level (colour in the colour camera's intrinsics), the
 * "surfel" images the base frame's (colour in the depth camera's intrinsics).  Cameras are the level's (scaled).
 * H (21, upper triangle row-major) and b (6) are valid on return; visible_count may be NULL. */
int bslam_accumulate_pose_coeffs_from_images(
    bslam_context* ctx, void* stream, int use_depth_residuals, int use_descriptor_residuals,
    const bslam_camera4f* color_camera, const bslam_camera4f* depth_camera, float baseline_fx, float threshold_factor,
    const bslam_buffer2d* downsampled_depth, const bslam_buffer2d* downsampled_normals, const bslam_buffer2d* downsampled_color,
    const bslam_mat3x4* estimate_frame_T_surfel_frame,
    const bslam_buffer2d* surfel_depth, const bslam_buffer2d* surfel_normals, const bslam_buffer2d* surfel_color,
    uint32_t* visible_count, float* H, float* b);
/* Replaces ComputeCostAndResidualCountFromImagesCUDA (BS/kernels.h:205-224, BS/kernel_opt_pose.cc:194-270). */
int bslam_compute_cost_and_residual_count_from_images(
    bslam_context* ctx, void* stream, int use_depth_residuals, int use_descriptor_residuals,
    const bslam_camera4f* color_camera, const bslam_camera4f* depth_camera, float baseline_fx, float threshold_factor,
    const bslam_buffer2d* downsampled_depth, const bslam_buffer2d* downsampled_normals, const bslam_buffer2d* downsampled_color,
    const bslam_mat3x4* estimate_frame_T_surfel_frame,
    const bslam_buffer2d* surfel_depth, const bslam_buffer2d* surfel_normals, const bslam_buffer2d* surfel_color,
    uint32_t* residual_count, float* residual_sum);
/* The use_gradmag = true branch of the two functions above (BS/kernel_opt_pose.cc:121-135, 212-221; kernels
 * BS/kernel_opt_pose.cu:713-937, 1173-1338): ONE colour residual per pixel, 255 x tex(tracked gradient magnitude) - base gradient
 * magnitude, on images produced by bslam_compute_sobel_gradient_magnitude instead of the brightness images. */
int bslam_accumulate_pose_coeffs_from_images_gradmag(
    bslam_context* ctx, void* stream, int use_depth_residuals, int use_descriptor_residuals,
    const bslam_camera4f* color_camera, const bslam_camera4f* depth_camera, float baseline_fx, float threshold_factor,
    const bslam_buffer2d* downsampled_depth, const bslam_buffer2d* downsampled_normals, const bslam_buffer2d* downsampled_color,
    const bslam_mat3x4* estimate_frame_T_surfel_frame,
    const bslam_buffer2d* surfel_depth, const bslam_buffer2d* surfel_normals, const bslam_buffer2d* surfel_color,
    uint32_t* visible_count, float* H, float* b);
int bslam_compute_cost_and_residual_count_from_images_gradmag(
    bslam_context* ctx, void* stream, int use_depth_residuals, int use_descriptor_residuals,
    const bslam_camera4f* color_camera, const bslam_camera4f* depth_camera, float baseline_fx, float threshold_factor,
    const bslam_buffer2d* downsampled_depth, const bslam_buffer2d* downsampled_normals, const bslam_buffer2d* downsampled_color,
    const bslam_mat3x4* estimate_frame_T_surfel_frame,
    const bslam_buffer2d* surfel_depth, const bslam_buffer2d* surfel_normals, const bslam_buffer2d* surfel_color,
    uint32_t* residual_count, float* residual_sum);
/* Batched form of bslam_accumulate_pose_coeffs_from_images for loop verification (BS/loop_detector.cc:440-712), which
 * tracks ONE base frame against several tracked frames (non-gradmag path only, BS/loop_detector.cc:228).  Pair p uses
 * tracked_depth[p] / tracked_normals[p] / tracked_color[p] and estimates_frame_T_surfel_frame[p]; the base ("surfel")
 * images and the cameras are shared.  1 <= pair_count <= BSLAM_MAX_PAIR_BATCH.  Outputs: H[21 * p .. 21 * p + 20],
 * b[6 * p .. 6 * p + 5], visible_counts[p] (may be NULL), valid on return; row p is bit-identical to the single-pair call
 * with pair p's arguments.  One launch per stage for all pairs, one copy, one stream synchronisation. */
#define BSLAM_MAX_PAIR_BATCH 8
int bslam_accumulate_pose_coeffs_from_images_batched(
    bslam_context* ctx, void* stream, int use_depth_residuals, int use_descriptor_residuals,
    const bslam_camera4f* color_camera, const bslam_camera4f* depth_camera, float baseline_fx, float threshold_factor,
    int pair_count,
    const bslam_buffer2d* tracked_depth, const bslam_buffer2d* tracked_normals, const bslam_buffer2d* tracked_color,
    const bslam_mat3x4* estimates_frame_T_surfel_frame,
    const bslam_buffer2d* base_depth, const bslam_buffer2d* base_normals, const bslam_buffer2d* base_color,
    uint32_t* visible_counts, float* H, float* b);
/* Replaces ComputeSobelGradientMagnitudeCUDA(stream, rgbi_texture, gradmag_buffer) (BS/cuda_image_processing.cu:104-167): Sobel
 * gradient magnitude of the luma channel of a uchar4 colour image, 0..255. */
int bslam_compute_sobel_gradient_magnitude(bslam_context* ctx, void* stream, const bslam_buffer2d* color_buffer, const bslam_buffer2d* gradmag_buffer);
/* Replaces CalibrateAndDownsampleImagesCUDA (BS/kernels.h:355-366, BS/kernel_downsample.cu:40-105, 237-270): first pyramid step of
 * a tracked frame whose level 0 is not used (use_pyramid_level_0 = false): u16 raw depth -> calibrated float depth at half
 * resolution; downsample_color = 0 when the colour image already has half the depth image's resolution. */
int bslam_calibrate_and_downsample_images(
    bslam_context* ctx, void* stream, int downsample_color, const bslam_depth_params* depth_params,
    const bslam_buffer2d* depth_buffer, const bslam_buffer2d* normals_buffer, const bslam_buffer2d* color_u8,
    const bslam_buffer2d* downsampled_depth, const bslam_buffer2d* downsampled_normals, const bslam_buffer2d* downsampled_color);

/* Multi-GPU (surfel-sharded) runs of the PCG and intrinsics entry points: every rank holds its own
 * surfel shard and the full keyframe list; `allreduce` sums a device buffer of floats in place across
 * ranks (ordered after prior work on `stream`, e.g. RCCL ncclAllReduce on that stream).  It is
 * called at fixed points with sizes that are identical on all ranks:
 *   bslam_pcg_init   1 x  [r | M] of the shared unknowns (poses, intrinsics, cfactor cells)
 *   bslam_pcg_init2  1 x  1 float (sharded part of alpha_n)
 *   bslam_pcg_step1  1 x  [g of the shared unknowns | 2 floats]
 *   bslam_pcg_step2  1 x  1 float (sharded part of beta_n)
 *   bslam_optimize_intrinsics  1 x  40 floats (A, b1, colour H, b), and with depth intrinsics 1 x  8 floats per cfactor cell
 * All ranks then hold bit-identical shared unknowns without any broadcast.  NULL (default) = single GPU.
 * The reference is single-GPU; this replaces nothing in it. */
int bslam_set_allreduce(bslam_context* ctx, bslam_allreduce_fn allreduce, void* allreduce_user);

/* The library's own exchange: an RCCL communicator owned by the context (bslam_comm_{init,destroy}).  One
 * process per GPU; rank 0 obtains a unique id and hands its 128 bytes to every rank over any channel the application has
 * (MPI, a socket, torch.distributed, a file); every rank then calls bslam_comm_init.  From then on every exchange point listed
 * above -- and the K x 32 Gauss-Newton rows of bslam_estimate_frame_poses_batched when no hook is passed to it -- is an in-place
 * ncclAllReduce(sum, float) enqueued on the call's own stream, i.e. on the BA stream: no host callback, no other runtime in
 * the loop (the C++ host class needs no Python to shard).  A hook set with bslam_set_allreduce takes precedence.  RCCL is
 * opened with dlopen at the first of these calls; the library has no link dependency on it.  The reference is single-GPU;
 * these replace nothing in it. */
#define BSLAM_COMM_UNIQUE_ID_BYTES 128
int bslam_comm_get_unique_id(void* out_id, size_t bytes);
int bslam_comm_init(bslam_context* ctx, const void* unique_id, int rank, int world_size);
int bslam_comm_destroy(bslam_context* ctx);
/* Rank and size as the communicator itself reports them (ncclCommUserRank / ncclCommCount); 0 and 1 without a communicator. */
int bslam_comm_query(bslam_context* ctx, int* rank, int* world_size);

/* ------------------------------------------------------------------------- */
/* PCG (matrix-free Gauss-Newton step)                                        */
/* ------------------------------------------------------------------------- */

/* Unknown layout of BS/direct_ba_pcg.cc:270-306:
 *   [6 per keyframe except the gauge keyframe | 1 or 3 per surfel |
 *    4 + 1 + cfactor cells | 4 colour intrinsics] */
typedef struct bslam_pcg_layout {
  uint32_t unknown_count;
  uint32_t surfel_unknown_start_index;
  uint32_t depth_intrinsics_unknown_start_index; /* 0xffffffff if unused */
  uint32_t a_unknown_index;                      /* 0xffffffff if unused */
  uint32_t color_intrinsics_unknown_start_index; /* 0xffffffff if unused */
  int32_t gauge_keyframe_id;                     /* pose of this keyframe is fixed */
  int32_t optimize_poses, optimize_geometry;
  int32_t optimize_depth_intrinsics, optimize_color_intrinsics;
  int32_t use_depth_residuals, use_descriptor_residuals;
} bslam_pcg_layout;

/* The five PCG vectors and three scalars (device, float = PCGScalar,
 * BS/kernels.cuh:62), each at least unknown_count long. */
typedef struct bslam_pcg_vectors {
  float* r;
  float* M;
  float* delta;
  float* g;
  float* p;
  float* alpha_n; /* 1 float */
  float* alpha_d; /* 1 float */
  float* beta_n;  /* 1 float */
} bslam_pcg_vectors;

/* Replaces the K x PCGInitCUDA loop + memsets (BS/kernels.h:397-416,
 * BS/direct_ba_pcg.cc:315-365): r0 = -J^T W F, M = diag(J^T W J). */
int bslam_pcg_init(
    bslam_context* ctx, void* stream, const bslam_pcg_layout* layout,
    const bslam_camera4f* color_camera, const bslam_camera4f* depth_camera,
    const bslam_depth_params* depth_params,
    int keyframe_count, const bslam_keyframe_view* keyframes,
    uint32_t surfels_size, const bslam_buffer2d* surfels,
    const bslam_pcg_vectors* v);

/* Replaces PCGInit2CUDA (BS/kernels.h:418-428). */
int bslam_pcg_init2(bslam_context* ctx, void* stream, const bslam_pcg_layout* layout,
                    float a, const bslam_pcg_vectors* v);

/* Replaces the K x PCGStep1CUDA loop incl. its alpha_d / g memsets
 * (BS/kernels.h:430-452, BS/direct_ba_pcg.cc:383-425).  Quirk Q7 (the epsilon
 * term added once per keyframe) is reproduced.  A step belongs to the solve its
 * bslam_pcg_init started: the surfel buffer must not have been modified by the caller
 * since that call (the reference's solve does not touch the surfels either,
 * BS/direct_ba_pcg.cc:339-425) -- the library re-uses its sorted copy of the surfel rows
 * when the preceding call on this context was the init or a step on the same buffer. */
int bslam_pcg_step1(
    bslam_context* ctx, void* stream, const bslam_pcg_layout* layout,
    const bslam_camera4f* color_camera, const bslam_camera4f* depth_camera,
    const bslam_depth_params* depth_params,
    int keyframe_count, const bslam_keyframe_view* keyframes,
    uint32_t surfels_size, const bslam_buffer2d* surfels,
    const bslam_pcg_vectors* v, int clear_g);

/* Replaces PCGStep2CUDA (BS/kernels.h:454-465); *beta_n_host (HOST) valid on return. */
int bslam_pcg_step2(bslam_context* ctx, void* stream, const bslam_pcg_layout* layout,
                    const bslam_pcg_vectors* v, float* beta_n_host);

/* Replaces PCGStep3CUDA (BS/kernels.h:467-473). */
int bslam_pcg_step3(bslam_context* ctx, void* stream, const bslam_pcg_layout* layout,
                    const bslam_pcg_vectors* v);

/* Replaces UpdateSurfelsFromPCGDeltaCUDA (BS/kernels.h:483-489). */
int bslam_update_surfels_from_pcg_delta(
    bslam_context* ctx, void* stream, uint32_t surfels_size, const bslam_buffer2d* surfels,
    int use_descriptor_residuals, uint32_t surfel_unknown_start_index, const float* pcg_delta);

/* Replaces UpdateCFactorsFromPCGDeltaCUDA (BS/kernels.h:491-495). */
int bslam_update_cfactors_from_pcg_delta(
    bslam_context* ctx, void* stream, const bslam_buffer2d* cfactor_buffer,
    uint32_t cfactor_unknown_start_index, const float* pcg_delta);

#ifdef __cplusplus
} /* extern "C" */
#endif

#endif /* BADSLAM_HIP_H_ */
