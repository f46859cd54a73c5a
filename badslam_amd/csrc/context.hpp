// context.hpp -- host-side context of libbadslam_hip: scratch slabs, keyframe table upload,
// error reporting.  Plays the role of the reference's PoseEstimationHelperBuffers /
// IntrinsicsOptimizationHelperBuffers (BS/kernels.h:46-89): scratch is allocated once and
// re-used, launch paths never allocate unless a slab has to grow.
#pragma once

#include <hip/hip_runtime.h>

#include <cstdarg>
#include <cstdio>
#include <string>
#include <vector>

#include "device_math.hpp"

namespace bslam {

extern thread_local std::string g_last_error;

inline int fail(int code, const char* fmt, ...) {
  char buf[512];
  va_list ap;
  va_start(ap, fmt);
  vsnprintf(buf, sizeof(buf), fmt, ap);
  va_end(ap);
  g_last_error = buf;
  return code;
}

#define BSLAM_HIP_TRY(expr)                                                                         \
  do {                                                                                              \
    hipError_t e_ = (expr);                                                                         \
    if (e_ != hipSuccess) return ::bslam::fail(BSLAM_ERR_HIP, "%s failed: %s", #expr, hipGetErrorString(e_)); \
  } while (0)

// Byte offsets of the small device scalars in bslam_context::misc (kMiscBytes, zeroed at creation).
constexpr size_t kMiscActive = 0;           // int[4]: active-keyframe counters of the batched pose loop, one per in-flight iteration
constexpr size_t kMiscPairCensus = 64;      // unsigned long long[2]: in-bounds / associated pairs (bslam_debug_count_pairs)
constexpr size_t kMiscPcgScratch = 128;     // float[3]: PCGStep1's epsilon term {shared, sharded} and this rank's pair sum of alpha_d
constexpr size_t kMiscPcgPair = 160;        // float[2]: {shared, sharded} of a multi-rank PCG dot product (pcg_final_sum)
constexpr size_t kMiscDeleted = 192;        // uint32_t: surfels deleted by bslam_delete_surfels_and_update_radii
constexpr size_t kMiscMinMaxDepth = 208;    // uint32_t[2]: bits of the min / max depth of bslam_compute_min_max_depth
constexpr size_t kMiscCullStats = 224;      // unsigned long long[2]: (work slot, keyframe) pairs tested / visited by the pose kernel
constexpr size_t kMiscBytes = 256;

// A slab that only ever grows: device memory, or pinned host memory when kPinned.  Freed with its owner.
template <bool kPinned>
struct GrowingSlab {
  void* ptr = nullptr;
  size_t bytes = 0;
  GrowingSlab() = default;
  GrowingSlab(const GrowingSlab&) = delete;
  GrowingSlab& operator=(const GrowingSlab&) = delete;
  ~GrowingSlab() { release(); }
  int reserve(size_t need) {
    if (need <= bytes) return BSLAM_OK;
    release();
    const size_t want = need + need / 4 + 256;
    const hipError_t e = kPinned ? hipHostMalloc(&ptr, want, hipHostMallocDefault) : hipMalloc(&ptr, want);
    if (e != hipSuccess) {
      ptr = nullptr;
      return fail(BSLAM_ERR_OUT_OF_MEMORY, "%s(%zu) failed: %s", kPinned ? "hipHostMalloc" : "hipMalloc", want, hipGetErrorString(e));
    }
    bytes = want;
    return BSLAM_OK;
  }
  void release() {
    if (ptr) { hipError_t e = kPinned ? hipHostFree(ptr) : hipFree(ptr); (void)e; }
    ptr = nullptr;
    bytes = 0;
  }
};
using Slab = GrowingSlab<false>;
using PinnedSlab = GrowingSlab<true>;

// What a cache built from a caller's surfel buffer was built from: its address, the surfel count and the pitch.
struct SurfelKey {
  const void* ptr = nullptr;
  uint32_t size = 0;
  size_t pitch = 0;
  bool matches(const bslam_buffer2d* s, uint32_t n) const { return ptr == s->address && size == n && pitch == s->pitch; }
  void set(const bslam_buffer2d* s, uint32_t n) { ptr = s->address; size = n; pitch = s->pitch; }
  void clear() { ptr = nullptr; }
};

// Ring of pinned upload buffers: an API call takes the next slot for its small host->device uploads and
// records an event after enqueuing the copy, so calls do not have to drain the stream before re-using
// staging memory (the wait only happens if the ring wraps onto a copy that has not finished yet).
struct StagingRing {
  static constexpr int kSlots = 8;
  PinnedSlab slot[kSlots];
  hipEvent_t done[kSlots] = {};
  bool pending[kSlots] = {};
  int next = 0;
  int cur = 0;
  int acquire(size_t bytes, void** out) {
    cur = next;
    next = (next + 1) % kSlots;
    if (pending[cur]) {
      hipError_t e = hipEventSynchronize(done[cur]);
      if (e != hipSuccess) return fail(BSLAM_ERR_HIP, "hipEventSynchronize failed: %s", hipGetErrorString(e));
      pending[cur] = false;
    }
    int rc = slot[cur].reserve(bytes);
    if (rc) return rc;
    *out = slot[cur].ptr;
    return BSLAM_OK;
  }
  int commit(hipStream_t stream) {   // after the copies out of the acquired slot were enqueued
    if (!done[cur]) {
      hipError_t e = hipEventCreateWithFlags(&done[cur], hipEventDisableTiming);
      if (e != hipSuccess) return fail(BSLAM_ERR_HIP, "hipEventCreate failed: %s", hipGetErrorString(e));
    }
    hipError_t e = hipEventRecord(done[cur], stream);
    if (e != hipSuccess) return fail(BSLAM_ERR_HIP, "hipEventRecord failed: %s", hipGetErrorString(e));
    pending[cur] = true;
    return BSLAM_OK;
  }
  ~StagingRing() {
    for (hipEvent_t e : done)
      if (e) { hipError_t err = hipEventDestroy(e); (void)err; }
  }
};

// The events at the stage boundaries of a call that times its stages while profiling is on: created at their first use, destroyed
// with their owner.
template <int kCount>
struct StageEvents {
  hipEvent_t event[kCount] = {};
  StageEvents() = default;
  StageEvents(const StageEvents&) = delete;
  StageEvents& operator=(const StageEvents&) = delete;
  ~StageEvents() {
    for (hipEvent_t e : event)
      if (e) { hipError_t err = hipEventDestroy(e); (void)err; }
  }
  // Boundary `at`: an event on the stream while profiling is on, nothing otherwise.
  int mark(bool profiling, hipStream_t stream, int at) {
    if (!profiling) return BSLAM_OK;
    if (!event[at]) BSLAM_HIP_TRY(hipEventCreate(&event[at]));
    BSLAM_HIP_TRY(hipEventRecord(event[at], stream));
    return BSLAM_OK;
  }
  // The time between two recorded boundaries; both have completed.
  int elapsed(int from, int to, float* ms) const {
    BSLAM_HIP_TRY(hipEventElapsedTime(ms, event[from], event[to]));
    return BSLAM_OK;
  }
};

}  // namespace bslam

struct bslam_context {
  int device = 0;
  int tex_mode = BSLAM_TEX_FIXED_POINT_1_8;
  int cu_count = 256;
  bslam::Slab kf_table;      // KfDev[K]
  bslam::Slab records;       // PixelRecord[K][h][w] derived pixel records (16 B)
  bslam::Slab quads;         // QuadEntry[K][ch+1][cw+1] derived luma quads, 8 bytes each (only when colour images are given)
  bslam::Slab partials;      // float[tiles][K][32]
  bslam::Slab coeffs;        // float[K][32]
  bslam::Slab pose_state;    // PoseState[K]
  bslam::Slab misc;          // small device scalars
  bslam::Slab intr_cells;    // B[5][cells], D, b2, obs of the intrinsics step; or the PCG path's fp64 cell sums
  int geom_kf_chunk = -1;    // geometry iteration: keyframes per launch (0: one launch for the whole list; -1: default = one launch)
  int intr_cells_owner = 0;  // 0: intrinsics step (zeroes per call), 1: PCG (kept zero between calls)
  size_t intr_cells_cells = 0;
  bslam::PinnedSlab staging2;       // pinned host memory of the results a call reads back (read_back)
  bslam::StagingRing upload_ring;   // keyframe table / pose state uploads
  hipEvent_t iter_done[4] = {};     // batched pose loop: one event per in-flight iteration (recorded behind its flag copy)
  hipEvent_t solve_done[4] = {};    // ... recorded on the BA stream behind the iteration's solve kernel
  hipStream_t copy_stream = nullptr;   // side stream that carries the 4-byte convergence flags to the host, off the BA stream's critical path
  // what the device copy of the keyframe table holds (upload_kf_table skips an identical upload; the pose kernels rewrite
  // frame_T_global on the device and invalidate it)
  std::vector<uint8_t> kf_table_host;
  const void* kf_table_host_ptr = nullptr;
  // derived-record cache (bslam_set_keyframe_cache)
  bool keyframe_cache = false;
  std::vector<uint64_t> records_signature;   // what the depth records were built from
  std::vector<uint64_t> quads_signature;     // what the luma quads were built from
  // XCD-aware schedule: granule order (short keyframe lists) and per-surfel order, each cached per surfel buffer
  bslam::Slab quads_aux;     // luma quads of the tracked frame's colour pyramid level (odometry)
  bslam::Slab lifecycle;     // supporting-surfel cell images, scan buffers, flags of the surfel lifecycle calls
  bslam::Slab zbuffer;       // uint32[h][w]: float bits of the nearest surface per target pixel (bslam_reproject_depth); or
                             // uint64[h][w]: (float bits of the depth << 32) | surfel index (bslam_render_surfels); or those keys with
                             // the triangle id, the error word, the queue of large triangles and the projected vertices (bslam_render_mesh)
  // bslam_render_mesh (bslam_set_render_mesh_tuning): the box sizes up to which a lane and a wave draw alone, whether a vertex pass
  // projects every vertex once into `zbuffer`, and whether the resolve pass reads those records; the views are the same bits either way
  int render_mesh_small_box = 64, render_mesh_wave_box = 256;
  bool render_mesh_project_once = false, render_mesh_resolve_projected = false;
  bslam::Slab place_pattern; // uint32[256]: the BRIEF point pairs of bslam_extract_keyframe_features, uploaded by its first call
  bool place_pattern_ready = false;
  bslam::Slab fusion;        // bslam_extract_mesh: active flags and quad counts u8[cells], vertex ids and quad offsets u32[cells], scan sums;
                             // bslam_mesh_components: parent and root sizes u32[V]; bslam_filter_mesh: keep flags, ranks, scan sums
  bslam::Slab distance;      // bslam_point_mesh_distance: triangle records, cell lists, sorted points, scan sums; bslam_registration_step: its per-call scratch
  bslam::Slab registration;  // bslam_registration_prepare: words | records | cell_count (all zero between calls) | cell_start | list -- a slab of its
                             // own, because a slab that grows discards what it held and `distance` is per-call scratch
  struct PreparedMesh {      // what that slab holds; the pointers lie inside it
    bool ready = false;
    float radius = 0.f;      // R0 of the dilated boxes
    float origin[3] = {0.f, 0.f, 0.f}, inv_cell = 0.f;
    int dim[3] = {0, 0, 0};
    uint32_t cells = 0, valid = 0, triangles = 0;
    void *records = nullptr, *cell_count = nullptr, *cell_start = nullptr, *list = nullptr;
  } prepared;
  bslam::Slab bvh;           // bslam_nearest_triangle: words | keys, sorted keys u64[T] | ids, sorted ids u32[T] | per node: parents, children, box keys |
                             // per leaf: boxes | packed nodes | leaf records | the radix sort's scratch; reserved by its first call
  struct BvhTree {           // the tree of the last call (bslam_debug_nearest_triangle_tree); the pointers lie inside that slab
    uint32_t leaves = 0, height = 0;
    void *words = nullptr, *sorted_ids = nullptr, *parent_internal = nullptr, *parent_leaf = nullptr, *box_min = nullptr, *box_max = nullptr;
    void *leaf_lo = nullptr, *leaf_hi = nullptr, *nodes = nullptr, *records = nullptr;
  } bvh_tree;
  bslam::Slab ray_views;     // bslam_mesh_visibility: float4[4 K], the rows of camera_T_global and the centre of every view
  bslam::Slab sampling;      // bslam_sample_mesh: words | counts u32[T] | offsets u32[T] | scan sums; reserved by its first call
  bslam::Slab simplify;      // bslam_simplify_mesh: words | keys, sorted keys u64[V] | ids, sorted ids, head flags, ranks, clusters [V] | keep flags, ranks [T] |
                             // scan sums | the radix sort's scratch; reserved by its first call
  // bslam_simplify_mesh while profiling is on: events around its five stages and the last call's times (bslam_simplify_stage_times)
  bslam::StageEvents<6> simplify_events;
  float simplify_stage_ms[5] = {0.f, 0.f, 0.f, 0.f, 0.f};
  bslam::Slab decimate;      // bslam_decimate_mesh: words | working attributes, quadrics, parents [V] | two triangle buffers | per slot: keys, sorted keys, slots,
                             // flags, ranks, candidate keys | per vertex: fans, flags, minima | scan sums | the radix sort's scratch; reserved by its first call
  // bslam_decimate_mesh while profiling is on: events around the seven stages of a round and their sums over the last call's rounds
  // (bslam_decimate_stage_times); the collapses of every round of the last call (bslam_decimate_round_collapses)
  bslam::StageEvents<8> decimate_events;
  float decimate_stage_ms[7] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
  std::vector<uint32_t> decimate_collapses;
  bslam::Slab smooth;        // bslam_smooth_mesh: words | per directed pair: keys, sorted keys, ids, slots, head flags, ranks, neighbours, rim flags | per corner:
                             // keys, sorted keys, fans | per vertex: list and fan ends, boundary flags | working positions | scan sums | the radix sort's scratch;
                             // reserved by its first call
  // bslam_smooth_mesh while profiling is on: events around keys, sorts and adjacency, then -- behind the read-back -- around steps and normals, and
  // the last call's five stage times (bslam_smooth_stage_times)
  bslam::StageEvents<7> smooth_events;
  float smooth_stage_ms[5] = {0.f, 0.f, 0.f, 0.f, 0.f};
  bslam::Slab repair;        // bslam_clean_mesh: words | per vertex or triangle: the keys of the two sorts, sorted keys, ids, ranks, run heads, head flags | per vertex:
                             // representatives, ranks, flags | per triangle: flags, ranks | scan sums | the radix sort's scratch; bslam_mesh_topology and
                             // bslam_fill_mesh_holes: words | per slot: keys, sorted keys, slots, head flags, ranks, run starts, boundary flags and numbers | per vertex:
                             // flags, boundary counts, first boundary slot | per boundary slot: two buffers of next, label and open, loop lengths, fans | scan sums |
                             // the sort's scratch; bslam_orient_mesh: both word blocks | per slot: keys, sorted keys, slots, head flags, ranks, run starts, seam codes |
                             // referenced flags [V] | per triangle: links, patches, the sums at the root, flags | scan sums | the sort's scratch; reserved by the
                             // first of these calls
  // those calls while profiling is on: a pair of events around each of up to eight stages and the last call's times (bslam_repair_stage_times)
  bslam::StageEvents<16> repair_events;
  float repair_stage_ms[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
  bslam::Slab exchange;      // staging of the multi-rank exchanges (PCG shared unknowns, intrinsics sums)
  bslam_allreduce_fn allreduce = nullptr;   // bslam_set_allreduce: sum across the ranks of a surfel-sharded run
  void* allreduce_user = nullptr;
  void* comm = nullptr;                     // bslam_comm_init: RCCL communicator (ncclComm_t) of the surfel-sharded run
  int comm_rank = 0, comm_world = 1;
  bslam::Slab order;
  bslam::Slab centroids;     // granule centroids (scratch of make_schedule)
  bslam::Slab perm;          // per-surfel Morton order (+ sort scratch), cached like `order`
  bslam::Slab sorted_rows;   // the seven persistent surfel rows in that order, rebuilt by every call that uses it
  bslam::Slab bounds;        // float4[2 * granules]: bounding box of every granule of the sorted copy, rebuilt with it
  // what the sorted copy holds (prepare_surfels): PCGStep1 re-uses the copy PCGInit / the previous PCGStep1 of the same solve
  // made -- the surfels do not change inside a solve (BS/direct_ba_pcg.cc:339-425) -- every other call rebuilds it
  bslam::SurfelKey sorted_key;
  int sorted_key_rows = 0;
  bool sorted_key_bounds = false;
  uint64_t sorted_key_perm_serial = 0;   // the permutation the copy was made with
  uint64_t perm_serial = 0;              // counts rebuilds of `perm`
  bslam::Slab pose_list;     // batched pose loop: int n | int list[K] (the unconverged keyframes, ascending) | int pos[K] (place in the list, or -1)
  bslam::Slab vis;           // uint64[chunks][slots]: keyframes of a chunk (<= 64) a work slot visited in the last pose_accumulate launch
  bool culling = true;       // block-level frustum culling in the pair kernels (bslam_set_culling)
  int pose_list_min_keyframes = 64;   // batched pose loop: walk the list of unconverged keyframes from this many keyframes on (bslam_set_pose_keyframe_list; 0: never)
  bslam::SurfelKey perm_key;
  hipEvent_t perm_ready = nullptr;   // recorded behind the sort that produced `perm`
  hipStream_t perm_stream = nullptr; // ... on this stream
  bool use_schedule = true;
  bslam::SurfelKey order_key;
  // kernel timing (bslam_profile_*)
  bool profiling = false;
  struct ProfEntry { hipEvent_t start, stop; int tag; };
  std::vector<ProfEntry> prof_pending;
  std::vector<std::pair<hipEvent_t, hipEvent_t>> prof_pool;
  int prof_launches[8] = {0, 0, 0, 0, 0, 0, 0, 0};
  float prof_ms[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
  bslam::Slab prof_counters; // unsigned long long[blocks][2]: work counters filled by the counting kernel variants while profiling
  size_t prof_counter_slots = 0;
  uint64_t prof_counter_base[8] = {0, 0, 0, 0, 0, 0, 0, 0};   // counts carried over a resize of the per-block array
  // The slabs free themselves; the device must be the context's (bslam_destroy).
  ~bslam_context() {
    for (hipEvent_t e : iter_done) if (e) { hipError_t err = hipEventDestroy(e); (void)err; }
    for (hipEvent_t e : solve_done) if (e) { hipError_t err = hipEventDestroy(e); (void)err; }
    if (perm_ready) { hipError_t err = hipEventDestroy(perm_ready); (void)err; }
    if (copy_stream) { hipError_t err = hipStreamDestroy(copy_stream); (void)err; }
    for (const ProfEntry& p : prof_pending) { hipError_t err = hipEventDestroy(p.start); err = hipEventDestroy(p.stop); (void)err; }
    for (const auto& p : prof_pool) { hipError_t err = hipEventDestroy(p.first); err = hipEventDestroy(p.second); (void)err; }
  }
};

namespace bslam {
// The exchange of a surfel-sharded run: an in-place float sum across ranks, ordered on `stream`.  A caller-supplied hook
// (bslam_set_allreduce) takes precedence over the library's own RCCL communicator (bslam_comm_init).
int rccl_allreduce_sum(bslam_context* ctx, hipStream_t stream, float* device_buffer, size_t count);   // badslam_hip.hip
inline bool has_exchange(const bslam_context* ctx) { return ctx->allreduce != nullptr || ctx->comm != nullptr; }
inline int exchange_sum(bslam_context* ctx, hipStream_t stream, float* device_buffer, size_t count) {
  if (ctx->allreduce) {
    const int arc = ctx->allreduce(ctx->allreduce_user, device_buffer, count, stream);
    if (arc) return fail(BSLAM_ERR_HIP, "allreduce callback failed with %d", arc);
    return BSLAM_OK;
  }
  if (ctx->comm) return rccl_allreduce_sum(ctx, stream, device_buffer, count);
  return BSLAM_OK;
}

// Brackets one kernel launch with events when profiling is on.
struct ProfScope {
  bslam_context* ctx; hipStream_t stream; std::pair<hipEvent_t, hipEvent_t> ev; bool on; int tag;
  ProfScope(bslam_context* c, hipStream_t s, int tag_ = 0) : ctx(c), stream(s), on(c->profiling), tag(tag_) {
    if (!on) return;
    if (!ctx->prof_pool.empty()) { ev = ctx->prof_pool.back(); ctx->prof_pool.pop_back(); }
    else { hipError_t e = hipEventCreate(&ev.first); e = hipEventCreate(&ev.second); (void)e; }
    hipError_t e = hipEventRecord(ev.first, stream); (void)e;
  }
  ~ProfScope() {
    if (!on) return;
    hipError_t e = hipEventRecord(ev.second, stream); (void)e;
    ctx->prof_pending.push_back(bslam_context::ProfEntry{ev.first, ev.second, tag});
  }
};
}  // namespace bslam
