// lifecycle_abi.inc -- surfel lifecycle entry points of include/badslam_hip.h (included by badslam_hip.hip).

namespace bslam {

// Device scratch of the lifecycle calls, carved out of one slab:
//   sup[3][cells] | cell_of[S] | flags8[pixels] | idx[max(pixels, S)] x 3 | tile sums | counters
struct LifecycleScratch {
  uint32_t* sup[3];
  uint32_t* cell_of;
  uint8_t* flags;
  uint32_t* a;   // scan output / invalid flags
  uint32_t* b;   // second scan output
  uint32_t* c;   // free list
  uint32_t* tile_sums;
  uint32_t* counters;   // [4]
};

static int lifecycle_scratch(bslam_context* ctx, size_t cells, size_t surfels, size_t pixels, LifecycleScratch* out) {
  const size_t n = std::max(pixels, surfels) + 16;
  const size_t tiles = n / kScanTile + 2;
  const size_t words = 3 * cells + surfels + 16 + (pixels + 15) / 4 + 3 * n + tiles + 16;
  int rc = ctx->lifecycle.reserve(words * sizeof(uint32_t));
  if (rc) return rc;
  uint32_t* p = (uint32_t*)ctx->lifecycle.ptr;
  for (int i = 0; i < 3; ++i) { out->sup[i] = p; p += cells; }
  out->cell_of = p; p += surfels + 16;
  out->flags = (uint8_t*)p; p += (pixels + 15) / 4;
  out->a = p; p += n;
  out->b = p; p += n;
  out->c = p; p += n;
  out->tile_sums = p; p += tiles;
  out->counters = p;
  return BSLAM_OK;
}

// out = scan(in) over n elements (kind: see scan_load); *total_dev (device) receives the grand total.
static int device_scan(hipStream_t stream, int kind, const void* in, uint32_t n, bool exclusive, uint32_t* out, uint32_t* tile_sums, uint32_t* total_dev) {
  if (n == 0) { BSLAM_HIP_TRY(hipMemsetAsync(total_dev, 0, sizeof(uint32_t), stream)); return BSLAM_OK; }
  const unsigned tiles = (n + kScanTile - 1) / kScanTile;
  hipLaunchKernelGGL(scan_tiles_kernel, dim3(tiles), dim3(kScanThreads), 0, stream, kind, in, n, exclusive ? 1 : 0, out, tile_sums);
  BSLAM_HIP_TRY(hipGetLastError());
  hipLaunchKernelGGL(scan_sums_kernel, dim3(1), dim3(256), 0, stream, tile_sums, (int)tiles, total_dev);
  BSLAM_HIP_TRY(hipGetLastError());
  hipLaunchKernelGGL(scan_add_kernel, dim3(tiles), dim3(kScanThreads), 0, stream, out, n, (const uint32_t*)tile_sums);
  BSLAM_HIP_TRY(hipGetLastError());
  return BSLAM_OK;
}

static int read_u32(bslam_context* ctx, hipStream_t stream, const uint32_t* dev, uint32_t* host_out) {
  const uint32_t* h = nullptr;
  int rc = read_back(ctx, stream, dev, 1, &h);
  if (rc) return rc;
  *host_out = *h;
  return BSLAM_OK;
}

// Setup of the two calls that work on one keyframe: the arguments every surfel call validates, the device, the keyframe's device
// view (with colour and radius images when a colour camera is given: creation), camera constants, cell grid and scratch.
struct KeyframeCall {
  KfDev kf;
  CamConsts c;
  int cells_w, cells_h;
  uint32_t pixels;
  LifecycleScratch sc;
};
// created: creation's output count, zeroed once check_surfel_call has passed (it is valid on every later return); may be null.
static int setup_keyframe_call(bslam_context* ctx, const bslam_camera4f* color_camera, const bslam_camera4f* depth_camera, const bslam_depth_params* dp,
                               const bslam_keyframe_view* keyframe, uint32_t surfels_size, const bslam_buffer2d* surfels, uint32_t* created,
                               KeyframeCall* o) {
  int rc = check_surfel_call(ctx, depth_camera, dp, surfels, surfels_size);
  if (rc) return rc;
  if (created) *created = 0;
  BSLAM_HIP_TRY(hipSetDevice(ctx->device));
  const bool creating = color_camera != nullptr;
  if ((rc = make_kf_dev(depth_camera, color_camera, *keyframe, creating, creating, &o->kf))) return rc;
  o->c = make_cam_consts(ctx, color_camera, depth_camera, dp);
  o->cells_w = (o->c.width - 1) / o->c.cell + 1;
  o->cells_h = (o->c.height - 1) / o->c.cell + 1;
  o->pixels = (uint32_t)(o->c.width * o->c.height);
  return lifecycle_scratch(ctx, (size_t)o->cells_w * o->cells_h, surfels_size, o->pixels, &o->sc);
}

// DetermineSupportingSurfelsCUDAImpl (BS/kernel_supporting_surfels.cc:38-112)
static int supporting_surfels(bslam_context* ctx, hipStream_t stream, bool merge, float merge_dist_factor, const KeyframeCall& k,
                              uint32_t surfels_size, const bslam_buffer2d* surfels, uint32_t* deleted_out) {
  const CamConsts& c = k.c;
  const LifecycleScratch& sc = k.sc;
  const size_t cells = (size_t)k.cells_w * k.cells_h;
  BSLAM_HIP_TRY(hipMemsetAsync(sc.sup[0], 0xff, 3 * cells * sizeof(uint32_t), stream));   // Clear(kInvalidIndex)
  if (deleted_out) *deleted_out = 0;
  if (surfels_size == 0) return BSLAM_OK;
  const SurfelRowsAll rows = surfel_rows_all(surfels);
  const dim3 grid((surfels_size + 255) / 256), block(256);
  hipLaunchKernelGGL(support_claim0_kernel, grid, block, 0, stream, c, k.kf, rows, surfels_size, k.cells_w, sc.cell_of, sc.sup[0]);
  BSLAM_HIP_TRY(hipGetLastError());
  if (!merge) return BSLAM_OK;   // creation only asks "is the cell occupied"
  hipLaunchKernelGGL(support_claim_next_kernel, grid, block, 0, stream, surfels_size, (const uint32_t*)sc.cell_of, (const uint32_t*)sc.sup[0],
                     (const uint32_t*)nullptr, sc.sup[1]);
  BSLAM_HIP_TRY(hipGetLastError());
  hipLaunchKernelGGL(support_claim_next_kernel, grid, block, 0, stream, surfels_size, (const uint32_t*)sc.cell_of, (const uint32_t*)sc.sup[0],
                     (const uint32_t*)sc.sup[1], sc.sup[2]);
  BSLAM_HIP_TRY(hipGetLastError());
  BSLAM_HIP_TRY(hipMemsetAsync(sc.counters, 0, sizeof(uint32_t), stream));
  const float cell_merge_dist_squared = (float)c.cell * (float)c.cell * merge_dist_factor * merge_dist_factor;   // BS/kernel_supporting_surfels.cc:74-76
  hipLaunchKernelGGL(merge_holders_kernel, dim3((unsigned)((cells + 255) / 256)), block, 0, stream, (int)cells, (const uint32_t*)sc.sup[0],
                     (const uint32_t*)sc.sup[1], (const uint32_t*)sc.sup[2], rows, cell_merge_dist_squared, kCosNormalCompat, sc.counters);
  BSLAM_HIP_TRY(hipGetLastError());
  hipLaunchKernelGGL(merge_others_kernel, grid, block, 0, stream, surfels_size, (const uint32_t*)sc.cell_of, (const uint32_t*)sc.sup[0],
                     (const uint32_t*)sc.sup[1], (const uint32_t*)sc.sup[2], rows, cell_merge_dist_squared, kCosNormalCompat, sc.counters);
  BSLAM_HIP_TRY(hipGetLastError());
  return read_u32(ctx, stream, sc.counters, deleted_out);
}

}  // namespace bslam

extern "C" {

int bslam_determine_supporting_surfels_and_merge(
    bslam_context* ctx, void* stream_, float merge_dist_factor, const bslam_camera4f* depth_camera, const bslam_depth_params* depth_params,
    const bslam_keyframe_view* keyframe, uint32_t surfels_size, const bslam_buffer2d* surfels, uint32_t* surfel_count) {
  hipStream_t stream = (hipStream_t)stream_;
  if (!keyframe || !surfel_count) return fail(BSLAM_ERR_INVALID_ARGUMENT, "null argument");
  KeyframeCall k;
  int rc = setup_keyframe_call(ctx, nullptr, depth_camera, depth_params, keyframe, surfels_size, surfels, nullptr, &k);
  if (rc) return rc;
  uint32_t deleted = 0;
  if ((rc = supporting_surfels(ctx, stream, true, merge_dist_factor, k, surfels_size, surfels, &deleted))) return rc;
  *surfel_count -= deleted;
  return BSLAM_OK;
}

int bslam_create_surfels_for_keyframe(
    bslam_context* ctx, void* stream_, int filter_new_surfels, int min_observation_count,
    const bslam_camera4f* color_camera, const bslam_camera4f* depth_camera, const bslam_depth_params* depth_params,
    const bslam_keyframe_view* keyframe, const bslam_mat3x4* global_T_frame,
    int covis_count, const bslam_keyframe_view* covis_keyframes, const bslam_mat3x4* covis_T_frame,
    uint32_t surfels_size, const bslam_buffer2d* surfels, uint32_t* new_surfel_count) {
  hipStream_t stream = (hipStream_t)stream_;
  if (!keyframe || !color_camera || !global_T_frame || !new_surfel_count) return fail(BSLAM_ERR_INVALID_ARGUMENT, "null argument");
  if (covis_count < 0 || (covis_count > 0 && filter_new_surfels && (!covis_keyframes || !covis_T_frame))) return fail(BSLAM_ERR_INVALID_ARGUMENT, "bad co-visibility list");
  KeyframeCall call;
  int rc = setup_keyframe_call(ctx, color_camera, depth_camera, depth_params, keyframe, surfels_size, surfels, new_surfel_count, &call);
  if (rc) return rc;
  const CamConsts& c = call.c;
  const KfDev& kf = call.kf;
  const LifecycleScratch& sc = call.sc;
  const int cells_w = call.cells_w, cells_h = call.cells_h;
  const uint32_t pixels = call.pixels;
  if ((rc = supporting_surfels(ctx, stream, false, 0.f, call, surfels_size, surfels, nullptr))) return rc;   // BS/direct_ba.cc:349-358

  BSLAM_HIP_TRY(hipMemsetAsync(sc.flags, 0, pixels, stream));
  hipLaunchKernelGGL(create_flag_kernel, dim3((unsigned)((cells_w + 255) / 256), (unsigned)cells_h), dim3(256), 0, stream, c, kf, cells_w, cells_h, sc.sup[0], sc.flags);
  BSLAM_HIP_TRY(hipGetLastError());
  uint32_t count = 0;
  if ((rc = device_scan(stream, 0, sc.flags, pixels, false, sc.a, sc.tile_sums, sc.counters + 1))) return rc;   // cub::DeviceScan::InclusiveSum (:427-460)
  if ((rc = read_u32(ctx, stream, sc.counters + 1, &count))) return rc;
  if (count == 0) return BSLAM_OK;
  if (filter_new_surfels) {   // BS/kernel_create_surfels.cc:84-136
    // the co-visibility list as a keyframe table of its own (raw images only: no records, no quads), entry k's frame_T_global
    // being covis_T_frame[k]; an empty list launches with a null table and removes every candidate
    const KfDev* covis_dev = nullptr;
    if (covis_count > 0) {
      const size_t bytes = (size_t)covis_count * sizeof(KfDev);
      if ((rc = ctx->exchange.reserve(bytes))) return rc;
      void* stage = nullptr;
      if ((rc = ctx->upload_ring.acquire(bytes, &stage))) return rc;
      KfDev* covis = (KfDev*)stage;
      for (int k = 0; k < covis_count; ++k) {
        if ((rc = make_kf_dev(depth_camera, nullptr, covis_keyframes[k], false, false, &covis[k]))) return rc;
        std::memcpy(covis[k].frame_T_global.m, covis_T_frame[k].m, sizeof(float) * 12);
      }
      BSLAM_HIP_TRY(hipMemcpyAsync(ctx->exchange.ptr, stage, bytes, hipMemcpyHostToDevice, stream));
      if ((rc = ctx->upload_ring.commit(stream))) return rc;
      covis_dev = (const KfDev*)ctx->exchange.ptr;
    }
    hipLaunchKernelGGL(create_filter_kernel, dim3((pixels + 255) / 256), dim3(256), 0, stream, c, kf, covis_count, covis_dev, min_observation_count, sc.flags);
    BSLAM_HIP_TRY(hipGetLastError());
    if ((rc = device_scan(stream, 0, sc.flags, pixels, false, sc.a, sc.tile_sums, sc.counters + 1))) return rc;
    if ((rc = read_u32(ctx, stream, sc.counters + 1, &count))) return rc;
    if (count == 0) return BSLAM_OK;
  }
  if ((uint64_t)surfels_size + count > (uint64_t)surfels->width)   // the reference logs an error and creates nothing (BS/kernel_create_surfels.cc:162-165)
    return fail(BSLAM_ERR_OUT_OF_MEMORY, "maximum surfel count exceeded: %u + %u > %d", surfels_size, count, surfels->width);
  M34 G;
  std::memcpy(G.m, global_T_frame->m, sizeof(float) * 12);
  hipLaunchKernelGGL(create_append_kernel, dim3((pixels + 255) / 256), dim3(256), 0, stream, c, kf, G, (const uint8_t*)sc.flags, (const uint32_t*)sc.a,
                     surfels_size, surfel_rows_all(surfels));
  BSLAM_HIP_TRY(hipGetLastError());
  *new_surfel_count = count;
  return BSLAM_OK;
}

int bslam_delete_surfels_and_update_radii(
    bslam_context* ctx, void* stream_, int min_observation_count, const bslam_camera4f* depth_camera, const bslam_depth_params* depth_params,
    int keyframe_count, const bslam_keyframe_view* keyframes, uint32_t* surfel_count, uint32_t surfels_size, const bslam_buffer2d* surfels) {
  hipStream_t stream = (hipStream_t)stream_;
  if (!surfel_count) return fail(BSLAM_ERR_INVALID_ARGUMENT, "null argument");
  int rc = check_surfel_call(ctx, depth_camera, depth_params, surfels, surfels_size);
  if (rc) return rc;
  if (keyframe_count < 0 || (keyframe_count > 0 && !keyframes)) return fail(BSLAM_ERR_INVALID_ARGUMENT, "bad keyframe list");
  if (surfels_size == 0) return BSLAM_OK;
  CamConsts c;
  if ((rc = setup_keyframe_table(ctx, stream, nullptr, depth_camera, depth_params, keyframe_count, keyframes, false, surfels_size, surfels, &c,
                                 nullptr, true))) return rc;
  uint32_t* counter = (uint32_t*)((uint8_t*)ctx->misc.ptr + kMiscDeleted);
  BSLAM_HIP_TRY(hipMemsetAsync(counter, 0, sizeof(uint32_t), stream));
  SurfelWork work;   // per-surfel order for >= 4 keyframes: sorted copy of position + normal, granule boxes for the culling
  if ((rc = prepare_surfels(ctx, stream, surfels, surfels_size, 1, keyframe_count, &work, false))) return rc;
  const Schedule sc = work.sc;
  hipLaunchKernelGGL(delete_and_update_radii_kernel, dim3(8u * sc.slots_per_xcd), dim3(256), 0, stream, c, (const KfDev*)ctx->kf_table.ptr,
                     keyframe_count, min_observation_count, surfels_size, sc, work.perm, work.rows, surfel_rows_all(surfels), counter);
  BSLAM_HIP_TRY(hipGetLastError());
  uint32_t deleted = 0;
  if ((rc = read_u32(ctx, stream, counter, &deleted))) return rc;
  *surfel_count -= deleted;
  return BSLAM_OK;
}

int bslam_compact_surfels(bslam_context* ctx, void* stream_, uint32_t surfel_count, uint32_t* surfels_size, const bslam_buffer2d* surfels,
                          const bslam_buffer2d* active_surfels) {
  hipStream_t stream = (hipStream_t)stream_;
  if (!ctx || !surfels || !surfels->address || !surfels_size) return fail(BSLAM_ERR_INVALID_ARGUMENT, "null argument");
  const uint32_t n = *surfels_size;
  if (n > (uint32_t)surfels->width || surfel_count > n) return fail(BSLAM_ERR_INVALID_ARGUMENT, "bad surfel counts %u / %u (buffer width %d)", surfel_count, n, surfels->width);
  if (n == surfel_count) return BSLAM_OK;   // BS/kernel_compact_surfels.cu:186-188
  BSLAM_HIP_TRY(hipSetDevice(ctx->device));
  LifecycleScratch sc;
  int rc = lifecycle_scratch(ctx, 1, n, 1, &sc);
  if (rc) return rc;
  const uint32_t free_spot_count = n - surfel_count;
  const dim3 grid((n + 255) / 256), block(256);
  const float* x = surfel_rows_all(surfels).x;
  uint32_t* invalid = sc.cell_of;   // [n]
  hipLaunchKernelGGL(compact_flag_kernel, grid, block, 0, stream, n, x, invalid);
  BSLAM_HIP_TRY(hipGetLastError());
  if ((rc = device_scan(stream, 1, invalid, n, true, sc.a, sc.tile_sums, sc.counters + 2))) return rc;    // free-spot ordinals
  hipLaunchKernelGGL(compact_free_list_kernel, grid, block, 0, stream, n, free_spot_count, (const uint32_t*)invalid, (const uint32_t*)sc.a, sc.c);
  BSLAM_HIP_TRY(hipGetLastError());
  if ((rc = device_scan(stream, 2, invalid, n, true, sc.b, sc.tile_sums, sc.counters + 3))) return rc;    // valid surfels behind, reversed order
  hipLaunchKernelGGL(compact_move_kernel, grid, block, 0, stream, n, free_spot_count, (const uint32_t*)invalid, (const uint32_t*)sc.b, (const uint32_t*)sc.c,
                     (uint8_t*)surfels->address, surfels->pitch, active_surfels ? (uint8_t*)active_surfels->address : (uint8_t*)nullptr);
  BSLAM_HIP_TRY(hipGetLastError());
  *surfels_size = surfel_count;
  return BSLAM_OK;
}

}  // extern "C"
