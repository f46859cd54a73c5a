// ray_abi.inc -- bslam_mesh_rays and bslam_mesh_visibility of include/badslam_hip.h (included by badslam_hip.hip behind bvh_abi.inc:
// bvh_build, which both calls use unchanged; mesh_abi.inc: check_mesh_spans, empty_mesh; render_abi.inc: load_views; read_back,
// cull_stats_ptr).

namespace bslam {

// What both calls do in front of their kernel: the tree into ctx->bvh_tree, *leaves.  *launch = false: V == 0, nothing to launch
// (the stream is synchronised and the result is in the return value).
static int ray_tree(bslam_context* ctx, hipStream_t stream, const char* call, uint32_t vertex_count, const float* positions, uint32_t triangle_count,
                    const uint32_t* indices, uint32_t* leaves, uint32_t* height, RayTree* tree, bool* launch) {
  BSLAM_HIP_TRY(hipSetDevice(ctx->device));
  if (leaves) *leaves = 0;
  if (height) *height = 0;
  ctx->bvh_tree = bslam_context::BvhTree();
  *launch = true;
  if (triangle_count != 0) {
    if (vertex_count == 0) { *launch = false; return empty_mesh(stream, triangle_count, call); }   // every index is beyond
    if (int rc = bvh_build(ctx, stream, call, vertex_count, positions, triangle_count, indices, height != nullptr)) return rc;
  }
  tree->leaves = ctx->bvh_tree.leaves;
  tree->nodes = (const float4*)ctx->bvh_tree.nodes;
  tree->records = (const float4*)ctx->bvh_tree.records;
  if (leaves) *leaves = tree->leaves;
  return BSLAM_OK;
}

// ... and behind it: the height, which waits for the stream, or the wait alone.
static int ray_finish(bslam_context* ctx, hipStream_t stream, uint32_t* height) {
  if (height && ctx->bvh_tree.leaves != 0) {
    const uint32_t* host = nullptr;
    if (int rc = read_back(ctx, stream, (const uint32_t*)ctx->bvh_tree.words, (size_t)kBvhWords, &host)) return rc;   // waits for the stream
    *height = host[kBvhHeight];
    ctx->bvh_tree.height = host[kBvhHeight];
    return BSLAM_OK;
  }
  BSLAM_HIP_TRY(hipStreamSynchronize(stream));
  return BSLAM_OK;
}

}  // namespace bslam

extern "C" {

int bslam_mesh_rays(bslam_context* ctx, void* stream_, uint32_t ray_count, const float* origins, const float* directions, const float* t_range,
                    uint32_t vertex_count, const float* positions, uint32_t triangle_count, const uint32_t* indices, int mode, float* out_t,
                    uint32_t* out_triangle, float* out_uv, uint8_t* out_front, uint8_t* out_hit, uint32_t* leaves, uint32_t* height) {
  hipStream_t stream = (hipStream_t)stream_;
  const char* call = "bslam_mesh_rays";
  if (!ctx) return fail(BSLAM_ERR_INVALID_ARGUMENT, "context is null");
  if (mode != BSLAM_RAYS_CLOSEST && mode != BSLAM_RAYS_ANY) return fail(BSLAM_ERR_INVALID_ARGUMENT, "mode must be 0 (closest hit) or 1 (any hit)");
  if (mode == BSLAM_RAYS_CLOSEST) {
    if (!out_t) return fail(BSLAM_ERR_INVALID_ARGUMENT, "out_t is null");
    if (out_hit) return fail(BSLAM_ERR_INVALID_ARGUMENT, "out_hit belongs to mode 1 (any hit)");
  } else {
    if (!out_hit) return fail(BSLAM_ERR_INVALID_ARGUMENT, "out_hit is null");
    if (out_t || out_triangle || out_uv || out_front) return fail(BSLAM_ERR_INVALID_ARGUMENT, "mode 1 (any hit) returns out_hit alone");
  }
  const size_t N = ray_count, V = vertex_count, T = triangle_count;
  // one thread per ray / per triangle in blocks of up to 256: the rounded-up thread index has to fit 32 bits
  if (N > 0xffffff00ull || T > 0xffffff00ull) return fail(BSLAM_ERR_INVALID_ARGUMENT, "more than 2^32 - 256 rays or triangles");
  const MeshSpan spans[10] = {{origins, 12 * N, "origins", false}, {directions, 12 * N, "directions", false}, {t_range, t_range ? 8 * N : 0, "t_range", false},
                              {positions, 12 * V, "positions", false}, {indices, 12 * T, "indices", false},
                              {out_t, out_t ? 4 * N : 0, "out_t", true}, {out_triangle, out_triangle ? 4 * N : 0, "out_triangle", true},
                              {out_uv, out_uv ? 8 * N : 0, "out_uv", true}, {out_front, out_front ? N : 0, "out_front", true}, {out_hit, out_hit ? N : 0, "out_hit", true}};
  int rc = check_mesh_spans(spans, 10);   // 4 byte alignment of every array, the two byte arrays included
  if (rc) return rc;
  MeshRays q;
  bool launch = true;
  if ((rc = ray_tree(ctx, stream, call, vertex_count, positions, triangle_count, indices, leaves, height, &q.tree, &launch)) || !launch) return rc;
  if (N != 0) {
    q.rays = ray_count; q.origins = origins; q.directions = directions; q.t_range = t_range;
    q.out_t = out_t; q.out_triangle = out_triangle; q.out_uv = out_uv; q.out_front = out_front; q.out_hit = out_hit;
    const dim3 grid((unsigned)((N + kBvhQueryBlock - 1) / kBvhQueryBlock)), block(kBvhQueryBlock);
    unsigned long long* stats = cull_stats_ptr(ctx);
    if (mode == BSLAM_RAYS_ANY) {
      if (stats) hipLaunchKernelGGL((mesh_rays_kernel<true, true>), grid, block, 0, stream, q, stats);
      else hipLaunchKernelGGL((mesh_rays_kernel<true, false>), grid, block, 0, stream, q, stats);
    } else {
      if (stats) hipLaunchKernelGGL((mesh_rays_kernel<false, true>), grid, block, 0, stream, q, stats);
      else hipLaunchKernelGGL((mesh_rays_kernel<false, false>), grid, block, 0, stream, q, stats);
    }
    BSLAM_HIP_TRY(hipGetLastError());
  }
  return ray_finish(ctx, stream, height);
}

int bslam_mesh_visibility(bslam_context* ctx, void* stream_, uint32_t point_count, const float* points, const float* normals, uint32_t vertex_count,
                          const float* positions, uint32_t triangle_count, const uint32_t* indices, uint32_t view_count, const bslam_mat3x4* camera_T_global,
                          const float* centres, const bslam_camera4f* camera, float min_depth, float max_depth, float margin, uint32_t* out_count,
                          uint32_t* out_first, uint32_t* leaves, uint32_t* height) {
  hipStream_t stream = (hipStream_t)stream_;
  const char* call = "bslam_mesh_visibility";
  if (!ctx || !camera) return fail(BSLAM_ERR_INVALID_ARGUMENT, "null argument");
  if (view_count > BSLAM_MESH_VISIBILITY_MAX_VIEWS) return fail(BSLAM_ERR_INVALID_ARGUMENT, "more than %u views", (unsigned)BSLAM_MESH_VISIBILITY_MAX_VIEWS);
  if (view_count != 0 && (!camera_T_global || !centres)) return fail(BSLAM_ERR_INVALID_ARGUMENT, "camera_T_global or centres is null");
  if (!std::isfinite(min_depth) || !std::isfinite(max_depth) || !std::isfinite(margin)) return fail(BSLAM_ERR_INVALID_ARGUMENT, "min_depth, max_depth and margin must be finite");
  if (min_depth > max_depth) return fail(BSLAM_ERR_INVALID_ARGUMENT, "need min_depth <= max_depth");
  if (margin < 0.f) return fail(BSLAM_ERR_INVALID_ARGUMENT, "margin must be >= 0");
  int rc = load_views(camera, {}, {}, "", nullptr);   // the camera limits of bslam_render_surfels
  if (rc) return rc;
  const size_t N = point_count, V = vertex_count, T = triangle_count, K = view_count;
  if (N > 0xffffff00ull || T > 0xffffff00ull) return fail(BSLAM_ERR_INVALID_ARGUMENT, "more than 2^32 - 256 points or triangles");
  if (N != 0 && !out_count) return fail(BSLAM_ERR_INVALID_ARGUMENT, "out_count is null");
  const MeshSpan spans[6] = {{points, 12 * N, "points", false}, {normals, normals ? 12 * N : 0, "normals", false}, {positions, 12 * V, "positions", false},
                             {indices, 12 * T, "indices", false}, {out_count, 4 * N, "out_count", true}, {out_first, out_first ? 4 * N : 0, "out_first", true}};
  if ((rc = check_mesh_spans(spans, 6))) return rc;
  MeshVisibility q;
  bool launch = true;
  if ((rc = ray_tree(ctx, stream, call, vertex_count, positions, triangle_count, indices, leaves, height, &q.tree, &launch)) || !launch) return rc;
  std::vector<float> rows(16 * K);   // lives until the stream has been waited for
  if (N != 0) {
    if ((rc = ctx->ray_views.reserve(std::max<size_t>(rows.size(), 16) * sizeof(float)))) return rc;
    for (size_t k = 0; k < K; ++k) {
      std::memcpy(rows.data() + 16 * k, camera_T_global[k].m, 12 * sizeof(float));
      rows[16 * k + 12] = centres[3 * k]; rows[16 * k + 13] = centres[3 * k + 1]; rows[16 * k + 14] = centres[3 * k + 2]; rows[16 * k + 15] = 0.f;
    }
    if (K != 0) BSLAM_HIP_TRY(hipMemcpyAsync(ctx->ray_views.ptr, rows.data(), rows.size() * sizeof(float), hipMemcpyHostToDevice, stream));
    q.points = point_count; q.views = view_count; q.xyz = points; q.normals = normals; q.view_rows = (const float4*)ctx->ray_views.ptr;
    q.fx = camera->fx; q.fy = camera->fy; q.cx = camera->cx; q.cy = camera->cy; q.width = (float)camera->width; q.height = (float)camera->height;
    q.min_depth = min_depth; q.max_depth = max_depth; q.margin = margin; q.out_count = out_count; q.out_first = out_first;
    const dim3 grid((unsigned)((N + kBvhQueryBlock - 1) / kBvhQueryBlock)), block(kBvhQueryBlock);
    unsigned long long* stats = cull_stats_ptr(ctx);
    if (stats) hipLaunchKernelGGL(mesh_visibility_kernel<true>, grid, block, 0, stream, q, stats);
    else hipLaunchKernelGGL(mesh_visibility_kernel<false>, grid, block, 0, stream, q, stats);
    BSLAM_HIP_TRY(hipGetLastError());
  }
  return ray_finish(ctx, stream, height);
}

}  // extern "C"
