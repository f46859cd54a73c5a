// simplify_abi.inc -- bslam_simplify_mesh of include/badslam_hip.h (included by badslam_hip.hip after mesh_abi.inc:
// check_attribute_pairs, mesh_array_spans, check_mesh_spans, mesh_error, empty_mesh, pad64, mesh_sort, remap_triangles; device_scan,
// flat_grid, read_back, carve).

extern "C" {

int bslam_simplify_mesh(bslam_context* ctx, void* stream_, uint32_t vertex_count, uint32_t triangle_count, const float* positions, const float* normals,
                        const void* colors, const uint32_t* indices, const float* origin, float cell_size, float* out_positions, float* out_normals,
                        void* out_colors, uint32_t* out_indices, uint32_t* vertex_cluster, uint32_t* out_vertex_count, uint32_t* out_triangle_count) {
  hipStream_t stream = (hipStream_t)stream_;
  const char* call = "bslam_simplify_mesh";
  if (!ctx || !out_vertex_count || !out_triangle_count) return fail(BSLAM_ERR_INVALID_ARGUMENT, "null argument");
  if (!origin) return fail(BSLAM_ERR_INVALID_ARGUMENT, "origin is null");
  for (int a = 0; a < 3; ++a)
    if (!std::isfinite(origin[a])) return fail(BSLAM_ERR_INVALID_ARGUMENT, "origin must be finite");
  if (!finite_positive(cell_size)) return fail(BSLAM_ERR_INVALID_ARGUMENT, "cell_size must be finite and > 0");
  const float inv_cell = 1.0f / cell_size;
  if (!finite_positive(inv_cell)) return fail(BSLAM_ERR_INVALID_ARGUMENT, "1 / cell_size is not a positive float");
  const MeshArrays arrays = {positions, normals, colors, indices, out_positions, out_normals, out_colors, out_indices};
  int rc = check_attribute_pairs(arrays);
  if (rc) return rc;
  const size_t V = vertex_count, T = triangle_count;
  // one thread per vertex / per triangle in blocks of 256: the rounded-up thread index has to fit 32 bits
  if (V > 0xffffff00ull || T > 0xffffff00ull) return fail(BSLAM_ERR_INVALID_ARGUMENT, "more than 2^32 - 256 vertices or triangles");
  MeshSpan spans[9];
  mesh_array_spans(arrays, V, T, spans, spans + 4);
  spans[8] = {vertex_cluster, vertex_cluster ? 4 * V : 0, "vertex_cluster", true};
  if ((rc = check_mesh_spans(spans, 9))) return rc;
  BSLAM_HIP_TRY(hipSetDevice(ctx->device));
  if (V == 0) {
    if ((rc = empty_mesh(stream, T, call)) == BSLAM_OK) *out_vertex_count = *out_triangle_count = 0;
    return rc;
  }
  // scratch: words | keys u64[V] | sorted keys u64[V] | ids u32[V] | sorted ids u32[V] | head u8[V] | cluster rank u32[V] |
  //          clusters u32[V] (when the caller takes none) | keep u8[T] | triangle rank u32[T] | tile sums | the sort's own
  const size_t nv = pad64(V), nt = pad64(T), tiles = std::max(nv, nt) / kScanTile + 2;
  size_t sort_bytes = 0;
  if ((rc = mesh_sort_bytes(V, stream, &sort_bytes))) return rc;
  uint32_t *words, *ids, *sorted_ids, *cluster_rank, *clusters = vertex_cluster, *triangle_rank, *tile_sums;
  unsigned long long *keys, *sorted_keys;
  uint8_t *head, *keep, *sort_temp;
  if ((rc = carve(ctx->simplify, [&](Carver& c) {
         words = c.take<uint32_t>(kSimplifyWords, 16); keys = c.take<unsigned long long>(nv, 64); sorted_keys = c.take<unsigned long long>(nv, 64);
         ids = c.take<uint32_t>(nv, 64); sorted_ids = c.take<uint32_t>(nv, 64); head = c.take<uint8_t>(nv, 64); cluster_rank = c.take<uint32_t>(nv, 64);
         if (!vertex_cluster) clusters = c.take<uint32_t>(nv, 64);
         keep = c.take<uint8_t>(nt, 64); triangle_rank = c.take<uint32_t>(nt, 64); tile_sums = c.take<uint32_t>(tiles, 16);
         sort_temp = c.take<uint8_t>(sort_bytes, 256);
       }))) return rc;
  const dim3 block(256);
  BSLAM_HIP_TRY(hipMemsetAsync(words, 0, kSimplifyWords * sizeof(uint32_t), stream));
  if ((rc = ctx->simplify_events.mark(ctx->profiling, stream, 0))) return rc;
  hipLaunchKernelGGL(simplify_key_kernel, flat_grid(V), block, 0, stream, vertex_count, positions, f3{origin[0], origin[1], origin[2]}, inv_cell, keys, ids, words);
  BSLAM_HIP_TRY(hipGetLastError());
  if ((rc = ctx->simplify_events.mark(ctx->profiling, stream, 1))) return rc;
  // stable: the members of a cluster stay in ascending vertex id
  if ((rc = mesh_sort(call, sort_temp, sort_bytes, keys, sorted_keys, ids, sorted_ids, V, 64, stream))) return rc;
  if ((rc = ctx->simplify_events.mark(ctx->profiling, stream, 2))) return rc;
  hipLaunchKernelGGL(simplify_heads_kernel, flat_grid(V), block, 0, stream, vertex_count, (const unsigned long long*)sorted_keys, head);
  BSLAM_HIP_TRY(hipGetLastError());
  if ((rc = device_scan(stream, 0, head, vertex_count, false, cluster_rank, tile_sums, words + kSimplifyClusters))) return rc;
  if ((rc = ctx->simplify_events.mark(ctx->profiling, stream, 3))) return rc;
  SimplifyClusters m;
  m.vertices = vertex_count; m.sorted_keys = sorted_keys; m.sorted_ids = sorted_ids; m.head = head; m.rank = cluster_rank;
  m.positions = positions; m.normals = normals; m.colors = (const uint32_t*)colors;
  m.out_positions = out_positions; m.out_normals = out_normals; m.out_colors = (uint32_t*)out_colors; m.vertex_cluster = clusters;
  hipLaunchKernelGGL(simplify_cluster_kernel, flat_grid(V), block, 0, stream, m);
  BSLAM_HIP_TRY(hipGetLastError());
  if ((rc = ctx->simplify_events.mark(ctx->profiling, stream, 4))) return rc;
  if ((rc = remap_triangles(stream, vertex_count, triangle_count, indices, clusters, keep, triangle_rank, tile_sums, words, words + kSimplifyTriangles, out_indices))) return rc;
  if ((rc = ctx->simplify_events.mark(ctx->profiling, stream, 5))) return rc;
  const uint32_t* host = nullptr;
  if ((rc = read_back(ctx, stream, (const uint32_t*)words, 4, &host))) return rc;
  if (ctx->profiling)
    for (int s = 0; s < 5; ++s)
      if ((rc = ctx->simplify_events.elapsed(s, s + 1, &ctx->simplify_stage_ms[s]))) return rc;
  if ((rc = mesh_error(host[kSimplifyError], call))) return rc;
  if (host[kSimplifyError] & kSimplifyBadVertex) return fail(BSLAM_ERR_INVALID_ARGUMENT, "%s: a vertex is not finite or lies outside the grid", call);
  *out_vertex_count = host[kSimplifyClusters];
  *out_triangle_count = host[kSimplifyTriangles];
  return BSLAM_OK;
}

int bslam_simplify_stage_times(bslam_context* ctx, float* stage_ms5) {
  if (!ctx || !stage_ms5) return fail(BSLAM_ERR_INVALID_ARGUMENT, "null argument");
  std::memcpy(stage_ms5, ctx->simplify_stage_ms, sizeof(ctx->simplify_stage_ms));
  return BSLAM_OK;
}

}  // extern "C"
