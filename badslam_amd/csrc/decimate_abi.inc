// decimate_abi.inc -- bslam_decimate_mesh of include/badslam_hip.h (included by badslam_hip.hip after mesh_abi.inc:
// check_attribute_pairs, mesh_array_spans, check_mesh_spans, mesh_error, empty_mesh, pad64, vertex_id_bits, mesh_sort, remap_triangles;
// device_scan, flat_grid, read_back, carve).

namespace bslam {
// Adds the times between the recorded boundaries first .. last of a round to the stage sums; the stream is idle.
static int decimate_collect(bslam_context* ctx, int first, int last) {
  if (!ctx->profiling) return BSLAM_OK;
  for (int s = first; s < last; ++s) {
    float ms = 0.f;
    if (int rc = ctx->decimate_events.elapsed(s, s + 1, &ms)) return rc;
    ctx->decimate_stage_ms[s] += ms;
  }
  return BSLAM_OK;
}
}  // namespace bslam

extern "C" {

int bslam_decimate_mesh(bslam_context* ctx, void* stream_, uint32_t vertex_count, uint32_t triangle_count, const float* positions, const float* normals,
                        const void* colors, const uint32_t* indices, uint32_t target_vertices, float boundary_weight, float max_cost, uint32_t max_rounds,
                        float* out_positions, float* out_normals, void* out_colors, uint32_t* out_indices, uint32_t* vertex_map, uint32_t* out_vertex_count,
                        uint32_t* out_triangle_count, uint32_t* out_rounds) {
  hipStream_t stream = (hipStream_t)stream_;
  const char* call = "bslam_decimate_mesh";
  if (!ctx || !out_vertex_count || !out_triangle_count || !out_rounds) return fail(BSLAM_ERR_INVALID_ARGUMENT, "null argument");
  if (!std::isfinite(boundary_weight) || boundary_weight < 0.f) return fail(BSLAM_ERR_INVALID_ARGUMENT, "boundary_weight must be finite and >= 0");
  if (!(max_cost >= 0.f)) return fail(BSLAM_ERR_INVALID_ARGUMENT, "max_cost must be >= 0 or +inf");
  const MeshArrays arrays = {positions, normals, colors, indices, out_positions, out_normals, out_colors, out_indices};
  int rc = check_attribute_pairs(arrays);
  if (rc) return rc;
  const size_t V = vertex_count, T = triangle_count;
  // one thread per slot (three per triangle) in blocks of 256, and a scan of 32-bit ranks over the slots
  if (V > 0xffffff00ull || 3 * T > 0xffffff00ull) return fail(BSLAM_ERR_INVALID_ARGUMENT, "more than 2^32 - 256 vertices or triangle corners");
  MeshSpan spans[9];
  mesh_array_spans(arrays, V, T, spans, spans + 4);
  spans[8] = {vertex_map, vertex_map ? 4 * V : 0, "vertex_map", true};
  if ((rc = check_mesh_spans(spans, 9))) return rc;
  BSLAM_HIP_TRY(hipSetDevice(ctx->device));
  ctx->decimate_collapses.clear();
  for (float& ms : ctx->decimate_stage_ms) ms = 0.f;
  if (V == 0) {
    if ((rc = empty_mesh(stream, T, call)) == BSLAM_OK) *out_vertex_count = *out_triangle_count = *out_rounds = 0;
    return rc;
  }
  const unsigned bits = vertex_id_bits(V);
  // scratch: words | working positions, normals, colours, quadrics, parents [V] | two triangle buffers [T] | per slot (E = 3 T): the keys
  //          of the two sorts and their sorted copies, slots, flags, ranks, candidate keys | per vertex: fans, flags, minima | scan sums | the sort's own
  const size_t E = 3 * T, nv = pad64(V), nt = pad64(T), ne = pad64(E), tiles = std::max(nv, ne) / kScanTile + 2;
  size_t sort_bytes = 0;
  if ((rc = mesh_sort_bytes(std::max<size_t>(E, 1), stream, &sort_bytes))) return rc;
  DecimateState s = {};
  uint32_t *tri_a, *tri_b, *triangle_rank, *live_rank, *tile_sums, *scratch32;
  uint8_t *keep, *live, *sort_temp;
  if ((rc = carve(ctx->decimate, [&](Carver& c) {
         s.words = c.take<uint32_t>(kDecimateWords, 16); s.positions = c.take<float>(3 * nv, 64); s.normals = normals ? c.take<float>(3 * nv, 64) : nullptr;
         s.colors = colors ? c.take<uint32_t>(nv, 64) : nullptr; s.quadrics = c.take<double>(10 * nv, 64); s.parent = c.take<uint32_t>(nv, 64);
         tri_a = c.take<uint32_t>(3 * nt, 64); tri_b = c.take<uint32_t>(3 * nt, 64); keep = c.take<uint8_t>(nt, 64); triangle_rank = c.take<uint32_t>(nt, 64);
         s.edge_keys = c.take<unsigned long long>(ne, 64); s.vertex_keys = c.take<unsigned long long>(ne, 64); s.ids = c.take<uint32_t>(ne, 64);
         s.sorted_edges = c.take<unsigned long long>(ne, 64); s.sorted_vertices = c.take<unsigned long long>(ne, 64); s.edge_slots = c.take<uint32_t>(ne, 64);
         s.fan = c.take<uint32_t>(ne, 64); s.head = c.take<uint8_t>(ne, 64); s.first = c.take<uint8_t>(ne, 64); s.single = c.take<uint8_t>(ne, 64);
         s.rank = c.take<uint32_t>(ne, 64); s.key = c.take<unsigned long long>(ne, 64); s.choice = c.take<uint8_t>(ne, 64); s.selected = c.take<uint8_t>(ne, 64);
         scratch32 = c.take<uint32_t>(ne, 64);
         s.fan_start = c.take<uint32_t>(nv, 64); s.fan_end = c.take<uint32_t>(nv, 64); s.boundary = c.take<uint8_t>(nv, 64);
         s.m1 = c.take<unsigned long long>(nv, 64); s.m2 = c.take<unsigned long long>(nv, 64); live = c.take<uint8_t>(nv, 64); live_rank = c.take<uint32_t>(nv, 64);
         tile_sums = c.take<uint32_t>(tiles, 16); sort_temp = c.take<uint8_t>(sort_bytes, 256);
       }))) return rc;
  s.vertices = vertex_count; s.bits = bits;
  const dim3 block(256);
  const uint32_t* host = nullptr;
  BSLAM_HIP_TRY(hipMemsetAsync(s.words, 0, kDecimateWords * sizeof(uint32_t), stream));
  hipLaunchKernelGGL(decimate_init_kernel, flat_grid(V), block, 0, stream, s, positions, normals, (const uint32_t*)colors);
  BSLAM_HIP_TRY(hipGetLastError());
  // the input's triangles without those that repeat an index; parent is the identity
  if ((rc = remap_triangles(stream, vertex_count, triangle_count, indices, s.parent, keep, triangle_rank, tile_sums, s.words, s.words + kDecimateTriangles, tri_a))) return rc;
  if ((rc = read_back(ctx, stream, (const uint32_t*)s.words, 4, &host))) return rc;
  if ((rc = mesh_error(host[kDecimateError], call))) return rc;
  uint32_t live_count = vertex_count, triangles = host[kDecimateTriangles], rounds = 0;
  uint32_t *tri = tri_a, *tri_next = tri_b;
  bool exact = true;   // `triangles` is the live count, not only a bound for it
  while (live_count > target_vertices && (max_rounds == 0 || rounds < max_rounds)) {
    ++rounds;
    if (triangles == 0) { ctx->decimate_collapses.push_back(0); break; }   // no edge, no candidate
    const uint32_t edges = 3 * triangles;
    s.tri = tri; s.triangles = triangles; s.edges = edges;
    if ((rc = ctx->decimate_events.mark(ctx->profiling, stream, 0))) return rc;
    BSLAM_HIP_TRY(hipMemsetAsync(s.fan_start, 0, V * sizeof(uint32_t), stream));
    BSLAM_HIP_TRY(hipMemsetAsync(s.fan_end, 0, V * sizeof(uint32_t), stream));
    BSLAM_HIP_TRY(hipMemsetAsync(s.boundary, 0, V, stream));
    BSLAM_HIP_TRY(hipMemsetAsync(s.m1, 0xff, V * sizeof(unsigned long long), stream));
    BSLAM_HIP_TRY(hipMemsetAsync(s.words + kDecimateSelected, 0, 2 * sizeof(uint32_t), stream));
    hipLaunchKernelGGL(decimate_keys_kernel, flat_grid(triangles), block, 0, stream, s);
    BSLAM_HIP_TRY(hipGetLastError());
    if ((rc = ctx->decimate_events.mark(ctx->profiling, stream, 1))) return rc;
    // stable: the uses of an edge and the fan of a vertex stay in ascending slot, so in ascending triangle
    if ((rc = mesh_sort(call, sort_temp, sort_bytes, s.edge_keys, s.sorted_edges, s.ids, s.edge_slots, edges, 2 * bits, stream))) return rc;
    if ((rc = mesh_sort(call, sort_temp, sort_bytes, s.vertex_keys, s.sorted_vertices, s.ids, s.fan, edges, bits, stream))) return rc;
    if ((rc = ctx->decimate_events.mark(ctx->profiling, stream, 2))) return rc;
    hipLaunchKernelGGL(decimate_heads_kernel, flat_grid(edges), block, 0, stream, s);
    BSLAM_HIP_TRY(hipGetLastError());
    if ((rc = device_scan(stream, 0, s.head, edges, false, s.rank, tile_sums, s.words + kDecimateEdges))) return rc;
    if (rounds == 1) {
      hipLaunchKernelGGL(decimate_quadrics_kernel, flat_grid(V), block, 0, stream, s, (double)boundary_weight);
      BSLAM_HIP_TRY(hipGetLastError());
    }
    if ((rc = ctx->decimate_events.mark(ctx->profiling, stream, 3))) return rc;
    hipLaunchKernelGGL(decimate_eval_kernel, flat_grid(edges), block, 0, stream, s, max_cost);
    BSLAM_HIP_TRY(hipGetLastError());
    if ((rc = ctx->decimate_events.mark(ctx->profiling, stream, 4))) return rc;
    hipLaunchKernelGGL(decimate_neighbourhood_kernel, flat_grid(V), block, 0, stream, s);
    BSLAM_HIP_TRY(hipGetLastError());
    hipLaunchKernelGGL(decimate_select_kernel, flat_grid(edges), block, 0, stream, s);
    BSLAM_HIP_TRY(hipGetLastError());
    if ((rc = ctx->decimate_events.mark(ctx->profiling, stream, 5))) return rc;
    // the read-back of the round: what was selected decides whether it is the last
    if ((rc = read_back(ctx, stream, (const uint32_t*)s.words, 4, &host))) return rc;
    if ((rc = decimate_collect(ctx, 0, 5))) return rc;
    if ((rc = mesh_error(host[kDecimateError], call))) return rc;
    uint32_t selected = host[kDecimateSelected];
    const uint32_t removed = host[kDecimateRemoved], room = live_count - target_vertices;
    if (selected == 0) { ctx->decimate_collapses.push_back(0); break; }
    if ((rc = ctx->decimate_events.mark(ctx->profiling, stream, 5))) return rc;
    const bool cut = selected > room;
    if (cut) {
      // only the first `room` by key collapse: the selected keys to the front, sorted, and the key at room - 1 is the last to pass
      unsigned long long *cut_keys = s.edge_keys, *cut_sorted = s.vertex_keys;   // free since the sorts
      if ((rc = device_scan(stream, 0, s.selected, edges, true, scratch32, tile_sums, s.words + kDecimateCut))) return rc;
      hipLaunchKernelGGL(decimate_cut_gather_kernel, flat_grid(edges), block, 0, stream, s, (const uint32_t*)scratch32, cut_keys);
      BSLAM_HIP_TRY(hipGetLastError());
      if ((rc = mesh_sort(call, sort_temp, sort_bytes, cut_keys, cut_sorted, s.ids, scratch32, selected, 64, stream))) return rc;
      hipLaunchKernelGGL(decimate_cut_kernel, flat_grid(edges), block, 0, stream, s, (const unsigned long long*)cut_sorted, room);
      BSLAM_HIP_TRY(hipGetLastError());
      selected = room;
    }
    hipLaunchKernelGGL(decimate_apply_kernel, flat_grid(edges), block, 0, stream, s);
    BSLAM_HIP_TRY(hipGetLastError());
    if ((rc = ctx->decimate_events.mark(ctx->profiling, stream, 6))) return rc;
    if ((rc = remap_triangles(stream, vertex_count, triangles, tri, s.parent, keep, triangle_rank, tile_sums, s.words, s.words + kDecimateTriangles, tri_next))) return rc;
    if ((rc = ctx->decimate_events.mark(ctx->profiling, stream, 7))) return rc;
    if (ctx->profiling) {
      BSLAM_HIP_TRY(hipStreamSynchronize(stream));
      if ((rc = decimate_collect(ctx, 5, 7))) return rc;
    }
    std::swap(tri, tri_next);
    ctx->decimate_collapses.push_back(selected);
    live_count -= selected;
    // every collapse drops the triangles on its edge and no other; a cut ends the call, and `triangles` stays a bound
    if (cut) { exact = false; break; }
    if (removed > triangles) return fail(BSLAM_ERR_INTERNAL, "%s: %u triangles on the collapsed edges of %u", call, removed, triangles);
    triangles -= removed;
  }
  // output: survivors in ascending id, the live triangles in their order; the device holds their number, `triangles` bounds it
  s.tri = tri;
  hipLaunchKernelGGL(decimate_live_kernel, flat_grid(V), block, 0, stream, vertex_count, (const uint32_t*)s.parent, live);
  BSLAM_HIP_TRY(hipGetLastError());
  if ((rc = device_scan(stream, 0, live, vertex_count, true, live_rank, tile_sums, s.words + kDecimateVertices))) return rc;
  hipLaunchKernelGGL(decimate_vertices_kernel, flat_grid(V), block, 0, stream, s, (const uint32_t*)live_rank, out_positions, out_normals, (uint32_t*)out_colors, vertex_map);
  BSLAM_HIP_TRY(hipGetLastError());
  if (triangles != 0) {
    hipLaunchKernelGGL(decimate_indices_kernel, flat_grid(triangles), block, 0, stream, triangles,(const uint32_t*)tri, (const uint32_t*)live_rank, (const uint32_t*)s.words, out_indices);
    BSLAM_HIP_TRY(hipGetLastError());
  }
  if ((rc = read_back(ctx, stream, (const uint32_t*)s.words, 8, &host))) return rc;
  if ((rc = mesh_error(host[kDecimateError], call))) return rc;
  if (host[kDecimateVertices] != live_count) return fail(BSLAM_ERR_INTERNAL, "%s: %u vertices survive where %u were counted", call, host[kDecimateVertices], live_count);
  if (exact ? host[kDecimateTriangles] != triangles : host[kDecimateTriangles] > triangles)
    return fail(BSLAM_ERR_INTERNAL, "%s: %u triangles are live where %u were counted", call, host[kDecimateTriangles], triangles);
  *out_vertex_count = host[kDecimateVertices];
  *out_triangle_count = host[kDecimateTriangles];
  *out_rounds = rounds;
  return BSLAM_OK;
}

int bslam_decimate_stage_times(bslam_context* ctx, float* stage_ms7) {
  if (!ctx || !stage_ms7) return fail(BSLAM_ERR_INVALID_ARGUMENT, "null argument");
  std::memcpy(stage_ms7, ctx->decimate_stage_ms, sizeof(ctx->decimate_stage_ms));
  return BSLAM_OK;
}

int bslam_decimate_round_collapses(bslam_context* ctx, uint32_t* collapses, uint32_t capacity, uint32_t* rounds) {
  if (!ctx || !rounds || (capacity != 0 && !collapses)) return fail(BSLAM_ERR_INVALID_ARGUMENT, "null argument");
  *rounds = (uint32_t)ctx->decimate_collapses.size();
  for (uint32_t r = 0; r < capacity && r < *rounds; ++r) collapses[r] = ctx->decimate_collapses[r];
  return BSLAM_OK;
}

}  // extern "C"
