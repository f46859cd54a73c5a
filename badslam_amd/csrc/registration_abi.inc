// registration_abi.inc -- bslam_registration_prepare and bslam_registration_step of include/badslam_hip.h (included by
// badslam_hip.hip after distance_abi.inc: pmd_census, pmd_check_budget, pmd_build_lists, pmd_query_points).

extern "C" {

int bslam_registration_prepare(bslam_context* ctx, void* stream_, uint32_t vertex_count, const float* positions, uint32_t triangle_count,
                               const uint32_t* indices, float max_distance, float cell_size, uint64_t max_grid_entries, uint64_t* grid_cells,
                               uint64_t* grid_entries) {
  hipStream_t stream = (hipStream_t)stream_;
  const char* call = "bslam_registration_prepare";
  if (!ctx) return fail(BSLAM_ERR_INVALID_ARGUMENT, "context is null");
  if (!finite_positive(max_distance)) return fail(BSLAM_ERR_INVALID_ARGUMENT, "max_distance must be finite and > 0");
  if (!finite_positive(cell_size)) return fail(BSLAM_ERR_INVALID_ARGUMENT, "cell_size must be finite and > 0");
  if (max_grid_entries == 0) return fail(BSLAM_ERR_INVALID_ARGUMENT, "max_grid_entries must be >= 1");
  const size_t V = vertex_count, T = triangle_count;
  if (T > 0xffffff00ull) return fail(BSLAM_ERR_INVALID_ARGUMENT, "more than 2^32 - 256 triangles");
  const MeshSpan spans[2] = {{positions, 12 * V, "positions", false}, {indices, 12 * T, "indices", false}};
  int rc = check_mesh_spans(spans, 2);
  if (rc) return rc;
  const float R = max_distance;
  const float inv_cell = 1.0f / cell_size;
  if (!finite_positive(inv_cell)) return fail(BSLAM_ERR_INVALID_ARGUMENT, "1 / cell_size is not a positive float");
  BSLAM_HIP_TRY(hipSetDevice(ctx->device));
  PmdCensus census;
  std::memset(&census.grid, 0, sizeof(census.grid));
  if (T != 0) {
    if (V == 0) return empty_mesh(stream, T, call);   // every index is beyond
    // the count passes use the words at the head of the slab; the prepared pieces behind them are not touched, so a prepare that is
    // refused up to here leaves the previous mesh in place
    if ((rc = ctx->registration.reserve(kPmdWords * sizeof(uint32_t)))) return rc;
    if ((rc = pmd_census(ctx, stream, call, vertex_count, positions, triangle_count, indices, R, inv_cell, (uint32_t*)ctx->registration.ptr, &census, grid_cells,
                         grid_entries))) return rc;
  }
  const uint64_t cells = census.cells, entries = census.entries;
  if (grid_cells) *grid_cells = cells;
  if (grid_entries) *grid_entries = entries;
  if ((rc = pmd_check_budget(call, census, max_grid_entries))) return rc;
  bslam_context::PreparedMesh& m = ctx->prepared;
  m.ready = false;
  float4* records = nullptr;
  uint32_t *cell_count = nullptr, *cell_start = nullptr, *list = nullptr, *tile_sums = nullptr;
  if (census.valid != 0) {
    if ((rc = carve(ctx->registration, [&](Carver& c) {
           c.take<uint32_t>(kPmdWords, 16); records = c.take<float4>((size_t)kPmdRecordQuads * T, 16); cell_count = c.take<uint32_t>(cells, 16);
           cell_start = c.take<uint32_t>(cells + 1, 16); list = c.take<uint32_t>(entries, 16);
         }))) return rc;
    if ((rc = carve(ctx->distance, [&](Carver& c) { tile_sums = c.take<uint32_t>(cells / kScanTile + 2, 16); }))) return rc;
    if ((rc = pmd_build_lists(stream, census, vertex_count, positions, triangle_count, indices, R, records, cell_count, cell_start, tile_sums, list))) return rc;
  }
  BSLAM_HIP_TRY(hipStreamSynchronize(stream));   // the caller's mesh arrays may go now
  m.radius = R;
  for (int a = 0; a < 3; ++a) { m.origin[a] = census.grid.origin[a]; m.dim[a] = census.grid.dim[a]; }
  m.inv_cell = census.grid.inv_cell;
  m.cells = census.grid.cells;
  m.valid = census.valid;
  m.triangles = triangle_count;
  m.records = records; m.cell_count = cell_count; m.cell_start = cell_start; m.list = list;
  m.ready = true;
  return BSLAM_OK;
}

int bslam_registration_step(bslam_context* ctx, void* stream_, uint32_t point_count, const float* points, const float* target_T_source, float max_distance,
                            int mode, float huber_k, float* out_distance, uint32_t* out_triangle, float* out_sums, uint64_t* out_counts) {
  hipStream_t stream = (hipStream_t)stream_;
  if (!ctx) return fail(BSLAM_ERR_INVALID_ARGUMENT, "context is null");
  if (!target_T_source || !out_sums || !out_counts) return fail(BSLAM_ERR_INVALID_ARGUMENT, "target_T_source, out_sums or out_counts is null");
  const bslam_context::PreparedMesh& m = ctx->prepared;
  if (!m.ready) return fail(BSLAM_ERR_INVALID_ARGUMENT, "bslam_registration_step: no prepared mesh (call bslam_registration_prepare first)");
  for (int k = 0; k < 12; ++k)
    if (!std::isfinite(target_T_source[k])) return fail(BSLAM_ERR_INVALID_ARGUMENT, "target_T_source[%d] is not finite", k);
  if (!finite_positive(max_distance)) return fail(BSLAM_ERR_INVALID_ARGUMENT, "max_distance must be finite and > 0");
  if (max_distance > m.radius) return fail(BSLAM_ERR_INVALID_ARGUMENT, "max_distance %g exceeds the prepared radius %g", max_distance, m.radius);
  if (!(huber_k > 0.f)) return fail(BSLAM_ERR_INVALID_ARGUMENT, "huber_k must be > 0 (+INFINITY: no robust weight)");
  if (mode != BSLAM_REGISTRATION_PLANE && mode != BSLAM_REGISTRATION_POINT) return fail(BSLAM_ERR_INVALID_ARGUMENT, "unknown registration mode %d", mode);
  const size_t N = point_count;
  if (N > 0xffffff00ull) return fail(BSLAM_ERR_INVALID_ARGUMENT, "more than 2^32 - 256 points");
  const MeshSpan spans[3] = {{points, 12 * N, "points", false}, {out_distance, out_distance ? 4 * N : 0, "out_distance", true},
                             {out_triangle, out_triangle ? 4 * N : 0, "out_triangle", true}};
  int rc = check_mesh_spans(spans, 3);
  if (rc) return rc;
  BSLAM_HIP_TRY(hipSetDevice(ctx->device));
  if (N == 0) {
    BSLAM_HIP_TRY(hipStreamSynchronize(stream));
    std::memset(out_sums, 0, 32 * sizeof(float));
    std::memset(out_counts, 0, 4 * sizeof(uint64_t));
    return BSLAM_OK;
  }
  // per-call scratch (every piece 16 byte aligned): point_start[cells + 1] | tile sums | point_cell[N] | sorted[N] | distance[N] and
  //   triangle[N] where the caller gave none | partial rows | parts | sums float[32], counters u64[4]
  const dim3 block(256);
  const size_t cells = m.cells, rows = (size_t)flat_grid(N).x * 4;
  uint32_t *point_start, *tile_sums, *point_cell, *sorted, *triangle = out_triangle, *result;
  float *distance = out_distance, *partials, *parts;
  if ((rc = carve(ctx->distance, [&](Carver& c) {
         point_start = c.take<uint32_t>(cells + 1, 16); tile_sums = c.take<uint32_t>(cells / kScanTile + 2, 16); point_cell = c.take<uint32_t>(N, 16);
         sorted = c.take<uint32_t>(N, 16);
         if (!out_distance) distance = c.take<float>(N, 16);
         if (!out_triangle) triangle = c.take<uint32_t>(N, 16);
         partials = c.take<float>(rows * kRow, 16); parts = c.take<float>((size_t)kReduceParts * kRow, 16); result = c.take<uint32_t>(kRow + 2 * kRegCounters, 16);
       }))) return rc;
  float* sums = (float*)result;
  unsigned long long* counters = (unsigned long long*)(result + kRow);
  BSLAM_HIP_TRY(hipMemsetAsync(counters, 0, kRegCounters * sizeof(unsigned long long), stream));
  PmdQuery q;
  std::memcpy(q.transform.m, target_T_source, sizeof(q.transform.m));
  q.cells = m.cells; q.points = points; q.point_cell = point_cell; q.point_start = point_start; q.sorted = sorted; q.cell_start = (const uint32_t*)m.cell_start;
  q.list = (const uint32_t*)m.list; q.records = (const float4*)m.records; q.r_squared = max_distance * max_distance; q.out_distance = distance; q.out_triangle = triangle;
  if (m.valid == 0) {   // nothing to be near to
    hipLaunchKernelGGL(pmd_miss_kernel, flat_grid(N), block, 0, stream, point_count, distance, triangle);
    BSLAM_HIP_TRY(hipGetLastError());
  } else {
    PmdGrid g;
    for (int a = 0; a < 3; ++a) { g.origin[a] = m.origin[a]; g.dim[a] = m.dim[a]; }
    g.inv_cell = m.inv_cell;
    g.cells = m.cells;
    if ((rc = pmd_query_points<true>(ctx, stream, g, point_count, (uint32_t*)m.cell_count, point_cell, point_start, tile_sums, sorted, q))) return rc;
  }
  RegStep s;
  s.points = point_count; s.xyz = points; s.transform = q.transform; s.records = q.records; s.triangle = triangle; s.huber_k = huber_k; s.partials = partials;
  s.counters = counters;
  if (mode == BSLAM_REGISTRATION_PLANE) hipLaunchKernelGGL(reg_rows_kernel<BSLAM_REGISTRATION_PLANE>, flat_grid(N), block, 0, stream, s);
  else hipLaunchKernelGGL(reg_rows_kernel<BSLAM_REGISTRATION_POINT>, flat_grid(N), block, 0, stream, s);
  BSLAM_HIP_TRY(hipGetLastError());
  // the partial rows in a fixed order: kReduceParts contiguous ranges, then the parts
  hipLaunchKernelGGL(pose_reduce_kernel, dim3(1, kReduceParts), block, 0, stream, (const float*)partials, (int)rows, parts);
  BSLAM_HIP_TRY(hipGetLastError());
  hipLaunchKernelGGL(reg_reduce_final_kernel, dim3(1), dim3(64), 0, stream, (const float*)parts, sums);
  BSLAM_HIP_TRY(hipGetLastError());
  const uint32_t* host = nullptr;
  if ((rc = read_back(ctx, stream, (const uint32_t*)result, (size_t)(kRow + 2 * kRegCounters), &host))) return rc;
  std::memcpy(out_sums, host, kRow * sizeof(float));
  uint64_t counted[kRegCounters];
  std::memcpy(counted, host + kRow, sizeof(counted));
  out_counts[0] = N; out_counts[1] = counted[kRegHits]; out_counts[2] = counted[kRegUsed]; out_counts[3] = counted[kRegDegenerate];
  return BSLAM_OK;
}

}  // extern "C"
