// distance_abi.inc -- bslam_point_mesh_distance of include/badslam_hip.h (included by badslam_hip.hip after mesh_abi.inc:
// check_mesh_spans, mesh_error, device_scan), and the pieces of its launch sequence that
// registration_abi.inc runs too: the triangle side once per prepared mesh, the point side once per step.

namespace bslam {

// Most cells a grid may have: the scans over the cells and the cell indices stay far inside 32 bits, and the four words a cell
// costs (triangle cursor / point cursor, triangle start, point start) stay at 1 GiB.
constexpr uint64_t kPmdMaxCells = BSLAM_POINT_MESH_MAX_CELLS;

static float pmd_unkey(uint32_t k) {
  const uint32_t u = (k & 0x80000000u) ? (k & 0x7fffffffu) : ~k;
  float f;
  std::memcpy(&f, &u, sizeof(f));
  return f;
}

// What the count passes found of a mesh under a grid.
struct PmdCensus {
  PmdGrid grid;
  uint64_t cells = 0, entries = 0;
  uint32_t valid = 0;   // triangles with nine finite coordinates
};

// The triangle side, part 1 (T > 0, V > 0): the index check, the bounds and the grid they give, the entry count; refuses a grid
// beyond the cap on the cells.  `words` are kPmdWords device words.  Two host read-backs.
static int pmd_census(bslam_context* ctx, hipStream_t stream, const char* call, uint32_t vertex_count, const float* positions, uint32_t triangle_count,
                      const uint32_t* indices, float R, float inv_cell, uint32_t* words, PmdCensus* census, uint64_t* grid_cells, uint64_t* grid_entries) {
  const dim3 block(256);
  const size_t T = triangle_count;
  PmdGrid& g = census->grid;
  int rc;
  BSLAM_HIP_TRY(hipMemsetAsync(words, 0, kPmdWords * sizeof(uint32_t), stream));
  BSLAM_HIP_TRY(hipMemsetAsync(words + kPmdMinKey, 0xff, 3 * sizeof(uint32_t), stream));
  hipLaunchKernelGGL(pmd_bounds_kernel, flat_grid(T), block, 0, stream, vertex_count, triangle_count, positions, indices, R, words);
  BSLAM_HIP_TRY(hipGetLastError());
  const uint32_t* host = nullptr;
  if ((rc = read_back(ctx, stream, (const uint32_t*)words, (size_t)kPmdWords, &host))) return rc;
  if ((rc = mesh_error(host[kPmdError], call))) return rc;
  census->valid = host[kPmdValid];
  if (census->valid == 0) return BSLAM_OK;
  // the grid: origin = min(lo.a - R); the last cell of an axis is the cell of max(hi.a + R), by monotonicity the largest any
  // triangle reaches
  double total = 1.0;
  bool finite = true;
  for (int a = 0; a < 3; ++a) {
    g.origin[a] = pmd_unkey(host[kPmdMinKey + a]);
    const float last = pmd_cell(pmd_unkey(host[kPmdMaxKey + a]), g.origin[a], inv_cell);
    if (!std::isfinite(g.origin[a]) || !(last >= 0.f) || !(last < 2147483520.f)) { finite = false; break; }
    g.dim[a] = (int)last + 1;
    total *= (double)g.dim[a];
  }
  g.inv_cell = inv_cell;
  if (!finite || total > (double)kPmdMaxCells) {
    if (grid_cells) *grid_cells = finite && total < 1.8e19 ? (uint64_t)total : ~0ull;
    if (grid_entries) *grid_entries = 0;
    return fail(BSLAM_ERR_INVALID_ARGUMENT, "%s: the grid would have %.0f cells, more than the cap of %llu: use a larger cell_size", call,
                finite ? total : INFINITY, (unsigned long long)kPmdMaxCells);
  }
  census->cells = (uint64_t)total;
  g.cells = (uint32_t)census->cells;
  hipLaunchKernelGGL(pmd_entries_kernel, flat_grid(T), block, 0, stream, g, vertex_count, triangle_count, positions, indices, R, words);
  BSLAM_HIP_TRY(hipGetLastError());
  if ((rc = read_back(ctx, stream, (const uint32_t*)words, (size_t)kPmdWords, &host))) return rc;
  std::memcpy(&census->entries, host + kPmdEntries, sizeof(census->entries));
  return BSLAM_OK;
}

// The budget of the lists, decided before one is built.
static int pmd_check_budget(const char* call, const PmdCensus& census, uint64_t max_grid_entries) {
  if (census.entries > max_grid_entries || census.entries > 0xffffffffull)
    return fail(BSLAM_ERR_INVALID_ARGUMENT, "%s: %llu (triangle, cell) entries in %llu cells exceed max_grid_entries %llu (and 2^32 - 1): "
                "use a larger cell_size", call, (unsigned long long)census.entries, (unsigned long long)census.cells, (unsigned long long)max_grid_entries);
  return BSLAM_OK;
}

// The triangle side, part 2: records, the scan over the cells and the lists.  cell_count is all zero again afterwards.
static int pmd_build_lists(hipStream_t stream, const PmdCensus& census, uint32_t vertex_count, const float* positions, uint32_t triangle_count,
                           const uint32_t* indices, float R, float4* records, uint32_t* cell_count, uint32_t* cell_start, uint32_t* tile_sums, uint32_t* list) {
  const dim3 block(256);
  const size_t T = triangle_count;
  const PmdGrid& g = census.grid;
  int rc;
  BSLAM_HIP_TRY(hipMemsetAsync(cell_count, 0, census.cells * sizeof(uint32_t), stream));
  hipLaunchKernelGGL(pmd_records_kernel, flat_grid(T), block, 0, stream, g, vertex_count, triangle_count, positions, indices, R, records, cell_count);
  BSLAM_HIP_TRY(hipGetLastError());
  if ((rc = device_scan(stream, 1, cell_count, g.cells, true, cell_start, tile_sums, cell_start + census.cells))) return rc;
  hipLaunchKernelGGL(pmd_fill_kernel, flat_grid(T), block, 0, stream, g, triangle_count, (const float4*)records, (const uint32_t*)cell_start, cell_count,
                     (uint32_t)census.entries, list);
  BSLAM_HIP_TRY(hipGetLastError());
  return BSLAM_OK;
}

// The point side: cells, counting sort and the query of q.points (kTransform: of q.transform applied to them) against the lists.
// cell_count has to be all zero and is so again afterwards.  Nothing is synchronised.
template <bool kTransform>
static int pmd_query_points(bslam_context* ctx, hipStream_t stream, const PmdGrid& g, uint32_t point_count, uint32_t* cell_count, uint32_t* point_cell,
                            uint32_t* point_start, uint32_t* tile_sums, uint32_t* sorted, const PmdQuery& q) {
  const dim3 block(256);
  const size_t N = point_count;
  int rc;
  hipLaunchKernelGGL(pmd_point_cells_kernel<kTransform>, flat_grid(N), block, 0, stream, g, point_count, q.points, q.transform, q.cell_start, cell_count,
                     point_cell, q.out_distance, q.out_triangle);
  BSLAM_HIP_TRY(hipGetLastError());
  if ((rc = device_scan(stream, 1, cell_count, g.cells, true, point_start, tile_sums, point_start + g.cells))) return rc;
  hipLaunchKernelGGL(pmd_point_fill_kernel, flat_grid(N), block, 0, stream, point_count, (const uint32_t*)point_cell, (const uint32_t*)point_start, cell_count, sorted);
  BSLAM_HIP_TRY(hipGetLastError());
  // one lane per point: the lanes beyond the sorted points (misses written above) find nothing to do
  if (ctx->profiling) hipLaunchKernelGGL((pmd_query_kernel<true, kTransform>), flat_grid(N), block, 0, stream, q, cull_stats_ptr(ctx));
  else hipLaunchKernelGGL((pmd_query_kernel<false, kTransform>), flat_grid(N), block, 0, stream, q, (unsigned long long*)nullptr);
  BSLAM_HIP_TRY(hipGetLastError());
  return BSLAM_OK;
}

}  // namespace bslam

extern "C" {

int bslam_point_mesh_distance(bslam_context* ctx, void* stream_, uint32_t point_count, const float* points, uint32_t vertex_count, const float* positions,
                              uint32_t triangle_count, const uint32_t* indices, float max_distance, float cell_size, uint64_t max_grid_entries,
                              float* out_distance, uint32_t* out_triangle, uint64_t* grid_cells, uint64_t* grid_entries) {
  hipStream_t stream = (hipStream_t)stream_;
  const char* call = "bslam_point_mesh_distance";
  if (!ctx) return fail(BSLAM_ERR_INVALID_ARGUMENT, "context is null");
  if (!finite_positive(max_distance)) return fail(BSLAM_ERR_INVALID_ARGUMENT, "max_distance must be finite and > 0");
  if (!finite_positive(cell_size)) return fail(BSLAM_ERR_INVALID_ARGUMENT, "cell_size must be finite and > 0");
  if (max_grid_entries == 0) return fail(BSLAM_ERR_INVALID_ARGUMENT, "max_grid_entries must be >= 1");
  if (!out_distance) return fail(BSLAM_ERR_INVALID_ARGUMENT, "out_distance is null");
  const size_t N = point_count, V = vertex_count, T = triangle_count;
  // one thread per point / per triangle in blocks of 256: the rounded-up thread index has to fit 32 bits
  if (N > 0xffffff00ull || T > 0xffffff00ull) return fail(BSLAM_ERR_INVALID_ARGUMENT, "more than 2^32 - 256 points or triangles");
  const MeshSpan spans[5] = {{points, 12 * N, "points", false}, {positions, 12 * V, "positions", false}, {indices, 12 * T, "indices", false},
                             {out_distance, 4 * N, "out_distance", true}, {out_triangle, out_triangle ? 4 * N : 0, "out_triangle", true}};
  int rc = check_mesh_spans(spans, 5);
  if (rc) return rc;
  const float R = max_distance;
  const float r_squared = R * R;
  const float inv_cell = 1.0f / cell_size;
  if (!finite_positive(inv_cell)) return fail(BSLAM_ERR_INVALID_ARGUMENT, "1 / cell_size is not a positive float");
  BSLAM_HIP_TRY(hipSetDevice(ctx->device));
  const dim3 block(256);
  PmdCensus census;
  std::memset(&census.grid, 0, sizeof(census.grid));
  if (T != 0) {
    if (V == 0) return empty_mesh(stream, T, call);   // every index is beyond
    if ((rc = ctx->distance.reserve(kPmdWords * sizeof(uint32_t)))) return rc;
    if ((rc = pmd_census(ctx, stream, call, vertex_count, positions, triangle_count, indices, R, inv_cell, (uint32_t*)ctx->distance.ptr, &census, grid_cells,
                         grid_entries))) return rc;
  }
  const uint64_t cells = census.cells, entries = census.entries;
  if (grid_cells) *grid_cells = cells;
  if (grid_entries) *grid_entries = entries;
  if ((rc = pmd_check_budget(call, census, max_grid_entries))) return rc;
  if (N == 0) {
    BSLAM_HIP_TRY(hipStreamSynchronize(stream));
    return BSLAM_OK;
  }
  if (census.valid == 0) {   // nothing to be near to
    hipLaunchKernelGGL(pmd_miss_kernel, flat_grid(N), block, 0, stream, point_count, out_distance, out_triangle);
    BSLAM_HIP_TRY(hipGetLastError());
    BSLAM_HIP_TRY(hipStreamSynchronize(stream));
    return BSLAM_OK;
  }
  // scratch (u32 units; every piece 16 byte aligned): words | records float4[9 T] | cell_count[cells] | cell_start[cells + 1] |
  //   point_start[cells + 1] | tile sums | list[entries] | point_cell[N] | sorted[N]
  const size_t tiles = cells / kScanTile + 2;
  float4* records;
  uint32_t *cell_count, *cell_start, *point_start, *tile_sums, *list, *point_cell, *sorted;
  if ((rc = carve(ctx->distance, [&](Carver& c) {
         c.take<uint32_t>(kPmdWords, 16); records = c.take<float4>((size_t)kPmdRecordQuads * T, 16); cell_count = c.take<uint32_t>(cells, 16);
         cell_start = c.take<uint32_t>(cells + 1, 16); point_start = c.take<uint32_t>(cells + 1, 16); tile_sums = c.take<uint32_t>(tiles, 16);
         list = c.take<uint32_t>(entries, 16); point_cell = c.take<uint32_t>(N, 16); sorted = c.take<uint32_t>(N, 16);
       }))) return rc;
  if ((rc = pmd_build_lists(stream, census, vertex_count, positions, triangle_count, indices, R, records, cell_count, cell_start, tile_sums, list))) return rc;
  // the points: cell_count is all zero again behind the fill
  PmdQuery q;
  std::memset(&q.transform, 0, sizeof(q.transform));
  q.cells = census.grid.cells; q.points = points; q.point_cell = point_cell; q.point_start = point_start; q.sorted = sorted; q.cell_start = cell_start; q.list = list;
  q.records = records; q.r_squared = r_squared; q.out_distance = out_distance; q.out_triangle = out_triangle;
  if ((rc = pmd_query_points<false>(ctx, stream, census.grid, point_count, cell_count, point_cell, point_start, tile_sums, sorted, q))) return rc;
  BSLAM_HIP_TRY(hipStreamSynchronize(stream));
  return BSLAM_OK;
}

}  // extern "C"
