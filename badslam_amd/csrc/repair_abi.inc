// repair_abi.inc -- bslam_clean_mesh, bslam_mesh_topology and bslam_fill_mesh_holes of include/badslam_hip.h (included by
// badslam_hip.hip after mesh_abi.inc: check_attribute_pairs, mesh_array_spans, check_mesh_spans, mesh_error, empty_mesh, pad64,
// vertex_id_bits, mesh_sort, edge_runs_layout, build_edge_runs; device_scan, flat_grid, read_back, carve).

namespace bslam {

constexpr int kRepairStages = 8;

// The stages of a repair call while profiling is on: stage s lies between the events 2 s and 2 s + 1, so a read-back between two
// stages is in neither.
struct RepairTimer {
  bslam_context* ctx; hipStream_t stream; unsigned used;
  RepairTimer(bslam_context* c, hipStream_t s) : ctx(c), stream(s), used(0) { for (float& ms : ctx->repair_stage_ms) ms = 0.f; }
  int begin(int stage) { used |= 1u << stage; return ctx->repair_events.mark(ctx->profiling, stream, 2 * stage); }
  int end(int stage) { return ctx->repair_events.mark(ctx->profiling, stream, 2 * stage + 1); }
  // The stream is idle.
  int collect() {
    if (!ctx->profiling) return BSLAM_OK;
    for (int s = 0; s < kRepairStages; ++s)
      if (used & (1u << s))
        if (int rc = ctx->repair_events.elapsed(2 * s, 2 * s + 1, &ctx->repair_stage_ms[s])) return rc;
    return BSLAM_OK;
  }
};

// The scratch of the topology pass for the V vertices and T triangles of `indices`, carved from `c`.
static void topology_layout(Carver& c, uint32_t V, uint32_t T, const uint32_t* indices, RepairTopology* s, uint32_t** tile_sums, uint8_t** sort_temp, size_t sort_bytes) {
  const size_t E = 3 * (size_t)T, nv = pad64(V), ne = pad64(E), tiles = std::max(nv, ne) / kScanTile + 2;
  s->words = c.take<uint32_t>(kRepairWords, 16);
  edge_runs_layout(c, V, T, indices, s->words + kRepairError, &s->runs);
  s->runs.referenced = c.take<uint8_t>(nv, 64); s->starts = c.take<uint32_t>(nv, 64); s->ends = c.take<uint32_t>(nv, 64); s->start_slot = c.take<uint32_t>(nv, 64);
  s->boundary = c.take<uint8_t>(ne, 64); s->boundary_id = c.take<uint32_t>(ne, 64); s->loop_slot = c.take<uint32_t>(ne, 64);
  for (int b = 0; b < 2; ++b) { s->next[b] = c.take<uint32_t>(ne, 64); s->label[b] = c.take<uint32_t>(ne, 64); s->open[b] = c.take<uint8_t>(ne, 64); }
  s->loop_length = c.take<uint32_t>(ne, 64);
  *tile_sums = c.take<uint32_t>(tiles, 16);
  *sort_temp = c.take<uint8_t>(sort_bytes, 256);
}

// The census and the loops of `s` (V >= 1; the words are zero but kRepairLongest, which is all ones).  Stages 0 .. 3: keys, sort, census,
// loops; the first two and the runs of the third are build_edge_runs.  With fill_flag the loops of at most max_hole_edges edges are
// flagged for bslam_fill_mesh_holes.  *boundary_slots and *buffer: B, and the buffer that holds the final labels.  The stream is left
// running; the words hold the report.
static int topology_pass(bslam_context* ctx, hipStream_t stream, const char* call, RepairTopology& s, uint32_t* tile_sums, uint8_t* sort_temp, size_t sort_bytes,
                         RepairTimer& timer, uint32_t max_hole_edges, uint8_t* fill_flag, uint32_t* fan, uint32_t* boundary_slots, int* buffer) {
  const dim3 block(256);
  const size_t V = s.runs.vertices, T = s.runs.triangles, E = s.runs.slots;
  int rc;
  *boundary_slots = 0;
  *buffer = 0;
  BSLAM_HIP_TRY(hipMemsetAsync(s.runs.referenced, 0, V, stream));
  BSLAM_HIP_TRY(hipMemsetAsync(s.starts, 0, V * sizeof(uint32_t), stream));
  BSLAM_HIP_TRY(hipMemsetAsync(s.ends, 0, V * sizeof(uint32_t), stream));
  BSLAM_HIP_TRY(hipMemsetAsync(s.start_slot, 0xff, V * sizeof(uint32_t), stream));
  if (T != 0) {
    if ((rc = timer.begin(0))) return rc;
    if ((rc = build_edge_runs(ctx, stream, call, s.runs, tile_sums, sort_temp, sort_bytes, timer, s.words + kRepairEdges))) return rc;
    hipLaunchKernelGGL(topology_census_kernel, flat_grid(E), block, 0, stream, s);
    BSLAM_HIP_TRY(hipGetLastError());
    if ((rc = device_scan(stream, 0, s.boundary, s.runs.slots, true, s.boundary_id, tile_sums, s.words + kRepairBoundarySlots))) return rc;
  } else {
    if ((rc = timer.begin(2))) return rc;
  }
  hipLaunchKernelGGL(topology_vertex_kernel, flat_grid(V), block, 0, stream, s);
  BSLAM_HIP_TRY(hipGetLastError());
  if ((rc = timer.end(2))) return rc;
  if (T == 0) return BSLAM_OK;
  // 0xffffffff where no loop passes; like every output, not written for a mesh that is refused
  if (s.loop_of_slot != nullptr) BSLAM_HIP_TRY(hipMemsetAsync(s.loop_of_slot, 0xff, E * sizeof(uint32_t), stream));
  // the rounds of the pointer jumping depend on the number of boundary slots alone
  const uint32_t* host = nullptr;
  if ((rc = read_back(ctx, stream, (const uint32_t*)s.words, kRepairWords, &host))) return rc;
  const uint32_t B = host[kRepairBoundarySlots];
  *boundary_slots = B;
  if (B == 0) return BSLAM_OK;
  if (B > E) return fail(BSLAM_ERR_INTERNAL, "%s: %u boundary slots among %zu", call, B, E);
  if ((rc = timer.begin(3))) return rc;
  BSLAM_HIP_TRY(hipMemsetAsync(s.loop_length, 0, (size_t)B * sizeof(uint32_t), stream));
  hipLaunchKernelGGL(topology_loop_init_kernel, flat_grid(E), block, 0, stream, s);
  BSLAM_HIP_TRY(hipGetLastError());
  int rounds = 1;   // ceil(log2 B) + 1
  while ((1ull << (rounds - 1)) < B) ++rounds;
  int at = 0;
  for (int r = 0; r < rounds; ++r, at ^= 1) {
    hipLaunchKernelGGL(topology_jump_kernel, flat_grid(B), block, 0, stream, s, B, at);
    BSLAM_HIP_TRY(hipGetLastError());
  }
  hipLaunchKernelGGL(topology_loop_label_kernel, flat_grid(B), block, 0, stream, s, B, at);
  BSLAM_HIP_TRY(hipGetLastError());
  hipLaunchKernelGGL(topology_loop_stats_kernel, flat_grid(B), block, 0, stream, s, B, at, max_hole_edges, fill_flag, fan);
  BSLAM_HIP_TRY(hipGetLastError());
  if ((rc = timer.end(3))) return rc;
  *buffer = at;
  return BSLAM_OK;
}

static void topology_report(const uint32_t* w, uint32_t triangles, bslam_mesh_report* r) {
  r->referenced_vertices = w[kRepairReferenced]; r->unique_edges = w[kRepairEdges]; r->boundary_edges = w[kRepairBoundary]; r->interior_edges = w[kRepairInterior];
  r->nonmanifold_edges = w[kRepairNonManifold]; r->inconsistent_edges = w[kRepairInconsistent]; r->blocked_vertices = w[kRepairBlocked];
  r->loops = w[kRepairLoops]; r->longest_loop = ~w[kRepairLongest]; r->loop_edges = w[kRepairLoopEdges]; r->open_boundary_slots = w[kRepairOpenSlots];
  r->reserved = 0;
  r->euler = (int64_t)w[kRepairReferenced] - (int64_t)w[kRepairEdges] + (int64_t)triangles;
}

// Zeroes the words of a call; the longest loop is kept as a minimum of complements.
static int repair_clear_words(uint32_t* words, hipStream_t stream) {
  BSLAM_HIP_TRY(hipMemsetAsync(words, 0, kRepairWords * sizeof(uint32_t), stream));
  BSLAM_HIP_TRY(hipMemsetAsync(words + kRepairLongest, 0xff, sizeof(uint32_t), stream));
  return BSLAM_OK;
}

}  // namespace bslam

extern "C" {

int bslam_clean_mesh(bslam_context* ctx, void* stream_, uint32_t vertex_count, uint32_t triangle_count, const float* positions, const float* normals,
                     const void* colors, const uint32_t* indices, int weld, int remove_duplicates, int remove_unreferenced, float* out_positions,
                     float* out_normals, void* out_colors, uint32_t* out_indices, uint32_t* vertex_map, uint32_t* triangle_map, uint32_t* out_vertex_count,
                     uint32_t* out_triangle_count, uint32_t* counts4) {
  hipStream_t stream = (hipStream_t)stream_;
  const char* call = "bslam_clean_mesh";
  if (!ctx || !out_vertex_count || !out_triangle_count || !counts4) return fail(BSLAM_ERR_INVALID_ARGUMENT, "null argument");
  if ((weld | remove_duplicates | remove_unreferenced) & ~1) return fail(BSLAM_ERR_INVALID_ARGUMENT, "weld, remove_duplicates and remove_unreferenced must be 0 or 1");
  const MeshArrays arrays = {positions, normals, colors, indices, out_positions, out_normals, out_colors, out_indices};
  int rc = check_attribute_pairs(arrays);
  if (rc) return rc;
  const size_t V = vertex_count, T = triangle_count;
  if (V > 0xffffff00ull || T > 0xffffff00ull) return fail(BSLAM_ERR_INVALID_ARGUMENT, "more than 2^32 - 256 vertices or triangles");
  MeshSpan spans[10];
  mesh_array_spans(arrays, V, T, spans, spans + 4);
  spans[8] = {vertex_map, vertex_map ? 4 * V : 0, "vertex_map", true};
  spans[9] = {triangle_map, triangle_map ? 4 * T : 0, "triangle_map", true};
  if ((rc = check_mesh_spans(spans, 10))) return rc;
  BSLAM_HIP_TRY(hipSetDevice(ctx->device));
  RepairTimer timer(ctx, stream);
  if (V == 0) {
    if ((rc = empty_mesh(stream, T, call)) == BSLAM_OK) *out_vertex_count = *out_triangle_count = counts4[0] = counts4[1] = counts4[2] = counts4[3] = 0;
    return rc;
  }
  const unsigned bits = vertex_id_bits(V);
  // scratch: words | keys of the two sorts by id, keys in sorted order, sorted keys u64[N] | ids and their two sorted copies, ranks, run heads u32[N] |
  //          head flags u8[N], N = max(V, T) | rep, vertex ranks u32[V] | referenced, kept u8[V] | kept u8[T], triangle ranks u32[T] | scan sums | the sort's own
  const size_t nv = pad64(V), nt = pad64(T), n = std::max(nv, nt), tiles = n / kScanTile + 2;
  size_t sort_bytes = 0;
  if ((rc = mesh_sort_bytes(std::max(V, T), stream, &sort_bytes))) return rc;
  uint32_t *words, *ids, *ids_a, *ids_b, *rank, *first, *rep, *vertex_rank, *triangle_rank, *tile_sums;
  unsigned long long *key_first, *key_second, *gathered, *sorted_keys;
  uint8_t *head, *referenced, *keep_vertex, *keep, *sort_temp;
  if ((rc = carve(ctx->repair, [&](Carver& c) {
         words = c.take<uint32_t>(kRepairWords, 16); key_first = c.take<unsigned long long>(n, 64); key_second = c.take<unsigned long long>(n, 64);
         gathered = c.take<unsigned long long>(n, 64); sorted_keys = c.take<unsigned long long>(n, 64); ids = c.take<uint32_t>(n, 64); ids_a = c.take<uint32_t>(n, 64);
         ids_b = c.take<uint32_t>(n, 64); rank = c.take<uint32_t>(n, 64); first = c.take<uint32_t>(n, 64); head = c.take<uint8_t>(n, 64);
         rep = c.take<uint32_t>(nv, 64); vertex_rank = c.take<uint32_t>(nv, 64); referenced = c.take<uint8_t>(nv, 64); keep_vertex = c.take<uint8_t>(nv, 64);
         keep = c.take<uint8_t>(nt, 64); triangle_rank = c.take<uint32_t>(nt, 64); tile_sums = c.take<uint32_t>(tiles, 16); sort_temp = c.take<uint8_t>(sort_bytes, 256);
       }))) return rc;
  const dim3 block(256);
  if ((rc = repair_clear_words(words, stream))) return rc;
  // stage 0: vertex keys
  if ((rc = timer.begin(0))) return rc;
  hipLaunchKernelGGL(repair_vertex_kernel, flat_grid(V), block, 0, stream, vertex_count, positions, weld, key_first, key_second, ids, rep, words);
  BSLAM_HIP_TRY(hipGetLastError());
  if ((rc = timer.end(0))) return rc;
  if (weld) {
    // stage 1: the two stable sorts, by z and then by (y, x): a run is in ascending vertex id
    if ((rc = timer.begin(1))) return rc;
    if ((rc = mesh_sort(call, sort_temp, sort_bytes, key_first, sorted_keys, ids, ids_a, V, 32, stream))) return rc;
    hipLaunchKernelGGL(mesh_gather_kernel, flat_grid(V), block, 0, stream, vertex_count, (const unsigned long long*)key_second, (const uint32_t*)ids_a, gathered);
    BSLAM_HIP_TRY(hipGetLastError());
    if ((rc = mesh_sort(call, sort_temp, sort_bytes, gathered, sorted_keys, ids_a, ids_b, V, 64, stream))) return rc;
    if ((rc = timer.end(1))) return rc;
    // stage 2: runs and representatives
    if ((rc = timer.begin(2))) return rc;
    hipLaunchKernelGGL(mesh_heads_kernel, flat_grid(V), block, 0, stream, vertex_count, (const unsigned long long*)sorted_keys, (const uint32_t*)ids_b,
                       (const unsigned long long*)key_first, head);
    BSLAM_HIP_TRY(hipGetLastError());
    if ((rc = device_scan(stream, 0, head, vertex_count, false, rank, tile_sums, words + kRepairUnique))) return rc;
    hipLaunchKernelGGL(repair_run_first_kernel, flat_grid(V), block, 0, stream, vertex_count, (const uint8_t*)head, (const uint32_t*)rank, (const uint32_t*)ids_b, first);
    BSLAM_HIP_TRY(hipGetLastError());
    hipLaunchKernelGGL(repair_representative_kernel, flat_grid(V), block, 0, stream, vertex_count, (const uint32_t*)rank, (const uint32_t*)ids_b, (const uint32_t*)first, rep);
    BSLAM_HIP_TRY(hipGetLastError());
    if ((rc = timer.end(2))) return rc;
  }
  // stage 3: triangles through rep, their keys
  if ((rc = timer.begin(3))) return rc;
  BSLAM_HIP_TRY(hipMemsetAsync(referenced, 0, V, stream));
  if (T != 0) {
    hipLaunchKernelGGL(repair_triangle_kernel, flat_grid(T), block, 0, stream, vertex_count, triangle_count, indices, (const uint32_t*)rep, remove_duplicates, bits, keep,
                       key_first, key_second, ids, words);
    BSLAM_HIP_TRY(hipGetLastError());
  }
  if ((rc = timer.end(3))) return rc;
  if (T != 0 && remove_duplicates) {
    // stage 4: the two stable sorts, by hi and then by (lo, mid): a run is in ascending triangle id
    if ((rc = timer.begin(4))) return rc;
    if ((rc = mesh_sort(call, sort_temp, sort_bytes, key_first, sorted_keys, ids, ids_a, T, bits, stream))) return rc;
    hipLaunchKernelGGL(mesh_gather_kernel, flat_grid(T), block, 0, stream, triangle_count, (const unsigned long long*)key_second, (const uint32_t*)ids_a, gathered);
    BSLAM_HIP_TRY(hipGetLastError());
    if ((rc = mesh_sort(call, sort_temp, sort_bytes, gathered, sorted_keys, ids_a, ids_b, T, 2 * bits, stream))) return rc;
    if ((rc = timer.end(4))) return rc;
    // stage 5: duplicates
    if ((rc = timer.begin(5))) return rc;
    hipLaunchKernelGGL(mesh_heads_kernel, flat_grid(T), block, 0, stream, triangle_count, (const unsigned long long*)sorted_keys, (const uint32_t*)ids_b,
                       (const unsigned long long*)key_first, head);
    BSLAM_HIP_TRY(hipGetLastError());
    hipLaunchKernelGGL(repair_duplicate_kernel, flat_grid(T), block, 0, stream, triangle_count, (const uint8_t*)head, (const uint32_t*)ids_b, keep, words);
    BSLAM_HIP_TRY(hipGetLastError());
    if ((rc = timer.end(5))) return rc;
  }
  // stage 6: kept flags and their scans
  if ((rc = timer.begin(6))) return rc;
  if (T != 0) {
    hipLaunchKernelGGL(repair_reference_kernel, flat_grid(T), block, 0, stream, triangle_count, indices, (const uint32_t*)rep, (const uint8_t*)keep, referenced);
    BSLAM_HIP_TRY(hipGetLastError());
  }
  hipLaunchKernelGGL(repair_keep_vertex_kernel, flat_grid(V), block, 0, stream, vertex_count, (const uint32_t*)rep, (const uint8_t*)referenced,
                     (!remove_unreferenced || T == 0) ? 1 : 0, keep_vertex);
  BSLAM_HIP_TRY(hipGetLastError());
  if ((rc = device_scan(stream, 0, keep_vertex, vertex_count, true, vertex_rank, tile_sums, words + kRepairVertices))) return rc;
  if ((rc = device_scan(stream, 0, keep, triangle_count, true, triangle_rank, tile_sums, words + kRepairTriangles))) return rc;
  if ((rc = timer.end(6))) return rc;
  // an index >= V was never looked up, but the scatter goes through rep: it runs behind the error word
  const uint32_t* host = nullptr;
  if ((rc = read_back(ctx, stream, (const uint32_t*)words, 8, &host))) return rc;
  if ((rc = mesh_error(host[kRepairError], call))) return rc;
  const uint32_t unique = weld ? host[kRepairUnique] : vertex_count, kept_vertices = host[kRepairVertices], kept_triangles = host[kRepairTriangles],
                 degenerate = host[kRepairDegenerates], duplicate = host[kRepairDuplicates];
  // stage 7: scatter
  if ((rc = timer.begin(7))) return rc;
  MeshCompact m;
  m.vertices = vertex_count; m.triangles = triangle_count; m.vertex_blocks = flat_grid(V).x;
  m.positions = positions; m.normals = normals; m.colors = (const uint32_t*)colors; m.indices = indices;
  m.keep_vertex = keep_vertex; m.keep_triangle = keep; m.vertex_rank = vertex_rank; m.triangle_rank = triangle_rank; m.rep = rep;
  m.out_positions = out_positions; m.out_normals = out_normals; m.out_colors = (uint32_t*)out_colors; m.out_indices = out_indices;
  m.vertex_map = vertex_map; m.triangle_map = triangle_map;
  hipLaunchKernelGGL(mesh_compact_kernel, dim3(m.vertex_blocks + flat_grid(T).x), block, 0, stream, m);
  BSLAM_HIP_TRY(hipGetLastError());
  if ((rc = timer.end(7))) return rc;
  BSLAM_HIP_TRY(hipStreamSynchronize(stream));
  if ((rc = timer.collect())) return rc;
  *out_vertex_count = kept_vertices;
  *out_triangle_count = kept_triangles;
  counts4[0] = vertex_count - unique; counts4[1] = unique - kept_vertices; counts4[2] = degenerate; counts4[3] = duplicate;
  return BSLAM_OK;
}

int bslam_mesh_topology(bslam_context* ctx, void* stream_, uint32_t vertex_count, uint32_t triangle_count, const uint32_t* indices, bslam_mesh_report* report,
                        uint32_t* edge_uses, uint32_t* loop_of_slot) {
  hipStream_t stream = (hipStream_t)stream_;
  const char* call = "bslam_mesh_topology";
  if (!ctx || !report) return fail(BSLAM_ERR_INVALID_ARGUMENT, "null argument");
  const size_t V = vertex_count, T = triangle_count, E = 3 * T;
  if (V > 0xffffff00ull || E > 0xffffff00ull) return fail(BSLAM_ERR_INVALID_ARGUMENT, "more than 2^32 - 256 vertices or triangle corners");
  const MeshSpan spans[3] = {{indices, 12 * T, "indices", false}, {edge_uses, edge_uses ? 4 * E : 0, "edge_uses", true},
                             {loop_of_slot, loop_of_slot ? 4 * E : 0, "loop_of_slot", true}};
  int rc = check_mesh_spans(spans, 3);
  if (rc) return rc;
  BSLAM_HIP_TRY(hipSetDevice(ctx->device));
  RepairTimer timer(ctx, stream);
  if (V == 0) {
    if ((rc = empty_mesh(stream, T, call)) == BSLAM_OK) std::memset(report, 0, sizeof(*report));
    return rc;
  }
  size_t sort_bytes = 0;
  if ((rc = mesh_sort_bytes(std::max<size_t>(E, 1), stream, &sort_bytes))) return rc;
  RepairTopology s = {};
  uint32_t* tile_sums;
  uint8_t* sort_temp;
  if ((rc = carve(ctx->repair, [&](Carver& c) { topology_layout(c, vertex_count, triangle_count, indices, &s, &tile_sums, &sort_temp, sort_bytes); }))) return rc;
  s.edge_uses = edge_uses; s.loop_of_slot = loop_of_slot;
  if ((rc = repair_clear_words(s.words, stream))) return rc;
  uint32_t B = 0;
  int at = 0;
  if ((rc = topology_pass(ctx, stream, call, s, tile_sums, sort_temp, sort_bytes, timer, 0, nullptr, nullptr, &B, &at))) return rc;
  const uint32_t* host = nullptr;
  if ((rc = read_back(ctx, stream, (const uint32_t*)s.words, kRepairWords, &host))) return rc;
  if ((rc = timer.collect())) return rc;
  if ((rc = mesh_error(host[kRepairError], call))) return rc;
  topology_report(host, triangle_count, report);
  return BSLAM_OK;
}

int bslam_fill_mesh_holes(bslam_context* ctx, void* stream_, uint32_t vertex_count, uint32_t triangle_count, const float* positions, const float* normals,
                          const void* colors, const uint32_t* indices, uint32_t max_hole_edges, uint32_t vertex_capacity, uint32_t triangle_capacity,
                          float* out_positions, float* out_normals, void* out_colors, uint32_t* out_indices, uint32_t* hole_of_triangle,
                          uint32_t* out_vertex_count, uint32_t* out_triangle_count, uint32_t* filled_holes) {
  hipStream_t stream = (hipStream_t)stream_;
  const char* call = "bslam_fill_mesh_holes";
  if (!ctx || !out_vertex_count || !out_triangle_count || !filled_holes) return fail(BSLAM_ERR_INVALID_ARGUMENT, "null argument");
  if (max_hole_edges < 3 || max_hole_edges > 4096) return fail(BSLAM_ERR_INVALID_ARGUMENT, "max_hole_edges must lie in [3, 4096]");
  const size_t V = vertex_count, T = triangle_count, E = 3 * T, VC = vertex_capacity, TC = triangle_capacity;
  if (V > 0xffffff00ull || E > 0xffffff00ull) return fail(BSLAM_ERR_INVALID_ARGUMENT, "more than 2^32 - 256 vertices or triangle corners");
  const bool buffers = out_positions != nullptr && out_indices != nullptr;
  const MeshArrays arrays = {positions, normals, colors, indices, out_positions, out_normals, out_colors, out_indices};
  int rc;
  if (buffers && (rc = check_attribute_pairs(arrays))) return rc;
  const size_t room = TC > T ? TC - T : 0;   // for appended triangles
  const MeshSpan spans[9] = {{positions, 12 * V, "positions", false}, {normals, normals ? 12 * V : 0, "normals", false}, {colors, colors ? 4 * V : 0, "colors", false},
                             {indices, 12 * T, "indices", false}, {out_positions, buffers ? 12 * VC : 0, "out_positions", true},
                             {out_normals, buffers && normals ? 12 * VC : 0, "out_normals", true}, {out_colors, buffers && colors ? 4 * VC : 0, "out_colors", true},
                             {out_indices, buffers ? 12 * TC : 0, "out_indices", true},
                             {hole_of_triangle, buffers && hole_of_triangle ? 4 * room : 0, "hole_of_triangle", true}};
  if ((rc = check_mesh_spans(spans, 9))) return rc;
  BSLAM_HIP_TRY(hipSetDevice(ctx->device));
  RepairTimer timer(ctx, stream);
  if (V == 0) {
    if ((rc = empty_mesh(stream, T, call)) == BSLAM_OK) *out_vertex_count = *out_triangle_count = *filled_holes = 0;
    return rc;
  }
  size_t sort_bytes = 0;
  if ((rc = mesh_sort_bytes(std::max<size_t>(E, 1), stream, &sort_bytes))) return rc;
  // scratch: that of the census | per boundary slot: fill flags u8, fan sizes, hole ordinals, fan offsets u32
  RepairTopology s = {};
  uint32_t *tile_sums, *fan, *ordinal, *fan_offset;
  uint8_t *sort_temp, *fill_flag;
  const size_t ne = pad64(E);
  if ((rc = carve(ctx->repair, [&](Carver& c) {
         topology_layout(c, vertex_count, triangle_count, indices, &s, &tile_sums, &sort_temp, sort_bytes);
         fill_flag = c.take<uint8_t>(ne, 64); fan = c.take<uint32_t>(ne, 64); ordinal = c.take<uint32_t>(ne, 64); fan_offset = c.take<uint32_t>(ne, 64);
       }))) return rc;
  if ((rc = repair_clear_words(s.words, stream))) return rc;
  const dim3 block(256);
  hipLaunchKernelGGL(mesh_check_positions_kernel, flat_grid(V), block, 0, stream, vertex_count, positions, s.words + kRepairError);
  BSLAM_HIP_TRY(hipGetLastError());
  uint32_t B = 0;
  int at = 0;
  if ((rc = topology_pass(ctx, stream, call, s, tile_sums, sort_temp, sort_bytes, timer, max_hole_edges, fill_flag, fan, &B, &at))) return rc;
  if (B != 0) {
    // stage 4: the holes in ascending loop id and the places of their fans
    if ((rc = timer.begin(4))) return rc;
    if ((rc = device_scan(stream, 0, fill_flag, B, true, ordinal, tile_sums, s.words + kRepairFilled))) return rc;
    if ((rc = device_scan(stream, 1, fan, B, true, fan_offset, tile_sums, s.words + kRepairFanTriangles))) return rc;
    if ((rc = timer.end(4))) return rc;
  }
  const uint32_t* host = nullptr;
  if ((rc = read_back(ctx, stream, (const uint32_t*)s.words, kRepairWords, &host))) return rc;
  if ((rc = mesh_error(host[kRepairError], call))) return rc;
  const size_t filled = host[kRepairFilled], added = host[kRepairFanTriangles], V2 = V + filled, T2 = T + added;
  if (V2 > 0xffffff00ull || T2 > 0xffffff00ull) return fail(BSLAM_ERR_INVALID_ARGUMENT, "%s: the filled mesh has more than 2^32 - 256 vertices or triangles", call);
  if (buffers && V2 <= VC && T2 <= TC) {
    // stage 5: the input, then the centroids and the fans
    if ((rc = timer.begin(5))) return rc;
    BSLAM_HIP_TRY(hipMemcpyAsync(out_positions, positions, 12 * V, hipMemcpyDeviceToDevice, stream));
    if (normals) BSLAM_HIP_TRY(hipMemcpyAsync(out_normals, normals, 12 * V, hipMemcpyDeviceToDevice, stream));
    if (colors) BSLAM_HIP_TRY(hipMemcpyAsync(out_colors, colors, 4 * V, hipMemcpyDeviceToDevice, stream));
    if (T != 0) BSLAM_HIP_TRY(hipMemcpyAsync(out_indices, indices, 12 * T, hipMemcpyDeviceToDevice, stream));
    if (filled != 0) {
      RepairFill f;
      f.vertices = vertex_count; f.triangles = triangle_count; f.positions = positions; f.normals = normals; f.colors = (const uint32_t*)colors;
      f.fill_flag = fill_flag; f.fan = fan; f.ordinal = ordinal; f.fan_offset = fan_offset;
      f.out_positions = out_positions; f.out_normals = out_normals; f.out_colors = (uint32_t*)out_colors; f.out_indices = out_indices;
      f.hole_of_triangle = hole_of_triangle;
      hipLaunchKernelGGL(repair_fill_kernel, flat_grid(B), block, 0, stream, s, f, B);
      BSLAM_HIP_TRY(hipGetLastError());
    }
    if ((rc = timer.end(5))) return rc;
    BSLAM_HIP_TRY(hipStreamSynchronize(stream));
  }
  if ((rc = timer.collect())) return rc;
  *out_vertex_count = (uint32_t)V2;
  *out_triangle_count = (uint32_t)T2;
  *filled_holes = (uint32_t)filled;
  return BSLAM_OK;
}

int bslam_repair_stage_times(bslam_context* ctx, float* stage_ms8) {
  if (!ctx || !stage_ms8) return fail(BSLAM_ERR_INVALID_ARGUMENT, "null argument");
  std::memcpy(stage_ms8, ctx->repair_stage_ms, sizeof(ctx->repair_stage_ms));
  return BSLAM_OK;
}

}  // extern "C"
