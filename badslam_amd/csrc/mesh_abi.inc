// mesh_abi.inc -- mesh component entry points of include/badslam_hip.h, and the host pieces the mesh operators behind it share
// (simplify_abi.inc, decimate_abi.inc, smooth_abi.inc, repair_abi.inc, orient_abi.inc): span checks, the error word, the triangle remap,
// the radix sort, the edge runs.  Included by badslam_hip.hip after lifecycle_abi.inc and fusion_abi.inc: device_scan, the fusion slab.

namespace bslam {

// A flat device array of `bytes` bytes a mesh call reads or writes.
struct MeshSpan { const void* ptr; size_t bytes; const char* name; bool output; };

// Every non-empty array is non-null and 4 byte aligned; no output overlaps an input or another output.
static int check_mesh_spans(const MeshSpan* spans, int count) {
  for (int i = 0; i < count; ++i) {
    if (spans[i].bytes == 0) continue;
    if (!spans[i].ptr) return fail(BSLAM_ERR_INVALID_ARGUMENT, "%s is null", spans[i].name);
    if ((uintptr_t)spans[i].ptr % 4 != 0) return fail(BSLAM_ERR_INVALID_ARGUMENT, "%s must be 4 byte aligned", spans[i].name);
  }
  for (int i = 0; i < count; ++i) {
    for (int j = i + 1; j < count; ++j) {
      if (!(spans[i].output || spans[j].output) || spans[i].bytes == 0 || spans[j].bytes == 0) continue;
      const uintptr_t a0 = (uintptr_t)spans[i].ptr, b0 = (uintptr_t)spans[j].ptr;
      if (a0 < b0 + spans[j].bytes && b0 < a0 + spans[i].bytes) return fail(BSLAM_ERR_INVALID_ARGUMENT, "%s and %s overlap", spans[i].name, spans[j].name);
    }
  }
  return BSLAM_OK;
}

// An attributed mesh in and out: normals and colors are optional, and each output is given exactly when its input is.
struct MeshArrays {
  const float* positions; const float* normals; const void* colors; const uint32_t* indices;
  float* out_positions; float* out_normals; void* out_colors; uint32_t* out_indices;
};

static int check_attribute_pairs(const MeshArrays& m) {
  if ((m.normals != nullptr) != (m.out_normals != nullptr)) return fail(BSLAM_ERR_INVALID_ARGUMENT, "out_normals must be given exactly when normals is");
  if ((m.colors != nullptr) != (m.out_colors != nullptr)) return fail(BSLAM_ERR_INVALID_ARGUMENT, "out_colors must be given exactly when colors is");
  return BSLAM_OK;
}

// The spans of `m` for V vertices and T triangles: the four inputs to in[0 .. 3], the four outputs to out[0 .. 3].  The caller places
// them among the spans of its own, in the order in which check_mesh_spans is to report.
static void mesh_array_spans(const MeshArrays& m, size_t V, size_t T, MeshSpan* in, MeshSpan* out) {
  const size_t nb = m.normals ? 12 * V : 0, cb = m.colors ? 4 * V : 0;
  in[0] = {m.positions, 12 * V, "positions", false}; in[1] = {m.normals, nb, "normals", false}; in[2] = {m.colors, cb, "colors", false};
  in[3] = {m.indices, 12 * T, "indices", false};
  out[0] = {m.out_positions, 12 * V, "out_positions", true}; out[1] = {m.out_normals, nb, "out_normals", true}; out[2] = {m.out_colors, cb, "out_colors", true};
  out[3] = {m.out_indices, 12 * T, "out_indices", true};
}

static int mesh_error(uint32_t bits, const char* call) {
  if (bits & kMeshBadIndex) return fail(BSLAM_ERR_INVALID_ARGUMENT, "%s: a triangle names a vertex beyond vertex_count", call);
  if (bits & kMeshOverrun) return fail(BSLAM_ERR_INTERNAL, "%s: a union-find loop ran into its cap", call);
  if (bits & kMeshBadPosition) return fail(BSLAM_ERR_INVALID_ARGUMENT, "%s: a vertex is not finite", call);
  if (bits & kMeshDegenerate) return fail(BSLAM_ERR_INVALID_ARGUMENT, "%s: a triangle repeats an index (bslam_clean_mesh drops such triangles)", call);
  return BSLAM_OK;
}

// The V == 0 case of a mesh call: nothing is launched, and any triangle names a vertex that does not exist.
static int empty_mesh(hipStream_t stream, size_t triangles, const char* call) {
  BSLAM_HIP_TRY(hipStreamSynchronize(stream));
  return triangles != 0 ? mesh_error(kMeshBadIndex, call) : BSLAM_OK;
}

// A count padded to a multiple of 64, as the scratch arrays of the mesh calls are (and as in bslam_extract_mesh).
static size_t pad64(size_t count) { return (count + 63) & ~(size_t)63; }

// The bits of a vertex id below V >= 1: at least one.
static unsigned vertex_id_bits(size_t V) {
  unsigned bits = 1;
  while (bits < 32 && (V - 1) >> bits) ++bits;
  return bits;
}

// The triangle remap of mesh_kernels.hpp: the keep flags of `triangles` triangles through `map`, their exclusive scan -- whose total
// goes to *kept, a word of the call's device block -- and the scatter into `out`.  words[0] is the call's error word.  Without
// triangles the scan alone runs: it writes the total.
static int remap_triangles(hipStream_t stream, uint32_t vertices, uint32_t triangles, const uint32_t* indices, const uint32_t* map, uint8_t* keep, uint32_t* rank,
                           uint32_t* tile_sums, uint32_t* words, uint32_t* kept, uint32_t* out) {
  const dim3 block(256);
  if (triangles != 0) {
    hipLaunchKernelGGL(mesh_remap_keep_kernel, flat_grid(triangles), block, 0, stream, vertices, triangles, indices, map, keep, words);
    BSLAM_HIP_TRY(hipGetLastError());
  }
  if (int rc = device_scan(stream, 0, keep, triangles, true, rank, tile_sums, kept)) return rc;
  if (triangles != 0) {
    hipLaunchKernelGGL(mesh_remap_scatter_kernel, flat_grid(triangles), block, 0, stream, triangles, indices, map, (const uint8_t*)keep, (const uint32_t*)rank, out);
    BSLAM_HIP_TRY(hipGetLastError());
  }
  return BSLAM_OK;
}

// mesh_sort.hip
hipError_t mesh_sort_pairs(void* temp, size_t* temp_bytes, const unsigned long long* keys, unsigned long long* sorted_keys, const uint32_t* ids,
                           uint32_t* sorted_ids, size_t count, unsigned end_bit, hipStream_t stream);

// The scratch a sort of up to `count` pairs over all 64 key bits needs.
static int mesh_sort_bytes(size_t count, hipStream_t stream, size_t* bytes) {
  BSLAM_HIP_TRY(mesh_sort_pairs(nullptr, bytes, nullptr, nullptr, nullptr, nullptr, count, 64, stream));
  return BSLAM_OK;
}

// One stable sort of `count` pairs over the key bits [0, end_bit) in the `temp_bytes` of scratch at `temp`.
static int mesh_sort(const char* call, void* temp, size_t temp_bytes, const unsigned long long* keys, unsigned long long* sorted_keys, const uint32_t* ids,
                     uint32_t* sorted_ids, size_t count, unsigned end_bit, hipStream_t stream) {
  size_t need = 0;
  BSLAM_HIP_TRY(mesh_sort_pairs(nullptr, &need, keys, sorted_keys, ids, sorted_ids, count, end_bit, stream));
  if (need > temp_bytes) return fail(BSLAM_ERR_INTERNAL, "%s: a sort of %zu pairs needs %zu bytes of scratch where %zu were reserved", call, count, need, temp_bytes);
  BSLAM_HIP_TRY(mesh_sort_pairs(temp, &need, keys, sorted_keys, ids, sorted_ids, count, end_bit, stream));
  return BSLAM_OK;
}

// The edge runs of mesh_kernels.hpp for the V >= 1 vertices and T triangles of `indices`: the scalars, and the arrays carved from `c`
// (referenced is left null).  `error` is the error word of the call.
static void edge_runs_layout(Carver& c, uint32_t V, uint32_t T, const uint32_t* indices, uint32_t* error, EdgeRuns* runs) {
  const size_t ne = pad64(3 * (size_t)T);
  runs->vertices = V; runs->triangles = T; runs->slots = 3 * T; runs->bits = vertex_id_bits(V); runs->indices = indices; runs->error = error;
  runs->keys = c.take<unsigned long long>(ne, 64); runs->sorted_keys = c.take<unsigned long long>(ne, 64); runs->ids = c.take<uint32_t>(ne, 64);
  runs->sorted_slots = c.take<uint32_t>(ne, 64); runs->head = c.take<uint8_t>(ne, 64); runs->rank = c.take<uint32_t>(ne, 64);
  runs->start_of = c.take<uint32_t>(ne + 64, 64);
}

// Builds `runs` in the stages 0 .. 2 of `timer` (RepairTimer; a template parameter only because repair_abi.inc, which defines it, is
// included behind this file).  The caller has opened stage 0 and may have launched kernels of its own there.  Here: the keys, the end of stage 0, the read-back of the error word -- nothing is decoded from the key of
// a triangle that must not be looked at, and no output is written for a mesh that is refused --, the stable sort as stage 1 (the uses
// of an edge stay in ascending slot) and, in stage 2, the heads, their scan, whose total goes to *unique_edges, a word on the device,
// and the starts.  Stage 2 is left open for the caller to close.  Without triangles it returns behind the read-back.
template <class Timer>
static int build_edge_runs(bslam_context* ctx, hipStream_t stream, const char* call, const EdgeRuns& runs, uint32_t* tile_sums, uint8_t* sort_temp, size_t sort_bytes,
                           Timer& timer, uint32_t* unique_edges) {
  const dim3 block(256);
  const size_t T = runs.triangles, E = runs.slots;
  int rc;
  if (T != 0) {
    hipLaunchKernelGGL(edge_keys_kernel, flat_grid(T), block, 0, stream, runs);
    BSLAM_HIP_TRY(hipGetLastError());
  }
  if ((rc = timer.end(0))) return rc;
  const uint32_t* host = nullptr;
  if ((rc = read_back(ctx, stream, (const uint32_t*)runs.error, 1, &host))) return rc;
  if ((rc = mesh_error(host[0], call))) return rc;
  if (T == 0) return BSLAM_OK;
  if ((rc = timer.begin(1))) return rc;
  if ((rc = mesh_sort(call, sort_temp, sort_bytes, runs.keys, runs.sorted_keys, runs.ids, runs.sorted_slots, E, 2 * runs.bits, stream))) return rc;
  if ((rc = timer.end(1))) return rc;
  if ((rc = timer.begin(2))) return rc;
  hipLaunchKernelGGL(mesh_heads_kernel, flat_grid(E), block, 0, stream, runs.slots, (const unsigned long long*)runs.sorted_keys, (const uint32_t*)runs.sorted_slots,
                     (const unsigned long long*)nullptr, runs.head);
  BSLAM_HIP_TRY(hipGetLastError());
  if ((rc = device_scan(stream, 0, runs.head, runs.slots, false, runs.rank, tile_sums, unique_edges))) return rc;
  hipLaunchKernelGGL(edge_starts_kernel, flat_grid(E), block, 0, stream, runs);
  BSLAM_HIP_TRY(hipGetLastError());
  return BSLAM_OK;
}

}  // namespace bslam

extern "C" {

int bslam_mesh_components(bslam_context* ctx, void* stream_, uint32_t vertex_count, uint32_t triangle_count, const uint32_t* indices, uint32_t* labels,
                          uint32_t* sizes, uint32_t* component_count) {
  hipStream_t stream = (hipStream_t)stream_;
  if (!ctx || !component_count) return fail(BSLAM_ERR_INVALID_ARGUMENT, "null argument");
  const size_t V = vertex_count, T = triangle_count;
  const MeshSpan spans[3] = {{indices, 12 * T, "indices", false}, {labels, 4 * V, "labels", true}, {sizes, 4 * V, "sizes", true}};
  int rc = check_mesh_spans(spans, 3);
  if (rc) return rc;
  BSLAM_HIP_TRY(hipSetDevice(ctx->device));
  if (V == 0) {
    if ((rc = empty_mesh(stream, T, "bslam_mesh_components")) == BSLAM_OK) *component_count = 0;
    return rc;
  }
  // scratch: parent u32[V] | size_of_root u32[V] | words u32[2] = {error bits, component count}
  uint32_t *parent, *size_of_root, *words;
  if ((rc = carve(ctx->fusion, [&](Carver& c) { parent = c.take<uint32_t>(V); size_of_root = c.take<uint32_t>(V); words = c.take<uint32_t>(16); }))) return rc;
  const dim3 block(256);
  hipLaunchKernelGGL(mesh_init_kernel, flat_grid(V), block, 0, stream, vertex_count, parent, size_of_root, words);
  BSLAM_HIP_TRY(hipGetLastError());
  if (T != 0) {
    hipLaunchKernelGGL(mesh_seed_kernel, flat_grid(T), block, 0, stream, vertex_count, triangle_count, indices, parent, words);
    BSLAM_HIP_TRY(hipGetLastError());
    hipLaunchKernelGGL(mesh_compress_kernel, flat_grid(V), block, 0, stream, vertex_count, parent, words);
    BSLAM_HIP_TRY(hipGetLastError());
    hipLaunchKernelGGL(mesh_union_kernel, flat_grid(T), block, 0, stream, vertex_count, triangle_count, indices, parent, words, cull_stats_ptr(ctx));
    BSLAM_HIP_TRY(hipGetLastError());
  }
  hipLaunchKernelGGL(mesh_flatten_kernel, flat_grid(V), block, 0, stream, vertex_count, (const uint32_t*)parent, labels, size_of_root, words);
  BSLAM_HIP_TRY(hipGetLastError());
  hipLaunchKernelGGL(mesh_sizes_kernel, flat_grid(V), block, 0, stream, vertex_count, (const uint32_t*)labels, (const uint32_t*)size_of_root, sizes);
  BSLAM_HIP_TRY(hipGetLastError());
  const uint32_t* host = nullptr;
  if ((rc = read_back(ctx, stream, (const uint32_t*)words, 2, &host))) return rc;
  if ((rc = mesh_error(host[0], "bslam_mesh_components"))) return rc;
  *component_count = host[1];
  return BSLAM_OK;
}

int bslam_filter_mesh(bslam_context* ctx, void* stream_, uint32_t vertex_count, uint32_t triangle_count, const float* positions, const float* normals,
                      const void* colors, const uint32_t* indices, const uint32_t* sizes, uint32_t min_vertices, float* out_positions, float* out_normals,
                      void* out_colors, uint32_t* out_indices, uint32_t* out_vertex_count, uint32_t* out_triangle_count) {
  hipStream_t stream = (hipStream_t)stream_;
  if (!ctx || !out_vertex_count || !out_triangle_count) return fail(BSLAM_ERR_INVALID_ARGUMENT, "null argument");
  if (min_vertices < 1) return fail(BSLAM_ERR_INVALID_ARGUMENT, "min_vertices must be >= 1");
  const MeshArrays arrays = {positions, normals, colors, indices, out_positions, out_normals, out_colors, out_indices};
  int rc = check_attribute_pairs(arrays);
  if (rc) return rc;
  const size_t V = vertex_count, T = triangle_count;
  MeshSpan spans[9];
  mesh_array_spans(arrays, V, T, spans, spans + 5);
  spans[4] = {sizes, 4 * V, "sizes", false};
  if ((rc = check_mesh_spans(spans, 9))) return rc;
  BSLAM_HIP_TRY(hipSetDevice(ctx->device));
  if (V == 0) {
    if ((rc = empty_mesh(stream, T, "bslam_filter_mesh")) == BSLAM_OK) *out_vertex_count = *out_triangle_count = 0;
    return rc;
  }
  // scratch: keep_vertex u8[V] | keep_triangle u8[T] | vertex_rank u32[V] | triangle_rank u32[T] | tile sums |
  //          words u32[4] = {error bits, unused, kept vertices, kept triangles}
  const size_t nv = pad64(V), nt = pad64(T), tiles = std::max(nv, nt) / kScanTile + 2;
  uint8_t *keep_vertex, *keep_triangle;
  uint32_t *vertex_rank, *triangle_rank, *tile_sums, *words;
  if ((rc = carve(ctx->fusion, [&](Carver& c) {
         keep_vertex = c.take<uint8_t>(nv, 64); keep_triangle = c.take<uint8_t>(nt, 64); vertex_rank = c.take<uint32_t>(nv, 64);
         triangle_rank = c.take<uint32_t>(nt, 64); tile_sums = c.take<uint32_t>(tiles); words = c.take<uint32_t>(16);
       }))) return rc;
  MeshFilter f;
  f.vertices = vertex_count; f.triangles = triangle_count; f.vertex_blocks = flat_grid(V).x; f.min_vertices = min_vertices; f.indices = indices; f.sizes = sizes;
  const dim3 grid(f.vertex_blocks + flat_grid(T).x), block(256);   // < 2^25 blocks
  BSLAM_HIP_TRY(hipMemsetAsync(words, 0, 2 * sizeof(uint32_t), stream));
  hipLaunchKernelGGL(mesh_keep_flags_kernel, grid, block, 0, stream, f, keep_vertex, keep_triangle, words);
  BSLAM_HIP_TRY(hipGetLastError());
  if ((rc = device_scan(stream, 0, keep_vertex, vertex_count, true, vertex_rank, tile_sums, words + 2))) return rc;
  if ((rc = device_scan(stream, 0, keep_triangle, triangle_count, true, triangle_rank, tile_sums, words + 3))) return rc;
  MeshCompact m = {};   // rep and the maps stay null: every vertex its own, no maps
  m.vertices = vertex_count; m.triangles = triangle_count; m.vertex_blocks = f.vertex_blocks;
  m.positions = positions; m.normals = normals; m.colors = (const uint32_t*)colors; m.indices = indices;
  m.keep_vertex = keep_vertex; m.keep_triangle = keep_triangle; m.vertex_rank = vertex_rank; m.triangle_rank = triangle_rank;
  m.out_positions = out_positions; m.out_normals = out_normals; m.out_colors = (uint32_t*)out_colors; m.out_indices = out_indices;
  hipLaunchKernelGGL(mesh_compact_kernel, grid, block, 0, stream, m);
  BSLAM_HIP_TRY(hipGetLastError());
  const uint32_t* host = nullptr;
  if ((rc = read_back(ctx, stream, (const uint32_t*)words, 4, &host))) return rc;
  if ((rc = mesh_error(host[0], "bslam_filter_mesh"))) return rc;
  *out_vertex_count = host[2];
  *out_triangle_count = host[3];
  return BSLAM_OK;
}

}  // extern "C"
