// orient_abi.inc -- bslam_orient_mesh of include/badslam_hip.h (included by badslam_hip.hip after mesh_abi.inc: check_mesh_spans,
// mesh_error, mesh_sort_bytes, edge_runs_layout, build_edge_runs; and repair_abi.inc: RepairTimer, repair_clear_words, the layout of
// the words; read_back, carve).

namespace bslam {

static void orient_report(const uint32_t* c, bslam_orient_report* r) {
  r->patches = c[kOrientPatches]; r->orientable_patches = c[kOrientOrientable]; r->nonorientable_patches = c[kOrientNonOrientable];
  r->closed_patches = c[kOrientClosed]; r->seams = c[kOrientSeams]; r->disagreeing_seams_before = c[kOrientDisagreeBefore];
  r->disagreeing_seams_after = c[kOrientDisagreeAfter]; r->flipped_triangles = c[kOrientFlipped]; r->inverted_patches = c[kOrientInverted];
  r->fallback_patches = c[kOrientFallback];
}

}  // namespace bslam

extern "C" {

int bslam_orient_mesh(bslam_context* ctx, void* stream_, uint32_t vertex_count, uint32_t triangle_count, const float* positions, const float* normals,
                      const uint32_t* indices, int mode, uint32_t* out_indices, uint8_t* flipped, uint32_t* patch_of_triangle, bslam_orient_report* report) {
  hipStream_t stream = (hipStream_t)stream_;
  const char* call = "bslam_orient_mesh";
  if (!ctx || !report) return fail(BSLAM_ERR_INVALID_ARGUMENT, "null argument");
  if (mode != kOrientMajority && mode != kOrientNormals && mode != kOrientVolume) return fail(BSLAM_ERR_INVALID_ARGUMENT, "mode must be 0 (majority), 1 (normals) or 2 (volume)");
  if (mode == kOrientNormals && !normals) return fail(BSLAM_ERR_INVALID_ARGUMENT, "mode 1 (normals) needs normals");
  const size_t V = vertex_count, T = triangle_count, E = 3 * T;
  if (V > 0xffffff00ull || E > 0xffffff00ull) return fail(BSLAM_ERR_INVALID_ARGUMENT, "more than 2^32 - 256 vertices or triangle corners");
  const MeshSpan spans[6] = {{positions, 12 * V, "positions", false}, {normals, mode == kOrientNormals ? 12 * V : 0, "normals", false},
                             {indices, 12 * T, "indices", false}, {out_indices, 12 * T, "out_indices", true}, {flipped, flipped ? T : 0, "flipped", true},
                             {patch_of_triangle, patch_of_triangle ? 4 * T : 0, "patch_of_triangle", true}};
  int rc = check_mesh_spans(spans, 6);
  if (rc) return rc;
  BSLAM_HIP_TRY(hipSetDevice(ctx->device));
  RepairTimer timer(ctx, stream);
  if (V == 0) {
    if ((rc = empty_mesh(stream, T, call)) == BSLAM_OK) std::memset(report, 0, sizeof(*report));
    return rc;
  }
  size_t sort_bytes = 0;
  if ((rc = mesh_sort_bytes(std::max<size_t>(E, 1), stream, &sort_bytes))) return rc;
  // scratch: words of the census and of this call | the edge runs | seam codes per slot | per triangle: links, patches, the five sums u32,
  //          volumes i64, open, flip0, invert u8 | scan sums | the sort's own
  const size_t nt = pad64(T), ne = pad64(E), tiles = ne / kScanTile + 2;
  OrientMesh m = {};
  uint32_t *words, *tile_sums;
  uint8_t* sort_temp;
  if ((rc = carve(ctx->repair, [&](Carver& c) {
         words = c.take<uint32_t>(kRepairWords + kOrientWords, 16);
         edge_runs_layout(c, vertex_count, triangle_count, indices, words + kRepairError, &m.runs);
         m.seam = c.take<uint8_t>(ne, 64);
         m.link = c.take<uint32_t>(nt, 64); m.patch = c.take<uint32_t>(nt, 64); m.state = c.take<uint32_t>(nt, 64); m.size = c.take<uint32_t>(nt, 64);
         m.ones = c.take<uint32_t>(nt, 64); m.positive = c.take<uint32_t>(nt, 64); m.negative = c.take<uint32_t>(nt, 64); m.volume = c.take<long long>(nt, 64);
         m.open = c.take<uint8_t>(nt, 64); m.flip0 = c.take<uint8_t>(nt, 64); m.invert = c.take<uint8_t>(nt, 64);
         tile_sums = c.take<uint32_t>(tiles, 16);
         sort_temp = c.take<uint8_t>(sort_bytes, 256);
       }))) return rc;
  m.mode = mode;
  while ((T >> m.size_bits) != 0) ++m.size_bits;
  m.positions = positions; m.normals = mode == kOrientNormals ? normals : nullptr;
  m.out_indices = out_indices; m.flipped = flipped; m.patch_of_triangle = patch_of_triangle;
  m.counts = words + kRepairWords;
  const dim3 block(256);
  if ((rc = repair_clear_words(words, stream))) return rc;
  BSLAM_HIP_TRY(hipMemsetAsync(m.counts, 0, kOrientWords * sizeof(uint32_t), stream));
  BSLAM_HIP_TRY(hipMemsetAsync(m.counts + kOrientMin, 0xff, 3 * sizeof(uint32_t), stream));
  // stage 0: the position check, the bounds of mode 2, the edge keys; stage 1: the stable sort of (edge, slot); stage 2: the runs
  if ((rc = timer.begin(0))) return rc;
  hipLaunchKernelGGL(mesh_check_positions_kernel, flat_grid(V), block, 0, stream, vertex_count, positions, m.runs.error);
  BSLAM_HIP_TRY(hipGetLastError());
  if (mode == kOrientVolume && T != 0) {
    hipLaunchKernelGGL(orient_bounds_kernel, flat_grid(V), block, 0, stream, vertex_count, positions, m.counts);
    BSLAM_HIP_TRY(hipGetLastError());
  }
  if ((rc = build_edge_runs(ctx, stream, call, m.runs, tile_sums, sort_temp, sort_bytes, timer, words + kRepairEdges))) return rc;
  if (T == 0) {
    if ((rc = timer.collect())) return rc;
    std::memset(report, 0, sizeof(*report));
    return BSLAM_OK;
  }
  if ((rc = timer.end(2))) return rc;
  // stage 3: the parity union-find, one launch
  if ((rc = timer.begin(3))) return rc;
  hipLaunchKernelGGL(orient_init_kernel, flat_grid(T), block, 0, stream, m);
  BSLAM_HIP_TRY(hipGetLastError());
  hipLaunchKernelGGL(orient_union_kernel, flat_grid(E), block, 0, stream, m);
  BSLAM_HIP_TRY(hipGetLastError());
  if ((rc = timer.end(3))) return rc;
  // stage 4: the seams again
  if ((rc = timer.begin(4))) return rc;
  hipLaunchKernelGGL(orient_conflict_kernel, flat_grid(E), block, 0, stream, m);
  BSLAM_HIP_TRY(hipGetLastError());
  if ((rc = timer.end(4))) return rc;
  // stage 5: patches, flip0 and the votes
  if ((rc = timer.begin(5))) return rc;
  hipLaunchKernelGGL(orient_flatten_kernel, flat_grid(T), block, 0, stream, m);
  BSLAM_HIP_TRY(hipGetLastError());
  if ((rc = timer.end(5))) return rc;
  // stage 6: the side of every patch, the indices
  if ((rc = timer.begin(6))) return rc;
  hipLaunchKernelGGL(orient_decide_kernel, flat_grid(T), block, 0, stream, m);
  BSLAM_HIP_TRY(hipGetLastError());
  const uint32_t triangle_blocks = flat_grid(T).x;
  hipLaunchKernelGGL(orient_write_kernel, dim3(triangle_blocks + flat_grid(E).x), block, 0, stream, m, triangle_blocks);
  BSLAM_HIP_TRY(hipGetLastError());
  if ((rc = timer.end(6))) return rc;
  const uint32_t* host = nullptr;
  if ((rc = read_back(ctx, stream, (const uint32_t*)words, (size_t)kRepairWords + kOrientWords, &host))) return rc;
  if ((rc = timer.collect())) return rc;
  if ((rc = mesh_error(host[kRepairError], call))) return rc;
  orient_report(host + kRepairWords, report);
  return BSLAM_OK;
}

}  // extern "C"
