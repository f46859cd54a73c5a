// orient_abi.inc -- bslam_orient_mesh of include/badslam_hip.h (included by badslam_hip.hip after repair_abi.inc: RepairTimer,
// repair_error, repair_clear_words, the kernels of the census; check_mesh_spans, mesh_sort, device_scan, read_back, carve).

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
  // scratch: words of the census and of this call | per slot: keys, sorted keys, slots, sorted slots u64 / u32, head flags, ranks, run starts, seam codes |
  //          referenced u8[V] | per triangle: links, patches, the five sums u32, volumes i64, open, flip0, invert u8 | scan sums | the sort's own
  const size_t nv = pad64(V), nt = pad64(T), ne = pad64(E), tiles = ne / kScanTile + 2;
  RepairTopology s = {};
  OrientMesh m = {};
  uint32_t* tile_sums;
  uint8_t* sort_temp;
  if ((rc = carve(ctx->repair, [&](Carver& c) {
         s.words = c.take<uint32_t>(kRepairWords + kOrientWords, 16);
         s.keys = c.take<unsigned long long>(ne, 64); s.sorted_keys = c.take<unsigned long long>(ne, 64); s.ids = c.take<uint32_t>(ne, 64);
         s.sorted_slots = c.take<uint32_t>(ne, 64); s.head = c.take<uint8_t>(ne, 64); s.rank = c.take<uint32_t>(ne, 64); s.start_of = c.take<uint32_t>(ne + 64, 64);
         m.seam = c.take<uint8_t>(ne, 64);
         s.referenced = c.take<uint8_t>(nv, 64);
         m.link = c.take<uint32_t>(nt, 64); m.patch = c.take<uint32_t>(nt, 64); m.state = c.take<uint32_t>(nt, 64); m.size = c.take<uint32_t>(nt, 64);
         m.ones = c.take<uint32_t>(nt, 64); m.positive = c.take<uint32_t>(nt, 64); m.negative = c.take<uint32_t>(nt, 64); m.volume = c.take<long long>(nt, 64);
         m.open = c.take<uint8_t>(nt, 64); m.flip0 = c.take<uint8_t>(nt, 64); m.invert = c.take<uint8_t>(nt, 64);
         tile_sums = c.take<uint32_t>(tiles, 16);
         sort_temp = c.take<uint8_t>(sort_bytes, 256);
       }))) return rc;
  s.vertices = vertex_count; s.triangles = triangle_count; s.slots = (uint32_t)E; s.bits = vertex_id_bits(V); s.indices = indices;
  m.vertices = vertex_count; m.triangles = triangle_count; m.slots = (uint32_t)E; m.mode = mode;
  while ((T >> m.size_bits) != 0) ++m.size_bits;
  m.positions = positions; m.normals = mode == kOrientNormals ? normals : nullptr; m.indices = indices;
  m.sorted_slots = s.sorted_slots; m.head = s.head; m.rank = s.rank; m.start_of = s.start_of;
  m.out_indices = out_indices; m.flipped = flipped; m.patch_of_triangle = patch_of_triangle;
  m.words = s.words; m.counts = s.words + kRepairWords;
  const dim3 block(256);
  if ((rc = repair_clear_words(s.words, stream))) return rc;
  BSLAM_HIP_TRY(hipMemsetAsync(m.counts, 0, kOrientWords * sizeof(uint32_t), stream));
  BSLAM_HIP_TRY(hipMemsetAsync(m.counts + kOrientMin, 0xff, 3 * sizeof(uint32_t), stream));
  BSLAM_HIP_TRY(hipMemsetAsync(s.referenced, 0, V, stream));
  // stage 0: the position check of bslam_clean_mesh, the bounds of mode 2, the edge keys
  if ((rc = timer.begin(0))) return rc;
  hipLaunchKernelGGL(repair_vertex_kernel, flat_grid(V), block, 0, stream, vertex_count, positions, 0, (unsigned long long*)nullptr, (unsigned long long*)nullptr,
                     (uint32_t*)nullptr, (uint32_t*)nullptr, s.words);
  BSLAM_HIP_TRY(hipGetLastError());
  if (mode == kOrientVolume && T != 0) {
    hipLaunchKernelGGL(orient_bounds_kernel, flat_grid(V), block, 0, stream, vertex_count, positions, m.counts);
    BSLAM_HIP_TRY(hipGetLastError());
  }
  if (T != 0) {
    hipLaunchKernelGGL(topology_keys_kernel, flat_grid(T), block, 0, stream, s);
    BSLAM_HIP_TRY(hipGetLastError());
  }
  if ((rc = timer.end(0))) return rc;
  // nothing is decoded from the key of a triangle that must not be looked at, and no output is written for a mesh that is refused
  const uint32_t* host = nullptr;
  if ((rc = read_back(ctx, stream, (const uint32_t*)s.words, 1, &host))) return rc;
  if ((rc = repair_error(host[kRepairError], call))) return rc;
  if (T == 0) {
    if ((rc = timer.collect())) return rc;
    std::memset(report, 0, sizeof(*report));
    return BSLAM_OK;
  }
  // stage 1: the stable sort of (edge, slot)
  if ((rc = timer.begin(1))) return rc;
  if ((rc = mesh_sort(call, sort_temp, sort_bytes, s.keys, s.sorted_keys, s.ids, s.sorted_slots, E, 2 * s.bits, stream))) return rc;
  if ((rc = timer.end(1))) return rc;
  // stage 2: the runs
  if ((rc = timer.begin(2))) return rc;
  hipLaunchKernelGGL(repair_heads_kernel, flat_grid(E), block, 0, stream, s.slots, (const unsigned long long*)s.sorted_keys, (const uint32_t*)s.sorted_slots,
                     (const unsigned long long*)nullptr, s.head);
  BSLAM_HIP_TRY(hipGetLastError());
  if ((rc = device_scan(stream, 0, s.head, s.slots, false, s.rank, tile_sums, s.words + kRepairEdges))) return rc;
  hipLaunchKernelGGL(topology_starts_kernel, flat_grid(E), block, 0, stream, s);
  BSLAM_HIP_TRY(hipGetLastError());
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
  if ((rc = read_back(ctx, stream, (const uint32_t*)s.words, (size_t)kRepairWords + kOrientWords, &host))) return rc;
  if ((rc = timer.collect())) return rc;
  if ((rc = repair_error(host[kRepairError], call))) return rc;
  orient_report(host + kRepairWords, report);
  return BSLAM_OK;
}

}  // extern "C"
