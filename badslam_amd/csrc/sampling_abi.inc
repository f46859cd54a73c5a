// sampling_abi.inc -- bslam_sample_mesh of include/badslam_hip.h (included by badslam_hip.hip after distance_abi.inc:
// check_mesh_spans, mesh_error, empty_mesh, device_scan).

extern "C" {

int bslam_sample_mesh(bslam_context* ctx, void* stream_, uint32_t vertex_count, const float* positions, uint32_t triangle_count, const uint32_t* indices,
                      float density, uint32_t seed, uint64_t capacity, float* out_points, float* out_normals, uint32_t* out_triangles, uint64_t* sample_count) {
  hipStream_t stream = (hipStream_t)stream_;
  const char* call = "bslam_sample_mesh";
  if (!ctx) return fail(BSLAM_ERR_INVALID_ARGUMENT, "context is null");
  if (!sample_count) return fail(BSLAM_ERR_INVALID_ARGUMENT, "sample_count is null");
  if (!finite_positive(density)) return fail(BSLAM_ERR_INVALID_ARGUMENT, "density must be finite and > 0");
  const size_t V = vertex_count, T = triangle_count;
  // one thread per triangle / per sample in blocks of 256: the rounded-up thread index has to fit 32 bits
  if (T > 0xffffff00ull) return fail(BSLAM_ERR_INVALID_ARGUMENT, "more than 2^32 - 256 triangles");
  const size_t room = capacity > 0xffffff00ull ? 0xffffff00ull : (size_t)capacity;   // more is never written
  const MeshSpan spans[5] = {{positions, 12 * V, "positions", false}, {indices, 12 * T, "indices", false},
                             {out_points, out_points ? 12 * room : 0, "out_points", true}, {out_normals, out_normals ? 12 * room : 0, "out_normals", true},
                             {out_triangles, out_triangles ? 4 * room : 0, "out_triangles", true}};
  int rc = check_mesh_spans(spans, 5);
  if (rc) return rc;
  BSLAM_HIP_TRY(hipSetDevice(ctx->device));
  if (T == 0 || V == 0) {
    if ((rc = empty_mesh(stream, T, call))) return rc;   // V == 0: every index is beyond
    *sample_count = 0;
    return BSLAM_OK;
  }
  // scratch (u32 units; every piece 16 byte aligned): words | counts[T] | offset[T] | tile sums
  uint32_t *words, *counts, *offset, *tile_sums;
  if ((rc = carve(ctx->sampling, [&](Carver& c) {
         words = c.take<uint32_t>(kSmpWords, 16); counts = c.take<uint32_t>(T, 16); offset = c.take<uint32_t>(T, 16); tile_sums = c.take<uint32_t>(T / kScanTile + 2, 16);
       }))) return rc;
  const dim3 block(256);
  BSLAM_HIP_TRY(hipMemsetAsync(words, 0, kSmpWords * sizeof(uint32_t), stream));
  hipLaunchKernelGGL(sample_count_kernel, flat_grid(T), block, 0, stream, vertex_count, triangle_count, positions, indices, density, seed, counts, words);
  BSLAM_HIP_TRY(hipGetLastError());
  const uint32_t* host = nullptr;
  if ((rc = read_back(ctx, stream, (const uint32_t*)words, (size_t)kSmpWords, &host))) return rc;
  if ((rc = mesh_error(host[kSmpError], call))) return rc;
  uint64_t N;
  std::memcpy(&N, host + kSmpTotal, sizeof(N));
  *sample_count = N;
  if (N > 0xffffff00ull)
    return fail(BSLAM_ERR_INVALID_ARGUMENT, "%s: %llu samples are more than 2^32 - 256: use a lower density", call, (unsigned long long)N);
  if (!out_points || N > capacity || N == 0) return BSLAM_OK;   // the counts alone; the read-back has waited for the stream
  // the total is below 2^32, so the 32-bit scan is exact
  if ((rc = device_scan(stream, 1, counts, triangle_count, true, offset, tile_sums, words + kSmpScanTotal))) return rc;
  int steps = 0;
  while ((1ull << steps) < T + 1) ++steps;   // ceil(log2(T + 1)): the cap of every search
  hipLaunchKernelGGL(sample_emit_kernel, flat_grid((size_t)N), block, 0, stream, triangle_count, (uint32_t)N, steps, seed, positions, indices,
                     (const uint32_t*)offset, out_points, out_normals, out_triangles);
  BSLAM_HIP_TRY(hipGetLastError());
  BSLAM_HIP_TRY(hipStreamSynchronize(stream));
  return BSLAM_OK;
}

}  // extern "C"
