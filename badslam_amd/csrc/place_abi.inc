// place_abi.inc -- place recognition entry points of include/badslam_hip.h (included by badslam_hip.hip).

namespace bslam {

// The 256 BRIEF point pairs (ax, ay, bx, by), each coordinate in -13 ... 13, from a linear congruential generator:
// s starts at 0x0BAD51A4, a draw is s = s * 1664525 + 1013904223 (mod 2^32) -> ((s >> 16) % 27) - 13, four draws per
// pair in the order ax, ay, bx, by, and a pair with a == b is drawn again.
static void make_place_pattern(int8_t (*pairs)[4]) {
  uint32_t s = 0x0BAD51A4u;
  for (int i = 0; i < 256;) {
    int8_t v[4];
    for (int j = 0; j < 4; ++j) {
      s = s * 1664525u + 1013904223u;
      v[j] = (int8_t)((int)((s >> 16) % 27u) - 13);
    }
    if (v[0] == v[2] && v[1] == v[3]) continue;
    for (int j = 0; j < 4; ++j) pairs[i][j] = v[j];
    ++i;
  }
}

static bool bytes_overlap(const void* a, size_t a_bytes, const void* b, size_t b_bytes) {
  const uintptr_t a0 = (uintptr_t)a, b0 = (uintptr_t)b;
  return a0 < b0 + b_bytes && b0 < a0 + a_bytes;
}
static size_t image_bytes(const Img& i) { return (size_t)i.height * i.pitch; }

}  // namespace bslam

extern "C" {

int bslam_place_pattern(int8_t* pairs) {
  if (!pairs) return fail(BSLAM_ERR_INVALID_ARGUMENT, "null argument");
  make_place_pattern((int8_t(*)[4])pairs);
  return BSLAM_OK;
}

int bslam_extract_keyframe_features(bslam_context* ctx, void* stream_, const bslam_buffer2d* color_buffer, const bslam_buffer2d* depth_buffer,
                                    int64_t score_threshold, uint32_t* out_xy, uint32_t* out_desc) {
  hipStream_t stream = (hipStream_t)stream_;
  if (!ctx || !out_xy || !out_desc) return fail(BSLAM_ERR_INVALID_ARGUMENT, "null argument");
  Img color, depth;
  int rc = make_img(color_buffer, 4, "colour", &color);
  if (rc) return rc;
  if ((rc = make_img(depth_buffer, 2, "depth", &depth))) return rc;
  if (!same_shape(color, depth)) return fail(BSLAM_ERR_INVALID_ARGUMENT, "colour and depth image differ in size");
  if (color.width > 65535 || color.height > 65535) return fail(BSLAM_ERR_INVALID_ARGUMENT, "the image must be at most 65535 pixels wide and high");
  if (!rows_aligned(color, 4)) return fail(BSLAM_ERR_INVALID_ARGUMENT, "colour rows must be 4 byte aligned");
  if (!rows_aligned(depth, 2)) return fail(BSLAM_ERR_INVALID_ARGUMENT, "depth rows must be 2 byte aligned");
  if (((uintptr_t)out_xy | (uintptr_t)out_desc) % 4) return fail(BSLAM_ERR_INVALID_ARGUMENT, "out_xy and out_desc must be 4 byte aligned");
  const int cells_x = color.width / kPlaceCell, cells_y = color.height / kPlaceCell;
  const size_t cells = (size_t)cells_x * cells_y, xy_bytes = cells * sizeof(uint32_t), desc_bytes = cells * kPlaceDescWords * sizeof(uint32_t);
  if (bytes_overlap(out_xy, xy_bytes, out_desc, desc_bytes)) return fail(BSLAM_ERR_INVALID_ARGUMENT, "out_xy and out_desc overlap");
  for (const Img* in : {&color, &depth})
    if (bytes_overlap(out_xy, xy_bytes, in->base, image_bytes(*in)) || bytes_overlap(out_desc, desc_bytes, in->base, image_bytes(*in)))
      return fail(BSLAM_ERR_INVALID_ARGUMENT, "an output overlaps an input image");
  if (cells == 0) return BSLAM_OK;
  BSLAM_HIP_TRY(hipSetDevice(ctx->device));
  if (!ctx->place_pattern_ready) {
    int8_t pairs[256][4];
    make_place_pattern(pairs);
    uint32_t words[256];
    for (int i = 0; i < 256; ++i)
      words[i] = (uint32_t)(pairs[i][0] + 13) | ((uint32_t)(pairs[i][1] + 13) << 8) | ((uint32_t)(pairs[i][2] + 13) << 16) | ((uint32_t)(pairs[i][3] + 13) << 24);
    if ((rc = ctx->place_pattern.reserve(sizeof(words)))) return rc;
    BSLAM_HIP_TRY(hipMemcpy(ctx->place_pattern.ptr, words, sizeof(words), hipMemcpyHostToDevice));   // synchronous: `words` is on the stack
    ctx->place_pattern_ready = true;
  }
  hipLaunchKernelGGL(extract_features_kernel, dim3((unsigned)cells), dim3(256), 0, stream, color, depth, (long long)score_threshold, cells_x,
                     (const uint32_t*)ctx->place_pattern.ptr, out_xy, out_desc);
  BSLAM_HIP_TRY(hipGetLastError());
  return BSLAM_OK;
}

int bslam_match_features(bslam_context* ctx, void* stream_, const uint32_t* query_xy, const uint32_t* query_desc, int cells, const uint32_t* database,
                         int n_db, int max_distance, int32_t* out_match, uint32_t* out_count) {
  hipStream_t stream = (hipStream_t)stream_;
  if (!ctx || !query_xy || !query_desc) return fail(BSLAM_ERR_INVALID_ARGUMENT, "null argument");
  if (cells <= 0 || cells > (1 << 24)) return fail(BSLAM_ERR_INVALID_ARGUMENT, "cells must lie in 1 ... 2^24");
  if (n_db < 0 || n_db > 65535) return fail(BSLAM_ERR_INVALID_ARGUMENT, "n_db must lie in 0 ... 65535");
  if (max_distance < 0 || max_distance > 256) return fail(BSLAM_ERR_INVALID_ARGUMENT, "max_distance must lie in 0 ... 256");
  if (((uintptr_t)query_xy | (uintptr_t)query_desc) % 4) return fail(BSLAM_ERR_INVALID_ARGUMENT, "query_xy and query_desc must be 4 byte aligned");
  if (n_db == 0) return BSLAM_OK;
  if (!database || !out_match || !out_count) return fail(BSLAM_ERR_INVALID_ARGUMENT, "null argument");
  if (((uintptr_t)database | (uintptr_t)out_match | (uintptr_t)out_count) % 4) return fail(BSLAM_ERR_INVALID_ARGUMENT, "database, out_match and out_count must be 4 byte aligned");
  const size_t xy_bytes = (size_t)cells * 4, desc_bytes = xy_bytes * kPlaceDescWords, db_bytes = (size_t)n_db * kPlaceRecordWords * xy_bytes,
               match_bytes = (size_t)n_db * xy_bytes, count_bytes = (size_t)n_db * 4;
  if (bytes_overlap(out_match, match_bytes, out_count, count_bytes)) return fail(BSLAM_ERR_INVALID_ARGUMENT, "out_match and out_count overlap");
  const void* outs[2] = {out_match, out_count};
  const size_t out_bytes[2] = {match_bytes, count_bytes};
  for (int o = 0; o < 2; ++o)
    if (bytes_overlap(outs[o], out_bytes[o], query_xy, xy_bytes) || bytes_overlap(outs[o], out_bytes[o], query_desc, desc_bytes) ||
        bytes_overlap(outs[o], out_bytes[o], database, db_bytes))
      return fail(BSLAM_ERR_INVALID_ARGUMENT, "an output overlaps the query or the database");
  BSLAM_HIP_TRY(hipSetDevice(ctx->device));
  BSLAM_HIP_TRY(hipMemsetAsync(out_count, 0, count_bytes, stream));
  hipLaunchKernelGGL(match_features_kernel, dim3((unsigned)((cells + 255) / 256), (unsigned)n_db), dim3(256), 0, stream, query_xy, query_desc, cells, database,
                     max_distance, (int*)out_match, out_count);
  BSLAM_HIP_TRY(hipGetLastError());
  return BSLAM_OK;
}

}  // extern "C"
