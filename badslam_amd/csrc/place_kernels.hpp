// place_kernels.hpp -- place recognition for gfx950: one Harris corner with an unoriented BRIEF descriptor per 16 x 16
// cell of a keyframe, and brute-force Hamming matching of one keyframe's features against a database of keyframes with
// a ratio test.  Stands in for the reference's FAST + BRIEF + DBoW2 front half of vis::LoopDetector::AddImage
// (BS/loop_detector.cc:98-127, 160-167).  All arithmetic is integer, so a NumPy restatement reproduces every output
// bit for bit, whatever the order in which blocks run.
#pragma once

#include "preprocess_kernels.hpp"

namespace bslam {

constexpr int kPlaceCell = 16;            // cell edge in pixels; also the border in which no pixel is eligible
constexpr int kPlaceTile = kPlaceCell + 6;   // intensity tile: the cell with a halo of 3 (window 2 + Sobel 1)
constexpr int kPlaceGrad = kPlaceCell + 4;   // gradient tile: the cell with a halo of 2
constexpr int kPlacePatch = 31;           // descriptor patch: point offsets up to 13 + box radius 2 on either side
constexpr int kPlaceDescWords = 8;
constexpr int kPlaceRecordWords = 1 + kPlaceDescWords;
constexpr uint32_t kPlaceEmpty = 0xFFFFFFFFu;
constexpr int kPlaceNoSecond = 257;       // one more than the largest Hamming distance
constexpr int kPlaceSkipped = 1000;       // distance an empty database slot is given: above every best and second
constexpr int kMatchChunk = 256;          // database entries staged in LDS at a time: 256 * 36 B = 9 KiB per block

// The BRIEF point pairs are generated on the host (place_abi.inc) and uploaded once per context: byte 0 ... 3 of word i
// are ax, ay, bx, by of pair i, each offset + 13.

struct CornerKey { long long score; int index; };   // index < 0: no eligible pixel
__device__ __forceinline__ bool corner_better(const CornerKey& a, const CornerKey& b) {
  if (a.index < 0) return false;
  if (b.index < 0) return true;
  return a.score > b.score || (a.score == b.score && a.index < b.index);
}

// One block per cell, one thread per pixel of it.
//   L(y, x)   = byte 3 of the colour image, coordinates clamped to the image
//   gx(y, x)  = (L(y-1, x+1) + 2 L(y, x+1) + L(y+1, x+1)) - (the same at x-1);  gy alike with rows
//   A, B, C   = sums of gx^2, gy^2, gx gy over the 5 x 5 window around the pixel (int32: 25 * 1020^2 < 2^31)
//   score     = 16 (A B - C C) - (A + B)^2 in int64
//   eligible  iff 16 <= x < w - 16, 16 <= y < h - 16, depth != 0 and bit 15 of it clear, score > score_threshold
//   feature   = the eligible pixel of highest score; among equal scores the lowest y, then the lowest x
//   S(y, x)   = 5 x 5 box sum of L;  bit i of the descriptor = S(y + ay_i, x + ax_i) < S(y + by_i, x + bx_i)
// An eligible pixel lies 16 pixels inside the image, so neither its window nor its descriptor patch is ever clamped.
__global__ __launch_bounds__(256) void extract_features_kernel(Img color, Img depth, long long score_threshold, int cells_x, const uint32_t* __restrict__ pattern,
                                                               uint32_t* __restrict__ out_xy, uint32_t* __restrict__ out_desc) {
  __shared__ uint8_t tile[kPlaceTile * kPlaceTile];
  __shared__ int grad[kPlaceGrad * kPlaceGrad];   // gx in the low half, gy in the high half, both as int16
  __shared__ uint8_t patch[kPlacePatch * kPlacePatch];
  __shared__ CornerKey wave_best[4];
  const int tid = (int)threadIdx.x, cell = (int)blockIdx.x;
  const int x0 = (cell % cells_x) * kPlaceCell, y0 = (cell / cells_x) * kPlaceCell;
  for (int i = tid; i < kPlaceTile * kPlaceTile; i += 256) {
    const int ty = i / kPlaceTile, tx = i - ty * kPlaceTile;
    const int y = min(max(y0 + ty - 3, 0), color.height - 1), x = min(max(x0 + tx - 3, 0), color.width - 1);
    tile[i] = (uint8_t)(color.at<uint32_t>(y, x) >> 24);
  }
  __syncthreads();
  for (int i = tid; i < kPlaceGrad * kPlaceGrad; i += 256) {
    const int gy_ = i / kPlaceGrad, gx_ = i - gy_ * kPlaceGrad;
    const uint8_t* t = tile + (gy_ + 1) * kPlaceTile + (gx_ + 1);   // the tile entry of this gradient position
    const int gx = ((int)t[-kPlaceTile + 1] + 2 * (int)t[1] + (int)t[kPlaceTile + 1]) - ((int)t[-kPlaceTile - 1] + 2 * (int)t[-1] + (int)t[kPlaceTile - 1]);
    const int gy = ((int)t[kPlaceTile - 1] + 2 * (int)t[kPlaceTile] + (int)t[kPlaceTile + 1]) - ((int)t[-kPlaceTile - 1] + 2 * (int)t[-kPlaceTile] + (int)t[-kPlaceTile + 1]);
    grad[i] = (gx & 0xffff) | (int)((uint32_t)gy << 16);
  }
  __syncthreads();
  const int ly = tid >> 4, lx = tid & 15, x = x0 + lx, y = y0 + ly;
  CornerKey mine;
  mine.score = 0;
  mine.index = -1;
  if (x >= kPlaceCell && x < color.width - kPlaceCell && y >= kPlaceCell && y < color.height - kPlaceCell) {
    const uint32_t d = depth.at<uint16_t>(y, x);
    int A = 0, B = 0, Cs = 0;
#pragma unroll
    for (int dy = 0; dy < 5; ++dy)
#pragma unroll
      for (int dx = 0; dx < 5; ++dx) {
        const int g = grad[(ly + dy) * kPlaceGrad + lx + dx];
        const int gx = (int)(short)(g & 0xffff), gy = g >> 16;
        A += gx * gx; B += gy * gy; Cs += gx * gy;
      }
    const long long score = 16ll * ((long long)A * B - (long long)Cs * Cs) - ((long long)A + B) * ((long long)A + B);
    if (d != 0u && !(d & 0x8000u) && score > score_threshold) { mine.score = score; mine.index = tid; }
  }
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) {
    CornerKey other;
    other.score = __shfl_down(mine.score, off, 64);
    other.index = __shfl_down(mine.index, off, 64);
    if (corner_better(other, mine)) mine = other;
  }
  if ((tid & 63) == 0) wave_best[tid >> 6] = mine;
  __syncthreads();
  CornerKey best = wave_best[0];
#pragma unroll
  for (int wv = 1; wv < 4; ++wv)
    if (corner_better(wave_best[wv], best)) best = wave_best[wv];
  if (best.index < 0) {   // block-uniform
    if (tid == 0) out_xy[cell] = kPlaceEmpty;
    if (tid < kPlaceDescWords) out_desc[(size_t)cell * kPlaceDescWords + tid] = 0u;
    return;
  }
  const int fx = x0 + (best.index & 15), fy = y0 + (best.index >> 4);
  for (int i = tid; i < kPlacePatch * kPlacePatch; i += 256) {
    const int py = i / kPlacePatch, px = i - py * kPlacePatch;
    patch[i] = (uint8_t)(color.at<uint32_t>(fy + py - 15, fx + px - 15) >> 24);
  }
  __syncthreads();
  const uint32_t pr = pattern[tid];
  int sum[2];
#pragma unroll
  for (int p = 0; p < 2; ++p) {
    const int ox = (int)((pr >> (16 * p)) & 0xffu), oy = (int)((pr >> (16 * p + 8)) & 0xffu);   // offset + 13 = patch column / row of the box's corner
    int s = 0;
#pragma unroll
    for (int dy = 0; dy < 5; ++dy)
#pragma unroll
      for (int dx = 0; dx < 5; ++dx) s += (int)patch[(oy + dy) * kPlacePatch + ox + dx];
    sum[p] = s;
  }
  const unsigned long long bits = __ballot(sum[0] < sum[1]);   // lane l of wave v holds bit 64 v + l
  if ((tid & 63) == 0) {
    uint32_t* o = out_desc + (size_t)cell * kPlaceDescWords + 2 * (tid >> 6);
    o[0] = (uint32_t)bits;
    o[1] = (uint32_t)(bits >> 32);
  }
  if (tid == 0) out_xy[cell] = (uint32_t)fx | ((uint32_t)fy << 16);
}

// One block per (256 query slots, database keyframe); a thread holds its query descriptor in registers and walks the
// database keyframe's records, staged in LDS kMatchChunk at a time (every lane reads the same entry: a broadcast).
//   database keyframe k = words [k * 9 * cells, (k + 1) * 9 * cells): xy[cells], then desc[cells][8]
//   best    = smallest Hamming distance over k's non-empty slots, the lowest slot among equals
//   second  = smallest over the remaining slots (a duplicate of the best gives second == best); 257 if there is none
//   accepted iff the query slot is non-empty, k has a feature, best <= max_distance and 4 best < 3 second
// out_count[k] must be zero at launch; every wave adds its accepted matches with one integer atomic.
__global__ __launch_bounds__(256) void match_features_kernel(const uint32_t* __restrict__ query_xy, const uint32_t* __restrict__ query_desc, int cells,
                                                             const uint32_t* __restrict__ database, int max_distance, int* __restrict__ out_match,
                                                             uint32_t* __restrict__ out_count) {
  __shared__ uint32_t lds_xy[kMatchChunk];
  __shared__ __attribute__((aligned(16))) uint32_t lds_desc[kMatchChunk * kPlaceDescWords];
  const int tid = (int)threadIdx.x, q = (int)blockIdx.x * 256 + tid, k = (int)blockIdx.y;
  const uint32_t* db_xy = database + (size_t)k * kPlaceRecordWords * cells;
  const uint32_t* db_desc = db_xy + cells;   // only 4-byte aligned for a general `cells`: staged word by word
  const bool live = q < cells && query_xy[q] != kPlaceEmpty;
  uint4 qa = make_uint4(0u, 0u, 0u, 0u), qb = qa;
  if (live) {
    const uint32_t* qd = query_desc + (size_t)q * kPlaceDescWords;
    qa = make_uint4(qd[0], qd[1], qd[2], qd[3]);
    qb = make_uint4(qd[4], qd[5], qd[6], qd[7]);
  }
  int best = kPlaceNoSecond, second = kPlaceNoSecond, best_slot = -1;
  for (int c0 = 0; c0 < cells; c0 += kMatchChunk) {
    const int n = min(kMatchChunk, cells - c0);
    __syncthreads();   // the previous chunk has been read
    if (tid < n) lds_xy[tid] = db_xy[c0 + tid];
    for (int i = tid; i < kPlaceDescWords * n; i += 256) lds_desc[i] = db_desc[(size_t)kPlaceDescWords * c0 + i];
    __syncthreads();
    // an empty slot takes part with a distance no update accepts: no branch in the loop, so that the reads and the
    // popcounts of the unrolled entries overlap
#pragma unroll 4
    for (int e = 0; e < n; ++e) {
      const uint4 da = ((const uint4*)lds_desc)[2 * e], db = ((const uint4*)lds_desc)[2 * e + 1];
      int d = __popc(qa.x ^ da.x) + __popc(qa.y ^ da.y) + __popc(qa.z ^ da.z) + __popc(qa.w ^ da.w) + __popc(qb.x ^ db.x) + __popc(qb.y ^ db.y) +
              __popc(qb.z ^ db.z) + __popc(qb.w ^ db.w);
      if (lds_xy[e] == kPlaceEmpty) d = kPlaceSkipped;
      if (d < best) { second = best; best = d; best_slot = c0 + e; }
      else if (d < second) second = d;
    }
  }
  const bool accepted = live && best_slot >= 0 && best <= max_distance && 4 * best < 3 * second;
  if (q < cells) out_match[(size_t)k * cells + q] = accepted ? best_slot : -1;
  const unsigned long long votes = __ballot(accepted);
  if ((tid & 63) == 0 && votes) atomicAdd(out_count + k, (uint32_t)__popcll(votes));
}

}  // namespace bslam
