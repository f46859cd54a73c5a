// raycast_kernels.hpp -- views of the fused TSDF volume for gfx950: one ray per pixel marches through the volume of
// bslam_fuse_keyframes and reports the first front-facing zero crossing as depth, normal and colour.  Next to the disc view of
// render_kernels.hpp this one has no holes where surfels are sparse; next to the mesh of fusion_kernels.hpp it needs no outside
// renderer.  Like both: all arithmetic is fp32 (the clip of the walked range: fp64, see below), nothing is contracted, / and
// sqrtf are correctly rounded, fused multiply-adds are written as fmaf, and the expression order is written out so that a NumPy
// float32 restatement reproduces depth and colour bit for bit.
#pragma once

#include "fusion_kernels.hpp"

namespace bslam {

// ---------------------------------------------------------------------------------------------
// The rule.  G = global_T_camera (3 x 4), camera fx, fy, cx, cy (pixel-corner), inv_voxel = fl(1 / voxel) from the host.
//   pixel (i, j):   dx = ((float(i) + 0.5f) - cx) / fx;  dy alike                           (the render rule's expressions)
//   sample k:       t  = fmaf(float(k), step, min_depth),  k = 0 .. N - 1 with N the number of k whose t <= max_depth
//                   P.a = fmaf(G[a][2], t, fmaf(G[a][1], dy * t, fmaf(G[a][0], dx * t, G[a][3])))
//                   g.a = (P.a - origin.a) * inv_voxel - 0.5f;   c.a = floorf(g.a);   f.a = g.a - c.a
//   in range  iff   g.a >= 0 and c.a <= float(n.a - 2) on all three axes (float comparisons; NaN is out of range)
//   cell (c) valid  iff its 8 corner samples have count >= min_count (the extraction rule's "observed"); a sample is valid iff
//                   it is in range and its cell is valid
//   value           D[dz][dy][dx] the cell's corner samples, lerp(a, b, w) = fmaf(w, b - a, a):
//                   e00 = lerp(D000, D001, f.x), e10 = lerp(D010, D011, f.x), e01 = lerp(D100, D101, f.x), e11 = lerp(D110, D111, f.x)
//                   y0 = lerp(e00, e10, f.y), y1 = lerp(e01, e11, f.y);  F = lerp(y0, y1, f.z)
//   The ray ends at the first k whose sample is valid with F_k < 0.  It is a hit iff k >= 1, sample k - 1 is valid and
//   F_{k-1} >= 0; then t* = t_{k-1} + step * (F_{k-1} / (F_{k-1} - F_k)).  Everything else is empty: a surface seen from behind,
//   entered from unobserved space or beginning inside, and a ray that reaches N.
// Outputs at a hit (empty: all 0), each optional:
//   depth   u16:     v = metres_to_depth * t* + 0.5f;  v < 65536 ? u16(v) : 0
//   The cell of the other two: that of P(t*) (the sample expressions with t* in place of t) if it is valid, else that of
//   sample k, each with its own fractions f.
//   normal  3 x f32: the gradient of the interpolant there, from the face lerps
//                    gx = lerp(lerp(D001, D011, f.y), lerp(D101, D111, f.y), f.z) - lerp(lerp(D000, D010, f.y), lerp(D100, D110, f.y), f.z)
//                    gy = lerp(e10, e11, f.z) - lerp(e00, e01, f.z);   gz = y1 - y0        (towards free space)
//                    rotated into the camera frame, n.a = (G[0][a] * gx + G[1][a] * gy) + G[2][a] * gz, and divided by
//                    sqrtf((n.x * n.x + n.y * n.y) + n.z * n.z); 0 where that root is 0
//   colour  uchar4:  over the corners 0 .. 7 (dx = corner & 1, dy = corner >> 1 & 1, dz = corner >> 2) whose colour sample has
//                    alpha 255, with w = (wx * wy) * wz and wx = dx ? f.x : 1.0f - f.x (alike):  W += w;  S.ch += w * float(ch);
//                    then {u8(S.ch / W + 0.5f) per channel, 255} if W > 0, else 0; 0 without a colour volume.
//
// Skipping.  lerp(a, b, w) with a, b not < 0 and 0 <= w < 1 is not < 0: b - a rounds to a value >= -a (rounding is monotone and
// -a is a float), so a + w (b - a) >= a (1 - w) >= 0 before the fma's single rounding, which keeps the sign.  By induction over
// the seven lerps a cell none of whose corners is < 0 cannot give F < 0 (f.a lies in [0, 1) for every in-range sample: g.a >= 0
// makes g.a - floorf(g.a) exact).  So a sample whose cell lies in a block of 8 x 8 x 8 cells that holds no valid cell with a
// corner < 0 can never end a ray, and the march passes it after one flag test.  Sample k - 1 of an ending ray is evaluated by the
// rule, whatever was skipped.  bslam_set_culling switches the flag test; the outputs are the same bits either way.
// ---------------------------------------------------------------------------------------------

constexpr int kRayBlockShift = 3;        // a flag per block of 8 x 8 x 8 cells
constexpr int kRayMaxSamples = 65536;    // per ray

// The prepared volume: what the march reads besides the tsdf samples.  Cells are (nx - 1) x (ny - 1) x (nz - 1).
//   bits   one validity bit per cell, 64-bit words along x: word (z * (ny - 1) + y) * words_x + (x >> 6), bit x & 63
//   flags  one bit per block: byte (bz * blocks_y + by) * groups_x + (bx >> 3), bit bx & 7  (a byte = 64 cells along x = one word,
//          so groups_x = words_x)
struct RayAux {
  const uint8_t* flags;
  const uint32_t* bits;    // the 64-bit words as pairs of 32-bit words (little endian)
  uint32_t words_x, groups_x, blocks_y;
};

// One workgroup per 64 x 8 x 8 cells (8 blocks along x): a wave takes the rows (y, z) of 64 cells one after the other, writes
// each row's ballot as its validity word and collects the ballots of "valid with a corner < 0"; byte b of those is block b.
__global__ __launch_bounds__(256) void raycast_prepare_kernel(VolumeDev vol, Img tsdf, Img count, uint32_t min_count, uint32_t words_x, uint32_t groups_y,
                                                              unsigned long long* __restrict__ bits, uint8_t* __restrict__ flags) {
  __shared__ uint32_t wave_flags[4];
  const uint32_t group = blockIdx.x;
  const uint32_t gz = group / (words_x * groups_y), rest = group - gz * (words_x * groups_y);
  const uint32_t gy = rest / words_x, gx = rest - gy * words_x;
  const int lane = (int)(threadIdx.x & 63u), wave = (int)(threadIdx.x >> 6);
  const int x = (int)gx * 64 + lane;
  const int cells_x = vol.nx - 1, cells_y = vol.ny - 1, cells_z = vol.nz - 1;
  unsigned long long negative = 0;
  for (int r = wave; r < 64; r += 4) {
    const int y = (int)gy * 8 + (r & 7), z = (int)gz * 8 + (r >> 3);
    if (y >= cells_y || z >= cells_z) continue;   // wave-uniform
    bool valid = x < cells_x, inside = false;
    if (valid) {
#pragma unroll
      for (int corner = 0; corner < 8; ++corner) {
        const int row = (z + (corner >> 2)) * vol.ny + y + ((corner >> 1) & 1), sx = x + (corner & 1);
        valid &= count.at<uint32_t>(row, sx) >= min_count;
        inside |= tsdf.at<float>(row, sx) < 0.0f;
      }
    }
    const unsigned long long word = __ballot(valid);
    negative |= __ballot(valid && inside);
    if (lane == 0) bits[((size_t)z * (size_t)cells_y + (size_t)y) * words_x + gx] = word;
  }
  uint32_t mine = 0;
#pragma unroll
  for (int b = 0; b < 8; ++b) mine |= ((negative >> (8 * b)) & 0xffull) ? (1u << b) : 0u;
  if (lane == 0) wave_flags[wave] = mine;
  __syncthreads();
  if (threadIdx.x == 0) flags[group] = (uint8_t)(wave_flags[0] | wave_flags[1] | wave_flags[2] | wave_flags[3]);   // group = (gz * groups_y + gy) * words_x + gx
}

struct RayCam { float fx, fy, cx, cy; int width, height; };
struct RayParams {
  float min_depth, step, metres_to_depth, inv_voxel;
  int samples;            // N
  int widen;              // samples added on each side of the clipped range (see raycast_clip)
  float fnx, fny, fnz;    // float(n.a - 2)
};

struct RaySample { float fx, fy, fz; int cx, cy, cz; bool in_range; };

__device__ __forceinline__ float ray_lerp(float a, float b, float w) { return fmaf(w, b - a, a); }

__device__ __forceinline__ RaySample ray_sample(const bslam_mat3x4& G, const VolumeDev& vol, const RayParams& p, float dx, float dy, float t) {
  const float a = dx * t, b = dy * t;
  const float Px = fmaf(G.m[2], t, fmaf(G.m[1], b, fmaf(G.m[0], a, G.m[3])));
  const float Py = fmaf(G.m[6], t, fmaf(G.m[5], b, fmaf(G.m[4], a, G.m[7])));
  const float Pz = fmaf(G.m[10], t, fmaf(G.m[9], b, fmaf(G.m[8], a, G.m[11])));
  const float gx = (Px - vol.ox) * p.inv_voxel - 0.5f, gy = (Py - vol.oy) * p.inv_voxel - 0.5f, gz = (Pz - vol.oz) * p.inv_voxel - 0.5f;
  const float cx = floorf(gx), cy = floorf(gy), cz = floorf(gz);
  RaySample s;
  s.in_range = gx >= 0.0f && gy >= 0.0f && gz >= 0.0f && cx <= p.fnx && cy <= p.fny && cz <= p.fnz;
  s.fx = gx - cx; s.fy = gy - cy; s.fz = gz - cz;
  s.cx = s.in_range ? (int)cx : 0; s.cy = s.in_range ? (int)cy : 0; s.cz = s.in_range ? (int)cz : 0;
  return s;
}

__device__ __forceinline__ bool ray_block_flagged(const RayAux& aux, const RaySample& s) {
  const uint32_t byte = ((uint32_t)(s.cz >> kRayBlockShift) * aux.blocks_y + (uint32_t)(s.cy >> kRayBlockShift)) * aux.groups_x + (uint32_t)(s.cx >> 6);
  return (aux.flags[byte] >> ((s.cx >> kRayBlockShift) & 7)) & 1u;
}
__device__ __forceinline__ bool ray_cell_valid(const RayAux& aux, const VolumeDev& vol, const RaySample& s) {
  const size_t word = ((size_t)s.cz * (size_t)(vol.ny - 1) + (size_t)s.cy) * aux.words_x + (size_t)(s.cx >> 6);
  return (aux.bits[2 * word + ((s.cx >> 5) & 1)] >> (s.cx & 31)) & 1u;
}
// D[corner], corner = dz * 4 + dy * 2 + dx
__device__ __forceinline__ void ray_corners(const VolumeDev& vol, const Img& tsdf, const RaySample& s, float D[8]) {
#pragma unroll
  for (int r = 0; r < 4; ++r) {
    const float* row = (const float*)(tsdf.base + (size_t)((s.cz + (r >> 1)) * vol.ny + s.cy + (r & 1)) * tsdf.pitch) + s.cx;
    D[2 * r] = row[0]; D[2 * r + 1] = row[1];
  }
}
__device__ __forceinline__ float ray_value(const float D[8], const RaySample& s) {
  const float e00 = ray_lerp(D[0], D[1], s.fx), e10 = ray_lerp(D[2], D[3], s.fx), e01 = ray_lerp(D[4], D[5], s.fx), e11 = ray_lerp(D[6], D[7], s.fx);
  return ray_lerp(ray_lerp(e00, e10, s.fy), ray_lerp(e01, e11, s.fy), s.fz);
}

// The range of k a ray has to walk.  Not part of the rule: any superset of the in-range samples gives the rule's result, and
// this one is a superset by the following argument (DESIGN.md 8 "Surface views" has it in full).  Let S.a = |G[a][3]| +
// t_max (|G[a][0] dx| + |G[a][1] dy| + |G[a][2]|) bound every partial result of P.a.  The two products and three fmas of P.a are
// five roundings, so P.a differs from the real-line point p.a(t) = G[a][3] + t (G[a][0] dx + G[a][1] dy + G[a][2]) by less than
// 2^-21 S.a.  g.a >= 0 implies P.a > origin.a (subtraction, product and the - 0.5f keep the sign), c.a <= n.a - 2 implies
// P.a - origin.a <= voxel (n.a + 0.5) (1 + 2^-21).  So p.a(t) of an in-range sample lies in [origin.a - m.a, origin.a + n.a voxel
// + m.a] with m.a = voxel + 2^-20 (S.a + |origin.a| + n.a voxel), a margin several times what is needed.  The slab test is
// done in fp64 on those fp32 values, whose own rounding (2^-53 relative) disappears in that margin.  It yields [t_in, t_out];
// t_k = (min_depth + k step)(1 + d), |d| <= 2^-24, so k lies within widen = ceil(2^-23 max_depth / step) + 2 samples of
// [(t_in - min_depth) / step, (t_out - min_depth) / step].  A NaN anywhere keeps the whole range.
__device__ __forceinline__ void raycast_clip(const bslam_mat3x4& G, const VolumeDev& vol, const RayParams& p, float dx, float dy, int* k0, int* k1) {
  const double t_max = fma((double)(p.samples - 1), (double)p.step, (double)p.min_depth);
  const double origin[3] = {vol.ox, vol.oy, vol.oz}, n[3] = {(double)vol.nx, (double)vol.ny, (double)vol.nz};
  double t_in = -1.0e300, t_out = 1.0e300;
  bool whole = false;
#pragma unroll
  for (int a = 0; a < 3; ++a) {
    const double g0 = G.m[4 * a], g1 = G.m[4 * a + 1], g2 = G.m[4 * a + 2], g3 = G.m[4 * a + 3];
    const double d = g0 * (double)dx + g1 * (double)dy + g2;
    const double S = fabs(g3) + t_max * (fabs(g0 * (double)dx) + fabs(g1 * (double)dy) + fabs(g2));
    const double extent = n[a] * (double)vol.voxel;
    const double m = (double)vol.voxel + 9.5367431640625e-07 * (S + fabs(origin[a]) + extent);
    const double lo = origin[a] - m, hi = origin[a] + extent + m;
    if (d == 0.0) {
      if (g3 < lo || g3 > hi) { t_in = 1.0e300; t_out = -1.0e300; }
    } else if (d == d) {
      const double ta = (lo - g3) / d, tb = (hi - g3) / d;
      t_in = fmax(t_in, fmin(ta, tb));
      t_out = fmin(t_out, fmax(ta, tb));
      whole |= ta != ta || tb != tb;
    } else {
      whole = true;
    }
  }
  const double last = (double)(p.samples - 1);
  double first_k = floor((t_in - (double)p.min_depth) / (double)p.step) - (double)p.widen;
  double last_k = ceil((t_out - (double)p.min_depth) / (double)p.step) + (double)p.widen;
  if (whole || first_k != first_k || last_k != last_k) { first_k = 0.0; last_k = last; }
  *k0 = (int)fmin(fmax(first_k, 0.0), last + 1.0);
  *k1 = (int)fmax(fmin(last_k, last), -1.0);
}

// One thread per pixel, a workgroup per 16 x 16 pixels, a wave per 8 x 8 tile of them.  stats: {in-range samples that reached
// the flag test, samples evaluated} of bslam_debug_cull_stats, or nullptr.
__global__ __launch_bounds__(256) void raycast_march_kernel(bslam_mat3x4 G, RayCam cam, VolumeDev vol, RayParams p, RayAux aux, int culling, uint32_t tiles_x, Img tsdf,
                                                            Img color_volume, Img out_depth, Img out_color, Img out_normal, unsigned long long* __restrict__ stats) {
  const uint32_t ty = blockIdx.x / tiles_x, tx = blockIdx.x - ty * tiles_x;
  const int lane = (int)(threadIdx.x & 63u), wave = (int)(threadIdx.x >> 6);
  const int i = (int)tx * 16 + (wave & 1) * 8 + (lane & 7), j = (int)ty * 16 + (wave >> 1) * 8 + (lane >> 3);
  const bool live = i < cam.width && j < cam.height;
  const float dx = (((float)i + 0.5f) - cam.cx) / cam.fx, dy = (((float)j + 0.5f) - cam.cy) / cam.fy;
  int k0 = 0, k1 = -1;
  if (live) raycast_clip(G, vol, p, dx, dy, &k0, &k1);

  uint32_t visited = 0, evaluated = 0;
  bool hit = false;
  float t_hit = 0.0f;
  RaySample cell;   // the cell of normal and colour
  cell.fx = cell.fy = cell.fz = 0.0f; cell.cx = cell.cy = cell.cz = 0; cell.in_range = false;
  for (int k = k0; k <= k1; ++k) {
    const RaySample s = ray_sample(G, vol, p, dx, dy, fmaf((float)k, p.step, p.min_depth));
    if (!s.in_range) continue;
    visited += 1;
    if (culling && !ray_block_flagged(aux, s)) continue;
    evaluated += 1;
    if (!ray_cell_valid(aux, vol, s)) continue;
    float D[8];
    ray_corners(vol, tsdf, s, D);
    const float F = ray_value(D, s);
    if (!(F < 0.0f)) continue;
    // the ray ends here; sample k - 1 by the rule
    if (k >= 1) {
      const float t_before = fmaf((float)(k - 1), p.step, p.min_depth);
      const RaySample b = ray_sample(G, vol, p, dx, dy, t_before);
      if (b.in_range && ray_cell_valid(aux, vol, b)) {
        float B[8];
        ray_corners(vol, tsdf, b, B);
        const float Fb = ray_value(B, b);
        if (Fb >= 0.0f) {
          hit = true;
          t_hit = t_before + p.step * (Fb / (Fb - F));
          const RaySample at = ray_sample(G, vol, p, dx, dy, t_hit);
          cell = (at.in_range && ray_cell_valid(aux, vol, at)) ? at : s;
        }
      }
    }
    break;
  }

  if (stats != nullptr) {   // wave-uniform; every lane of the wave is here
    unsigned long long a = visited, b = evaluated;
#pragma unroll
    for (int offset = 32; offset >= 1; offset >>= 1) { a += __shfl_xor(a, offset); b += __shfl_xor(b, offset); }
    if (lane == 0) { atomicAdd(&stats[0], a); atomicAdd(&stats[1], b); }
  }
  if (!live) return;

  if (out_depth.base) {
    uint16_t value = 0;
    if (hit) {
      const float v = p.metres_to_depth * t_hit + 0.5f;
      if (v < 65536.0f) value = (uint16_t)v;
    }
    out_depth.at<uint16_t>(j, i) = value;
  }
  if (!out_normal.base && !out_color.base) return;
  float D[8];
  if (hit && out_normal.base) ray_corners(vol, tsdf, cell, D);
  if (out_normal.base) {
    float nx = 0.0f, ny = 0.0f, nz = 0.0f;
    if (hit) {
      const float e00 = ray_lerp(D[0], D[1], cell.fx), e10 = ray_lerp(D[2], D[3], cell.fx), e01 = ray_lerp(D[4], D[5], cell.fx), e11 = ray_lerp(D[6], D[7], cell.fx);
      const float gx = ray_lerp(ray_lerp(D[1], D[3], cell.fy), ray_lerp(D[5], D[7], cell.fy), cell.fz) - ray_lerp(ray_lerp(D[0], D[2], cell.fy), ray_lerp(D[4], D[6], cell.fy), cell.fz);
      const float gy = ray_lerp(e10, e11, cell.fz) - ray_lerp(e00, e01, cell.fz);
      const float gz = ray_lerp(e01, e11, cell.fy) - ray_lerp(e00, e10, cell.fy);
      const float rx = (G.m[0] * gx + G.m[4] * gy) + G.m[8] * gz, ry = (G.m[1] * gx + G.m[5] * gy) + G.m[9] * gz, rz = (G.m[2] * gx + G.m[6] * gy) + G.m[10] * gz;
      const float len = sqrtf((rx * rx + ry * ry) + rz * rz);
      if (len != 0.0f) { nx = rx / len; ny = ry / len; nz = rz / len; }
    }
    float* o = (float*)(out_normal.base + (size_t)j * out_normal.pitch) + 3 * (size_t)i;
    o[0] = nx; o[1] = ny; o[2] = nz;
  }
  if (out_color.base) {
    uint32_t packed = 0;
    if (hit && color_volume.base) {
      float W = 0.0f, R = 0.0f, Gc = 0.0f, B = 0.0f;
#pragma unroll
      for (int corner = 0; corner < 8; ++corner) {
        const uint32_t rgba = color_volume.at<uint32_t>((cell.cz + (corner >> 2)) * vol.ny + cell.cy + ((corner >> 1) & 1), cell.cx + (corner & 1));
        const float wx = (corner & 1) ? cell.fx : 1.0f - cell.fx, wy = (corner & 2) ? cell.fy : 1.0f - cell.fy, wz = (corner & 4) ? cell.fz : 1.0f - cell.fz;
        const float w = (wx * wy) * wz;
        if ((rgba >> 24) == 255u) {
          W += w;
          R += w * (float)(rgba & 0xffu); Gc += w * (float)((rgba >> 8) & 0xffu); B += w * (float)((rgba >> 16) & 0xffu);
        }
      }
      if (W > 0.0f) packed = (uint32_t)(R / W + 0.5f) | ((uint32_t)(Gc / W + 0.5f) << 8) | ((uint32_t)(B / W + 0.5f) << 16) | 0xff000000u;
    }
    out_color.at<uint32_t>(j, i) = packed;
  }
}

}  // namespace bslam
