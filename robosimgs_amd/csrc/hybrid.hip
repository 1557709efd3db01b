// hybrid.hip -- the exact mesh-over-splat composite (include/mgs_hybrid.h), gfx950.
//
// raster_over_opaque_kernel walks one camera's tile lists the way raster_labels_kernel does (weight_walk.h: one wave per
// 16x16 tile, four pixels per lane, started in tile_group_order), so the w of every (Gaussian, pixel) pair is the
// forward's bit for bit.  What is this kernel's own:
//
// Open pixels.  open[k] is the ballot of "has foreground and inside the image": only those are walked.  Every other
//   in-image pixel gets mgs_composite_over's third rule from the given frame, and a tile with no open pixel returns
//   without touching its list.
// List truncation.  The lists are ordered by (depth bits, index), so the Gaussians with depths < d are a prefix of every
//   pixel's walk, and nothing at or behind the tile's largest open d can be in F at any of its pixels: a binary search
//   over depths[flatten_ids[j]] (wave-uniform addresses) finds the first such entry and the walk ends there.
// Payload.  The lane that loads a list entry also loads that Gaussian's three colours and its depth into four registers
//   of its own (64 rows in flight per batch), and the queue entry carries that lane's number.  The entry callback gets
//   the number as a wave-uniform scalar and reads the four values with v_readlane: wave-uniform scalars without a memory
//   access on the walk's serial path.  (Measured on the 1 M-Gaussian 1080p frame with the open box: 116.6 us; with the
//   flat id as the payload and four scalar loads per entry in the callback, whose latency nothing hides on a SIMD that
//   holds one wave: 142.7 us.  profiles/hybrid/README.md.)
// Accumulators.  4 quadrants x (3 colours + depth + T_F) floats in registers; per reached quadrant the lane tests
//   z < d[k] and, where true, adds with the forward's own expression acc = fma(w, c, acc) and takes w off T_F (the walk
//   hands out w, not alpha: include/mgs_hybrid.h states the form).  No LDS beyond the walk's queue, no atomics.
#include "weight_walk.h"
#include "tile_order.h"
#include "../../include/mgs_hybrid.h"

namespace mgs {
namespace {

// c + t b with the product and the sum rounded separately (include/mgs_hybrid.h: the pass-through pixels are compared
// byte for byte with a restatement that has no fused multiply-add)
__device__ __forceinline__ float over_backdrop(float c, float t, float b) {
#pragma clang fp contract(off)
  return c + t * b;
}

__global__ __launch_bounds__(64) void raster_over_opaque_kernel(
    const float* __restrict__ means2d, const float* __restrict__ conics, const float* __restrict__ opacities,
    const float* __restrict__ feats, int feat_stride, const float* __restrict__ depths, const float* __restrict__ fg_rgb,
    const float* __restrict__ fg_depth, const float* __restrict__ render, const float* __restrict__ alphas,
    const float* __restrict__ backdrop, int width, int height, int tile_w, int n_tiles,
    const int32_t* __restrict__ tile_offsets, const int32_t* __restrict__ flatten_ids,
    const int32_t* __restrict__ group_order, float* __restrict__ out_rgb, float* __restrict__ out_depth,
    float* __restrict__ fg_visibility) {
  __shared__ WeightEntry queue[kQueue + 1];
  const int tile = tile_of_unit((int)blockIdx.x, n_tiles, group_order);      // tile_order.h
  if (tile < 0) return;
  const unsigned lane = threadIdx.x & 63u;
  const TileFrame fr = tile_frame(tile, tile_w, lane);
  const int ix = fr.ix, iy = fr.iy;

  float d[4];                                     // the foreground's depth; -inf where the pixel is not open
  unsigned long long open[4];
  float d_max = 0.f;
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    const int x = ix + 8 * (k & 1), y = iy + 8 * (k >> 1);
    const bool inside = x < width && y < height;
    const size_t p = (size_t)y * width + x;
    const float zf = inside ? fg_depth[p] : 0.f;
    const bool has_fg = zf > 0.f && zf < INFINITY;                           // (a NaN depth is no foreground)
    open[k] = ballot(has_fg);
    d[k] = has_fg ? zf : -INFINITY;
    d_max = fmaxf(d_max, has_fg ? zf : 0.f);
    if (inside && !has_fg) {                      // no foreground: composite_over's third rule on the given frame
      const float4 px = reinterpret_cast<const float4*>(render)[p];
      const float a = alphas[p];
      float r0 = px.x, r1 = px.y, r2 = px.z;
      if (backdrop) {
        const float t = 1.f - a;
        r0 = over_backdrop(r0, t, backdrop[0]);
        r1 = over_backdrop(r1, t, backdrop[1]);
        r2 = over_backdrop(r2, t, backdrop[2]);
      }
      out_rgb[3 * p] = r0; out_rgb[3 * p + 1] = r1; out_rgb[3 * p + 2] = r2;
      out_depth[p] = a > 0.f ? px.w : INFINITY;
      if (fg_visibility) fg_visibility[p] = 0.f;
    }
  }
  if ((open[0] | open[1] | open[2] | open[3]) == 0ull) return;              // wave-uniform: the list is not touched

  // the tile's largest open depth, and the first list entry at or behind it
#pragma unroll
  for (int s = 32; s >= 1; s >>= 1) d_max = fmaxf(d_max, __shfl_xor(d_max, s));
  const float d_cut = __int_as_float(__builtin_amdgcn_readfirstlane(__float_as_int(d_max)));
  const int start = __builtin_amdgcn_readfirstlane(tile_offsets[tile]);
  int lo = start, hi = __builtin_amdgcn_readfirstlane(tile_offsets[tile + 1]);
  while (lo < hi) {
    const int mid = lo + ((hi - lo) >> 1);
    if (depths[flatten_ids[mid]] >= d_cut) hi = mid; else lo = mid + 1;
  }
  const int stop = lo;                            // in [start, end]: nothing from here on is in F at any pixel of the tile

  float acc[4][4];                                // sum_F w (r, g, b, z)
  float t_f[4];
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    acc[k][0] = 0.f; acc[k][1] = 0.f; acc[k][2] = 0.f; acc[k][3] = 0.f;
    t_f[k] = 1.f;
  }

  // this batch's entry of the lane: its three colours and its depth; the payload is the lane's number
  float own_c0 = 0.f, own_c1 = 0.f, own_c2 = 0.f, own_z = 0.f;
  auto uniform_of = [](float v, int src) {
    return __int_as_float(__builtin_amdgcn_readlane(__float_as_int(v), src));
  };
  if (start < stop)
    weight_walk(queue, fr, lane, start, stop, static_cast<const float4*>(nullptr), means2d, conics, opacities, flatten_ids,
                open,
                [&](int g) {
                  const float* f = feats + (size_t)g * feat_stride;
                  own_c0 = f[0]; own_c1 = f[1]; own_c2 = f[2]; own_z = depths[g];
                  return (int)lane;
                },
                [&](int src, auto quad) {
                  const float c0 = uniform_of(own_c0, src), c1 = uniform_of(own_c1, src), c2 = uniform_of(own_c2, src),
                              z = uniform_of(own_z, src);
#pragma unroll
                  for (int k = 0; k < 4; ++k) {
                    float w;
                    if (quad(k, w)) {
                      const float wf = z < d[k] ? w : 0.f;               // strictly in front of the foreground
                      acc[k][0] = fmaf(wf, c0, acc[k][0]);
                      acc[k][1] = fmaf(wf, c1, acc[k][1]);
                      acc[k][2] = fmaf(wf, c2, acc[k][2]);
                      acc[k][3] = fmaf(wf, z, acc[k][3]);
                      t_f[k] -= wf;
                    }
                  }
                });

#pragma unroll
  for (int k = 0; k < 4; ++k) {
    const int x = ix + 8 * (k & 1), y = iy + 8 * (k >> 1);
    if (d[k] > 0.f) {                             // open: inside the image, with foreground
      const size_t p = (size_t)y * width + x;
      const float t = t_f[k];
      const bool bare = t == 1.f;                 // F is empty (a counted w is >= 1/255): the foreground's very bits
      const float f0 = fg_rgb[3 * p], f1 = fg_rgb[3 * p + 1], f2 = fg_rgb[3 * p + 2];
      out_rgb[3 * p] = bare ? f0 : fmaf(t, f0, acc[k][0]);
      out_rgb[3 * p + 1] = bare ? f1 : fmaf(t, f1, acc[k][1]);
      out_rgb[3 * p + 2] = bare ? f2 : fmaf(t, f2, acc[k][2]);
      out_depth[p] = bare ? d[k] : fmaf(t, d[k], acc[k][3]);
      if (fg_visibility) fg_visibility[p] = t;
    }
  }
}

}  // namespace
}  // namespace mgs

using namespace mgs;

extern "C" int mgs_raster_over_opaque(int n, const float* means2d, const float* conics, const float* opacities,
                                      const float* feats, int feat_stride, const float* depths, const float* fg_rgb,
                                      const float* fg_depth, const float* render, const float* alphas,
                                      const float* backdrop, int width, int height, int tile_w, int tile_h,
                                      const int32_t* tile_offsets, const int32_t* flatten_ids,
                                      const int32_t* tile_group_order, float* out_rgb, float* out_depth,
                                      float* fg_visibility, mgs_stream_t stream) {
  MGS_REQUIRE(n >= 0 && width > 0 && height > 0, "raster_over_opaque: bad sizes (n %d, %dx%d)", n, width, height);
  MGS_REQUIRE(feat_stride >= 3, "raster_over_opaque: feature stride %d below 3 (rgb in the first three columns)", feat_stride);
  MGS_REQUIRE(tile_w == (width + 15) / 16 && tile_h == (height + 15) / 16,
              "raster_over_opaque: tile grid %dx%d does not match %dx%d at tile size 16", tile_w, tile_h, width, height);
  MGS_REQUIRE(means2d && conics && opacities, "raster_over_opaque: means2d, conics or opacities is null");
  MGS_REQUIRE(feats && depths, "raster_over_opaque: feats or depths is null");
  MGS_REQUIRE(fg_rgb && fg_depth, "raster_over_opaque: null foreground (fg_rgb, fg_depth)");
  MGS_REQUIRE(render && alphas, "raster_over_opaque: null frame (render, alphas)");
  MGS_REQUIRE(tile_offsets && flatten_ids, "raster_over_opaque: null tile lists");
  MGS_REQUIRE(out_rgb && out_depth, "raster_over_opaque: null output (out_rgb, out_depth)");
  MGS_REQUIRE(((uintptr_t)render & 15) == 0, "raster_over_opaque: render must be 16-byte aligned");
  const int n_tiles = tile_w * tile_h, n_units = tile_launch_units(n_tiles, tile_group_order);
  hipLaunchKernelGGL(raster_over_opaque_kernel, dim3(n_units), dim3(64), 0, (hipStream_t)stream, means2d, conics, opacities,
                     feats, feat_stride, depths, fg_rgb, fg_depth, render, alphas, backdrop, width, height, tile_w, n_tiles,
                     tile_offsets, flatten_ids, tile_group_order, out_rgb, out_depth, fg_visibility);
  return check_launch("raster_over_opaque");
}
