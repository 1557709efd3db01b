// lift.hip -- 2D part masks lifted onto Gaussians (include/mgs_lift.h), gfx950.
//
// raster_votes_kernel is the transpose of raster_labels_kernel (labels.hip): the one walk of a camera's tile lists both
// call (weight_walk.h: weight_walk, started in tile_group_order) -- so the T and w of every voting pixel are the forward's
// bit for bit -- but where the label kernel sums w over the Gaussians of a class per PIXEL, this one sums w over the
// pixels of a class per GAUSSIAN:  V[i,k] = sum over p with mask(p) == k of w_i(p).  What is this kernel's own: which
// pixels start open, the entry's payload (the votes row) and the reduction below.
//
// Mask.  A lane keeps the mask bytes of its four pixels in one register (byte k = quadrant k); a pixel outside the image
// or with a mask value outside 0..K-1 holds 255 and starts finished, exactly as a pixel outside the image does in the
// other raster kernels: it is never evaluated, casts no vote, and no other pixel's chain depends on it.  The classes
// present among the tile's voting pixels are found once per tile as a scalar bit mask (wave_or); a tile without a voting
// pixel returns before the walk.
//
// Reduction.  For every queue entry the wave loops over the SET BITS of that mask -- never over a register array indexed
// by class, which would go to scratch -- and for class c sums the w of the lane's pixels of class c, then the 64 lanes
// with the fixed DPP tree wave_reduce_to_lane63: a fixed order, so the fp32 sum of a (tile, entry, class) is the same bits
// in every run.  Lane 63 adds rint(sum * 2^32) into votes[row, c] with a no-return 64-bit integer atomic
// (global_atomic_add_x2): integer addition is associative, so the order in which tiles and cameras arrive cannot change
// a bit.  A tile under one part pays one reduction per entry; an entry that reaches no voting pixel pays none.
//
// lift_assign_kernel: one thread per Gaussian scans its K votes in ascending class with a strict >.
#include "weight_walk.h"
#include "tile_order.h"
#include "../../include/mgs_lift.h"

#include <math.h>

namespace mgs {
namespace {

constexpr float kVoteOne = 4294967296.f;             // 2^32: one pixel of full weight

__global__ __launch_bounds__(64) void raster_votes_kernel(
    const float* __restrict__ means2d, const float* __restrict__ conics, const float* __restrict__ opacities,
    const float4* __restrict__ splats, const uint8_t* __restrict__ mask, int n_classes, int width, int height, int tile_w,
    int n_tiles, const int32_t* __restrict__ tile_offsets, const int32_t* __restrict__ flatten_ids,
    const int32_t* __restrict__ group_order, int row_offset, int n_rows, unsigned long long* __restrict__ votes) {
  __shared__ WeightEntry queue[kQueue + 1];
  const int tile = tile_of_unit((int)blockIdx.x, n_tiles, group_order);      // tile_order.h
  if (tile < 0) return;
  const unsigned lane = threadIdx.x & 63u;
  const int start = tile_offsets[tile], end = tile_offsets[tile + 1];
  if (start >= end) return;                       // no list: nobody to vote for
  const TileFrame fr = tile_frame(tile, tile_w, lane);

  // the mask bytes of the lane's four pixels; 255: casts no vote
  unsigned cls_of[4];
  unsigned have = 0u;
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    const int x = fr.ix + 8 * (k & 1), y = fr.iy + 8 * (k >> 1);
    unsigned m = 255u;
    if (x < width && y < height) m = mask[(size_t)y * width + x];
    if (m >= (unsigned)n_classes) m = 255u;
    else have |= 1u << m;
    cls_of[k] = m;
  }
  const unsigned mask4 = cls_of[0] | cls_of[1] << 8 | cls_of[2] << 16 | cls_of[3] << 24;
  const unsigned present = wave_or(have);         // wave-uniform: the classes that can be voted for in this tile
  if (present == 0u) return;

  unsigned long long alive[4];                    // the quadrant's open voting pixels
#pragma unroll
  for (int k = 0; k < 4; ++k) alive[k] = ballot(((mask4 >> (8 * k)) & 255u) != 255u);

  weight_walk(queue, fr, lane, start, end, splats, means2d, conics, opacities, flatten_ids, alive,
              [&](int g) { return g - row_offset; },
              [&](int row, auto quad) {
                float w[4] = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
                for (int k = 0; k < 4; ++k) quad(k, w[k]);
                // a row outside 0..n_rows-1 occludes only
                if ((unsigned)row >= (unsigned)n_rows) return;
                if (ballot((w[0] + w[1]) + (w[2] + w[3]) > 0.f) == 0ull) return;      // counted at no voting pixel
                unsigned long long* dst = votes + (size_t)row * (size_t)n_classes;
                unsigned todo = present;
                while (todo != 0u) {
                  const unsigned c = (unsigned)__builtin_ctz(todo);
                  todo &= todo - 1u;
                  float s[4];
#pragma unroll
                  for (int k = 0; k < 4; ++k) s[k] = ((mask4 >> (8 * k)) & 255u) == c ? w[k] : 0.f;
                  const float sum = wave_reduce_to_lane63((s[0] + s[1]) + (s[2] + s[3]));     // fixed order: lane 63 holds it
                  if (lane == 63u && sum > 0.f)
                    atomicAdd(dst + c, (unsigned long long)rintf(sum * kVoteOne));            // global_atomic_add_x2, no return
                }
              });
}

__global__ __launch_bounds__(256) void lift_assign_kernel(int n_rows, int n_classes,
                                                          const unsigned long long* __restrict__ votes,
                                                          unsigned long long min_vote, int32_t* __restrict__ class_ids,
                                                          float* __restrict__ confidence) {
  const int g = (int)(blockIdx.x * 256u + threadIdx.x);
  if (g >= n_rows) return;
  const unsigned long long* v = votes + (size_t)g * (size_t)n_classes;
  unsigned long long best = 0ull, total = 0ull;
  int cls = 0;
  for (int c = 0; c < n_classes; ++c) {           // ascending class, strict >: ties go to the lowest class
    const unsigned long long x = v[c];
    total += x;
    if (x > best) { best = x; cls = c; }
  }
  const bool assigned = best > min_vote;          // (best > 0 at the least: a row without a vote has no class)
  class_ids[g] = assigned ? cls : -1;
  if (confidence) confidence[g] = assigned ? (float)((double)best / (double)total) : 0.f;
}

}  // namespace
}  // namespace mgs

using namespace mgs;

extern "C" int mgs_raster_votes(int n, const float* means2d, const float* conics, const float* opacities,
                                const float* splats, const uint8_t* mask, int n_classes, int width, int height, int tile_w,
                                int tile_h, const int32_t* tile_offsets, const int32_t* flatten_ids,
                                const int32_t* tile_group_order, int row_offset, int n_rows, uint64_t* votes,
                                mgs_stream_t stream) {
  MGS_REQUIRE(n_classes >= 1 && n_classes <= MGS_LABELS_MAX_CLASSES, "raster_votes: n_classes %d outside 1..%d", n_classes,
              MGS_LABELS_MAX_CLASSES);
  MGS_REQUIRE(mask, "raster_votes: mask is null");
  MGS_REQUIRE(votes, "raster_votes: votes is null");
  MGS_REQUIRE(n_rows >= 0, "raster_votes: n_rows %d is negative", n_rows);
  MGS_REQUIRE(splats || (means2d && conics && opacities),
              "raster_votes: neither packed records (splats) nor means2d, conics and opacities given");
  MGS_REQUIRE(n >= 0 && width > 0 && height > 0, "raster_votes: bad sizes");
  MGS_REQUIRE(tile_w == (width + 15) / 16 && tile_h == (height + 15) / 16,
              "raster_votes: tile grid %dx%d does not match %dx%d at tile size 16", tile_w, tile_h, width, height);
  MGS_REQUIRE(tile_offsets && flatten_ids, "raster_votes: null tile lists");
  const int n_tiles = tile_w * tile_h, n_units = tile_launch_units(n_tiles, tile_group_order);
  hipLaunchKernelGGL(raster_votes_kernel, dim3(n_units), dim3(64), 0, (hipStream_t)stream, means2d, conics, opacities,
                     reinterpret_cast<const float4*>(splats), mask, n_classes, width, height, tile_w, n_tiles, tile_offsets,
                     flatten_ids, tile_group_order, row_offset, n_rows, reinterpret_cast<unsigned long long*>(votes));
  return check_launch("raster_votes");
}

extern "C" int mgs_lift_assign(int n_rows, int n_classes, const uint64_t* votes, float min_vote, int32_t* class_ids,
                               float* confidence, mgs_stream_t stream) {
  MGS_REQUIRE(n_rows >= 0, "lift_assign: n_rows %d is negative", n_rows);
  MGS_REQUIRE(n_classes >= 1 && n_classes <= MGS_LABELS_MAX_CLASSES, "lift_assign: n_classes %d outside 1..%d", n_classes,
              MGS_LABELS_MAX_CLASSES);
  MGS_REQUIRE(votes, "lift_assign: votes is null");
  MGS_REQUIRE(class_ids, "lift_assign: class_ids is null");
  MGS_REQUIRE(min_vote >= 0.f && min_vote < 2147483648.f, "lift_assign: min_vote %g outside 0 <= min_vote < 2^31",
              (double)min_vote);
  if (n_rows == 0) return MGS_OK;
  const unsigned long long min_q = (unsigned long long)rint((double)min_vote * 4294967296.0);
  hipLaunchKernelGGL(lift_assign_kernel, dim3(div_up((unsigned)n_rows, 256u)), dim3(256), 0, (hipStream_t)stream, n_rows,
                     n_classes, reinterpret_cast<const unsigned long long*>(votes), min_q, class_ids, confidence);
  return check_launch("lift_assign");
}
