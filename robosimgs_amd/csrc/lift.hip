// lift.hip -- 2D part masks lifted onto Gaussians (include/mgs_lift.h), gfx950.
//
// raster_votes_kernel is the transpose of raster_labels_kernel (labels.hip): the same walk of one camera's tile lists
// (raster_common.h: one wave per 16x16 tile, four pixels per lane, batches of kQueue entries culled with quadrant_reach and
// queued in LDS, started in tile_group_order), the same pair_weight (pair_weight.h) -- so the T and w of every voting pixel
// are the forward's bit for bit -- but where the label kernel sums w over the Gaussians of a class per PIXEL, this one
// sums w over the pixels of a class per GAUSSIAN:  V[i,k] = sum over p with mask(p) == k of w_i(p).
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
#include "raster_common.h"
#include "pair_weight.h"
#include "tile_order.h"
#include "../../include/mgs_lift.h"

#include <math.h>

namespace mgs {
namespace {

constexpr float kVoteOne = 4294967296.f;             // 2^32: one pixel of full weight

struct VoteEntry {
  float4 geo0;                       // q0, q1, q2, A   (raster_common.h: poly_coefs; A, B, C: conic pre-scaled)
  float4 geo1;                       // B, C, votes row (bits), unused
  float4 geo3;                       // mean - tile centre (x, y): read only by batches that test sigma >= 0
};

__global__ __launch_bounds__(64) void raster_votes_kernel(
    const float* __restrict__ means2d, const float* __restrict__ conics, const float* __restrict__ opacities,
    const float4* __restrict__ splats, const uint8_t* __restrict__ mask, int n_classes, int width, int height, int tile_w,
    int n_tiles, const int32_t* __restrict__ tile_offsets, const int32_t* __restrict__ flatten_ids,
    const int32_t* __restrict__ group_order, int row_offset, int n_rows, unsigned long long* __restrict__ votes) {
  __shared__ VoteEntry queue[kQueue + 1];
  const int tile = tile_of_unit((int)blockIdx.x, n_tiles, group_order);      // tile_order.h
  if (tile < 0) return;
  const unsigned lane = threadIdx.x & 63u;
  const int tx = tile % tile_w, ty = tile / tile_w;
  const float tile_x = (float)(tx * 16), tile_y = (float)(ty * 16);
  const int start = tile_offsets[tile], end = tile_offsets[tile + 1];
  if (start >= end) return;                       // no list: nobody to vote for
  const int ix = tx * 16 + (int)(lane & 7), iy = ty * 16 + (int)(lane >> 3);

  // the mask bytes of the lane's four pixels; 255: casts no vote
  unsigned cls_of[4];
  unsigned have = 0u;
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    const int x = ix + 8 * (k & 1), y = iy + 8 * (k >> 1);
    unsigned m = 255u;
    if (x < width && y < height) m = mask[(size_t)y * width + x];
    if (m >= (unsigned)n_classes) m = 255u;
    else have |= 1u << m;
    cls_of[k] = m;
  }
  const unsigned mask4 = cls_of[0] | cls_of[1] << 8 | cls_of[2] << 16 | cls_of[3] << 24;
  const unsigned present = wave_or(have);         // wave-uniform: the classes that can be voted for in this tile
  if (present == 0u) return;

  const float xo = (float)(lane & 7) - 7.5f, yo = (float)(lane >> 3) - 7.5f;
  PixelPoly pq[4];
#pragma unroll
  for (int k = 0; k < 4; ++k) pq[k] = pixel_poly(xo + 8.f * (k & 1), yo + 8.f * (k >> 1));
  const float ctr_x = tile_x + 8.f, ctr_y = tile_y + 8.f;

  float T[4];
  unsigned long long alive[4];                    // the quadrant's open voting pixels
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    T[k] = 1.f;
    alive[k] = ballot(((mask4 >> (8 * k)) & 255u) != 255u);
  }

  for (int b = start; b < end; b += kQueue) {
    unsigned live = 0;
#pragma unroll
    for (int k = 0; k < 4; ++k)
      if (alive[k] != 0ull) live |= 1u << k;
    if (live == 0) break;

    // this batch's entries: one list entry per lane
    const int c_idx = b + (int)lane;
    const bool c_ok = c_idx < end;
    float2 c_xy = make_float2(0.f, 0.f);
    float c_ca = 1.f, c_cb = 0.f, c_cc = 1.f, c_op = 0.f;
    int c_row = -1;
    if (c_ok) {
      const int g = flatten_ids[c_idx];
      c_row = g - row_offset;
      if (splats) {                               // the packed 48-byte record: its first two quarters
        const float4 p0 = splats[3 * (size_t)g], p1 = splats[3 * (size_t)g + 1];
        c_xy = make_float2(p0.x, p0.y);
        c_ca = p0.z; c_cb = p0.w; c_cc = p1.x; c_op = p1.y;
      } else {
        c_xy = reinterpret_cast<const float2*>(means2d)[g];
        c_ca = conics[3 * (size_t)g + 0];
        c_cb = conics[3 * (size_t)g + 1];
        c_cc = conics[3 * (size_t)g + 2];
        c_op = opacities[g];
      }
    }

    unsigned long long reach[4];
    quadrant_reach(c_xy.x, c_xy.y, c_ca, c_cb, c_cc, c_op, c_ok, tile_x, tile_y, live, reach);
    const unsigned long long keep = reach[0] | reach[1] | reach[2] | reach[3];
    const bool queued = __builtin_amdgcn_inverse_ballot_w64(keep);
    const bool all_safe = ballot(queued && !entry_is_safe(c_ca, c_cb, c_cc, c_op)) == 0ull;
    if (queued) {
      VoteEntry& e = queue[mask_rank(keep)];
      const float sA = -0.5f * kLog2e * c_ca, sB = -kLog2e * c_cb, sC = -0.5f * kLog2e * c_cc;
      const float m_x = c_xy.x - ctr_x, m_y = c_xy.y - ctr_y;
      const PolyCoef q = poly_coefs(m_x, m_y, sA, sB, sC, __log2f(c_op));
      e.geo0 = make_float4(q.q0, q.q1, q.q2, sA);
      e.geo1 = make_float4(sB, sC, __int_as_float(c_row), 0.f);
      e.geo3 = make_float4(m_x, m_y, 0.f, 0.f);
    }
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");

    auto walk = [&](auto safe_tag) {
      constexpr bool SAFE = decltype(safe_tag)::value;
      // entry j was queued by the lane of the j-th set bit of `keep`
      unsigned long long rest = keep;
      const VoteEntry* e = queue;
      while (rest != 0ull) {
        const int at = __builtin_ctzll(rest);
        rest &= rest - 1ull;
        const float4 g0 = e->geo0, g1 = e->geo1;
        float4 g3 = make_float4(0.f, 0.f, 0.f, 0.f);
        if constexpr (!SAFE) g3 = e->geo3;
        ++e;
        float w[4] = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int k = 0; k < 4; ++k) {
          if ((reach[k] >> at) & 1ull) {
            w[k] = pair_weight<SAFE>(T[k], alive[k], pq[k], g0.x, g0.y, g0.z, g0.w, g1.x, g1.y, g3.x, g3.y);
            if (alive[k] == 0ull) reach[k] = 0ull;         // the quadrant's last pixel closed: the batch skips it
          }
        }
        // the row is the same for all 64 lanes of the evaluation: a scalar; outside 0..n_rows-1 it occludes only
        const int row = __builtin_amdgcn_readfirstlane(__float_as_int(g1.z));
        if ((unsigned)row >= (unsigned)n_rows) continue;
        if (ballot((w[0] + w[1]) + (w[2] + w[3]) > 0.f) == 0ull) continue;      // counted at no voting pixel
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
      }
    };
    if (all_safe) walk(std::true_type{}); else walk(std::false_type{});
    __builtin_amdgcn_wave_barrier();   // queue is rewritten by the next batch
  }
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
  const int n_tiles = tile_w * tile_h;
  const int n_units = tile_group_order ? (n_tiles + 3) / 4 * 4 : n_tiles;       // tile slots of the launch
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
