// weight_walk.h -- the walk of a tile's list for the kernels that need only the blend WEIGHT of every (Gaussian, pixel)
// pair and blend no features: raster_labels_kernel (labels.hip) and raster_votes_kernel (lift.hip).  The walk is
// raster_fwd_kernel's (raster_common.h: one wave per 16x16 tile, four pixels per lane, batches of kQueue entries culled
// with quadrant_reach and queued in LDS) and every pair is re-evaluated with the forward's own chain -- pair_power_poly on
// poly_coefs, v_exp, the clamp and the sigma test on batches that are not entry_is_safe, next_T = fma(-alpha, T, T),
// w = alpha T -- so the T and w of every pixel are the forward's bit for bit, as the backward's are.
#ifndef MGS_WEIGHT_WALK_H_
#define MGS_WEIGHT_WALK_H_

#include <type_traits>

#include "raster_common.h"

namespace mgs {

// One Gaussian against the 64 pixels of one quadrant: raster_fwd.hip's blend_pixel with the lane-mask form of "finished"
// and nothing accumulated; returns the weight the forward adds the Gaussian's features with (0 where it does not count).
template <bool SAFE>
__device__ __forceinline__ float pair_weight(float& T, unsigned long long& alive, const PixelPoly& pp, float q0, float q1,
                                             float q2, float A, float B, float C, float m_x, float m_y) {
  const float ov = __builtin_amdgcn_exp2f(pair_power_poly(pp, q0, q1, q2, A, B, C));
  const float alpha = SAFE ? ov : fminf(kAlphaMax, ov);
  bool valid = alpha >= kAlphaMin;
  if (!SAFE) valid = valid && pair_power_sign(m_x - pp.x, m_y - pp.y, A, B, C) <= 0.f;
  valid = valid && __builtin_amdgcn_inverse_ballot_w64(alive);
  const float a_eff = valid ? alpha : 0.f;
  const float next_T = fmaf(-a_eff, T, T);
  const bool acc = next_T > kTStop;               // false for the closing Gaussian
  const float w = __fmul_rn(a_eff, T);            // (never contracted into the accumulator's add)
  T = acc ? next_T : T;
  alive &= ~ballot(!acc);
  return acc ? w : 0.f;
}

struct WeightEntry {
  float4 geo0;                       // q0, q1, q2, A   (raster_common.h: queue_geometry; A, B, C: conic pre-scaled)
  float4 geo1;                       // B, C, the entry's payload (bits), unused
  float4 geo3;                       // mean - tile centre (x, y): read only by batches that test sigma >= 0
};

// Walks list entries [start, end) of the lane's tile, front to back, until every pixel is finished.  open[k]: the lanes
// whose pixel of quadrant k starts open (the caller decides); the others are never evaluated.
//   payload(g): the 32 bits the entry of Gaussian g carries to the walk (a class, a row), fetched once per list entry;
//   entry(p, quad): called once per queued entry with its payload p as a wave-uniform scalar.  quad(k, w), for
//     k = 0..3 in any order, evaluates quadrant k: false if the Gaussian does not reach it (nothing is evaluated), else
//     w = the weight of the lane's pixel there.  What entry does with w it does per quadrant, between the calls.
template <class Payload, class Entry>
__device__ __forceinline__ void weight_walk(WeightEntry* queue, const TileFrame& fr, unsigned lane, int start, int end,
                                            const float4* __restrict__ splats, const float* __restrict__ means2d,
                                            const float* __restrict__ conics, const float* __restrict__ opacities,
                                            const int32_t* __restrict__ flatten_ids, const unsigned long long (&open)[4],
                                            Payload payload, Entry entry) {
  // (element by element into arrays of the walk's own.  By the compiler's resource report, not a timing: on the caller's
  //  array the masks left the SGPRs, 82 VGPRs against 57, and brace-initialised arrays kept a second set of masks alive,
  //  103 SGPRs against 87 -- a wave less per SIMD)
  float T[4];
  unsigned long long alive[4];
#pragma unroll
  for (int k = 0; k < 4; ++k) { T[k] = 1.f; alive[k] = open[k]; }
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
    int c_pay = -1;
    if (c_ok) {
      const int g = flatten_ids[c_idx];
      c_pay = payload(g);
      load_geometry(g, splats, means2d, conics, opacities, c_xy, c_ca, c_cb, c_cc, c_op);
    }

    unsigned long long reach[4];
    quadrant_reach(c_xy.x, c_xy.y, c_ca, c_cb, c_cc, c_op, c_ok, fr.tile_x, fr.tile_y, live, reach);
    const unsigned long long keep = reach[0] | reach[1] | reach[2] | reach[3];
    const bool queued = __builtin_amdgcn_inverse_ballot_w64(keep);
    const bool all_safe = ballot(queued && !entry_is_safe(c_ca, c_cb, c_cc, c_op)) == 0ull;
    if (queued) {
      WeightEntry& e = queue[mask_rank(keep)];
      const QueueGeo q = queue_geometry(c_xy, c_ca, c_cb, c_cc, c_op, fr.ctr_x, fr.ctr_y);
      e.geo0 = q.geo0;
      e.geo1 = make_float4(q.sB, q.sC, __int_as_float(c_pay), 0.f);
      e.geo3 = make_float4(q.m_x, q.m_y, 0.f, 0.f);
    }
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");

    auto walk = [&](auto safe_tag) {
      constexpr bool SAFE = decltype(safe_tag)::value;
      // entry j was queued by the lane of the j-th set bit of `keep`
      unsigned long long rest = keep;
      const WeightEntry* e = queue;
      while (rest != 0ull) {
        const int at = __builtin_ctzll(rest);
        rest &= rest - 1ull;
        const float4 g0 = e->geo0, g1 = e->geo1;
        float4 g3 = make_float4(0.f, 0.f, 0.f, 0.f);
        if constexpr (!SAFE) g3 = e->geo3;
        ++e;
        auto quad = [&](int k, float& w) {
          if (!((reach[k] >> at) & 1ull)) return false;
          w = pair_weight<SAFE>(T[k], alive[k], fr.pq[k], g0.x, g0.y, g0.z, g0.w, g1.x, g1.y, g3.x, g3.y);
          if (alive[k] == 0ull) reach[k] = 0ull;           // the quadrant's last pixel closed: the batch skips it
          return true;
        };
        // the payload is the same for all 64 lanes of the evaluation: a scalar
        entry(__builtin_amdgcn_readfirstlane(__float_as_int(g1.z)), quad);
      }
    };
    if (all_safe) walk(std::true_type{}); else walk(std::false_type{});
    __builtin_amdgcn_wave_barrier();   // queue is rewritten by the next batch
  }
}

}  // namespace mgs
#endif
