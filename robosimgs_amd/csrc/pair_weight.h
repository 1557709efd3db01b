// pair_weight.h -- the blend weight of one (Gaussian, quadrant) evaluation, shared bit for bit by the kernels that walk a
// camera's tile lists without blending features: raster_labels_kernel (labels.hip) and raster_votes_kernel (lift.hip).
#ifndef MGS_PAIR_WEIGHT_H_
#define MGS_PAIR_WEIGHT_H_

#include "raster_common.h"

namespace mgs {

constexpr float kLog2e = 1.4426950408889634f;

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

}  // namespace mgs
#endif
