// Host build (g++) of the raster's cull in robosimgs_amd/csrc/raster_common.h -- quadrant_mask / rect_min_sigma --
// and of the per-pixel alpha chain it must never contradict, so that both can be held against fp64 arithmetic
// without a GPU.  Test-only: never linked into libmgs.so.  A "wave" here is one lane: ballot(p) is p.
#include <cmath>
#include <cstddef>
#include <cstdint>

#define MGS_COMMON_H_             // (mgs_common.h is HIP host plumbing and wave helpers: none of it is needed here)
#define __device__
#define __host__
#define __forceinline__ inline

namespace mgs {
inline unsigned long long ballot(bool p) { return p ? 1ull : 0ull; }
}
static inline bool __builtin_amdgcn_inverse_ballot_w64(unsigned long long m) { return (m & 1ull) != 0ull; }
static inline float __builtin_amdgcn_rcpf(float x) { return 1.0f / x; }
static inline float __builtin_amdgcn_logf(float x) { return log2f(x); }          // v_log_f32 is the base-2 logarithm
// v_med3_f32: the median of three; min3 (which ignores a NaN, like fminf) when an operand is NaN
static inline float __builtin_amdgcn_fmed3f(float a, float b, float c) {
  if (std::isnan(a) || std::isnan(b) || std::isnan(c)) return fminf(fminf(a, b), c);
  return fmaxf(fminf(a, b), fminf(fmaxf(a, b), c));
}

#include "../../robosimgs_amd/csrc/raster_common.h"

using namespace mgs;

// quadrant_mask of every case: the one-wave-per-tile kernels' cull (forward and backward)
extern "C" void ch_quadrant_mask(int n, const float* mx, const float* my, const float* a, const float* b, const float* c,
                                 const float* op, const float* tile_x, const float* tile_y, uint8_t* mask) {
  for (int i = 0; i < n; ++i) mask[i] = (uint8_t)quadrant_mask(mx[i], my[i], a[i], b[i], c[i], op[i], tile_x[i], tile_y[i]);
}

// the same with some quadrants closed: bit k of `live` clear skips quadrant k's arithmetic
extern "C" void ch_quadrant_mask_live(int n, const float* mx, const float* my, const float* a, const float* b,
                                      const float* c, const float* op, const float* tile_x, const float* tile_y, int live,
                                      uint8_t* mask) {
  for (int i = 0; i < n; ++i)
    mask[i] = (uint8_t)quadrant_mask(mx[i], my[i], a[i], b[i], c[i], op[i], tile_x[i], tile_y[i], (unsigned)live);
}

// the per-block kernel's cull: rect_min_sigma of each quadrant's rectangle under that kernel's own threshold
// (raster_fwd.hip, raster_fwd_q_kernel: the same expressions)
extern "C" void ch_block_mask(int n, const float* mx, const float* my, const float* a, const float* b, const float* c,
                              const float* op, const float* tile_x, const float* tile_y, uint8_t* mask) {
  for (int i = 0; i < n; ++i) {
    unsigned m = 0;
    if (cull_opacity_ok(op[i])) {
      const float thr = 0.6931471805599453f * __builtin_amdgcn_logf(255.0f * op[i]);
      const float fx = fmaxf(fabsf(tile_x[i] - mx[i]), fabsf(tile_x[i] + 16.f - mx[i]));
      const float fy = fmaxf(fabsf(tile_y[i] - my[i]), fabsf(tile_y[i] + 16.f - my[i]));
      const float slack = 0.05f + 4e-6f * (fabsf(a[i]) + fabsf(c[i]) + 2.f * fabsf(b[i])) * (fx * fx + fy * fy);
      for (int k = 0; k < 4; ++k) {
        QuadRect r;
        r.x0 = tile_x[i] + (float)(8 * (k & 1)) + 0.5f; r.x1 = r.x0 + 7.f;
        r.y0 = tile_y[i] + (float)(8 * (k >> 1)) + 0.5f; r.y1 = r.y0 + 7.f;
        const float smin = rect_min_sigma(mx[i], my[i], a[i], b[i], c[i], __builtin_amdgcn_rcpf(a[i]),
                                          __builtin_amdgcn_rcpf(c[i]), r);
        if (!(smin > thr + slack)) m |= 1u << k;
      }
    }
    mask[i] = (uint8_t)m;
  }
}

// Bit k of reached[i]: some pixel centre of quadrant k has an fp32 alpha -- the kernels' own chain: the conic
// pre-scaled by -log2(e), poly_coefs about the tile centre, pair_power_poly, exp2 -- of at least 1/255.  exp2f and
// log2f stand in for v_exp_f32 and v_log_f32.
// Pixels whose exponent, estimated in plain arithmetic, lies 0.5 below the threshold's are not evaluated: the chain's
// own rounding is below 0.02 there (|A| m^2 2^-23 with |A| <= 2.4, m <= 56).
extern "C" void ch_reached(int n, const float* mx, const float* my, const float* a, const float* b, const float* c,
                           const float* op, const float* tile_x, const float* tile_y, uint8_t* reached) {
  const float kLog2e = 1.4426950408889634f;
  const float amin = kAlphaMin, lmin = log2f(kAlphaMin) - 0.5f;
  for (int i = 0; i < n; ++i) {
    const float sA = -0.5f * kLog2e * a[i], sB = -kLog2e * b[i], sC = -0.5f * kLog2e * c[i];
    const float m_x = mx[i] - (tile_x[i] + 8.f), m_y = my[i] - (tile_y[i] + 8.f);
    const float L = log2f(op[i]);
    const PolyCoef q = poly_coefs(m_x, m_y, sA, sB, sC, L);
    unsigned m = 0;
    for (int py = 0; py < 16; ++py)
      for (int px = 0; px < 16; ++px) {
        const float x = (float)px - 7.5f, y = (float)py - 7.5f;
        const float dx = m_x - x, dy = m_y - y;
        const float est = sA * dx * dx + sB * dx * dy + sC * dy * dy + L;
        if (!(est >= lmin)) continue;                       // (NaN cases are not judged by this function)
        const float alpha = exp2f(pair_power_poly(pixel_poly(x, y), q.q0, q.q1, q.q2, sA, sB, sC));
        if (alpha >= amin) m |= 1u << ((px >> 3) + 2 * (py >> 3));
      }
    reached[i] = (uint8_t)m;
  }
}
