// Host build (g++) of robosimgs_amd/csrc/tile_rect.h -- tile_rect, tighten_rect, pack_tile_rect -- and of the per-pixel
// alpha chain of raster_common.h that a tightened rectangle must never contradict, so that the rule can be held against
// fp64 arithmetic without a GPU (tests/test_tile_rect_host.py).  Test-only: never linked into libmgs.so.
#include <algorithm>
#include <climits>
#include <cmath>
#include <cstddef>
#include <cstdint>

#define MGS_COMMON_H_             // (mgs_common.h is HIP host plumbing and wave helpers: none of it is needed here)
#define __device__
#define __host__
#define __forceinline__ inline
#define __logf logf               // the fast logarithm's stand-in: the rule's slack is five orders above either one's error

struct uint2 { uint32_t x, y; };
static inline uint2 make_uint2(uint32_t x, uint32_t y) { return uint2{x, y}; }
using std::max;
using std::min;

namespace mgs {
inline unsigned long long ballot(bool p) { return p ? 1ull : 0ull; }
}
static inline bool __builtin_amdgcn_inverse_ballot_w64(unsigned long long m) { return (m & 1ull) != 0ull; }
static inline float __builtin_amdgcn_rcpf(float x) { return 1.0f / x; }
static inline float __builtin_amdgcn_logf(float x) { return log2f(x); }
static inline float __builtin_amdgcn_fmed3f(float a, float b, float c) {
  if (std::isnan(a) || std::isnan(b) || std::isnan(c)) return fminf(fminf(a, b), c);
  return fmaxf(fminf(a, b), fminf(fmaxf(a, b), c));
}

#include "../../robosimgs_amd/csrc/raster_common.h"
#include "../../robosimgs_amd/csrc/tile_rect.h"

using namespace mgs;

static const float kTile = 16.f;

// The classic rectangle of every case as x0, y0, w, h.  overload 1: tile_rect(mx, my, radius, ...) on rx alone;
// overload 2: the per-axis one on (rx, ry).
extern "C" void tr_classic(int n, const float* mx, const float* my, const int32_t* rx, const int32_t* ry,
                           const int32_t* tile_w, const int32_t* tile_h, int overload, int32_t* rect) {
  for (int i = 0; i < n; ++i) {
    const TileRect r = overload == 1 ? tile_rect(mx[i], my[i], rx[i], kTile, tile_w[i], tile_h[i])
                                     : tile_rect(mx[i], my[i], rx[i], ry[i], kTile, tile_w[i], tile_h[i]);
    rect[4 * i + 0] = r.x0; rect[4 * i + 1] = r.y0; rect[4 * i + 2] = r.w; rect[4 * i + 3] = r.h;
  }
}

// What tile_count_kernel (binning.hip) and the seed of project_color_fwd_kernel (projection.hip) compute per Gaussian: a
// culled row (radius 0) gets kEmptyTileRect and rectangle 0 0 0 0, any other the classic rectangle, tightened, packed.
extern "C" void tr_tight(int n, const float* mx, const float* my, const float* a, const float* b, const float* c,
                         const float* op, const int32_t* rx, const int32_t* ry, const int32_t* tile_w,
                         const int32_t* tile_h, int32_t* rect, uint32_t* packed) {
  for (int i = 0; i < n; ++i) {
    uint2 info = make_uint2(kEmptyTileRect, 0u);
    TileRect r{0, 0, 0, 0};
    if (rx[i] > 0) {
      r = tile_rect(mx[i], my[i], rx[i], ry[i], kTile, tile_w[i], tile_h[i]);
      r = tighten_rect(r, mx[i], my[i], a[i], b[i], c[i], op[i], kTile);
      info = pack_tile_rect(r);
    }
    rect[4 * i + 0] = r.x0; rect[4 * i + 1] = r.y0; rect[4 * i + 2] = r.w; rect[4 * i + 3] = r.h;
    packed[2 * i + 0] = info.x; packed[2 * i + 1] = info.y;
  }
}

// pack_tile_rect of arbitrary rectangles (the packing's own limits: x0, y0, w up to 1023)
extern "C" void tr_pack(int n, const int32_t* rect, uint32_t* packed) {
  for (int i = 0; i < n; ++i) {
    const uint2 p = pack_tile_rect(TileRect{rect[4 * i], rect[4 * i + 1], rect[4 * i + 2], rect[4 * i + 3]});
    packed[2 * i + 0] = p.x; packed[2 * i + 1] = p.y;
  }
}
extern "C" uint32_t tr_empty_word() { return kEmptyTileRect; }
extern "C" int tr_cull_opacity_ok(float op) { return cull_opacity_ok(op) ? 1 : 0; }    // the raster's gate (raster_common.h)

// bbox[i] = x0, y0, x1, y1 (exclusive; 0 0 0 0 when there is none): the bounding box of the tiles of the CLASSIC
// rectangle rect[i] that hold a pixel centre whose fp32 alpha -- the kernels' own chain: the conic pre-scaled by
// -log2(e), poly_coefs about that tile's centre, pair_power_poly, exp2 (exp2f / log2f stand in for v_exp_f32 /
// v_log_f32) -- is at least 1/255, for a Gaussian that passes the gate in front of that chain in every kernel that walks
// a list (cull_opacity_ok: an opacity under it is never evaluated, so it reaches nothing).
// Pre-filter, as in cull_harness.cpp's ch_reached: a pixel whose exponent, estimated in plain arithmetic, lies 0.5 below
// the threshold's is not evaluated.  There the chain's own rounding is below 0.02 because the mean is within 56 px of
// the tile centre; a classic rectangle reaches a radius away, so here the 0.5 grows by k d^2, d the pixel's distance
// from the mean and k = 2e-6 (|A| + |B| + |C|): the estimate and the chain each round a handful of terms no larger than
// (|A| + |B| + |C|) d^2 to 2^-24 relative, under 3e-7 (|A| + |B| + |C|) d^2 each.
// Two accelerators that change no answer (brute != 0 switches both off; the test compares the two on a subset):
//  - along a pixel row the filter's pass set lies inside an interval of columns: the estimate is a concave quadratic
//    in dx, solved in double with the margin doubled (2 k d^2 + 0.01, so that the float estimate's rounding, < k d^2,
//    cannot put a passing pixel outside it) and widened by two columns;
//  - a tile inside the box found so far cannot change the box and is skipped.
extern "C" void tr_reached(int n, const float* mx, const float* my, const float* a, const float* b, const float* c,
                           const float* op, const int32_t* rect, int brute, int32_t* bbox, long long* evaluated) {
  const float amin = kAlphaMin, lmin = log2f(kAlphaMin) - 0.5f;
  long long evals = 0;
  for (int i = 0; i < n; ++i) {
    int32_t* bb = bbox + 4 * i;
    bb[0] = bb[1] = bb[2] = bb[3] = 0;
    const int x0 = rect[4 * i], y0 = rect[4 * i + 1], w = rect[4 * i + 2], h = rect[4 * i + 3];
    if (w <= 0 || h <= 0 || !cull_opacity_ok(op[i])) continue;
    const float sA = -0.5f * kLog2e * a[i], sB = -kLog2e * b[i], sC = -0.5f * kLog2e * c[i];
    const float L = log2f(op[i]);
    const float k = 2e-6f * (fabsf(sA) + fabsf(sB) + fabsf(sC));
    int bx0 = INT_MAX, by0 = INT_MAX, bx1 = -1, by1 = -1;
    for (int ty = y0; ty < y0 + h; ++ty) {
      const float m_y = my[i] - (kTile * (float)ty + 8.f);
      for (int r = 0; r < 16; ++r) {
        const float y = (float)r - 7.5f, dy = m_y - y;
        int pl = 16 * x0, ph = 16 * (x0 + w) - 1;
        const double qa = (double)sA + 2.0 * k;
        if (!brute && qa < 0.0) {
          const double qb = (double)sB * dy, qc = ((double)sC + 2.0 * k) * dy * dy + L - lmin + 0.01;
          const double disc = qb * qb - 4.0 * qa * qc;
          if (disc < 0.0) continue;                         // (NaN: the whole row, like brute)
          if (disc >= 0.0) {
            const double sq = sqrt(disc), d_lo = (-qb + sq) / (2.0 * qa), d_hi = (-qb - sq) / (2.0 * qa);  // qa < 0
            // dx = mean - (px + 0.5) in [d_lo, d_hi]
            const double lo = floor((double)mx[i] - 0.5 - d_hi) - 2.0, hi = ceil((double)mx[i] - 0.5 - d_lo) + 2.0;
            if (lo > (double)ph || hi < (double)pl) continue;
            if (lo > (double)pl) pl = (int)lo;
            if (hi < (double)ph) ph = (int)hi;
          }
        }
        int tx_q = INT_MIN;
        float m_x = 0.f;
        PolyCoef q{0.f, 0.f, 0.f};
        for (int px = pl; px <= ph; ++px) {
          const int tx = px >> 4;
          if (!brute && tx >= bx0 && tx <= bx1 && ty >= by0 && ty <= by1) { px = 16 * tx + 15; continue; }
          if (tx != tx_q) {
            tx_q = tx;
            m_x = mx[i] - (kTile * (float)tx + 8.f);
            q = poly_coefs(m_x, m_y, sA, sB, sC, L);
          }
          const float x = (float)(px & 15) - 7.5f;
          const float dx = m_x - x;
          const float est = sA * dx * dx + sB * dx * dy + sC * dy * dy + L;
          if (!(est + k * (dx * dx + dy * dy) >= lmin)) continue;      // (NaN cases are not judged by this function)
          ++evals;
          const float alpha = exp2f(pair_power_poly(pixel_poly(x, y), q.q0, q.q1, q.q2, sA, sB, sC));
          if (alpha >= amin) {
            bx0 = std::min(bx0, tx); bx1 = std::max(bx1, tx); by0 = std::min(by0, ty); by1 = std::max(by1, ty);
          }
        }
      }
    }
    if (bx1 >= 0) { bb[0] = bx0; bb[1] = by0; bb[2] = bx1 + 1; bb[3] = by1 + 1; }
  }
  if (evaluated) *evaluated = evals;
}
