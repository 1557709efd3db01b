// raster_common.h -- pieces shared by the kernels that walk a camera's tile lists: the forward and backward raster
// (raster_fwd.hip, raster_bwd.hip) and, through weight_walk.h, the label and vote kernels (labels.hip, lift.hip).
//
// Geometry (raster_fwd_kernel, raster_bwd_kernel; raster_fwd_q_kernel gives each of the four
// quadrants its own wave, one pixel per lane).  One wave64 owns one 16x16 tile.  Lane l holds FOUR pixels, one in each 8x8
// quadrant k of the tile: (x, y) = (8*(k&1) + (l&7), 8*(k>>1) + (l>>3)).  A Gaussian's
// parameters are therefore fetched once per 256 pixel evaluations, the four per-lane pixel
// chains give the VALU independent work, and a quadrant whose 64 pixels cannot be touched
// by a Gaussian (or are all finished) is skipped with a scalar branch.
//
// Queue.  The tile's depth-ordered list is consumed in batches of 64 (one Gaussian per
// lane).  Each lane tests its Gaussian against the four quadrants with an EXACT minimum of
// the conic's quadratic form over the quadrant's pixel-centre rectangle; Gaussians that
// cannot reach alpha >= 1/255 anywhere in the tile are dropped, survivors are compacted
// into a wave-private LDS queue with ballot + mbcnt, and the wave then walks the queue with
// broadcast ds_read_b128 (the forward keeps the four quadrants' lane masks in SGPRs and tests them at the entry's lane;
// the backward reads the entry's own mask).  Dropping a Gaussian never changes a pixel: every pixel it would
// have evaluated fails the alpha >= 1/255 test of A.2 step 9.  No workgroup barrier exists
// anywhere in the kernel.
#ifndef MGS_RASTER_COMMON_H_
#define MGS_RASTER_COMMON_H_

#include "mgs_common.h"

namespace mgs {

constexpr float kAlphaMin = 1.0f / 255.0f;
constexpr float kAlphaMax = 0.999f;
constexpr float kTStop = 1e-4f;
constexpr int kQueue = 64;
constexpr float kLog2e = 1.4426950408889634f;   // the one definition: every kernel scales the conic with these bits (pair_power)

struct QuadRect { float x0, x1, y0, y1; };   // pixel-centre extents of an 8x8 quadrant

// ---- the cull: exact minimum of the conic's quadratic form over a rectangle of pixel centres ---------------
// Off the rectangle's interior the minimum lies on one of its four edges.  An edge lies on a LINE: a fixed offset e
// (line coordinate - mean) on the "u" axis with weight w_u, a free offset v in [lo, hi] on the "v" axis with weight
// w_v, cross term b.  Along the line sigma(v) = 0.5 w_u e^2 + v (0.5 w_v v + b e), smallest at v = k e with
// k = -b / w_v, clamped to the edge.  What depends on the line alone is computed once per line -- b e, k e and
// E = 0.5 w_u e^2 -- and an edge then costs one v_med3_f32 and two FMAs.  The 16 edges of a tile's four quadrants lie
// on only 8 lines.  (v_med3_f32 returns min3 when an operand is NaN and needs no canonicalising v_max of its inputs;
// a NaN mean or conic still makes every edge value NaN through b e or E, and NaN keeps the quadrant.)
struct EdgeLine { float be, ke, E; };
__device__ __forceinline__ EdgeLine edge_line(float e, float b, float k, float half_wu) {
  return EdgeLine{b * e, k * e, (half_wu * e) * e};
}
__device__ __forceinline__ float edge_min_sigma(const EdgeLine& l, float half_wv, float lo, float hi) {
  const float v = __builtin_amdgcn_fmed3f(l.ke, lo, hi);
  return fmaf(v, fmaf(half_wv, v, l.be), l.E);
}

// min over the rectangle of 0.5*(a dx^2 + c dy^2) + b dx dy, (dx,dy) = p - mean.
__device__ __forceinline__ float rect_min_sigma(float mx, float my, float a, float b, float c,
                                                float inv_a, float inv_c, const QuadRect& r) {
  float lx = r.x0 - mx, hx = r.x1 - mx, ly = r.y0 - my, hy = r.y1 - my;
  if (lx <= 0.f && hx >= 0.f && ly <= 0.f && hy >= 0.f) return 0.f;
  const float ha = 0.5f * a, hc = 0.5f * c, kx = -b * inv_c, ky = -b * inv_a;
  float s0 = edge_min_sigma(edge_line(lx, b, kx, ha), hc, ly, hy);
  float s1 = edge_min_sigma(edge_line(hx, b, kx, ha), hc, ly, hy);
  float s2 = edge_min_sigma(edge_line(ly, b, ky, hc), ha, lx, hx);
  float s3 = edge_min_sigma(edge_line(hy, b, ky, hc), ha, lx, hx);
  return fminf(fminf(s0, s1), fminf(s2, s3));
}

// The cull's opacity gate.  alpha <= opacity, but only in exact arithmetic: log2(opacity) and the exponent's polynomial
// round, and the blend's fp32 alpha does come out at 1/255 at the mean of a Gaussian whose opacity is an ulp short of
// it (tests/test_cull_host.py).  The polynomial's terms reach |A| m^2 ~ 2e4 for a mean 60 px from the tile centre, five
// roundings of that are 6e-3 in the exponent, 0.4 % in alpha: the gate sits 5 % below 1/255 -- the constant part of
// the cull's slack -- and opacities between there and 1/255 are judged like any other, by lim.  False for NaN.
__device__ __forceinline__ bool cull_opacity_ok(float opac) { return opac >= 0.95f * kAlphaMin; }

// reach[k] = the lanes of the wave whose Gaussian (`valid`: the lane holds one) may reach alpha >= 1/255 at some pixel
// centre of quadrant k, for the quadrants that still have an open pixel (bit k of the wave-uniform `live`; 0 for the
// others).  Conservative by `slack` (fp32 rounding of both this test and the per-pixel sigma).  Lane masks, not a
// per-lane bit mask: the compares leave them in SGPRs, where the forward's walk tests them at an entry's lane.
// The line offsets are d + 0.5, 7.5, 8.5, 15.5 with d = tile corner - mean: two roundings instead of the one of
// (corner + offset) - mean, each at most half an ulp of an offset no larger than f = max(|d|, |d + 16|), so sigma
// moves by at most (|a| + |b|) f * 1.2e-7 f -- a thirtieth of the slack's relative term.  (f as |d + 8| + 8: the same
// number without fmaxf's canonicalising v_max of an operand from another basic block.)
// The two lines of a tile column (row) serve the two quadrants of that column (row): the columns come first and
// leave each live quadrant's smaller edge value in s_k, the rows finish it.  The arithmetic of a quadrant that is not
// live is skipped with scalar branches (s_k is read only under the bit it was written under).  No lane leaves EXEC.
__device__ __forceinline__ void quadrant_reach(float mx, float my, float a, float b, float c, float opac, bool valid,
                                               float tile_x, float tile_y, unsigned live,
                                               unsigned long long (&reach)[4]) {
  // (Every condition below is the ballot of ONE compare, combined as 64-bit integers: a ballot of a combined condition
  //  costs a v_cndmask and a v_cmp to rebuild the lane mask, and as a condition of the quadrants' arithmetic `ok`
  //  would put it behind a divergent branch.)
  const unsigned long long ok = ballot(valid) & ballot(cull_opacity_ok(opac));
  // (one v_log_f32: __logf compiles to the denormal-safe sequence of fourteen; 255 opac >= 0.95 where it counts, and
  //  the slack below is five orders above the instruction's error)
  const float thr = 0.6931471805599453f * __builtin_amdgcn_logf(255.0f * opac);
  // (v_rcp_f32, not the IEEE divide's eleven instructions each: the reciprocals only place the clamped minimiser on an
  //  edge, where the quadratic is flat to second order -- a 1-ulp reciprocal moves sigma by ~1e-13 relative, the test
  //  below carries a slack of 0.05; profiles/r5/00_experiments.md section 21)
  const float kx = -b * __builtin_amdgcn_rcpf(c), ky = -b * __builtin_amdgcn_rcpf(a);
  const float ha = 0.5f * a, hc = 0.5f * c;
  const float dx = tile_x - mx, dy = tile_y - my;
  const float fx = fabsf(dx + 8.f) + 8.f, fy = fabsf(dy + 8.f) + 8.f;
  const float slack = 0.05f + 4e-6f * (fabsf(a) + fabsf(c) + 2.f * fabsf(b)) * (fx * fx + fy * fy);
  const float lim = thr + slack;
  const float ex[4] = {dx + 0.5f, dx + 7.5f, dx + 8.5f, dx + 15.5f};
  const float ey[4] = {dy + 0.5f, dy + 7.5f, dy + 8.5f, dy + 15.5f};
  // the mean lies between the two lines of column g / row g: with both, inside the rectangle, where the minimum is 0
  const unsigned long long in_x[2] = {ballot(ex[0] <= 0.f) & ballot(ex[1] >= 0.f), ballot(ex[2] <= 0.f) & ballot(ex[3] >= 0.f)};
  const unsigned long long in_y[2] = {ballot(ey[0] <= 0.f) & ballot(ey[1] >= 0.f), ballot(ey[2] <= 0.f) & ballot(ey[3] >= 0.f)};
  float s0, s1, s2, s3;
  auto column = [&](int g, float& s_top, float& s_bottom) {      // quadrants g and g + 2
    if (live & (5u << g)) {
      const EdgeLine l0 = edge_line(ex[2 * g], b, kx, ha), l1 = edge_line(ex[2 * g + 1], b, kx, ha);
      if (live & (1u << g)) s_top = fminf(edge_min_sigma(l0, hc, ey[0], ey[1]), edge_min_sigma(l1, hc, ey[0], ey[1]));
      if (live & (4u << g)) s_bottom = fminf(edge_min_sigma(l0, hc, ey[2], ey[3]), edge_min_sigma(l1, hc, ey[2], ey[3]));
    }
  };
  auto row = [&](int g, float s_left, float s_right, unsigned long long& r_left, unsigned long long& r_right) {   // 2 g, 2 g + 1
    r_left = r_right = 0ull;
    if (live & (3u << (2 * g))) {
      const EdgeLine l0 = edge_line(ey[2 * g], b, ky, hc), l1 = edge_line(ey[2 * g + 1], b, ky, hc);
      if (live & (1u << (2 * g))) {
        const float s = fminf(s_left, fminf(edge_min_sigma(l0, ha, ex[0], ex[1]), edge_min_sigma(l1, ha, ex[0], ex[1])));
        r_left = ok & ((in_x[0] & in_y[g]) | ~ballot(s > lim));           // NaN keeps the quadrant
      }
      if (live & (2u << (2 * g))) {
        const float s = fminf(s_right, fminf(edge_min_sigma(l0, ha, ex[2], ex[3]), edge_min_sigma(l1, ha, ex[2], ex[3])));
        r_right = ok & ((in_x[1] & in_y[g]) | ~ballot(s > lim));
      }
    }
  };
  column(0, s0, s2);
  column(1, s1, s3);
  row(0, s0, s1, reach[0], reach[1]);
  row(1, s2, s3, reach[2], reach[3]);
}

// the same for one lane: bit k <=> this lane's Gaussian reaches (live) quadrant k
__device__ __forceinline__ unsigned quadrant_mask(float mx, float my, float a, float b, float c, float opac,
                                                  float tile_x, float tile_y, unsigned live = 0xfu) {
  unsigned long long reach[4];
  quadrant_reach(mx, my, a, b, c, opac, true, tile_x, tile_y, live, reach);
  unsigned m = 0;
#pragma unroll
  for (int k = 0; k < 4; ++k) m |= __builtin_amdgcn_inverse_ballot_w64(reach[k]) ? 1u << k : 0u;
  return m;
}

// The blend skips a pair whose sigma comes out negative (A.2 step 9).  For a positive definite conic
// that can only be a rounding artefact, and only if sigma is tiny against its own terms: with
// S = 0.5 (|a| dx^2 + |c| dy^2) + |b dx dy|, sigma >= (lambda_min / 2 lambda_max) S while fp32 evaluates
// it to within ~6e-7 S.  A conic with lambda_min / lambda_max >= 1e-4 (det >= 1e-4 trace^2) can therefore
// never produce sigma < 0 and the test is dead for it.  When every queued conic of a 64-entry batch is
// such (nearly always) the batch is walked by a copy of the loop without the test: one compare and one
// scalar AND less per 64 pairs; a batch holding a needle-like conic keeps the full test.  Results are identical
// (the exponent below is evaluated by the same expression either way).
__device__ __forceinline__ bool sigma_sign_is_safe(float a, float b, float c) {
  const float tr = a + c;
  return a > 0.f && c > 0.f && fmaf(a, c, -b * b) >= 1e-4f * tr * tr;     // false for NaN
}

// ---- alpha of one pixel-Gaussian pair, shared bit for bit by the forward and the backward ------------------
// The queue entry carries the conic pre-scaled by -log2(e) (A = -0.5 log2e a, B = -log2e b, C = -0.5 log2e c) and
// L = log2(opacity), so that   opacity * exp(-sigma) = exp2(A dx^2 + B dx dy + C dy^2 + L)
// is ONE v_exp_f32 of ONE fused expression: L rides in the addend of the last-but-one FMA (no multiply by the
// opacity afterwards).  `pair_power` is that exponent; `pair_power_sign` is the same expression without L, needed
// only where sigma >= 0 must be tested (conics that are not sigma_sign_is_safe).
__device__ __forceinline__ float pair_power(float dx, float dy, float A, float B, float C, float L) {
  return fmaf(dx, fmaf(B, dy, A * dx), fmaf(C * dy, dy, L));
}
__device__ __forceinline__ float pair_power_sign(float dx, float dy, float A, float B, float C) {
  return fmaf(dx, fmaf(B, dy, A * dx), (C * dy) * dy);
}
// The same exponent as a polynomial in the pixel's offset (x, y) from the TILE CENTRE (half-integers up to 7.5: x,
// y, x^2, x y, y^2 are exact per-lane constants).  With m = mean - centre,
//   A (m_x - x)^2 + B (m_x - x)(m_y - y) + C (m_y - y)^2 + L  =  q0 + q1 x + q2 y + A x^2 + B x y + C y^2,
//   q0 = pair_power(m_x, m_y, A, B, C, L),  q1 = -(2 A m_x + B m_y),  q2 = -(2 C m_y + B m_x):
// five FMAs per pair and no subtraction of the mean (the q's cost a dozen instructions per QUEUED Gaussian, one lane
// each).  Evaluation error against exact arithmetic on the same fp32 inputs: median 2e-7, 99.99 % under 6e-6, worst
// 1.2e-5 relative in alpha over 4.4 M visible pairs of the configs[1] scene (the dx / dy form: 7e-8 / 1.2e-6 / 1.1e-5)
// -- both far below what the fp32 rounding of mean2d itself costs (median 8e-6, worst 1.9e-4).  Every kernel that
// needs the alpha of a (Gaussian, pixel) pair -- both forward schedules and the backward -- evaluates exactly this
// chain on exactly these coefficients: same bits everywhere.
struct PolyCoef { float q0, q1, q2; };
__device__ __forceinline__ PolyCoef poly_coefs(float m_x, float m_y, float A, float B, float C, float L) {
  PolyCoef q;
  q.q0 = pair_power(m_x, m_y, A, B, C, L);
  q.q1 = -fmaf(2.f * A, m_x, B * m_y);
  q.q2 = -fmaf(2.f * C, m_y, B * m_x);
  return q;
}
struct PixelPoly { float x, y, xx, xy, yy; };       // offsets from the tile centre and their products (exact)
__device__ __forceinline__ PixelPoly pixel_poly(float x, float y) { return PixelPoly{x, y, x * x, x * y, y * y}; }
__device__ __forceinline__ float pair_power_poly(const PixelPoly& p, float q0, float q1, float q2, float A, float B,
                                                 float C) {
  return fmaf(C, p.yy, fmaf(B, p.xy, fmaf(A, p.xx, fmaf(q2, p.y, fmaf(q1, p.x, q0)))));
}

// Batches whose queued Gaussians all have a well conditioned conic AND an opacity <= kSafeOpacity are walked
// without the sigma >= 0 test and without the 0.999 clamp: exp2(power + L) <= opacity (1 + 2^-22) < 0.999.
constexpr float kSafeOpacity = 0.998f;
// The bound above holds for the polynomial about the tile centre while its absolute error ~2^-24 |A| m^2 (m <= ~11 px)
// stays far below 2^-10: conics of the default eps2d = 0.3 have a, c <= 3.4.  A caller with a tiny eps2d can hand over
// conics of 1e3 and more; those take the clamped, sign-tested body (a + c <= 8 is always true at eps2d >= 0.25).
constexpr float kSafeConicTrace = 8.0f;
__device__ __forceinline__ bool entry_is_safe(float a, float b, float c, float op) {
  return sigma_sign_is_safe(a, b, c) && op <= kSafeOpacity && a + c <= kSafeConicTrace;
}

// ---- forward checkpoints for the segmented backward ---------------------------------------------------------
// A tile's list is cut into SEGMENTS of S = 1 << shift entries (S a multiple of the 64-entry batch, aligned to the
// list's start, so the batches -- and with them every queue and every per-entry value -- are those of the unsegmented
// walk).  The training forward stores, at the first batch of every segment s >= 1 that some pixel of the block still
// reaches, the per-pixel state in front of that batch -- T and the accumulated channels -- and the backward then walks
// every segment as an independent unit of work: a segment that has a successor starts from the successor's
// checkpoint (T as stored; colour behind = final - checkpoint) instead of from the far end of the list.
// Unit of (tile t, segment s) = (start_t >> shift) + t + s: injective (floor((a + L) / S) - floor(a / S) >=
// ceil(L / S) - 1), bounded by (capacity >> shift) + n_tiles, and needs no prefix sum over the tiles.
// Layout: checkpoints[unit][1 + channels][256] floats, pixel k * 64 + lane of the tile (quadrant k, raster_common.h),
// behind a header of 4 int32 per tile: the largest last_id of each of the tile's four 8x8 blocks (-1: not written by
// this forward schedule) -- where the backward's walk of the tile ends, known before any pixel is loaded.
__host__ __device__ constexpr size_t ckpt_units(uint32_t capacity, int n_tiles, int shift) {
  return ((size_t)capacity >> shift) + (size_t)n_tiles + 1;
}
__host__ __device__ constexpr size_t ckpt_header_floats(int n_tiles) { return ((size_t)n_tiles * 4 + 255) / 256 * 256; }
__device__ __forceinline__ size_t ckpt_unit(int start, int tile, int seg, int shift) {
  return (size_t)(start >> shift) + (size_t)tile + (size_t)seg;
}

#if defined(__HIPCC__)     // (below: wave-level helpers; the geometry above also compiles for the host, tests/test_cull_host.py)
// A queue entry part is read from LDS as ONE ds_read_b128: an empty asm that "uses" all four lanes of the register
// tuple keeps the compiler from narrowing the load to the components the caller happens to touch (it split a 16-byte
// read into b64 + b32 + 2 x read2_b32: five LDS instructions per entry instead of three).
typedef float mgs_f4 __attribute__((ext_vector_type(4)));
__device__ __forceinline__ void lds_read_3f4(const float4* pa, const float4* pb, const float4* pc, float4& a, float4& b,
                                             float4& c) {
  mgs_f4 va = *reinterpret_cast<const mgs_f4*>(pa), vb = *reinterpret_cast<const mgs_f4*>(pb),
         vc = *reinterpret_cast<const mgs_f4*>(pc);
  asm volatile("" : "+v"(va), "+v"(vb), "+v"(vc));      // (one statement: the three reads stay in flight together)
  a = make_float4(va.x, va.y, va.z, va.w);
  b = make_float4(vb.x, vb.y, vb.z, vb.w);
  c = make_float4(vc.x, vc.y, vc.z, vc.w);
}

// ---- what the kernels that walk a camera's tile lists share (raster_fwd.hip, raster_bwd.hip, weight_walk.h) ----------
// The lane's tile: one wave owns one 16x16 tile, lane l holds the pixel (l & 7, l >> 3) of each 8x8 quadrant.
struct TileFrame {
  int tx, ty;                        // the tile's column and row
  float tile_x, tile_y;              // its corner, in pixels
  float ctr_x, ctr_y;                // its centre
  int ix, iy;                        // pixel centres of quadrant 0; quadrant k adds (8*(k&1), 8*(k>>1))
  PixelPoly pq[4];                   // offsets of the lane's four pixels from the tile centre, and their products
};
__device__ __forceinline__ TileFrame tile_frame(int tile, int tile_w, unsigned lane) {
  TileFrame f;
  f.tx = tile % tile_w; f.ty = tile / tile_w;
  f.tile_x = (float)(f.tx * 16); f.tile_y = (float)(f.ty * 16);
  f.ctr_x = f.tile_x + 8.f; f.ctr_y = f.tile_y + 8.f;
  f.ix = f.tx * 16 + (int)(lane & 7); f.iy = f.ty * 16 + (int)(lane >> 3);
  const float xo = (float)(lane & 7) - 7.5f, yo = (float)(lane >> 3) - 7.5f;
#pragma unroll
  for (int k = 0; k < 4; ++k) f.pq[k] = pixel_poly(xo + 8.f * (k & 1), yo + 8.f * (k >> 1));
  return f;
}

// Gaussian g's mean, conic and opacity: the first two quarters of the packed 48-byte record, or the separate arrays.
__device__ __forceinline__ void load_geometry(int g, const float4* __restrict__ splats, const float* __restrict__ means2d,
                                              const float* __restrict__ conics, const float* __restrict__ opacities,
                                              float2& xy, float& a, float& b, float& c, float& op) {
  if (splats) {
    const float4 p0 = splats[3 * (size_t)g], p1 = splats[3 * (size_t)g + 1];
    xy = make_float2(p0.x, p0.y);
    a = p0.z; b = p0.w; c = p1.x; op = p1.y;
  } else {
    xy = reinterpret_cast<const float2*>(means2d)[g];
    a = conics[3 * (size_t)g + 0];
    b = conics[3 * (size_t)g + 1];
    c = conics[3 * (size_t)g + 2];
    op = opacities[g];
  }
}

// The rest of the record: its four features and, for a caller that wants them, the two words mgs_isect_tiles leaves
// behind them (the record slots).
__device__ __forceinline__ void load_record_tail(int g, const float4* __restrict__ splats, float (&f)[4],
                                                 float2* slot_words = nullptr) {
  const float4 p1 = splats[3 * (size_t)g + 1], p2 = splats[3 * (size_t)g + 2];
  f[0] = p1.z; f[1] = p1.w; f[2] = p2.x; f[3] = p2.y;
  if (slot_words) *slot_words = make_float2(p2.z, p2.w);
}

// The geometry of a queue entry: the conic pre-scaled by -log2 e, the mean relative to the tile centre, L = log2(opacity)
// and the exponent's polynomial about the centre (pair_power, poly_coefs).  Every walker queues exactly these expressions.
struct QueueGeo {
  float4 geo0;                       // q0, q1, q2, A
  float sB, sC, m_x, m_y, L;
};
__device__ __forceinline__ QueueGeo queue_geometry(float2 xy, float a, float b, float c, float op, float ctr_x, float ctr_y) {
  QueueGeo q;
  const float sA = -0.5f * kLog2e * a;
  q.sB = -kLog2e * b; q.sC = -0.5f * kLog2e * c; q.L = __log2f(op);
  q.m_x = xy.x - ctr_x; q.m_y = xy.y - ctr_y;
  const PolyCoef pc = poly_coefs(q.m_x, q.m_y, sA, q.sB, q.sC, q.L);
  q.geo0 = make_float4(pc.q0, pc.q1, pc.q2, sA);
  return q;
}

// A Gaussian's CHT features as the queue entry's float4[(CHT + 3) / 4] (padded with zeros), and back.
template <int CHT>
__device__ __forceinline__ void pack_features(const float (&f)[CHT], float4 (&out)[(CHT + 3) / 4]) {
#pragma unroll
  for (int j = 0; j < (CHT + 3) / 4; ++j)
    out[j] = make_float4(f[4 * j], 4 * j + 1 < CHT ? f[4 * j + 1] : 0.f, 4 * j + 2 < CHT ? f[4 * j + 2] : 0.f,
                         4 * j + 3 < CHT ? f[4 * j + 3] : 0.f);
}
template <int CHT>
__device__ __forceinline__ void unpack_features(const float4* in, float (&f)[CHT]) {
#pragma unroll
  for (int j = 0; j < (CHT + 3) / 4; ++j) {
    const float4 v = in[j];
    f[4 * j] = v.x;
    if (4 * j + 1 < CHT) f[4 * j + 1] = v.y;
    if (4 * j + 2 < CHT) f[4 * j + 2] = v.z;
    if (4 * j + 3 < CHT) f[4 * j + 3] = v.w;
  }
}

// full-wave sum: result valid in lane 63
__device__ __forceinline__ float wave_reduce_to_lane63(float v) {
  int i;
#define MGS_DPP_ADD(CTRL, RMASK)                                                               \
  i = __builtin_amdgcn_update_dpp(0, __float_as_int(v), CTRL, RMASK, 0xf, false);              \
  v += __int_as_float(i);
  MGS_DPP_ADD(0xB1, 0xf)    // quad_perm [1,0,3,2]
  MGS_DPP_ADD(0x4E, 0xf)    // quad_perm [2,3,0,1]
  MGS_DPP_ADD(0x141, 0xf)   // row_half_mirror
  MGS_DPP_ADD(0x140, 0xf)   // row_mirror
  MGS_DPP_ADD(0x142, 0xa)   // row_bcast15 -> rows 1,3
  MGS_DPP_ADD(0x143, 0xc)   // row_bcast31 -> rows 2,3
#undef MGS_DPP_ADD
  return v;
}


// ---- reduce-scatter butterfly over the wave ----------------------------------------------
// Sums V values (V = 8, 4, 2 or 1) held by every lane over all 64 lanes in about 3V + 5
// instructions instead of 6V.  Scatter steps halve the value count while pairing lanes over
// lane bits 0, 1 and 3 (xor 1 / xor 2 via quad_perm, xor 8 via row_ror:8): a lane keeps the
// half selected by its own bit and adds the partner's copy of that half.  The remaining lane
// bits are then summed with plain shifted adds.  The total of value i ends in the lane of row 0
// with (bit0, bit1, bit3) spelling i as  i = bit3 + 2*bit1 + 4*bit0  (V = 8),
// i = bit1 + 2*bit0 (V = 4), i = bit0 (V = 2), lane 0 (V = 1), and lane bits 2, 4, 5 clear.
__device__ __forceinline__ float dpp_f(float x, int ctrl) {   // ctrl must fold to a constant
  switch (ctrl) {
    case 0xB1: return __int_as_float(__builtin_amdgcn_update_dpp(0, __float_as_int(x), 0xB1, 0xf, 0xf, false));
    case 0x4E: return __int_as_float(__builtin_amdgcn_update_dpp(0, __float_as_int(x), 0x4E, 0xf, 0xf, false));
    case 0x128: return __int_as_float(__builtin_amdgcn_update_dpp(0, __float_as_int(x), 0x128, 0xf, 0xf, false));
    default: return __int_as_float(__builtin_amdgcn_update_dpp(0, __float_as_int(x), 0x104, 0xf, 0xf, false));
  }
}
constexpr int kDppXor1 = 0xB1, kDppXor2 = 0x4E, kDppRor8 = 0x128, kDppShl4 = 0x104;

template <int V>
__device__ __forceinline__ float wave_reduce_scatter(const float* v, unsigned lane) {
  static_assert(V == 8 || V == 4 || V == 2 || V == 1, "V must be 8, 4, 2 or 1");
  const bool b0 = lane & 1u, b1 = lane & 2u, b3 = lane & 8u;
  float t;
  if constexpr (V == 8) {
    float w[4], u[2];
#pragma unroll
    for (int i = 0; i < 4; ++i) w[i] = (b0 ? v[i + 4] : v[i]) + dpp_f(b0 ? v[i] : v[i + 4], kDppXor1);
#pragma unroll
    for (int i = 0; i < 2; ++i) u[i] = (b1 ? w[i + 2] : w[i]) + dpp_f(b1 ? w[i] : w[i + 2], kDppXor2);
    t = (b3 ? u[1] : u[0]) + dpp_f(b3 ? u[0] : u[1], kDppRor8);
  } else if constexpr (V == 4) {
    float u[2];
#pragma unroll
    for (int i = 0; i < 2; ++i) u[i] = (b0 ? v[i + 2] : v[i]) + dpp_f(b0 ? v[i] : v[i + 2], kDppXor1);
    t = (b1 ? u[1] : u[0]) + dpp_f(b1 ? u[0] : u[1], kDppXor2);
    t += dpp_f(t, kDppRor8);
  } else if constexpr (V == 2) {
    t = (b0 ? v[1] : v[0]) + dpp_f(b0 ? v[0] : v[1], kDppXor1);
    t += dpp_f(t, kDppXor2);
    t += dpp_f(t, kDppRor8);
  } else {
    t = v[0] + dpp_f(v[0], kDppXor1);
    t += dpp_f(t, kDppXor2);
    t += dpp_f(t, kDppRor8);
  }
  t += dpp_f(t, kDppShl4);             // lane bit 2 (valid where bit 2 is clear)
  t += __shfl_down(t, 16);             // rows 1,3 into rows 0,2
  t += __shfl_down(t, 32);             // row 2 into row 0
  return t;
}
// which value index a holder lane (row 0, bit 2 clear) carries; -1 for other lanes
template <int V>
__device__ __forceinline__ int wave_reduce_scatter_index(unsigned lane) {
  if (lane & ~0xBu) return -1;         // only lanes 0,1,2,3,8,9,10,11 can hold a total
  const int b0 = lane & 1, b1 = (lane >> 1) & 1, b3 = (lane >> 3) & 1;
  if (V == 8) return b3 + 2 * b1 + 4 * b0;
  if (V == 4) return b3 ? -1 : b1 + 2 * b0;
  if (V == 2) return (b3 || b1) ? -1 : b0;
  return lane == 0 ? 0 : -1;
}

#endif  // __HIPCC__

}  // namespace mgs
#endif
