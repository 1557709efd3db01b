// raster_fwd.hip -- per-tile depth-ordered alpha compositing, forward (A.2 step 9), gfx950.
// Geometry, queue and culling: raster_common.h.  Not bandwidth-bound: 15 vector instructions per 64 pixel-Gaussian
// pairs (five FMAs for the exponent's polynomial about the tile centre, v_exp, the alpha test and the T (1 - alpha) > 1e-4
// test as v_cmpx under an EXEC that starts as the quadrant's open pixels, one move, the colour FMAs: 12 FMA-class + 2
// compare-class + one v_exp = 45 cycles by scripts/ubench/valu_issue.hip) against 44 bytes per tile-Gaussian pair, so
// the design spends its effort on evaluating
// fewer pairs, on cheaper evaluations and on keeping enough waves resident, not on moving bytes.  Two schedules of the
// same blend: raster_fwd_kernel (one wave per 16x16 tile, four pixels per lane: fewest instructions, what several
// frames in flight run) and raster_fwd_q_kernel (one wave per 8x8 block: shortest launch); DESIGN.md 4.3.
#include <type_traits>

#include "raster_common.h"
#include "tile_order.h"
#include "dataset_pixel.h"

namespace mgs {
namespace {

// min waves per SIMD asked of the register allocator (one-wave-per-tile kernel).  5 = at most 96 VGPRs: with the
// hand-written blend body the 4-channel kernels sat at 106-107 registers (4 waves) -- at 5 the same box renders
// 3,818 instead of 3,674 frames/s with three frames in flight (189.5 vs 191.6 us alone); 6 (80 VGPRs) spills: 3,571
constexpr int kFwdMinWaves = 5;
// Independent tiles (waves) per workgroup of the INFERENCE variant; no workgroup barrier is ever
// used.  One-wave workgroups grab every wave slot the moment it frees up and starve the 4-wave
// workgroups of the other frames' binning kernels, which need four slots on one CU at once; with
// 4 tiles per workgroup the frames in flight interleave better: 2873 -> 2956 frames/s (8 / 16
// tiles: 2858 / 2832, load imbalance).  A lone launch is 3 % slower that way (the workgroup lives
// as long as its heaviest tile), so the training variant, which runs alone, keeps one tile.
constexpr int kFwdWgWaves = 4;

template <int CHT>
struct QueueEntry {
  float4 geo0;                       // q0, q1, q2, A   (raster_common.h: poly_coefs; A,B,C: conic pre-scaled)
  float4 geo1;                       // B, C, unused (0), list index (bits)
  float4 feat[(CHT + 3) / 4];
  float4 geo3;                       // mean - tile centre (x, y): written and read only by batches that test sigma >= 0
};

// Per-pixel state.  Two ways to remember that a pixel is finished (A.2 step 9's "done" flag):
//   * sign of T (kernels without the hand-written body): T > 0 open, T < 0 finished with |T| its final transmittance --
//     no separate flag, and a finished pixel can never accumulate again: T*(1-alpha) < 0 < 1e-4;
//   * `alive` (kMasks kernels: 3 and 4 channels): one 64-bit lane mask per quadrant in SGPRs, T stays positive.  The
//     blend runs with EXEC = alive & (alpha >= 1/255) & (T (1 - alpha) > 1e-4), so "finished" costs no vector
//     instruction at all -- the sign form pays a compare-class select on w and one on T per 64 pairs.
template <int CHT>
struct PixelState {
  float T;
  float C[CHT];
  int last;
#ifdef MGS_RASTER_STATS
  unsigned n_valid = 0, n_acc = 0;
#endif
};

#ifdef MGS_RASTER_STATS
// Instrumented build only (python robosimgs_amd/csrc/build.py with MGS_EXTRA_FLAGS=-DMGS_RASTER_STATS):
// counts the work the forward raster really does; read back with mgs_debug_read_raster_stats().
//   0 list entries fetched   1 entries queued after the cull   2 quadrant evaluations (x64 lanes)
//   3 lanes with a valid alpha   4 lanes accumulated   5 batches processed   6 batches in lists
__device__ unsigned long long g_raster_stats[8];
#define MGS_STAT(i, v) stat[i] += (v)
#else
#define MGS_STAT(i, v)
#endif

// One Gaussian against the 64 pixels of one quadrant (one pixel per lane).
//   alpha = opacity exp(-sigma) = exp2(A dx^2 + C dy^2 + B dx dy + L)  with  A = -0.5 log2e a, B = -log2e b,
//   C = -0.5 log2e c, L = log2(opacity): one v_exp_f32, no multiply by the opacity (raster_common.h pair_power);
//   "sigma >= 0" is "pair_power_sign <= 0".
// TRACK_LAST: record the list index of the last blended Gaussian (the backward starts there);
// an inference render drops that select (compares / selects issue at half the FMA rate on gfx950).
template <int CHT, bool TRACK_LAST, bool SAFE = false, bool MASKS = false>
__device__ __forceinline__ void blend_pixel(PixelState<CHT>& px, unsigned long long& alive, const PixelPoly& pp, float q0,
                                            float q1, float q2, float A, float B, float C, float m_x, float m_y,
                                            const float* feat, int idx) {
  // SAFE: the conic cannot round sigma below zero (sigma_sign_is_safe) and opacity <= kSafeOpacity: the sigma test
  // is dead and exp2(power) <= opacity (1 + 2^-22) < 0.999, so the clamp is the identity too
  const float ov = __builtin_amdgcn_exp2f(pair_power_poly(pp, q0, q1, q2, A, B, C));   // the backward repeats it bit for bit
  float alpha = SAFE ? ov : fminf(kAlphaMax, ov);
  bool valid = alpha >= kAlphaMin;
  if (!SAFE) valid = valid && pair_power_sign(m_x - pp.x, m_y - pp.y, A, B, C) <= 0.f;
  if (MASKS) valid = valid && __builtin_amdgcn_inverse_ballot_w64(alive);     // the mask IS the condition register
  // alpha forced to 0 where the Gaussian does not count: an open pixel (T > 1e-4 by invariant)
  // then keeps T and adds nothing, with no second mask to combine
  float a_eff = valid ? alpha : 0.f;
  float next_T = fmaf(-a_eff, px.T, px.T);
  bool acc = next_T > kTStop;                     // false for the closing Gaussian (and, in the sign form, for finished pixels)
  float w = a_eff * px.T;
  w = acc ? w : 0.f;      // (w = |T| - |T_new| -- a subtraction instead of a multiply and a select -- puts the weight
                          //  behind the T select on the dependency chain: measured 218 -> 226 us, 3,575 -> 3,417 frames/s)
#pragma unroll
  for (int c = 0; c < CHT; ++c) px.C[c] = fmaf(w, feat[c], px.C[c]);
  if (MASKS) {
    px.T = acc ? next_T : px.T;                   // a pixel this Gaussian closes keeps the T it had and leaves the mask
    alive &= ~ballot(!acc);
  } else {
    px.T = acc ? next_T : -fabsf(px.T);           // not accumulated: the pixel is (or stays) finished
  }
  if (TRACK_LAST) px.last = (acc && valid) ? idx : px.last;
#ifdef MGS_RASTER_STATS
  px.n_valid += valid && px.T > 0.f;
  px.n_acc += acc && valid;
#endif
}

// Kernels of 3 and 4 channels keep "finished" in lane masks (PixelState above) and run the SAFE blend as the
// hand-written body below.
template <int CHT>
constexpr bool kMasks = CHT == 3 || CHT == 4;

// The SAFE blend (3 or 4 channels; inference and, with one more move for last_ids, training) as hand-written gfx950
// code: the same arithmetic in the same order as blend_pixel<CHT, ., true> -- bit-identical pixels -- under an EXEC that
// is narrowed three times instead of selects: to the quadrant's open pixels (s_mov from `alive`), by the alpha >= 1/255
// test (v_cmpx; a Gaussian that does not count leaves the pixel untouched) and by the T (1 - alpha) > 1e-4 test
// (v_cmpx again: what is left accumulates; the lanes the second test dropped -- vcc & ~exec -- are the pixels this
// Gaussian closes and leave `alive`).  On gfx9 a VOP3 v_cmpx writes a scalar destination as well as EXEC: the second
// one names EXEC itself, so no SGPR pair is spent on the accumulating lanes.
// 15 vector instructions per 64 pairs -- 12 FMA-class, two compares, one v_exp: 45 cycles by
// scripts/ubench/valu_issue.hip; the round-3 form with the sign of T as the flag had two selects more (16, 51 cycles).
// gfx940+ needs one wait state after a transcendental before its result is read (s_nop 0).
// Scalar issue slots per body: s_mov exec | s_nop | s_andn2 vcc | s_andn2 alive, and, per statement, s_mov exec, -1.
// MGS_SAFE_BODY(k) is that body on the operands of quadrant k; it leaves EXEC narrowed and SCC = "some pixel of the
// quadrant is still open".
#define MGS_SAFE_BODY(k)                                                                                   \
  "s_mov_b64 exec, %[alive" #k "]\n"                                                                       \
  "v_fma_f32 %[t1], %[q1], %[x" #k "], %[q0]\n"           /* pair_power_poly, same order */                \
  "v_fmac_f32 %[t1], %[q2], %[y" #k "]\n"                                                                  \
  "v_fmac_f32 %[t1], %[A], %[xx" #k "]\n"                                                                  \
  "v_fmac_f32 %[t1], %[B], %[xy" #k "]\n"                                                                  \
  "v_fmac_f32 %[t1], %[C], %[yy" #k "]\n"                                                                  \
  "v_exp_f32 %[t1], %[t1]\n"                                                                               \
  "s_nop 0\n"                                                                                              \
  "v_cmpx_le_f32 vcc, %[amin], %[t1]\n"                   /* EXEC = VCC = open pixels the Gaussian counts for */ \
  "v_fma_f32 %[t0], -%[t1], %[T" #k "], %[T" #k "]\n"                                                      \
  "v_mul_f32 %[dx], %[t1], %[T" #k "]\n"                                                                   \
  "v_cmpx_lt_f32_e64 exec, %[tstop], %[t0]\n"             /* EXEC = those of them that accumulate */       \
  "v_mov_b32 %[T" #k "], %[t0]\n"                                                                          \
  "v_fmac_f32 %[c0" #k "], %[dx], %[f0]\n"                                                                 \
  "v_fmac_f32 %[c1" #k "], %[dx], %[f1]\n"                                                                 \
  "v_fmac_f32 %[c2" #k "], %[dx], %[f2]\n"                                                                 \
  ".if %[four]\n"                                                                                          \
  "v_fmac_f32 %[c3" #k "], %[dx], %[f3]\n"                                                                 \
  ".endif\n"                                                                                               \
  ".if %[track]\n"                                                                                         \
  "v_mov_b32 %[last" #k "], %[idx]\n"                                                                      \
  ".endif\n"                                                                                               \
  "s_andn2_b64 vcc, vcc, exec\n"                          /* counted but not accumulated: the pixels this Gaussian closes */ \
  "s_andn2_b64 %[alive" #k "], %[alive" #k "], vcc\n"     /* (SCC = some pixel of the quadrant is still open) */
// One wave per tile: `quad` holds the lanes of the batch whose Gaussian reaches quadrant k and `at` the lane that queued
// this entry.  The body runs only if bit `at` of `quad` is set (s_bitcmp1_b64 and a branch over it), and `quad` is
// emptied the moment the quadrant's last pixel closes (one s_cselect_b64 on the SCC above), so that the rest of the batch
// skips the quadrant: scalar instructions only (re-deriving the live quadrants with ballots every 8 / 16 / 32 entries
// was a loss in round 3).
#define MGS_SAFE_WALK_BODY(k)                                                                              \
  "s_bitcmp1_b64 %[quad" #k "], %[at]\n"                                                                   \
  "s_cbranch_scc0 .Lmgs_next_quadrant" #k "_%=\n"                                                          \
  MGS_SAFE_BODY(k)                                                                                         \
  "s_cselect_b64 %[quad" #k "], %[quad" #k "], 0\n"                                                        \
  ".Lmgs_next_quadrant" #k "_%=:\n"
#define MGS_SAFE_STATE(k, px, alive_k, c3_k)                                                                            \
  [alive##k] "+s"(alive_k), [T##k] "+v"((px).T), [c0##k] "+v"((px).C[0]), [c1##k] "+v"((px).C[1]), [c2##k] "+v"((px).C[2]), \
  [c3##k] "+v"(c3_k), [last##k] "+v"((px).last)
#define MGS_SAFE_PIXEL(k, pp) [x##k] "v"((pp).x), [y##k] "v"((pp).y), [xx##k] "v"((pp).xx), [xy##k] "v"((pp).xy), [yy##k] "v"((pp).yy)
// dx: the weight w, t0: T (1 - alpha), t1: exponent, then alpha
#define MGS_SAFE_TEMPS [dx] "=&v"(dx), [t0] "=&v"(t0), [t1] "=&v"(t1)
#define MGS_SAFE_ENTRY                                                                                                     \
  [q0] "v"(q0), [q1] "v"(q1), [q2] "v"(q2), [A] "v"(A), [B] "v"(B), [C] "v"(C), [f0] "v"(feat[0]), [f1] "v"(feat[1]),       \
  [f2] "v"(feat[2]), [f3] "v"(f3), [amin] "s"(amin), [tstop] "s"(tstop), [four] "n"(CHT == 4 ? 1 : 0),                      \
  [track] "n"(TRACK_LAST ? 1 : 0), [idx] "v"(idx)

// One wave per 8x8 block: one body per queue entry.
template <int CHT, bool TRACK_LAST>
__device__ __forceinline__ void blend_pixel_safe_asm(PixelState<CHT>& px, unsigned long long& alive, const PixelPoly& pp,
                                                     float q0, float q1, float q2, float A, float B, float C,
                                                     const float* feat, int idx) {
  static_assert(CHT == 3 || CHT == 4, "hand-written blend: 3 or 4 channels");
  float dx, t0, t1;
  const float amin = kAlphaMin, tstop = kTStop;
  float c3 = CHT == 4 ? px.C[CHT - 1] : 0.f;
  const float f3 = CHT == 4 ? feat[CHT - 1] : 0.f;
  asm volatile(MGS_SAFE_BODY(0)
               "s_mov_b64 exec, -1\n"
               : MGS_SAFE_TEMPS, MGS_SAFE_STATE(0, px, alive, c3)
               : MGS_SAFE_ENTRY, MGS_SAFE_PIXEL(0, pp)
               : "vcc", "scc");            // (the s_andn2 write SCC: the loop counter's compare must not straddle the body)
  if (CHT == 4) px.C[CHT - 1] = c3;
}

// One wave per tile: the bodies of an entry's four quadrants as ONE statement.  EXEC is restored once, at its end (a
// skipped body leaves the EXEC of the one before it, and every body starts by setting its own), and the compiler's
// wait state between two asm statements that share a register -- an s_nop 0 in front of each, taken or skipped -- is
// paid once per entry instead of four times.  Measured against the one-statement-per-quadrant forms in
// scripts/ubench/blend_body_scalar.hip (profiles/raster_scalar/README.md).
template <int CHT, bool TRACK_LAST>
__device__ __forceinline__ void blend_entry_safe_asm(PixelState<CHT>* st, unsigned long long* alive, unsigned long long* quad,
                                                     int at, const PixelPoly* pq, float q0, float q1, float q2, float A,
                                                     float B, float C, const float* feat, int idx) {
  static_assert(CHT == 3 || CHT == 4, "hand-written blend: 3 or 4 channels");
  float dx, t0, t1;
  const float amin = kAlphaMin, tstop = kTStop;
  float c3[4];
#pragma unroll
  for (int k = 0; k < 4; ++k) c3[k] = CHT == 4 ? st[k].C[CHT - 1] : 0.f;
  const float f3 = CHT == 4 ? feat[CHT - 1] : 0.f;
  asm volatile(MGS_SAFE_WALK_BODY(0) MGS_SAFE_WALK_BODY(1) MGS_SAFE_WALK_BODY(2) MGS_SAFE_WALK_BODY(3)
               "s_mov_b64 exec, -1\n"
               : MGS_SAFE_TEMPS, MGS_SAFE_STATE(0, st[0], alive[0], c3[0]), MGS_SAFE_STATE(1, st[1], alive[1], c3[1]),
                 MGS_SAFE_STATE(2, st[2], alive[2], c3[2]), MGS_SAFE_STATE(3, st[3], alive[3], c3[3]),
                 [quad0] "+s"(quad[0]), [quad1] "+s"(quad[1]), [quad2] "+s"(quad[2]), [quad3] "+s"(quad[3])
               : MGS_SAFE_ENTRY, [at] "s"(at), MGS_SAFE_PIXEL(0, pq[0]), MGS_SAFE_PIXEL(1, pq[1]), MGS_SAFE_PIXEL(2, pq[2]),
                 MGS_SAFE_PIXEL(3, pq[3])
               : "vcc", "scc");
  if (CHT == 4) {
#pragma unroll
    for (int k = 0; k < 4; ++k) st[k].C[CHT - 1] = c3[k];
  }
}

// DATASET (4 channels, inference, "ED"): the epilogue writes the dataset frame the reference reads -- RGBA8 + ray distance,
// dataset_pixel.h -- instead of (or, when render / alphas are given, beside) the float frame: 6 - 12 bytes per pixel leave
// the kernel instead of 20, and no conversion pass reads them back.  A separate instantiation: the float-frame kernels'
// code is what it was.
struct NoDataset {};
// The epilogue of one pixel (x, y) inside the image, both schedules: background, "ED" division, the stores.
template <int CHT, bool TRACK_LAST, bool DATASET>
__device__ __forceinline__ void store_pixel(const PixelState<CHT>& st, int x, int y, int width, int channels,
                                            const float* __restrict__ background, int expected_last,
                                            float* __restrict__ render, float* __restrict__ alphas,
                                            int32_t* __restrict__ last_ids,
                                            const std::conditional_t<DATASET, DatasetOut, NoDataset>& ds) {
  const size_t p = (size_t)y * width + x;
  const float alpha = 1.0f - fabsf(st.T);
  // "ED": the last channel (depth sum) leaves as the expected depth, A.2 step 9
  const float inv_alpha = expected_last ? 1.0f / fmaxf(alpha, 1e-10f) : 1.0f;
  if constexpr (DATASET) {
    static_assert(CHT == 4 && !TRACK_LAST, "dataset epilogue: RGB + expected depth, inference");
    float v[4];
#pragma unroll
    for (int c = 0; c < 4; ++c) v[c] = st.C[c] + (background ? fabsf(st.T) * background[c] : 0.f);
    v[3] *= inv_alpha;
    dataset_store(ds, p, x, y, v[0], v[1], v[2], v[3], alpha);
    if (render) {
#pragma unroll
      for (int c = 0; c < 4; ++c) render[p * 4 + c] = v[c];
      alphas[p] = alpha;
    }
  } else {
#pragma unroll
    for (int c = 0; c < CHT; ++c)
      if (c < channels) {
        float v = st.C[c] + (background ? fabsf(st.T) * background[c] : 0.f);
        if (c == channels - 1) v *= inv_alpha;
        render[p * channels + c] = v;
      }
    alphas[p] = alpha;
    if (TRACK_LAST) last_ids[p] = st.last;
  }
}

template <int CHT, bool TRACK_LAST, bool DATASET = false>
__global__ __launch_bounds__(64 * (TRACK_LAST ? 1 : kFwdWgWaves), (CHT <= 4 ? kFwdMinWaves : 1)) void raster_fwd_kernel(
    const float* __restrict__ means2d, const float* __restrict__ conics,
    const float* __restrict__ feats, const float* __restrict__ opacities,
    const float4* __restrict__ splats, const float* __restrict__ background, int channels,
    int width, int height, int tile_w, int n_tiles, const int32_t* __restrict__ tile_offsets,
    const int32_t* __restrict__ flatten_ids, float* __restrict__ render,
    float* __restrict__ alphas, int32_t* __restrict__ last_ids, int cull, int expected_last, int opts,
    const int32_t* __restrict__ group_order, float* __restrict__ ckpt, int ckpt_shift,
    std::conditional_t<DATASET, DatasetOut, NoDataset> ds) {
  constexpr int kWgWaves = TRACK_LAST ? 1 : kFwdWgWaves;
  __shared__ QueueEntry<CHT> queues[kWgWaves][kQueue + 1];
  QueueEntry<CHT>* queue = queues[threadIdx.x >> 6];
  const int tile = tile_of_unit(blockIdx.x * kWgWaves + (int)(threadIdx.x >> 6), n_tiles, group_order);   // tile_order.h
  if (tile < 0) return;
  const unsigned lane = threadIdx.x & 63u;
  const TileFrame fr = tile_frame(tile, tile_w, lane);     // raster_common.h: the lane's four pixels, the tile's centre
  const int ix = fr.ix, iy = fr.iy;
  const int start = tile_offsets[tile], end = tile_offsets[tile + 1];
  if (opts & 1) {
    // Issue priority by list length.  A tile is one wave's serial job; while every SIMD is full each of
    // its five waves advances at a fifth of the SIMD's rate, so the longest lists -- started no earlier
    // than the others -- set the kernel's duration.  Waves with long lists get priority and finish at
    // their own issue limit; short ones fill the gaps.
    const int avg = (tile_offsets[n_tiles] - tile_offsets[0]) / n_tiles, len = end - start;   // this camera's own total
    if (len > 2 * avg) __builtin_amdgcn_s_setprio(3);
    else if (2 * len > 3 * avg) __builtin_amdgcn_s_setprio(2);
    else if (len > avg) __builtin_amdgcn_s_setprio(1);
  }

#ifdef MGS_RASTER_STATS
  unsigned long long stat[8] = {0, 0, 0, 0, 0, 0, 0, 0};
  stat[6] = (unsigned)(end - start + kQueue - 1) / kQueue;
#endif
  PixelState<CHT> st[4];
  unsigned long long alive[4];                   // kMasks: the quadrant's open pixels
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    const bool inside = ix + 8 * (k & 1) < width && iy + 8 * (k >> 1) < height;
    st[k].T = (inside || kMasks<CHT>) ? 1.f : -1.f;    // pixels outside the image start finished
    alive[k] = ballot(inside);
    st[k].last = 0;
#pragma unroll
    for (int c = 0; c < CHT; ++c) st[k].C[c] = 0.f;
  }

  // the batch registers: the list entries of the batch about to be queued (fetched when the batch starts)
  int r_idx = start + (int)lane;
  bool r_ok = r_idx < end;
  float2 r_xy = make_float2(0.f, 0.f);
  float r_ca = 1.f, r_cb = 0.f, r_cc = 1.f, r_op = 0.f;
  float r_feat[CHT];
#pragma unroll
  for (int c = 0; c < CHT; ++c) r_feat[c] = 0.f;
  auto fetch = [&](int idx, bool ok) {
    if (ok && CHT <= 4 && splats) {   // one packed 48-byte record instead of four gathers
      int g = flatten_ids[idx];
      float ff[4];
      load_geometry(g, splats, nullptr, nullptr, nullptr, r_xy, r_ca, r_cb, r_cc, r_op);
      load_record_tail(g, splats, ff);
#pragma unroll
      for (int c = 0; c < CHT; ++c) r_feat[c] = ff[c & 3];
    } else if (ok) {
      int g = flatten_ids[idx];
      load_geometry(g, nullptr, means2d, conics, opacities, r_xy, r_ca, r_cb, r_cc, r_op);
#pragma unroll
      for (int c = 0; c < CHT; ++c) r_feat[c] = c < channels ? feats[(size_t)g * channels + c] : 0.f;
    }
  };
  fetch(r_idx, r_ok);

  for (int b = start; b < end; b += kQueue) {
    // which quadrants still have an unfinished pixel
    unsigned live = 0;
#pragma unroll
    for (int k = 0; k < 4; ++k)
      if ((kMasks<CHT> ? alive[k] : ballot(st[k].T > 0.f)) != 0ull) live |= 1u << k;
    if (live == 0) break;
    if constexpr (TRACK_LAST) {
      // first batch of a segment (raster_common.h: checkpoints): the state in front of it, for the segmented backward
      if (ckpt && b != start && ((b - start) & ((1 << ckpt_shift) - 1)) == 0) {
        float* cp = ckpt + ckpt_header_floats(n_tiles) + ckpt_unit(start, tile, (b - start) >> ckpt_shift, ckpt_shift) * (size_t)(1 + channels) * 256 + lane;
#pragma unroll
        for (int k = 0; k < 4; ++k) {
          cp[64 * k] = fabsf(st[k].T);
#pragma unroll
          for (int c = 0; c < CHT; ++c)
            if (c < channels) cp[256 * (1 + c) + 64 * k] = st[k].C[c];
        }
      }
    }

    // take the prefetched batch, start the next one
    if (b != start) { r_idx = b + (int)lane; r_ok = r_idx < end; fetch(r_idx, r_ok); }
    const int c_idx = r_idx;
    const bool c_ok = r_ok;
    const float2 c_xy = r_xy;
    const float c_ca = r_ca, c_cb = r_cb, c_cc = r_cc, c_op = r_op;
    float c_feat[CHT];
#pragma unroll
    for (int c = 0; c < CHT; ++c) c_feat[c] = r_feat[c];

    // the cull leaves lane masks: reach[k] = the lanes whose Gaussian reaches (live) quadrant k.  They stay in SGPRs
    // for the walk, which tests them at the entry's lane instead of reading the entry's mask back from LDS.
    unsigned long long reach[4];
    if (cull) {
      quadrant_reach(c_xy.x, c_xy.y, c_ca, c_cb, c_cc, c_op, c_ok, fr.tile_x, fr.tile_y, live, reach);
    } else {
#pragma unroll
      for (int k = 0; k < 4; ++k) reach[k] = ((live >> k) & 1u) ? ballot(c_ok) : 0ull;
    }
    const unsigned long long keep = reach[0] | reach[1] | reach[2] | reach[3];
    const bool queued = __builtin_amdgcn_inverse_ballot_w64(keep);
    // every queued Gaussian of this batch has a well conditioned conic and an opacity <= 0.999 (nearly
    // always): the sigma >= 0 test and the 0.999 clamp are dead for the whole batch and the walk below runs
    // without them (raster_common.h: sigma_sign_is_safe) -- two compare / min class instructions less per 64 pairs
    const bool all_safe = ballot(queued && !entry_is_safe(c_ca, c_cb, c_cc, c_op)) == 0ull;
    MGS_STAT(0, __popcll(ballot(c_ok)));
    MGS_STAT(1, __popcll(keep));
    MGS_STAT(5, 1);
    if (queued) {
      QueueEntry<CHT>& e = queue[mask_rank(keep)];
      const QueueGeo q = queue_geometry(c_xy, c_ca, c_cb, c_cc, c_op, fr.ctr_x, fr.ctr_y);
      e.geo0 = q.geo0;
      e.geo1 = make_float4(q.sB, q.sC, 0.f, __int_as_float(c_idx));
      if (!all_safe) e.geo3 = make_float4(q.m_x, q.m_y, 0.f, 0.f);
      pack_features(c_feat, e.feat);
    }
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");

    // (measured and rejected in round 1: reading entry j+1 while blending entry j, 307 vs 292 us; two entries per trip
    //  of the counted loop, 291 vs 288 us.  The four-entry trip of the walk below is about the queue pointer's v_add.)
    // `at`: the lane that queued this entry
    auto blend_entry = [&](auto safe_tag, int at, const float4& g0, const float4& g1, const float4* ef,
                           const float4& g3) {
      constexpr bool SAFE = decltype(safe_tag)::value;
      float feat[CHT];
      unpack_features(ef, feat);
      const int idx = __float_as_int(g1.w);
      // (measured and rejected, profiles/r3/00_experiments.md: one straight-line body per quadrant SET behind a
      //  switch on the mask, 268-278 us against 197; the live quadrants re-derived every 8 / 16 / 32 entries, +2 %)
      // (kMasks: reach[k] is emptied the moment the quadrant's last pixel closes, blend_entry_safe_asm)
#pragma unroll
      for (int k = 0; k < 4; ++k) MGS_STAT(2, (unsigned)((reach[k] >> at) & 1ull));
      if constexpr (kMasks<CHT> && SAFE) {
        // (the bodies test reach[k] at `at` themselves, s_bitcmp1_b64 and a branch: the compiler's own test of a
        //  variable bit of a 64-bit mask is a shift, an AND and a compare on top of the branch)
        blend_entry_safe_asm<CHT, TRACK_LAST>(st, alive, reach, at, fr.pq, g0.x, g0.y, g0.z, g0.w, g1.x, g1.y, feat, idx);
      } else {
        auto quad = [&](auto kc) {
          constexpr int k = decltype(kc)::value;
          if ((reach[k] >> at) & 1ull)
            blend_pixel<CHT, TRACK_LAST, SAFE, kMasks<CHT>>(st[k], alive[k], fr.pq[k], g0.x, g0.y, g0.z, g0.w, g1.x, g1.y, g3.x,
                                                             g3.y, feat, idx);
        };
        quad(std::integral_constant<int, 0>{});
        quad(std::integral_constant<int, 1>{});
        quad(std::integral_constant<int, 2>{});
        quad(std::integral_constant<int, 3>{});
      }
    };
    auto walk = [&](auto safe_tag) {
      constexpr bool SAFE = decltype(safe_tag)::value;
      // entry j was queued by the lane of the j-th set bit of `keep`: the walk scans those bits (s_ff1 / s_bitset0)
      unsigned long long rest = keep;
      auto entry = [&](const QueueEntry<CHT>& e) {
        const int at = __builtin_ctzll(rest);
        asm("s_bitset0_b64 %0, %1" : "+s"(rest) : "s"(at));
        float4 g0, g1, ef[(CHT + 3) / 4];
        if constexpr (CHT <= 4) {
          lds_read_3f4(&e.geo0, &e.geo1, &e.feat[0], g0, g1, ef[0]);
        } else {
          g0 = e.geo0; g1 = e.geo1;
#pragma unroll
          for (int f = 0; f < (CHT + 3) / 4; ++f) ef[f] = e.feat[f];
        }
        float4 g3 = make_float4(0.f, 0.f, 0.f, 0.f);
        if constexpr (!SAFE) g3 = e.geo3;            // the mean's offset: only the sigma >= 0 test reads it
        blend_entry(safe_tag, at, g0, g1, ef, g3);
      };
      if (rest == 0ull) return;
      const QueueEntry<CHT>* e = queue;
      if constexpr (kMasks<CHT> && SAFE) {
        // four entries per trip, each leaving the moment the queue is empty: the LDS address advances through the
        // reads' immediate offsets, one v_add per four entries (no remainder loop: the exits are the loop test)
        for (;; e += 4) {
          entry(e[0]);
          if (rest == 0ull) break;
          entry(e[1]);
          if (rest == 0ull) break;
          entry(e[2]);
          if (rest == 0ull) break;
          entry(e[3]);
          if (rest == 0ull) break;
        }
      } else {
        do entry(*e++); while (rest != 0ull);
      }
    };
    if (all_safe) walk(std::true_type{}); else walk(std::false_type{});
    __builtin_amdgcn_wave_barrier();   // queue is rewritten by the next batch
  }

#ifdef MGS_RASTER_STATS
  {
    unsigned nv = 0, na = 0;
    for (int k = 0; k < 4; ++k) { nv += st[k].n_valid; na += st[k].n_acc; }
    for (int d = 32; d >= 1; d >>= 1) { nv += __shfl_xor(nv, d); na += __shfl_xor(na, d); }
    stat[3] = nv; stat[4] = na;
    if (lane == 0)
      for (int i = 0; i < 7; ++i) atomicAdd(&g_raster_stats[i], stat[i]);
  }
#endif
  if constexpr (TRACK_LAST) {
    if (ckpt) {       // where the backward's walk of this tile ends (header of the checkpoint buffer)
      int h = max(max(st[0].last, st[1].last), max(st[2].last, st[3].last));
#pragma unroll
      for (int d = 32; d >= 1; d >>= 1) h = max(h, __shfl_xor(h, d));
      if (lane < 4) reinterpret_cast<int32_t*>(ckpt)[4 * tile + lane] = lane == 0 ? h : -1;
    }
  }
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    const int x = ix + 8 * (k & 1), y = iy + 8 * (k >> 1);
    if (x < width && y < height)
      store_pixel<CHT, TRACK_LAST, DATASET>(st[k], x, y, width, channels, background, expected_last, render, alphas, last_ids, ds);
  }
}


// ---- one wave per 8x8 block ------------------------------------------------------------------
// Same blend, finer work units: a workgroup is one tile, wave k of it owns quadrant k with ONE pixel
// per lane.  Four times the waves, each a quarter of the serial work and half the registers (8 waves
// per SIMD instead of 5): the chip is filled in ~4 even rounds instead of 1.6 uneven ones, no
// quadrant branches in the inner loop, and a quadrant that saturates frees its wave slot at once.
// The price is that the list is fetched and culled by each of the four waves (L2 hits) and that the
// pixel offset (2 subtractions) is paid per evaluation instead of per queue entry.
template <int CHT, bool TRACK_LAST, bool DATASET = false>
__global__ __launch_bounds__(256) void raster_fwd_q_kernel(    // (bounded to 64 VGPRs / 8 waves per SIMD: 166-172 -> 182 us, left free: 66)
    const float* __restrict__ means2d, const float* __restrict__ conics,
    const float* __restrict__ feats, const float* __restrict__ opacities,
    const float4* __restrict__ splats, const float* __restrict__ background, int channels,
    int width, int height, int tile_w, int n_tiles, const int32_t* __restrict__ tile_offsets,
    const int32_t* __restrict__ flatten_ids, float* __restrict__ render,
    float* __restrict__ alphas, int32_t* __restrict__ last_ids, int cull, int expected_last,
    const int32_t* __restrict__ group_order, float* __restrict__ ckpt, int ckpt_shift,
    std::conditional_t<DATASET, DatasetOut, NoDataset> ds) {
  __shared__ QueueEntry<CHT> queues[4][kQueue];
  const int k = (int)(threadIdx.x >> 6);
  QueueEntry<CHT>* queue = queues[k];
  const int tile = tile_of_unit(blockIdx.x, n_tiles, group_order);      // tile_order.h
  if (tile < 0) return;
  const unsigned lane = threadIdx.x & 63u;
  const int tx = tile % tile_w, ty = tile / tile_w;
  const int start = tile_offsets[tile], end = tile_offsets[tile + 1];
  const int ix = tx * 16 + 8 * (k & 1) + (int)(lane & 7), iy = ty * 16 + 8 * (k >> 1) + (int)(lane >> 3);
  // this lane's pixel as an offset from the TILE centre (the same coordinates as the one-wave-per-tile kernel: same bits)
  const PixelPoly pp = pixel_poly((float)(8 * (k & 1) + (int)(lane & 7)) - 7.5f, (float)(8 * (k >> 1) + (int)(lane >> 3)) - 7.5f);
  const bool inside = ix < width && iy < height;
  QuadRect rect;
  rect.x0 = (float)(tx * 16 + 8 * (k & 1)) + 0.5f; rect.x1 = rect.x0 + 7.f;
  rect.y0 = (float)(ty * 16 + 8 * (k >> 1)) + 0.5f; rect.y1 = rect.y0 + 7.f;
  const float tile_x = (float)(tx * 16), tile_y = (float)(ty * 16);

  PixelState<CHT> st;
  st.T = (inside || kMasks<CHT>) ? 1.f : -1.f;
  unsigned long long alive = ballot(inside);     // kMasks: the block's open pixels
  st.last = 0;
#pragma unroll
  for (int c = 0; c < CHT; ++c) st.C[c] = 0.f;

  int r_idx = start + (int)lane;
  bool r_ok = r_idx < end;
  float2 r_xy = make_float2(0.f, 0.f);
  float r_ca = 1.f, r_cb = 0.f, r_cc = 1.f, r_op = 0.f;
  float r_feat[CHT];
#pragma unroll
  for (int c = 0; c < CHT; ++c) r_feat[c] = 0.f;
  // (Both branches keep their loads written out, not through load_geometry / load_record_tail as in the kernel above.
  //  This kernel prefetches: what is loaded here is waited for a batch later.  Through load_geometry the array path's
  //  three conic loads merge into one and the compiler's s_waitcnt vmcnt(3) / (4) in front of the cull become vmcnt(0);
  //  through the two helpers on the record the 1-channel inference instantiation takes 55 VGPRs instead of 53.  Both
  //  from the compiler's report and listing, profiles/raster_shared/README.md.)
  auto fetch = [&](int idx, bool ok) {
    if (ok && CHT <= 4 && splats) {
      int g = flatten_ids[idx];
      const float4 p0 = splats[3 * (size_t)g], p1 = splats[3 * (size_t)g + 1], p2 = splats[3 * (size_t)g + 2];
      r_xy = make_float2(p0.x, p0.y);
      r_ca = p0.z; r_cb = p0.w; r_cc = p1.x; r_op = p1.y;
      const float ff[4] = {p1.z, p1.w, p2.x, p2.y};
#pragma unroll
      for (int c = 0; c < CHT; ++c) r_feat[c] = ff[c & 3];
    } else if (ok) {
      int g = flatten_ids[idx];
      r_xy = reinterpret_cast<const float2*>(means2d)[g];
      r_ca = conics[3 * (size_t)g + 0];
      r_cb = conics[3 * (size_t)g + 1];
      r_cc = conics[3 * (size_t)g + 2];
      r_op = opacities[g];
#pragma unroll
      for (int c = 0; c < CHT; ++c) r_feat[c] = c < channels ? feats[(size_t)g * channels + c] : 0.f;
    }
  };
  fetch(r_idx, r_ok);

  for (int b = start; b < end; b += kQueue) {
    if ((kMasks<CHT> ? alive : ballot(st.T > 0.f)) == 0ull) break;          // every pixel of the block is finished
    if constexpr (TRACK_LAST) {
      // first batch of a segment (raster_common.h: checkpoints): this block's state in front of it.  A block that is
      // finished by then stores nothing: none of its pixels has a last_id in or past the segment, and the backward
      // takes a checkpoint only for pixels that do.
      if (ckpt && b != start && ((b - start) & ((1 << ckpt_shift) - 1)) == 0) {
        float* cp = ckpt + ckpt_header_floats(n_tiles) + ckpt_unit(start, tile, (b - start) >> ckpt_shift, ckpt_shift) * (size_t)(1 + channels) * 256 + 64 * k + lane;
        cp[0] = fabsf(st.T);
#pragma unroll
        for (int c = 0; c < CHT; ++c)
          if (c < channels) cp[256 * (1 + c)] = st.C[c];
      }
    }
    const int c_idx = r_idx;
    const bool c_ok = r_ok;
    const float2 c_xy = r_xy;
    const float c_ca = r_ca, c_cb = r_cb, c_cc = r_cc, c_op = r_op;
    float c_feat[CHT];
#pragma unroll
    for (int c = 0; c < CHT; ++c) c_feat[c] = r_feat[c];
    r_idx = b + kQueue + (int)lane;
    r_ok = r_idx < end;
    fetch(r_idx, r_ok);

    // same exact test as quadrant_mask (raster_common.h), for this block only
    bool keep_me = false;
    if (c_ok) {
      keep_me = true;
      if (cull) {
        keep_me = false;
        if (cull_opacity_ok(c_op)) {
          // (single v_log_f32 / v_rcp_f32, as in quadrant_mask: the slack is orders above their error)
          const float thr = 0.6931471805599453f * __builtin_amdgcn_logf(255.0f * c_op);
          const float fx = fmaxf(fabsf(tile_x - c_xy.x), fabsf(tile_x + 16.f - c_xy.x));
          const float fy = fmaxf(fabsf(tile_y - c_xy.y), fabsf(tile_y + 16.f - c_xy.y));
          const float slack = 0.05f + 4e-6f * (fabsf(c_ca) + fabsf(c_cc) + 2.f * fabsf(c_cb)) * (fx * fx + fy * fy);
          const float smin = rect_min_sigma(c_xy.x, c_xy.y, c_ca, c_cb, c_cc, __builtin_amdgcn_rcpf(c_ca), __builtin_amdgcn_rcpf(c_cc), rect);
          keep_me = !(smin > thr + slack);
        }
      }
    }
    const unsigned long long keep = ballot(keep_me);
    const int count = __popcll(keep);
    const bool all_safe = ballot(keep_me && !entry_is_safe(c_ca, c_cb, c_cc, c_op)) == 0ull;
    if (keep_me) {
      QueueEntry<CHT>& e = queue[mask_rank(keep)];
      const QueueGeo q = queue_geometry(c_xy, c_ca, c_cb, c_cc, c_op, tile_x + 8.f, tile_y + 8.f);
      e.geo0 = q.geo0;
      e.geo1 = make_float4(q.sB, q.sC, 0.f, __int_as_float(c_idx));
      // (the instantiations that are launched, <= 4 channels: behind the branch <8, true> takes 74 VGPRs instead of 72)
      if (CHT > 4 || !all_safe) e.geo3 = make_float4(q.m_x, q.m_y, 0.f, 0.f);
      pack_features(c_feat, e.feat);
    }
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
    auto walk = [&](auto safe_tag) {
      constexpr bool SAFE = decltype(safe_tag)::value;
      // A block whose 64 pixels are all finished stops at the next multiple of 8 entries instead of the end
      // of the 64-entry batch -- in the training variant only: measured 206 -> 194 us there, 184 -> 191 us
      // for the inference variant (whose loop the compiler unrolls four times when left whole).
      constexpr int kChunk = TRACK_LAST ? 8 : kQueue;
      for (int j0 = 0; j0 < count; j0 += kChunk) {
        if (j0 && (kMasks<CHT> ? alive : ballot(st.T > 0.f)) == 0ull) break;
        const int j1 = min(j0 + kChunk, count);
      for (int j = j0; j < j1; ++j) {
        const QueueEntry<CHT>& e = queue[j];
        float4 g0, g1, ef[(CHT + 3) / 4];
        if constexpr (CHT <= 4) {
          lds_read_3f4(&e.geo0, &e.geo1, &e.feat[0], g0, g1, ef[0]);
        } else {
          g0 = e.geo0; g1 = e.geo1;
#pragma unroll
          for (int f = 0; f < (CHT + 3) / 4; ++f) ef[f] = e.feat[f];
        }
        float feat[CHT];
        unpack_features(ef, feat);
        if constexpr (kMasks<CHT> && SAFE) {
          blend_pixel_safe_asm<CHT, TRACK_LAST>(st, alive, pp, g0.x, g0.y, g0.z, g0.w, g1.x, g1.y, feat, __float_as_int(g1.w));
        } else {
          float4 g3 = make_float4(0.f, 0.f, 0.f, 0.f);
          if constexpr (!SAFE) g3 = e.geo3;
          blend_pixel<CHT, TRACK_LAST, SAFE, kMasks<CHT>>(st, alive, pp, g0.x, g0.y, g0.z, g0.w, g1.x, g1.y, g3.x, g3.y, feat,
                                                           __float_as_int(g1.w));
        }
      }
      }
    };
    if (all_safe) walk(std::true_type{}); else walk(std::false_type{});
    __builtin_amdgcn_wave_barrier();
  }

  if constexpr (TRACK_LAST) {
    if (ckpt) {       // where the backward's walk of this block ends (header of the checkpoint buffer)
      int h = inside ? st.last : -1;
#pragma unroll
      for (int d = 32; d >= 1; d >>= 1) h = max(h, __shfl_xor(h, d));
      if (lane == 0) reinterpret_cast<int32_t*>(ckpt)[4 * tile + k] = h;
    }
  }
  if (inside)
    store_pixel<CHT, TRACK_LAST, DATASET>(st, ix, iy, width, channels, background, expected_last, render, alphas, last_ids, ds);
}

}  // namespace
}  // namespace mgs

using namespace mgs;

// Test hook: 0 disables the exact quadrant cull (every listed Gaussian is evaluated against every
// live quadrant).  The image must not change; tests/test_gpu_forward.py checks that bit for bit.
// Both knobs exist in libmgs_debug.so only (-DMGS_DEBUG_HOOKS; tests and A/B scripts load that build): the shipped
// libmgs.so has no process-global state -- two renderers in one process cannot race on a knob (include/mgs.h:
// "stateless and re-entrant").
#ifdef MGS_DEBUG_HOOKS
static int g_raster_cull = 1;
extern "C" void mgs_debug_set_raster_cull(int enabled) { g_raster_cull = enabled; }
#else
static constexpr int g_raster_cull = 1;
#endif
// Scheduling knobs for A/B measurements (scripts/raster_ab.py); they never change a pixel.
//   bit 0: issue priority by tile-list length in the one-wave-per-tile kernel (default on)
//   bit 1: honour MGS_RASTER_LATENCY (one wave per 8x8 block, raster_fwd_q_kernel, <= 4 channels); default on
//   bit 2: use that kernel whatever the flags say
//   bit 3: ignore tile_group_order (index-order launch); bit 4: ignore it in the one-wave-per-tile inference kernel only
//   bits 8..: KiB of unused dynamic LDS per workgroup of that kernel (caps its occupancy: experiments)
#ifdef MGS_DEBUG_HOOKS
static int g_raster_opts = 3;
extern "C" void mgs_debug_set_raster_opts(int opts) { g_raster_opts = opts; }
#else
static constexpr int g_raster_opts = 3;
#endif

#ifdef MGS_RASTER_STATS
// instrumented build only: copy the counters out (synchronous) and zero them
extern "C" int mgs_debug_read_raster_stats(unsigned long long* out8) {
  unsigned long long zero[8] = {0, 0, 0, 0, 0, 0, 0, 0};
  if (hipMemcpyFromSymbol(out8, HIP_SYMBOL(g_raster_stats), sizeof(zero)) != hipSuccess) return -1;
  if (hipMemcpyToSymbol(HIP_SYMBOL(g_raster_stats), zero, sizeof(zero)) != hipSuccess) return -1;
  return 0;
}
#endif

extern "C" size_t mgs_raster_checkpoint_floats(uint32_t isect_capacity, int tile_w, int tile_h, int channels,
                                               int checkpoint_interval) {
  if (checkpoint_interval < 64 || (checkpoint_interval & (checkpoint_interval - 1)) || tile_w <= 0 || tile_h <= 0 || channels < 1)
    return 0;
  int shift = 0;
  while ((1 << shift) < checkpoint_interval) ++shift;
  return ckpt_header_floats(tile_w * tile_h) + ckpt_units(isect_capacity, tile_w * tile_h, shift) * (size_t)(1 + channels) * 256;
}

extern "C" int mgs_rasterize_fwd(int n, const float* means2d, const float* conics,
                                 const float* feats, const float* opacities, const float* splats,
                                 const float* background, int channels, int width, int height,
                                 int tile_w, int tile_h, const int32_t* tile_offsets,
                                 const int32_t* flatten_ids, const int32_t* tile_group_order, int flags,
                                 float* render, float* alphas, int32_t* last_ids, float* checkpoints,
                                 int checkpoint_interval, uint8_t* ds_rgba, void* ds_distance, int ds_distance_type,
                                 const double* ds_Kinv_host, mgs_stream_t stream) {
  MGS_REQUIRE(n >= 0 && width > 0 && height > 0, "rasterize_fwd: bad sizes");
  MGS_REQUIRE(channels >= 1 && channels <= MGS_MAX_CHANNELS, "rasterize_fwd: channels %d outside 1..%d", channels, MGS_MAX_CHANNELS);
  MGS_REQUIRE(tile_w == (width + 15) / 16 && tile_h == (height + 15) / 16,
              "rasterize_fwd: tile grid %dx%d does not match %dx%d at tile size 16", tile_w, tile_h, width, height);
  MGS_REQUIRE(!splats || channels <= 4, "rasterize_fwd: packed splats carry at most 4 channels");
  MGS_REQUIRE((n == 0 || splats || (means2d && conics && feats && opacities)) && tile_offsets &&
                  flatten_ids && ((render && alphas) || (ds_rgba && !render && !alphas)), "rasterize_fwd: null pointer");
  DatasetOut ds{};
  if (ds_rgba || ds_distance) {
    // the dataset frame (RGBA8 + ray distance) straight out of the raster: "RGB+ED" inference frames only
    MGS_REQUIRE(ds_rgba && channels == 4 && (flags & MGS_RASTER_EXPECTED_LAST) && !last_ids,
                "rasterize_fwd: the dataset output needs ds_rgba, 4 channels, MGS_RASTER_EXPECTED_LAST and no last_ids");
    MGS_REQUIRE(((uintptr_t)ds_rgba & 3) == 0, "rasterize_fwd: ds_rgba must be 4-byte aligned");
    MGS_REQUIRE(!ds_distance || ds_Kinv_host, "rasterize_fwd: the distance map needs K^-1 (host pointer, 9 doubles)");
    MGS_REQUIRE(ds_distance_type >= 0 && ds_distance_type <= 2, "rasterize_fwd: distance type %d not in {0: f32, 1: f64, 2: f16}",
                ds_distance_type);
    ds.rgba = reinterpret_cast<uint32_t*>(ds_rgba);
    ds.dist = ds_distance;
    ds.type = ds_distance_type;
    for (int i = 0; i < 9; ++i) ds.ki.m[i] = ds_Kinv_host ? ds_Kinv_host[i] : 0.0;
  }
  int ckpt_shift = 0;
  if (checkpoints) {
    MGS_REQUIRE(last_ids, "rasterize_fwd: checkpoints are written by the training variant (last_ids given)");
    MGS_REQUIRE(checkpoint_interval >= 64 && (checkpoint_interval & (checkpoint_interval - 1)) == 0,
                "rasterize_fwd: checkpoint_interval %d is not a power of two >= 64", checkpoint_interval);
    while ((1 << ckpt_shift) < checkpoint_interval) ++ckpt_shift;
  }
  const int n_tiles = tile_w * tile_h;
  hipStream_t s = (hipStream_t)stream;
  const bool per_block = (g_raster_opts & 4) || ((g_raster_opts & 2) && (flags & MGS_RASTER_LATENCY));
  if (g_raster_opts & 8) tile_group_order = nullptr;
  if ((g_raster_opts & 16) && !per_block && !last_ids) tile_group_order = nullptr;
  const int n_units = tile_launch_units(n_tiles, tile_group_order);
  const int expected_last = (flags & MGS_RASTER_EXPECTED_LAST) ? 1 : 0;
  const size_t opts_lds = (size_t)(g_raster_opts >> 8) * 1024;
  // ds_arg: NoDataset{}, or the DatasetOut of a dataset frame (4 channels, inference, "ED")
  auto launch = [&](auto cht, auto track_last, auto ds_arg) {
    constexpr int C = decltype(cht)::value;
    constexpr bool T = decltype(track_last)::value, DS = std::is_same<decltype(ds_arg), DatasetOut>::value;
    if (per_block && C <= 4) {    // (a run-time test: the wider instantiations exist, unlaunched)
      hipLaunchKernelGGL((raster_fwd_q_kernel<C, T, DS>), dim3(n_units), dim3(256), opts_lds, s, means2d, conics, feats,
                         opacities, reinterpret_cast<const float4*>(splats), background, channels, width, height, tile_w,
                         n_tiles, tile_offsets, flatten_ids, render, alphas, last_ids, g_raster_cull, expected_last,
                         tile_group_order, checkpoints, ckpt_shift, ds_arg);
      return;
    }
    hipLaunchKernelGGL((raster_fwd_kernel<C, T, DS>), dim3(div_up(n_units, T ? 1 : kFwdWgWaves)),
                       dim3(64 * (T ? 1 : kFwdWgWaves)), T ? 0 : opts_lds, s, means2d, conics, feats, opacities,
                       reinterpret_cast<const float4*>(splats), background, channels, width, height, tile_w, n_tiles,
                       tile_offsets, flatten_ids, render, alphas, last_ids, g_raster_cull, expected_last, g_raster_opts,
                       tile_group_order, checkpoints, ckpt_shift, ds_arg);
  };
  if (ds.rgba) launch(int_c<4>{}, bool_c<false>{}, ds);
  else
    with_channels(channels, [&](auto cht) { with_bool(last_ids != nullptr, [&](auto t) { launch(cht, t, NoDataset{}); }); });
  return check_launch("rasterize_fwd");
}
