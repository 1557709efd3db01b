/* mgs_hybrid.h -- C ABI of the exact mesh-over-splat composite of libmgs.so: a frame's own front-to-back blend, stopped
 * per pixel at the depth of an opaque foreground, with the foreground entering at the transmittance reached there.
 * Compiled into the same libmgs.so / libmgs_debug.so as include/mgs.h's render path and bound by the same conventions
 * (see the top of mgs.h): device pointers unless marked "host", the caller owns every buffer, all work is enqueued on
 * `stream`, nothing synchronises or reads a count back, and the return value is 0, <0 MGS_ERR_* or >0 a hipError_t from
 * a launch.  MGS_VERSION is mgs.h's: this header adds an entry point and changes no parameter list.
 *
 * Inputs, for one camera: the frame's own raster inputs (means2d, conics, the opacities the raster saw, per-Gaussian
 * features whose first three columns are rgb, per-Gaussian camera depths) and tile lists; an opaque foreground fg_rgb
 * [H,W,3], fg_depth [H,W] (z-depth, 0 where no face is -- what mgs_rasterize_mesh returns); the plain frame render
 * [H,W,4] with the expected depth in its last channel ("RGB+ED") and alphas [H,W]; an optional backdrop[3].
 *
 * A pixel HAS FOREGROUND iff 0 < fg_depth < inf (a NaN depth is no foreground; there is no mask).
 *
 * With foreground, d = fg_depth.  The pixel's list is walked exactly as the frame walks it (mgs_labels.h states the
 * rule): alpha = min(0.999, opacity exp(-sigma)), counted iff sigma >= 0 and alpha >= 1/255, w = alpha T, and the
 * Gaussian at which T (1 - alpha) <= 1e-4 closes the pixel and is not counted.  F = the counted Gaussians with
 * depths[i] < d -- a strict fp32 comparison of the two given arrays.  The lists are ordered by (depth bits, index), so F
 * is a prefix of the pixel's counted Gaussians.  With T_F = prod over F of (1 - alpha_i):
 *   out_rgb       = sum_F w_i c_i + T_F fg_rgb
 *   out_depth     = sum_F w_i z_i + T_F d          (the weights sum to 1: the hybrid frame's expected depth, no division)
 *   fg_visibility = T_F                            (the share of the foreground that reaches the eye)
 * A pixel that closes before d hands the foreground the residual T, as the frame does a background; a Gaussian with
 * depths[i] == d is behind.  w_i is the frame's own weight bit for bit and the sums are accumulated with the forward's own
 * expression, acc = fma(w, c, acc).  T_F is kept as T_F -= w_i: the frame's T is fma(-alpha, T, T), one rounding where this
 * makes two, so T_F is the frame's T after F to within one ulp of T per member of F.
 *
 * Without foreground the pixel is mgs_composite_over's third rule on the given frame, comparison by comparison:
 *   out_rgb       = render_rgb + (1 - alpha) backdrop     (product and sum rounded separately; without a backdrop
 *                                                          render_rgb's bits)
 *   out_depth     = alpha > 0 ? render_depth : +inf
 *   fg_visibility = 0
 *
 * Forward only: there is no backward.  One launch, no atomics, no workspace: the same inputs give the same bytes. */
#ifndef MGS_HYBRID_H_
#define MGS_HYBRID_H_

#include "mgs.h"

#ifdef __cplusplus
extern "C" {
#endif

/* One camera, on the list arguments of mgs_rasterize_fwd (tile size 16; tile_offsets[tile_w * tile_h + 1], flatten_ids,
 * tile_group_order nullable: a launch order, never a result).  feats[n * feat_stride], rgb in the first three columns of
 * a row (feat_stride >= 3: an "RGB+ED" frame's [n,4] rows work as they are); depths[n]; render[height * width * 4];
 * alphas, fg_depth, out_depth, fg_visibility [height * width]; fg_rgb, out_rgb [height * width * 3].  The outputs may
 * not overlap the inputs.  The lists must be in the order mgs_isect_tiles leaves them, by the depths given here: the
 * kernel ends a tile's walk at the first entry at or behind the tile's largest foreground depth, found by bisection.
 * MGS_ERR_INVALID_ARGUMENT, before any launch: n < 0 or width, height <= 0; feat_stride < 3; a tile grid that is not
 * ceil(width / 16) x ceil(height / 16); any pointer NULL except tile_group_order, backdrop and fg_visibility. */
int mgs_raster_over_opaque(int n, const float *means2d, const float *conics, const float *opacities,
                           const float *feats, int feat_stride, const float *depths,
                           const float *fg_rgb, const float *fg_depth, const float *render, const float *alphas,
                           const float *backdrop /* nullable */, int width, int height, int tile_w, int tile_h,
                           const int32_t *tile_offsets, const int32_t *flatten_ids,
                           const int32_t *tile_group_order /* nullable */,
                           float *out_rgb, float *out_depth, float *fg_visibility /* nullable */, mgs_stream_t stream);

#ifdef __cplusplus
}
#endif
#endif /* MGS_HYBRID_H_ */
