/* mgs_lift.h -- C ABI of lifting 2D part masks onto Gaussians: the inverse direction of include/mgs_labels.h.
 * Compiled into the same libmgs.so / libmgs_debug.so as include/mgs.h's render path and bound by the same conventions
 * (see the top of mgs.h): device pointers unless marked "host", the caller owns every buffer, all work is enqueued on
 * `stream`, nothing synchronises or reads a count back, every call is capturable in a hipGraph, and the return value is
 * 0, <0 MGS_ERR_* or >0 a hipError_t from a launch.  The version is mgs.h's: this header adds entry points and changes no
 * parameter list.
 *
 * Votes.  mask[height * width] uint8 gives every pixel of one camera's view a class in 0..K-1, K = n_classes with
 * 1 <= K <= MGS_LABELS_MAX_CLASSES; any other value (255, say) means "no class here".  For Gaussian i and class k
 *     V[i,k] = sum over the pixels p of the view with mask(p) == k of w_i(p),
 * where w_i(p) is exactly the weight the frame blends Gaussian i with at p (mgs_rasterize_fwd on the same lists; the
 * rules are spelled out in mgs_labels.h: counted iff sigma >= 0 and alpha >= 1/255, w = alpha T, the Gaussian that closes a
 * pixel and everything behind it not counted).  It is the transpose of mgs_labels.h's W_k(p).
 * Votes are UNSIGNED 64-BIT FIXED POINT with 32 fractional bits: one unit is 2^-32 of a pixel's full weight.  A tile adds
 * rint(s * 2^32) for the fp32 sum s of its pixels' weights (a fixed summation order), with an integer atomic add: integer
 * addition is associative, so the votes are the same bits under any launch order, in every run, and over any split of
 * the cameras into calls.  A row's vote from one view is below the number of pixels the Gaussian is counted at, so a
 * buffer cannot wrap while views x pixels covered per view stays below 2^31. */
#ifndef MGS_LIFT_H_
#define MGS_LIFT_H_

#include "mgs.h"
#include "mgs_labels.h"

#ifdef __cplusplus
extern "C" {
#endif

/* One camera, on the list arguments of mgs_rasterize_fwd (tile size 16; tile_offsets[tile_w * tile_h + 1], flatten_ids,
 * tile_group_order nullable: a launch order, never a result) and the Gaussian arrays of mgs_raster_labels.
 * votes[n_rows * n_classes] is ACCUMULATED into: zero it before the first camera.  The row of list id `id` is
 * id - row_offset (camera c of a [C*N] id space passes c * N and n_rows = N); an id whose row falls outside 0..n_rows-1
 * occludes as usual and votes nowhere.
 * MGS_ERR_INVALID_ARGUMENT, before any launch: n_classes outside 1..MGS_LABELS_MAX_CLASSES; mask or votes NULL; n_rows < 0;
 * neither `splats` nor all of means2d / conics / opacities given; bad sizes; a tile grid that is not the frame's; NULL lists.
 * One launch. */
int mgs_raster_votes(int n, const float *means2d, const float *conics, const float *opacities,
                     const float *splats /* nullable; when given the three above are not read */,
                     const uint8_t *mask /* [height*width] */, int n_classes,
                     int width, int height, int tile_w, int tile_h,
                     const int32_t *tile_offsets, const int32_t *flatten_ids,
                     const int32_t *tile_group_order /* nullable */,
                     int row_offset, int n_rows, uint64_t *votes /* [n_rows, n_classes] */,
                     mgs_stream_t stream);

/* class_ids[g] = the class with the most votes of row g (ties to the lowest class) if that vote exceeds min_vote, else
 * -1; confidence[g] (nullable) = that vote / the row's total, 0 where the class is -1.  min_vote is in pixels of full
 * weight, 0 <= min_vote < 2^31, and is compared as fixed point (rint(min_vote * 2^32)): a row without a vote is never
 * given a class.  MGS_ERR_INVALID_ARGUMENT, before any launch: n_rows < 0; n_classes outside 1..MGS_LABELS_MAX_CLASSES;
 * votes or class_ids NULL; min_vote negative, not finite or >= 2^31.  One launch. */
int mgs_lift_assign(int n_rows, int n_classes, const uint64_t *votes, float min_vote,
                    int32_t *class_ids, float *confidence /* nullable */, mgs_stream_t stream);

#ifdef __cplusplus
}
#endif
#endif /* MGS_LIFT_H_ */
