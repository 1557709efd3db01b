/* mgs_loss_rgbd.h -- the masked RGB-D training loss on the frame the renderer produces (csrc/loss.hip: ssim_kernel's
 * masked, strided form).  Compiled into the same libmgs.so / libmgs_debug.so and bound by the conventions of mgs.h, whose
 * entry points and parameter lists it leaves as they are; the version is mgs.h's.  No atomics, every sum in a fixed
 * order: the same inputs give the same bytes.  Nothing is read back to the host.  Capturable.
 *
 * Layouts (fp32, channel-last, images = the product of the leading dimensions):
 *   render        [images, height, width, render_channels], render_channels 3 or 4: colour c, then depth d;
 *   target_rgb    [images, height, width, 3]   c*;
 *   target_depth  [images, height, width]      d*, nullable;
 *   mask          [images, height, width]      m in [0, 1] (may be soft), nullable: m = 1;
 *   v_render      as render: the complete cotangent, channel 3 included.
 *
 * Masked images x = m c, y = m c* where m > 0 and exactly 0 where m == 0 -- a select, not a product: a NaN or inf in
 * render or target_rgb under m == 0 adds exactly 0 to the loss and receives exactly 0 gradient.
 *   colour = (1 - ssim_weight) mean|x - y| + ssim_weight (1 - SSIM(x, y, padding)),
 * the mean over all 3 * height * width * images elements (not divided by the mask's area: splatfacto's form), SSIM as
 * mgs_image_loss states it (mgs.h), over all of its positions.
 *   w = m where d* is finite and > 0, else 0 (a select again);   D = sum w |d - d*| / sum w over all images together,
 * D = 0 with zero gradient where sum w == 0 (decided on the device);   loss = colour + depth_weight D.
 * With depth_weight == 0 there is no depth term: target_depth is not read, D and sum w are reported as 0.
 *
 * Gradient (with respect to render only), for a cotangent v:
 *   channels 0..2   v m (dcolour/dx)(x, y), the gradient mgs_l1_loss_fwd_grad leaves, evaluated at the masked images,
 *                   sign(0) = 0; exactly 0 where m == 0;
 *   channel 3       v depth_weight w sign(d - d*) / sum w; written as 0 where there is no depth term.
 * Where render_channels == 3, mask is NULL (or all ones) and depth_weight == 0, loss and gradient are the bytes
 * mgs_l1_loss_fwd_grad gives under the mgs_image_loss of the same sizes.
 *
 * Launches: the tile kernel and a one-block sum; with depth_weight > 0 one small reduction over mask and target_depth in
 * front (sum w, which channel 3 needs before it is written).  mgs_rgbd_loss_bwd: the tile kernel, and that reduction. */
#ifndef MGS_LOSS_RGBD_H_
#define MGS_LOSS_RGBD_H_

#include "mgs.h"

#ifdef __cplusplus
extern "C" {
#endif

typedef struct mgs_rgbd_loss {
  int images, height, width, render_channels; /* render_channels 3 or 4 */
  float ssim_weight;                           /* lambda in [0, 1] */
  int padding;                                 /* MGS_SSIM_VALID or MGS_SSIM_SAME */
  float depth_weight;                          /* lambda_d >= 0; > 0 needs render_channels == 4 and target_depth */
} mgs_rgbd_loss;

/* All three: with workspace == NULL only *workspace_bytes is written (the descriptor is checked first).
 * MGS_ERR_INVALID_ARGUMENT, before any launch: everything mgs_l1_loss_fwd refuses of the mgs_image_loss {images, height,
 * width, 3, ssim_weight, padding}; render_channels not 3 or 4; depth_weight negative or not finite; depth_weight > 0 with
 * render_channels == 3 or (past the size query) without target_depth; a NULL desc, workspace_bytes, render, target_rgb,
 * loss or v_render.  MGS_ERR_WORKSPACE_TOO_SMALL likewise.
 * terms (nullable, 4 floats on the device) receives {mean|x - y|, SSIM, D, sum w}. */
int mgs_rgbd_loss_fwd(const mgs_rgbd_loss *desc, const float *render, const float *target_rgb,
                      const float *target_depth, const float *mask, float *loss, float *terms, void *workspace,
                      size_t *workspace_bytes, mgs_stream_t stream);
/* loss AND v_render, the gradient for a cotangent of 1, in the same launches: the same loss bytes as mgs_rgbd_loss_fwd. */
int mgs_rgbd_loss_fwd_grad(const mgs_rgbd_loss *desc, const float *render, const float *target_rgb,
                           const float *target_depth, const float *mask, float *loss, float *terms, float *v_render,
                           void *workspace, size_t *workspace_bytes, mgs_stream_t stream);
/* The gradient for the v_loss that arrived (one float on the device), recomputed: the same bytes as
 * mgs_rgbd_loss_fwd_grad's v_render times *v_loss. */
int mgs_rgbd_loss_bwd(const mgs_rgbd_loss *desc, const float *render, const float *target_rgb,
                      const float *target_depth, const float *mask, const float *v_loss, float *v_render,
                      void *workspace, size_t *workspace_bytes, mgs_stream_t stream);

#ifdef __cplusplus
}
#endif
#endif /* MGS_LOSS_RGBD_H_ */
