/* mgs_optim.h -- C ABI of the optimiser step of libmgs.so: one fused, visibility-masked Adam update of all
 * parameter groups of a Gaussian scene.  Compiled into the same libmgs.so / libmgs_debug.so as include/mgs.h's render
 * path and bound by the same conventions (see the top of mgs.h): device pointers unless marked "host", the caller owns
 * every buffer, all work is enqueued on `stream`, nothing synchronises, the call is capturable in a hipGraph, and the
 * return value is 0, <0 MGS_ERR_* or >0 a hipError_t from the launch.  MGS_VERSION is mgs.h's: this header adds
 * entry points and changes no parameter list.
 *
 * The update is torch.optim.Adam's (amsgrad = False, weight_decay = 0, maximize = False) for update number t = 1, 2, ...:
 *   m <- beta1 m + (1 - beta1) g
 *   v <- beta2 v + (1 - beta2) g^2
 *   p <- p - (lr_t / (1 - beta1^t)) m / (sqrt(v) / sqrt(1 - beta2^t) + eps)
 * in fp32 per element, with the per-step scalars (1 - beta^t = -expm1(t ln beta), lr_t) evaluated in fp64 on the device.
 *
 * Step counter.  step_state is two device int32 the caller zero-initialises once: { steps taken, ticket }.  The
 * launch reads `steps taken`, performs update number t = steps taken + 1 and stores t when its last workgroup retires,
 * so a replayed graph takes update t + 1 on the next replay with no host involvement.  Calls that share a step_state
 * must be ordered on one stream.
 *
 * Schedule (per group).  decay_steps == 0: lr_t = lr.  Otherwise
 *   lr_t = lr (lr_final / lr)^(min(t - 1, decay_steps) / decay_steps)
 * (nerfstudio's ExponentialDecayScheduler without warm-up, stepped after each optimiser step; lr, lr_final > 0).
 *
 * Row split (per group).  A group is n rows of row_floats floats.  head_floats == 0: every element uses lr_t.
 * Otherwise the elements at row offset >= head_floats use lr_t * rest_lr_scale (the [N, 16, 3] SH tensor with
 * head_floats = 3, rest_lr_scale = 1 / 20 trains features_dc and features_rest at splatfacto's two rates).
 *
 * Visibility (nullable; at most one of the two forms).  Row i of every group belongs to Gaussian i, so every group must
 * have the same n.
 *   radii[n_cams rows of n int32, cam_stride elements apart] (+ radii_y of the same layout, nullable: the second axis
 *   under MGS_RADIUS_OPACITY_AWARE): Gaussian i is visible iff radii > 0 (or radii_y > 0) in some camera;
 *   mask[n] uint8: visible iff non-zero.
 * Nothing of p, m or v of an invisible Gaussian is read or written (gsplat's SelectiveAdam); t advances all the same.
 *
 * The result is bit-reproducible: every element is updated by one thread in a fixed evaluation order, no atomics
 * touch the data. */
#ifndef MGS_OPTIM_H_
#define MGS_OPTIM_H_

#include "mgs.h"

#ifdef __cplusplus
extern "C" {
#endif

#define MGS_ADAM_MAX_GROUPS 8

/* host struct; param / grad / exp_avg / exp_avg_sq are device arrays of n * row_floats floats, 16-byte aligned */
typedef struct mgs_adam_group {
  float *param;
  const float *grad;
  float *exp_avg;
  float *exp_avg_sq;
  int64_t n;             /* rows (Gaussians); n * row_floats < 2^32 */
  int32_t row_floats;    /* >= 1 */
  int32_t head_floats;   /* 0 (no split) .. row_floats */
  double lr;             /* >= 0 */
  double lr_final;       /* read when decay_steps > 0 */
  int32_t decay_steps;   /* 0: constant lr */
  double rest_lr_scale;  /* read when head_floats > 0 */
} mgs_adam_group;

/* n_groups 1..MGS_ADAM_MAX_GROUPS; beta1, beta2 in [0, 1); eps >= 0.  One launch. */
int mgs_adam_step(int n_groups, const mgs_adam_group *groups /* host */, double beta1, double beta2, double eps,
                  int32_t *step_state /* device: { steps taken, ticket } */, const int32_t *radii,
                  const int32_t *radii_y, int n_cams, size_t cam_stride, const uint8_t *mask, mgs_stream_t stream);

#ifdef __cplusplus
}
#endif
#endif /* MGS_OPTIM_H_ */
