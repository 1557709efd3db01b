/* mgs_refine.h -- C ABI of the refinement step of libmgs.so: splatfacto-mcmc's strategy ("3D Gaussian Splatting as Markov
 * Chain Monte Carlo", gsplat's MCMCStrategy) on the device.  Compiled into the same libmgs.so / libmgs_debug.so as
 * include/mgs.h's render path and bound by the same conventions (see the top of mgs.h): device pointers unless marked
 * "host", the caller owns every buffer, all work is enqueued on `stream`, nothing synchronises or reads a count back,
 * every call is capturable in a hipGraph, and the return value is 0, <0 MGS_ERR_* or >0 a hipError_t from a launch.
 * MGS_VERSION is mgs.h's: this header adds entry points and changes no parameter list.
 *
 * All parameters are in RAW form (MGS_PARAMS_RAW): opacity logits, log-scales, un-normalised wxyz quaternions.
 *
 * (a) Weights and dead list (mgs_mcmc_weights; the first launches of mgs_mcmc_relocate).  For each of n Gaussians
 *       o = 1 / (1 + exp(-logit)) in fp32;  dead = o <= min_opacity;
 *       w[i] = dead ? 0 : o   (MGS_MCMC_RELOCATE)        w[i] = o   (MGS_MCMC_ADD)
 *     w is stored as fp32; dead[0 .. n_dead) are the dead indices in ascending order; stats receives
 *     { double T = sum of w (accumulated in fp64), int32 n_dead, int32 n_live = #{ w > 0 } }.
 *
 * (b) Sample and relocate (mgs_mcmc_relocate).  The targets are the dead list (MGS_MCMC_RELOCATE: their number stays on
 *     the device) or the append range [n, n + n_new) (MGS_MCMC_ADD).  Target j draws the source
 *       i_j = the smallest i with cdf64[i] > (double)u[j] * T,
 *     cdf64 the inclusive fp64 prefix sum of the stored w: a row of zero weight is never drawn, and if rounding puts
 *     u T >= T the last row of positive weight is.  With c[i] the number of times i was drawn and
 *     r = min(c[i] + 1, MGS_MCMC_MAX_RATIO), every drawn source becomes, evaluated in fp64 from its fp32 parameters,
 *       o     = min(sigmoid(logit), 1 - 2^-23)
 *       o_new = 1 - (1 - o)^(1 / r)
 *       D     = sum_{k=0}^{r-1} C(r, k+1) (-1)^k o_new^(k+1) / sqrt(k+1)
 *               ( = sum_{i=1..r} sum_{k=0..i-1} C(i-1, k) (-1)^k o_new^(k+1) / sqrt(k+1), gsplat's double loop )
 *       logit   <- logit(clamp(o_new, min_opacity, 1 - 2^-23))
 *       log_s   <- log_s + ln(o / D)                      (all three axes)
 *     each stored once by the one thread that owns the source.  The clamp of the SOURCE opacity departs from gsplat on
 *     purpose: at o = 1.0f the sum has no meaning.  D is evaluated at the unclamped o_new, as gsplat does.
 *     Then every target row becomes a bitwise copy of its source's updated row in every group.  Moments:
 *     MGS_MCMC_RELOCATE zeroes those of the drawn sources and leaves the dead rows' untouched; MGS_MCMC_ADD zeroes
 *     those of the new rows and leaves the sources' untouched (both gsplat's).  T == 0 or no target: no parameter and no
 *     moment is written.
 *
 * (c) Noise (mgs_mcmc_noise).  One streaming launch, 56 B read and 12 B written per Gaussian:
 *       Sigma = R(q / |q|) diag(exp(2 log_s)) R^T,    gate = 1 / (1 + exp(-100 ((1 - o) - 0.995))),
 *       means += Sigma (z * gate * lambda),           lambda = noise_lr * lr_next,
 *       lr_next = lr (lr_final / lr)^(min(t, decay_steps) / decay_steps),  t = step_state[0]
 *     (decay_steps == 0: lr_next = lr), evaluated in fp64 on the device: t is the number of updates mgs_adam_step has
 *     ALREADY taken, so lr_next is the rate of the next update -- what a scheduler stepped after the optimiser reports.
 *     step_state == NULL: lambda = noise_lr * lr.  The counter is only read.
 *
 * Results are bit-reproducible: the only atomics are integer (the draw counts). */
#ifndef MGS_REFINE_H_
#define MGS_REFINE_H_

#include "mgs.h"

#ifdef __cplusplus
extern "C" {
#endif

#define MGS_MCMC_RELOCATE 0
#define MGS_MCMC_ADD 1
#define MGS_MCMC_MAX_RATIO 51
#define MGS_REFINE_MAX_GROUPS 8 /* == MGS_ADAM_MAX_GROUPS */

/* host struct; param / exp_avg / exp_avg_sq are device arrays of `capacity` rows of row_floats floats, 16-byte aligned;
 * exp_avg and exp_avg_sq may both be null (a group without optimiser state) */
typedef struct mgs_refine_group {
  float *param;
  float *exp_avg;
  float *exp_avg_sq;
  int32_t row_floats;    /* >= 1; capacity * row_floats < 2^32 */
} mgs_refine_group;

/* device struct written by (a) */
typedef struct mgs_mcmc_stats {
  double total;          /* T */
  int32_t n_dead;
  int32_t n_live;
} mgs_mcmc_stats;

/* (a) alone.  opacities, w: n floats, 16-byte aligned; dead: n int32; n in 0..2^31-1; min_opacity in (0, 1).
 * workspace == NULL: only *workspace_bytes is written. */
int mgs_mcmc_weights(int64_t n, const float *opacities, float min_opacity, int mode, float *w, int32_t *dead,
                     mgs_mcmc_stats *stats, void *workspace, size_t *workspace_bytes /* host */, mgs_stream_t stream);

/* (a) + (b).  opacities [capacity], scales [capacity, 3]: the arrays (b) updates, normally also rows of `groups`.
 * u: n uniforms in [0, 1) (MGS_MCMC_RELOCATE) or n_new (MGS_MCMC_ADD); sources (out): as many int32, the source of each
 * target (entries past the number of targets are left alone).  MGS_MCMC_RELOCATE ignores n_new; MGS_MCMC_ADD needs
 * n + n_new <= capacity.  w, dead: `n` entries as in mgs_mcmc_weights. */
int mgs_mcmc_relocate(int mode, int64_t n, int64_t n_new, int64_t capacity, float *opacities, float *scales,
                      int n_groups, const mgs_refine_group *groups /* host */, float min_opacity, const float *u,
                      float *w, int32_t *dead, mgs_mcmc_stats *stats, int32_t *sources, void *workspace,
                      size_t *workspace_bytes /* host */, mgs_stream_t stream);

/* (c).  means, scales, z: [n, 3]; quats [n, 4]; opacities [n]; all 16-byte aligned.  noise_lr >= 0, lr >= 0;
 * decay_steps > 0 needs lr, lr_final > 0.  step_state: GaussianAdam's device counter, or NULL. */
int mgs_mcmc_noise(int64_t n, float *means, const float *quats, const float *scales, const float *opacities,
                   const float *z, double noise_lr, double lr, double lr_final, int32_t decay_steps,
                   const int32_t *step_state, mgs_stream_t stream);

#ifdef __cplusplus
}
#endif
#endif /* MGS_REFINE_H_ */
