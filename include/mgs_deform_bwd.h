/* mgs_deform_bwd.h -- C ABI of the backward of mgs_deform_apply, mode 0 (csrc/deform.hip): from the cotangents of the
 * deformed Gaussians, the gradient of a loss with respect to the particles' current positions and to the rest state.
 * Compiled into the same libmgs.so / libmgs_debug.so as include/mgs.h's render path and bound by the conventions of
 * mgs_deform.h: device pointers, the caller owns every buffer, all work is enqueued on `stream`, nothing synchronises or
 * reads a value back, every call is capturable in a hipGraph, and the return value is 0, <0 MGS_ERR_* or >0 a hipError_t
 * from a launch.  The version is mgs.h's: this header adds entry points and changes no parameter list.  No floating-point
 * atomic anywhere: the same inputs give the same bytes in every run.
 *
 * Forward (mgs_deform.h, mode 0), per Gaussian with x_k = particles_now[idx_k], k = 0..7:
 *     e_k = x_k - x_0 (k = 1..7),  c = sum w_k e_k,  xbar = x_0 + c,  P = sum e_k p_k^T,
 *     R = argmax over SO(3) of tr(R^T P),  mu' = xbar + R d0,  q' = normalise(q_R (x) q),  s' = s.
 * Backward, with ct_mu, ct_q, ct_s the cotangents of mu', q', s' (each nullable, null meaning zero):
 *   Tangent of the rotation, under R <- exp([d_omega]x) R, the conventions of mgs_pose.h:
 *     v_omega = (R d0) x ct_mu + 1/2 sum_k e_k <ct_q, (0, e_k) (x) q'>          (e_k here the k-th unit vector)
 *   Polar factor.  S = R^T P is symmetric with eigenvalues sigma_1, sigma_2, s sigma_3, s = sign det P;
 *     G = tr(S) I - S (eigenvalues sigma_2 + s sigma_3, sigma_1 + s sigma_3, sigma_1 + sigma_2),
 *     y = G^-1 R^T v_omega (G's inverse by cofactors, fp64),  v_P = R [y]x.
 *   Particles.  v_e_k = w_k ct_mu + v_P p_k,  v_x_k = v_e_k (k = 1..7),  v_x_0 = ct_mu - sum_k v_e_k.
 *   Rest state.  v_d0 = R^T ct_mu,  v_q = conj(q_R) (x) (ct_q - <ct_q, q'> q') / |q_R (x) q|,  v_s = ct_s bit for bit.
 *   Thin rows (forward status bit 2): v_P = 0, v_d0 = ct_mu, and v_q = ct_q, v_s = ct_s bit for bit; the particle part
 *     comes from c alone.
 *   Pass-through rows (forward status bit 0 or 3): the three rest gradients are the cotangents bit for bit and the row
 *     contributes exactly 0 to every particle.
 *   Guard.  For det P > 0 the forward's thin test keeps sigma_2 + s sigma_3 >= 1e-3 sigma_1; for an inverted neighbourhood
 *     (det P < 0) it can vanish, and G with it.  Where sigma_2 + s sigma_3 = tr(S) - sigma_1 < 1e-3 sigma_1 (the forward's
 *     thin constant, a design constant) the rotation's gradient is dropped: v_P = 0 and v_q = ct_q bit for bit, with the
 *     forward's R held constant (v_d0 = R^T ct_mu; the particles get w_k ct_mu).  bwd_status bit 0 reports such a row.
 *
 * The mean.  A bound Gaussian's position comes from d0 in the binding, not from `means`: v_means of a bound row is
 * DEFINED as v_d0, the derivative with the binding's neighbours and weights held fixed and d0 = mu - Xbar following the
 * mean.  A trained mean takes effect by adding its change to rest rows 0..2 (no re-bind).
 *
 * The forward's status is an INPUT: the kernel follows the branch the forward took (bits 0 / 3 pass-through, bit 2 thin,
 * otherwise rigid) instead of deciding again.  It must come from a mode-0 mgs_deform_apply on the same arguments.
 *
 * Two launches.
 *   1  one thread per Gaussian.  c and P are the forward's fp32 fma chains in the same order, the eigenpairs of P^T P the
 *      same fp64 Jacobi solve, so R is the forward's R bit for bit; the chain above runs in fp64.  Writes the rest
 *      gradients, and the 24 values v_x_k (3 each, k = 0..7), each rounded to fp32 once, into the workspace
 *      float [8][3][n] (neighbour-major); a pass-through row writes 24 zeros.  Every word of the workspace is written.
 *   2  one wave of 64 lanes per particle j, through the transposed binding
 *          t_start int32 [m + 1]   entries t_start[j] .. t_start[j + 1] - 1 of t_entry belong to particle j
 *          t_entry int32 [8 n]     k n + i for every (neighbour row k, Gaussian i) with idx[k][i] = j, ascending within j
 *      (a stable sort of idx by particle; entries of unbound Gaussians, idx -1, sort in front of t_start[0] and are never
 *      referenced).  Order of additions, per component, all fp32: lane l adds the workspace values of the entries
 *      t_start[j] + l, + 64, + 128, ... in that order, starting from +0; then the lanes are summed by a fixed xor tree,
 *      v += shuffle_xor(v, d) for d = 32, 16, 8, 4, 2, 1.  v_particles[j] of a particle nobody references is +0.
 *      An entry outside [0, 8 n) or a range outside t_entry is skipped, never followed. */
#ifndef MGS_DEFORM_BWD_H_
#define MGS_DEFORM_BWD_H_

#include "mgs_deform.h"

#ifdef __cplusplus
extern "C" {
#endif

/* Bytes of the workspace mgs_deform_apply_bwd needs for n Gaussians: float [8][3][n] (0 where n <= 0). */
size_t mgs_deform_apply_bwd_workspace_bytes(int n);

/* quats [n,4]: the REST quaternions the forward read.  idx, w, p, rest, flags: the binding.  status uint8 [n]: what the
 * forward wrote.  ct_means [n,3] / ct_quats [n,4] / ct_scales [n,3]: EACH nullable, null meaning zero.
 * v_means [n,3] / v_quats [n,4] / v_scales [n,3]: nullable as a set; they may not alias the cotangents.  v_particles [m,3]
 * is always written, all of it.  bwd_status uint8 [n], nullable: bit 0 the guard dropped this row's rotation gradient.
 * Alignment: quats, ct_quats and v_quats are read and written as 16-byte vectors.
 * workspace: 256-byte aligned, at least mgs_deform_apply_bwd_workspace_bytes(n); nothing in it need be initialised and
 * nothing in it outlives the call.
 * MGS_ERR_INVALID_ARGUMENT, before any launch: n < 0 or n > 2^28 - 1 (t_entry is int32); m < 8; quats, a binding array,
 * particles_now, status, t_start, t_entry, v_particles or workspace NULL; rest gradients given only in part; a workspace
 * that is too small.  n = 0 writes zeros to v_particles (one launch). */
int mgs_deform_apply_bwd(int n, const float *quats, const int32_t *idx, const float *w, const float *p, const float *rest,
                         const uint8_t *flags, int m, const float *particles_now, const uint8_t *status,
                         const float *ct_means, const float *ct_quats, const float *ct_scales,
                         const int32_t *t_start, const int32_t *t_entry,
                         float *v_means, float *v_quats, float *v_scales, float *v_particles,
                         uint8_t *bwd_status /* nullable [n] */, void *workspace, size_t workspace_bytes,
                         mgs_stream_t stream);

#ifdef __cplusplus
}
#endif
#endif /* MGS_DEFORM_BWD_H_ */
