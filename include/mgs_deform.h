/* mgs_deform.h -- C ABI of deforming Gaussians with simulated particles (csrc/deform.hip): bind once, move per frame.
 * Compiled into the same libmgs.so / libmgs_debug.so as include/mgs.h's render path and bound by the same conventions
 * (see the top of mgs.h): device pointers unless marked "host", the caller owns every buffer, all work is enqueued on
 * `stream`, nothing synchronises or reads a value back, every call is capturable in a hipGraph, and the return value is
 * 0, <0 MGS_ERR_* or >0 a hipError_t from a launch.  The version is mgs.h's: this header adds entry points and changes no
 * parameter list.  No floating-point atomic anywhere: the same inputs give the same bytes in every run.
 *
 * A soft object is n Gaussians (means [n,3], quats [n,4] wxyz, scales [n,3], activated) and m particles of a simulator
 * ([m,3] fp32).  mgs_deform_bind, once per object, ties every Gaussian to its MGS_DEFORM_K = 8 nearest particles of the
 * rest state; mgs_deform_apply, once per frame, moves the Gaussians with the particles' current positions: a rotation by
 * shape matching (Mueller et al. 2005) or the affine map of the neighbourhood with Sigma' = A Sigma A^T (PhysGaussian).
 * Opacities and colours are not touched and SH rows are not rotated (what mgs_transform_gaussians does without SH rows);
 * mgs_deform_sh.h adds the call that also turns each Gaussian's SH rows.
 *
 * The binding arrays are neighbour-major, so that one thread per Gaussian reads coalesced (N = n):
 *     idx    int32 [8][N]      neighbour indices, row 0 the nearest (the anchor); -1 in every row of an unbound Gaussian
 *     w      float [8][N]      weights, sum 1
 *     p      float [8][3][N]   weighted rest offsets p_j = w_j (X_j - Xbar)
 *     rest   float [12][N]     rows 0..2 d0 = mu - Xbar | 3..8 Q^-1 as xx xy xz yy yz zz | 9 h^2 | 10 lambda_mid / lambda_max |
 *                              11 lambda_min / lambda_max
 *     flags  uint8 [N]         bit 0 unbound | bit 1 flat | bit 2 thin
 *
 * ---- mgs_deform_bind ----
 * Eligibility.  A particle with a non-finite coordinate is nobody's neighbour.  A Gaussian is eligible if select is null
 * or select[i] != 0, and its mean is finite.  If fewer than 8 finite particles exist, nobody is bound.
 * Distances.  d2_ij is fp32, fma(dz, dz, fma(dy, dy, dx * dx)) of the fp32 differences (never the expanded form).  A pair
 * whose d2 is not below +inf (an overflow) is not a neighbour.
 * Neighbours.  The 8 smallest by the key (d2, j), ascending: a tie in d2 goes to the lower index, so the result is the
 * same under any tiling.  (The particle set is not split across workgroups: one workgroup walks all of it for its 256
 * Gaussians, so there is no merge pass.)
 * Unbound.  A Gaussian that is ineligible, or whose sqrtf(d2_i0) > max_distance (+inf switches the test off), gets idx -1,
 * zeros in w, p and rest, and flag bit 0.
 * Weights and moments, fp64 on the fp32 inputs, every stored value rounded to fp32 once:
 *     h^2 = d2_i7,  wt_j = exp(-d2_ij / h^2) (all 1 where h^2 = 0),  w_j = wt_j / sum wt,  Xbar = sum w_j X_j,
 *     r_j = X_j - Xbar,  p_j = w_j r_j,  Q = sum w_j r_j r_j^T,  d0 = mu_i - Xbar.
 * Q's eigenvalues lambda_min <= lambda_mid <= lambda_max come from a cyclic Jacobi solve in fp64.
 * Flag bit 1, flat (a sheet of cloth): lambda_min < 1e-3 lambda_max; the Q^-1 rows are zero (also where lambda_max = 0).
 * Flag bit 2, thin (a strand): lambda_mid < 1e-3 lambda_max, or lambda_max = 0.  The threshold is a design constant:
 * inverting Q amplifies P's fp32 rounding by at most 1 / 1e-3, which leaves A good to about 1e-4.
 *
 * ---- mgs_deform_apply ---- one launch, no workspace; per Gaussian, with x_j = particles_now[idx_j]:
 * Status (nullable uint8 [n]): bit 0 unbound | bit 1 affine fell back to rigid | bit 2 thin: translated only | bit 3 a
 * current neighbour position was non-finite.
 * Pass-through.  An unbound Gaussian (status bit 0), or one with a non-finite x_j or an idx_j outside [0, m) (status bit
 * 3), gets outputs that are its inputs bit for bit.
 * Shared.  e_j = x_j - x_0 in fp32; c = sum_{j=1..7} w_j e_j; xbar = x_0 + c; P = sum_{j=1..7} e_j p_j^T; both sums are fp32
 * fma chains in order of j (the first term a product).
 * Thin.  Flag bit 2, or this frame's sigma_mid(P) < 1e-3 sigma_max(P) (or sigma_max = 0): mu' = xbar + d0, quats and scales
 * bit-identical, status bit 2.  The singular values are the roots of the eigenvalues of P^T P (fp64 Jacobi).
 * Rigid (mode 0; also a flat Gaussian in mode 1 or det A <= 0 there, both with status bit 1).  R = argmax over SO(3) of
 * tr(R^T P): with V, lambda the eigenpairs of P^T P in descending order, u1 = P v1 / sqrt(lambda1), u2 = P v2 made
 * orthonormal to u1, u3 = u1 x u2, v3 = v1 x v2, R = sum u_k v_k^T (no inverse, unique for a P of rank 2).
 * mu' = xbar + R d0, q' = normalise(q_R (x) q) (Hamilton, wxyz), scales bit-identical.
 * Affine (mode 1).  A = P Q^-1 in fp32, mu' = xbar + A d0, M = A R(q) diag(s) and Sigma' = M M^T in fp64, Jacobi of
 * Sigma': s'_k = sqrt(max(lambda_k, 0)) in ascending order, floored at the smallest positive normal float, q' from the
 * eigenvector matrix with its third column negated where that makes it proper. */
#ifndef MGS_DEFORM_H_
#define MGS_DEFORM_H_

#include "mgs.h"

#define MGS_DEFORM_K 8

#ifdef __cplusplus
extern "C" {
#endif

/* Bytes of the workspace mgs_deform_bind needs for n Gaussians and m particles (0 where n <= 0 or m < 8). */
size_t mgs_deform_bind_workspace_bytes(int n, int m);

/* workspace: 256-byte aligned, at least mgs_deform_bind_workspace_bytes(n, m); nothing in it need be initialised and
 * nothing in it outlives the call.  MGS_ERR_INVALID_ARGUMENT, before any launch: n < 0; m < 8; means, particles_rest,
 * workspace or an output NULL; a workspace that is too small; a max_distance that is NaN or <= 0.  n = 0 enqueues nothing.
 * Two launches. */
int mgs_deform_bind(int n, const float *means, const uint8_t *select /* nullable [n] */, int m,
                    const float *particles_rest, float max_distance, void *workspace, size_t workspace_bytes,
                    int32_t *idx, float *w, float *p, float *rest, uint8_t *flags, mgs_stream_t stream);

/* mode: 0 rigid, 1 affine.  The outputs must not alias the inputs.  MGS_ERR_INVALID_ARGUMENT, before any launch: n < 0;
 * m < 8; a mode that is neither; any pointer but status NULL.  n = 0 enqueues nothing.  One launch. */
int mgs_deform_apply(int n, const float *means, const float *quats, const float *scales, const int32_t *idx,
                     const float *w, const float *p, const float *rest, const uint8_t *flags, int mode, int m,
                     const float *particles_now, float *out_means, float *out_quats, float *out_scales,
                     uint8_t *status /* nullable [n] */, mgs_stream_t stream);

#ifdef __cplusplus
}
#endif
#endif /* MGS_DEFORM_H_ */
