/* mgs_deform_sh.h -- mgs_deform_apply that also turns each Gaussian's spherical-harmonics rows with it (csrc/deform.hip,
 * csrc/sh_rotate.h).  Compiled into the same libmgs.so / libmgs_debug.so and bound by the conventions of mgs.h and
 * mgs_deform.h, whose entry points and parameter lists it leaves as they are; the version is mgs.h's.  One launch, no
 * workspace, no atomics: the same inputs give the same bytes.  Capturable.
 *
 * The means, quats, scales and status this call writes are the bytes mgs_deform_apply writes for the same inputs.
 *
 * The rotation.  A Gaussian's SH rows rotate by R, the rotation the rigid branch of mgs_deform_apply applies: the argmax
 * over SO(3) of tr(R^T P), built from the eigenpairs of P^T P exactly as mgs_deform.h states it (u1, u2, u3, v3).  This holds
 * in both modes, and in mode 1 also for rows that did not fall back: the colour field turns with the neighbourhood's
 * rotation and does not shear, so colours are the same in mode 0 and mode 1.
 *
 * What a row of out_sh receives (rows are [coeff_stride][3] floats, coefficient-major, as everywhere in mgs.h).
 *   - A row whose status has bit 0, 2 or 3 (unbound, thin, a non-finite neighbour) receives its input row bit for bit.
 *   - In a rotated row coefficient 0 and every coefficient above the active degree, (sh_degree + 1)^2 .. coeff_stride - 1,
 *     are the input's bits.
 *   - Band l = 1 .. sh_degree (coefficients l^2 .. l^2 + 2l) becomes c'_l = M_l(R) c_l per channel, M_l the real-SH
 *     rotation in the renderer's ordering and signs: sum_k Y_k(d) c'_k = sum_k Y_k(R^T d) c_k for every d.
 *   - sh_degree 0 rotates nothing and copies by the same rule.
 * copy_unbound.  With 1, rows of Gaussians whose flag bit 0 is set are copied through.  With 0 they are not written at
 * all (the caller's buffer already holds them).  Rows of bound Gaussians are always written, rotated or copied: a row
 * rotated last frame and thin this frame returns to its rest bytes.
 *
 * The arithmetic, fp32 on R rounded to fp32 (row-major R_ab), every sum an fma chain in the order written, the first
 * term a product.  M_l is never formed.
 *   Band 1.  M_1 = Pi R Pi^T, Pi: (x, y, z) -> (-y, z, -x).  v = (-c_3, -c_1, c_2); u_a = R_a0 v_0 + R_a1 v_1 + R_a2 v_2;
 *   (c'_1, c'_2, c'_3) = (-u_y, u_z, -u_x).
 *   Bands 2 and 3.  The old colour field of the band is evaluated at 2l+1 fixed directions d_k turned by R^T and the
 *   samples are multiplied by a constant inverse:
 *       t = R^T d_k,  t_a = R_0a d_x + R_1a d_y + R_2a d_z;      F_k = sum_j Y_j(t) c_j  (j ascending);
 *       c'_m = sum_k W_mk F_k  (k ascending),  W = B^-1,  B_kj = Y_j(d_k)  (fp64, rounded to fp32 once).
 *   Y_j(t) is the band's basis in homogeneous form, so |t| = 1 is not assumed (with s = fma(x, x, y y), q = fma(4, z z, -s)):
 *       band 2:  K1 (x y) | -K1 (y z) | K2 fma(2, z z, -s) | -K1 (x z) | K3 fma(x, x, -y y)
 *       band 3:  K4 (y fma(-3, x x, y y)) | K5 ((x y) z) | -K6 (y q) | K7 (z fma(2, z z, -(3 s))) | -K6 (x q) |
 *                K8 (z fma(x, x, -y y)) | -K4 (x fma(-3, y y, x x))
 *       K1 = 1.092548430592079, K2 = 0.31539156525252, K3 = 0.5462742152960395, K4 = 0.5900435899266435,
 *       K5 = 2.890611442640554, K6 = 0.4570457994644658, K7 = 0.3731763325901154, K8 = 1.445305721320277.
 *   The directions d_k and W are the tables of csrc/sh_rotate.h (cond B = 1.55 for band 2, 1.74 for band 3).
 * Rows of 16 coefficients are staged through LDS, so that the 192-byte rows meet HBM lane-linearly, and only rows that
 * are written are fetched; shorter or longer rows are read and written per lane. */
#ifndef MGS_DEFORM_SH_H_
#define MGS_DEFORM_SH_H_

#include "mgs_deform.h"

#ifdef __cplusplus
extern "C" {
#endif

/* The first sixteen parameters are mgs_deform_apply's.  sh_coeffs and out_sh: [n, coeff_stride, 3] floats.
 * MGS_ERR_INVALID_ARGUMENT, before any launch: everything mgs_deform_apply refuses; sh_degree outside 0..3;
 * coeff_stride < (sh_degree + 1)^2; sh_coeffs or out_sh NULL; out_sh == sh_coeffs.  n = 0 enqueues nothing.  One launch. */
int mgs_deform_apply_sh(int n, const float *means, const float *quats, const float *scales, const int32_t *idx,
                        const float *w, const float *p, const float *rest, const uint8_t *flags, int mode, int m,
                        const float *particles_now, float *out_means, float *out_quats, float *out_scales,
                        uint8_t *status /* nullable [n] */, int sh_degree, int coeff_stride,
                        const float *sh_coeffs /* [n,coeff_stride,3] */, float *out_sh, int copy_unbound,
                        mgs_stream_t stream);

#ifdef __cplusplus
}
#endif
#endif /* MGS_DEFORM_SH_H_ */
