/* mgs_pose.h -- C ABI of the backward of mgs_transform_gaussians (csrc/pose.hip): the gradient of a loss with respect to
 * the pose of every group of Gaussians, and with respect to the Gaussians at rest.
 * Compiled into the same libmgs.so / libmgs_debug.so as include/mgs.h's render path and bound by the same conventions
 * (see the top of mgs.h): device pointers unless marked "host", the caller owns every buffer, all work is enqueued on
 * `stream`, nothing synchronises or reads a value back, every call is capturable in a hipGraph, and the return value is
 * 0, <0 MGS_ERR_* or >0 a hipError_t from a launch.  The version is mgs.h's: this header adds entry points and changes no
 * parameter list.
 *
 * Forward (mgs.h, "Similarity transforms"), for a Gaussian of group g with xforms[g] = { M = s R, t, q_R, s }:
 *     p' = s R p + t,   q' = q_R (x) q,   sigma' = s sigma,   c'_l = M_l(R) c_l  for the SH degrees l = 1..sh_degree.
 * With ct_* the cotangents of the posed outputs, the pose gradient is taken in the tangent space at the current pose,
 * under R <- exp([d_omega]x) R, t <- t + d_t, s <- s exp(d_lambda).  Per group, summed over its members:
 *     v_omega  = sum (p' - t) x ct_p + 1/2 sum_k e_k <ct_q, e_k (x) q'> + sum_l sum_ch sum_k e_k <ct_c, L_k^(l) c'>
 *     v_t      = sum ct_p
 *     v_lambda = sum <ct_p, p' - t> + sum <ct_sigma, sigma'>
 * where e_k is the k-th unit vector (as a quaternion the pure unit (0, e_k)) and L_k^(l) = d/d_eps M_l(exp(eps [e_k]x)) at
 * eps = 0 are the constant antisymmetric generators of the real-SH rotation in the renderer's basis.  Only posed values
 * and cotangents enter.  Per Gaussian, the gradient of the rest pose:
 *     v_p = (s R)^T ct_p,   v_q = conj(q_R) (x) ct_q,   v_sigma = s ct_sigma,   v_c,l = M_l^T ct_c,l
 * and the DC term, coefficients above sh_degree and every row of a Gaussian that does not move (group id outside
 * [0, n_groups)) take their cotangent bit for bit.
 *
 * v_pose[n_groups,8] = { v_omega[3], v_t[3], v_lambda, 0 }.  A group without members gets a row of zeros.  Each wave of 64
 * consecutive Gaussians reduces its addends per group id present with a fixed shuffle tree and stores one partial row
 * per id; each group's rows are then summed in fp64 in a fixed order (per chunk of 64 waves, then over the chunks).  No
 * floating-point atomic anywhere: the result is the same bits in every run.  The call writes every word of the workspace
 * that it reads, and all of v_pose. */
#ifndef MGS_POSE_H_
#define MGS_POSE_H_

#include "mgs.h"

#ifdef __cplusplus
extern "C" {
#endif

/* Bytes of the workspace mgs_pose_bwd needs for n Gaussians in n_groups groups (0 where n < 0 or n_groups < 1): one
 * count per wave, min(64, n_groups) partial rows of 32 bytes per wave, and 64 bytes per group and chunk of 64 waves. */
size_t mgs_pose_bwd_workspace_bytes(int n, int n_groups);

/* means / quats / scales / sh_coeffs: the POSED outputs of mgs_transform_gaussians ([n,3], [n,4], [n,3],
 * [n,coeff_stride,3]; sh_coeffs nullable = the SH rows were not rotated, then sh_rot, ct_sh and v_sh must be null too).
 * group_ids (nullable = all in group 0), xforms[n_groups,20] and sh_rot[n_groups,84] (needed for sh_degree >= 1 with SH
 * rows) are what the forward read.
 * ct_means / ct_quats / ct_scales / ct_sh: cotangents of the posed outputs, EACH nullable, null meaning zero.
 * v_means / v_quats / v_scales (and v_sh where there are SH rows): the rest-pose gradients, nullable as a set; they may
 * not alias the cotangents.  v_pose[n_groups,8] is always written.
 * Alignment: quats, ct_quats and v_quats are read and written as 16-byte vectors, and so are sh_coeffs, ct_sh and v_sh
 * when coeff_stride is 16: these pointers must be 16-byte aligned (every other array: 4 bytes).
 * workspace: 256-byte aligned, at least mgs_pose_bwd_workspace_bytes(n, n_groups); nothing in it need be initialised and
 * nothing in it outlives the call.
 * MGS_ERR_INVALID_ARGUMENT, before any launch: n < 0; n_groups < 1; means, quats, scales, xforms, v_pose or workspace
 * NULL; sh_degree outside 0..3 or coeff_stride < (sh_degree + 1)^2 with SH rows; sh_rot NULL where it is needed; SH
 * cotangent or gradient without SH rows; rest-pose gradients given only in part; a workspace that is too small.
 * Three launches.  Cost of the reduce: the second launch runs one wave per (group, 64 waves of the first) whose lanes
 * scan their wave's rows for the group's id, so it reads n / 64 * n_groups * (ids per wave) * 32 bytes: nothing beside
 * the pass for scenes stored part by part (one or two ids per wave), but with 70 groups mixed in every wave of 1 M
 * Gaussians of the order of 1-2 GB -- more than the pass itself.  Order such a scene by part. */
int mgs_pose_bwd(int n, const float *means, const float *quats, const float *scales,
                 int sh_degree, int coeff_stride, const float *sh_coeffs /* nullable */,
                 const int32_t *group_ids /* nullable */, int n_groups, const float *xforms,
                 const float *sh_rot /* nullable */,
                 const float *ct_means, const float *ct_quats, const float *ct_scales, const float *ct_sh,
                 float *v_means, float *v_quats, float *v_scales, float *v_sh,
                 float *v_pose /* [n_groups,8] */, void *workspace, size_t workspace_bytes, mgs_stream_t stream);

#ifdef __cplusplus
}
#endif
#endif /* MGS_POSE_H_ */
