/* mgs_register.h -- C ABI of point-set registration: ICP with a radius-bounded nearest-neighbour search on a uniform grid
 * (csrc/register.hip).  Compiled into the same libmgs.so / libmgs_debug.so as include/mgs.h's render path and bound by the
 * same conventions (see the top of mgs.h and mgs_hinge.h): device pointers unless marked "host", the caller owns every
 * buffer, all work is enqueued on `stream`, nothing synchronises or reads a value back, every call is capturable in a
 * hipGraph, and the return value is 0, <0 MGS_ERR_* or >0 a hipError_t from a launch.  The version is mgs.h's: this header
 * adds entry points and changes no parameter list.
 *
 * Semantics.  source P (n_s points) and target Q (n_t points) are fp32 [n,3] arrays; a point with a non-finite coordinate
 * takes no part (flag bit 1 records that one was seen).  T = (s, R, t) maps x to s R x + t, in fp64.
 *   Matching under T.  p'_i = s R p_i + t in fp64, rounded once to fp32.  c_i = argmin over the finite q_j of
 * |p'_i - q_j|^2, each pair as fma(dz, dz, fma(dy, dy, dx * dx)) of the fp32 differences (mgs_hinge.h's form); ties go to
 * the lowest j.  i is an inlier iff that minimum is <= limit2 = max_distance * max_distance (fp32); otherwise c_i = -1 and
 * distance2_i = +inf.  The grid only finds that answer faster: it is the brute-force one.
 *   rmse(T) = sqrt(sum over inliers of |s R p_i + t - q_ci|^2 / n_in) with the residual in fp64 (0 where n_in = 0),
 * fitness = n_in / (number of finite source points) (0 where there is none).
 *   Update from the inliers (Kabsch / Umeyama, absolute): with the inlier means pm, qm and S = sum (q - qm)(p - pm)^T over
 * the original fp32 points in fp64, R' = argmax over SO(3) of tr(R'^T S) (never a reflection), s' = tr(R'^T S) /
 * sum |p - pm|^2 with with_scale and 1 without, t' = qm - s' R' pm.  Where there are fewer than 3 inliers, or the inlier
 * covariance of either set has a second eigenvalue <= 1e-12 x its first (collinear), or S itself has rank below 2 so that
 * no rotation comes out finite, the rotation is undetermined: flag bit 0 is set, T is left as it is and the loop ends.
 *   Loop, k = 0 .. iterations-1: match under T_k; history row k = [n_in, rmse(T_k), s_k, 0]; update to T_k+1; where k > 0
 * and |rmse_k - rmse_k-1| <= tol * rmse_k-1 the update is applied, `converged` is set and the loop ends.  History rows past
 * the last executed iteration are not written.  A last matching pass under the final T gives correspondence, distance2,
 * rmse, fitness and n_inliers: iterations = 0 is a pure radius-bounded nearest-neighbour query under `init`.
 *   All sums are fp64, taken about fixed pivots (the first finite source point, the low corner of the target's bounds) as
 * per-workgroup partial sums reduced in a fixed order (index order inside eight ranges of workgroups, then the ranges in
 * order), so a permutation of the target permutes the correspondences and changes nothing else; the bounds, the cell
 * counts and the scatter use integer atomics only.  No floating-point atomic anywhere: the outputs are the same bytes in
 * every run.
 *
 * result[32], doubles:  0..8 R (row-major) | 9..11 t | 12 s | 13 rmse | 14 fitness | 15 n_inliers | 16 iterations executed |
 *                       17 converged | 18 flags (bit 0: rotation undetermined, bit 1: a non-finite point was skipped) |
 *                       19 cell edge used | 20..22 grid dims (x, y, z) | 23..31 zero. */
#ifndef MGS_REGISTER_H_
#define MGS_REGISTER_H_

#include "mgs.h"

#ifdef __cplusplus
extern "C" {
#endif

/* Bytes of the workspace mgs_register_icp needs (0 where n_s or n_t is not positive or iterations is outside 0..256).  It
 * depends on these three numbers only: the cell table has a fixed capacity. */
size_t mgs_register_workspace_bytes(int n_s, int n_t, int iterations);

/* init: 13 doubles R (row-major) | t | s, NULL for the identity.  workspace: 256-byte aligned, at least
 * mgs_register_workspace_bytes(n_s, n_t, iterations); nothing in it need be initialised and nothing in it outlives the
 * call.  correspondence [n_s] (nullable), distance2 [n_s] (nullable), history [iterations,4] (nullable), result [32].
 * MGS_ERR_INVALID_ARGUMENT, before any launch: n_s <= 0 or n_t <= 0; source, target, result or workspace NULL; a workspace
 * that is misaligned or too small; max_distance not finite or <= 0; tol not finite or < 0; iterations outside 0..256.
 * One memset node and 8 + 2 * (iterations + 1) launches, a linear chain. */
int mgs_register_icp(int n_s, const float *source, int n_t, const float *target, float max_distance,
                     int iterations, int with_scale, double tol, const double *init /* nullable [13] */,
                     void *workspace, size_t workspace_bytes,
                     int32_t *correspondence /* nullable [n_s] */, float *distance2 /* nullable [n_s] */,
                     double *history /* nullable [iterations,4] */, double *result /* [32] */, mgs_stream_t stream);

#ifdef __cplusplus
}
#endif
#endif /* MGS_REGISTER_H_ */
