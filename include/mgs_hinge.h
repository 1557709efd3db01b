/* mgs_hinge.h -- C ABI of fitting the hinge of an articulated part from two point sets (csrc/hinge.hip).
 * Compiled into the same libmgs.so / libmgs_debug.so as include/mgs.h's render path and bound by the same conventions
 * (see the top of mgs.h): device pointers unless marked "host", the caller owns every buffer, all work is enqueued on
 * `stream`, nothing synchronises or reads a value back, every call is capturable in a hipGraph, and the return value is
 * 0, <0 MGS_ERR_* or >0 a hipError_t from a launch.  The version is mgs.h's: this header adds entry points and changes no
 * parameter list.
 *
 * Semantics.  A (the moving part, n_a points) and B (n_b points) are fp32 [n,3] arrays.  A point with a non-finite
 * coordinate takes no part: it is never contact and never anyone's neighbour.
 *     nn2_A[i] = min over j of |a_i - b_j|^2,   nn2_B[j] = min over i of |b_j - a_i|^2
 * in fp32, each pair as fma(dz, dz, fma(dy, dy, dx * dx)) of the fp32 differences (never the expanded form); a minimum
 * does not depend on order, so nn2 is the same bits under any tiling.  min2 = min over i of nn2_A[i], min_distance =
 * sqrtf(min2).  A point of EITHER set is contact iff sqrtf(nn2) < sqrtf(min2) + threshold (both sets use A's minimum).
 *     position = (mean(contact A) + mean(contact B)) / 2
 * and the axis is the unit eigenvector of the largest eigenvalue of the covariance (n - 1 denominator) of all contact
 * points together, its component of largest magnitude positive (ties: the lowest index); axis_confidence = lambda_max /
 * sum of lambda.  Where that is below 0.5 (or undefined) the axis is (1, 0, 0) and flag bit 0 is set.
 * The moments are accumulated in fp64 about the first finite point of A, as per-workgroup partial sums reduced in index
 * order: no floating-point atomic anywhere, so the record is the same bytes in every run.  The 3x3 eigenproblem is solved
 * on the device in fp64 (cyclic Jacobi).
 *
 * joint[16], doubles:  0..2 position | 3..5 axis | 6 axis_confidence | 7 min_distance | 8 n_contact_a | 9 n_contact_b |
 *                      10..12 the covariance's eigenvalues, ascending | 13 flags (bit 0: fallback axis used, bit 1: some
 *                      point was non-finite and skipped) | 14, 15 zero. */
#ifndef MGS_HINGE_H_
#define MGS_HINGE_H_

#include "mgs.h"

#ifdef __cplusplus
extern "C" {
#endif

/* Bytes of the workspace mgs_hinge_fit needs for sets of n_a and n_b points (0 where either is not positive). */
size_t mgs_hinge_workspace_bytes(int n_a, int n_b);

/* contact_a[n_a] / contact_b[n_b] (nullable) receive 1 for a contact point and 0 otherwise.  workspace: 256-byte aligned,
 * at least mgs_hinge_workspace_bytes(n_a, n_b); nothing in it need be initialised and nothing in it outlives the call.
 * MGS_ERR_INVALID_ARGUMENT, before any launch: n_a <= 0 or n_b <= 0; pts_a, pts_b, joint or workspace NULL; a workspace
 * that is too small; a threshold that is not finite or <= 0.  One memset node and four launches. */
int mgs_hinge_fit(int n_a, const float *pts_a, int n_b, const float *pts_b, float threshold,
                  void *workspace, size_t workspace_bytes,
                  uint8_t *contact_a /* nullable [n_a] */, uint8_t *contact_b /* nullable [n_b] */,
                  double *joint /* [16] */, mgs_stream_t stream);

#ifdef __cplusplus
}
#endif
#endif /* MGS_HINGE_H_ */
