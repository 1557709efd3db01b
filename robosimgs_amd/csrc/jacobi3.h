// jacobi3.h -- the symmetric 3x3 eigenproblem in fp64 by cyclic Jacobi sweeps, shared by hinge.hip (the covariance of the
// contact set), deform.hip (a neighbourhood's moment matrix) and deform_shape.h (P^T P and a deformed covariance, once per
// Gaussian).
// Scalars throughout and every index a compile-time constant: each entry stays in a register, no scratch.
#ifndef MGS_JACOBI3_H_
#define MGS_JACOBI3_H_

#include <math.h>

#if defined(__HIPCC__)
namespace mgs {

// one Jacobi rotation of a symmetric 3x3 matrix that zeroes its (p, q) entry; r is the third index, and v's columns p and q
// follow.
__device__ __forceinline__ void jacobi_rotate(double& app, double& aqq, double& apq, double& arp, double& arq, double& v0p,
                                              double& v0q, double& v1p, double& v1q, double& v2p, double& v2q) {
  if (apq == 0.0) return;
  const double theta = (aqq - app) / (2.0 * apq);
  const double tn = (theta < 0.0 ? -1.0 : 1.0) / (fabs(theta) + sqrt(theta * theta + 1.0));
  const double c = 1.0 / sqrt(tn * tn + 1.0), sn = tn * c;
  app -= tn * apq;
  aqq += tn * apq;
  apq = 0.0;
  double x = arp, y = arq;
  arp = c * x - sn * y; arq = sn * x + c * y;
  x = v0p; y = v0q; v0p = c * x - sn * y; v0q = sn * x + c * y;
  x = v1p; y = v1q; v1p = c * x - sn * y; v1q = sn * x + c * y;
  x = v2p; y = v2q; v2p = c * x - sn * y; v2q = sn * x + c * y;
}

// Up to 16 sweeps over (0,1), (0,2), (1,2), ended as soon as every off-diagonal entry is exactly zero (the entries fall
// quadratically and underflow: about ten sweeps at the most).  On return a00, a11, a22 are the eigenvalues in no particular
// order and column k of v (v0k, v1k, v2k) is the unit eigenvector of akk; v starts as the identity.
__device__ __forceinline__ void jacobi_solve3(double& a00, double& a01, double& a02, double& a11, double& a12, double& a22,
                                              double& v00, double& v01, double& v02, double& v10, double& v11, double& v12,
                                              double& v20, double& v21, double& v22) {
  v00 = 1.0; v01 = 0.0; v02 = 0.0; v10 = 0.0; v11 = 1.0; v12 = 0.0; v20 = 0.0; v21 = 0.0; v22 = 1.0;
#pragma unroll 1
  for (int sweep = 0; sweep < 16; ++sweep) {
    if (a01 == 0.0 && a02 == 0.0 && a12 == 0.0) break;
    jacobi_rotate(a00, a11, a01, a02, a12, v00, v01, v10, v11, v20, v21);        // (0, 1), r = 2
    jacobi_rotate(a00, a22, a02, a01, a12, v00, v02, v10, v12, v20, v22);        // (0, 2), r = 1
    jacobi_rotate(a11, a22, a12, a01, a02, v01, v02, v11, v12, v21, v22);        // (1, 2), r = 0
  }
}

}  // namespace mgs
#endif
#endif  // MGS_JACOBI3_H_
