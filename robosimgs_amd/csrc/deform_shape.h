// deform_shape.h -- the shape-matching core of deform.hip, device-only: what deform_apply_kernel and deform_apply_bwd_kernel
// both compute, defined once.  The backward is only right if it rebuilds the forward's rotation bit for bit, so both
// kernels call THESE functions: the neighbour gather, the fp32 moment P, the eigenpairs of P^T P, the rotation and the
// quaternion product.  An edit here reaches both; do not re-associate an expression (the contraction the compiler picks
// is part of the result).
// Matrices and quaternions are structs of named scalars, passed by value or const reference and always inlined: every
// member stays in a register.  No member is an array -- an indexed private array becomes scratch; the per-neighbour
// arrays are the callers' locals, walked by fully unrolled loops only.
#ifndef MGS_DEFORM_SHAPE_H_
#define MGS_DEFORM_SHAPE_H_

#include "jacobi3.h"
#include "../../include/mgs_deform.h"

#if defined(__HIPCC__)
namespace mgs {

constexpr int kK = MGS_DEFORM_K;

struct Mat3d { double m00, m01, m02, m10, m11, m12, m20, m21, m22; };      // row-major names
struct Mat3f { float m00, m01, m02, m10, m11, m12, m20, m21, m22; };
struct Sym3d { double m00, m01, m02, m11, m12, m22; };
struct Quatd { double w, x, y, z; };
struct Eig3 { double l0, l1, l2; Mat3d v; };        // eigenvalue lk belongs to column k of v (m0k, m1k, m2k)
struct Moment { Mat3f P; float c0, c1, c2; };

__device__ __forceinline__ bool finite3(float x, float y, float z) { return isfinite(x) && isfinite(y) && isfinite(z); }
__device__ __forceinline__ Mat3d widen(const Mat3f& a) {
  return {a.m00, a.m01, a.m02, a.m10, a.m11, a.m12, a.m20, a.m21, a.m22};
}
__device__ __forceinline__ Mat3d transposed(const Mat3d& a) {
  return {a.m00, a.m10, a.m20, a.m01, a.m11, a.m21, a.m02, a.m12, a.m22};
}

// The 8 current positions of Gaussian i's neighbours, the only random access; false where an index is outside 0..m-1
// (position 0 is read in its place) or, with FINITE, a position is not finite.  The forward asks with FINITE and records
// the answer in its status; the backward follows that status and asks only that nothing be followed out of range.
template <bool FINITE>
__device__ __forceinline__ bool gather_neighbours(const int32_t* idx, size_t N, long long i, int m, const float* now,
                                                  float (&x)[kK][3]) {
  bool ok = true;
#pragma unroll
  for (int k = 0; k < kK; ++k) {
    const int j = idx[k * N + i];
    const bool in = j >= 0 && j < m;
    const size_t jj = in ? (size_t)j : 0;
    x[k][0] = now[3 * jj + 0]; x[k][1] = now[3 * jj + 1]; x[k][2] = now[3 * jj + 2];
    if constexpr (FINITE) ok = ok && in && finite3(x[k][0], x[k][1], x[k][2]);
    else ok = ok && in;
  }
  return ok;
}

// P = sum e_k p_k^T over k = 1..7, e_k = x_k - x_0: an fp32 fma chain in order of k, the first term a plain product.
// WITH_C (the forward): also c = sum w_k e_k, the same way; wk and pk are not touched.  Without (the backward, where c has
// no part): wk and pk receive the weights and weighted rest offsets that were loaded (row 0: zeros), so that they stay in
// registers for the 24 contributions.
template <bool WITH_C>
__device__ __forceinline__ Moment moment_P(const float (&x)[kK][3], const float* w, const float* p, size_t N, long long i,
                                           float (&wk)[kK], float (&pk)[kK][3]) {
  Moment o = {};
  Mat3f& P = o.P;
  if constexpr (!WITH_C) { wk[0] = 0.f; pk[0][0] = 0.f; pk[0][1] = 0.f; pk[0][2] = 0.f; }
#pragma unroll
  for (int k = 1; k < kK; ++k) {
    const float e0 = x[k][0] - x[0][0], e1 = x[k][1] - x[0][1], e2 = x[k][2] - x[0][2];
    const float wt = w[k * N + i];
    const float pk0 = p[(3 * k + 0) * N + i], pk1 = p[(3 * k + 1) * N + i], pk2 = p[(3 * k + 2) * N + i];
    if constexpr (!WITH_C) { wk[k] = wt; pk[k][0] = pk0; pk[k][1] = pk1; pk[k][2] = pk2; }
    if (k == 1) {
      if constexpr (WITH_C) { o.c0 = wt * e0; o.c1 = wt * e1; o.c2 = wt * e2; }
      P.m00 = e0 * pk0; P.m01 = e0 * pk1; P.m02 = e0 * pk2;
      P.m10 = e1 * pk0; P.m11 = e1 * pk1; P.m12 = e1 * pk2;
      P.m20 = e2 * pk0; P.m21 = e2 * pk1; P.m22 = e2 * pk2;
    } else {
      if constexpr (WITH_C) {
        o.c0 = __builtin_fmaf(wt, e0, o.c0); o.c1 = __builtin_fmaf(wt, e1, o.c1); o.c2 = __builtin_fmaf(wt, e2, o.c2);
      }
      P.m00 = __builtin_fmaf(e0, pk0, P.m00); P.m01 = __builtin_fmaf(e0, pk1, P.m01); P.m02 = __builtin_fmaf(e0, pk2, P.m02);
      P.m10 = __builtin_fmaf(e1, pk0, P.m10); P.m11 = __builtin_fmaf(e1, pk1, P.m11); P.m12 = __builtin_fmaf(e1, pk2, P.m12);
      P.m20 = __builtin_fmaf(e2, pk0, P.m20); P.m21 = __builtin_fmaf(e2, pk1, P.m21); P.m22 = __builtin_fmaf(e2, pk2, P.m22);
    }
  }
  return o;
}

// P^T P (M M^T is gram(transposed(M)))
__device__ __forceinline__ Sym3d gram(const Mat3d& p) {
  return {p.m00 * p.m00 + p.m10 * p.m10 + p.m20 * p.m20, p.m00 * p.m01 + p.m10 * p.m11 + p.m20 * p.m21,
          p.m00 * p.m02 + p.m10 * p.m12 + p.m20 * p.m22, p.m01 * p.m01 + p.m11 * p.m11 + p.m21 * p.m21,
          p.m01 * p.m02 + p.m11 * p.m12 + p.m21 * p.m22, p.m02 * p.m02 + p.m12 * p.m12 + p.m22 * p.m22};
}

// exchange the eigenpairs a and b (the eigenvalue and column of v)
__device__ __forceinline__ void swap_pair(double& la, double& lb, double& va0, double& va1, double& va2, double& vb0,
                                          double& vb1, double& vb2) {
  double t = la; la = lb; lb = t;
  t = va0; va0 = vb0; vb0 = t; t = va1; va1 = vb1; vb1 = t; t = va2; va2 = vb2; vb2 = t;
}

// The eigenpairs of a symmetric matrix (jacobi3.h), sorted by three conditional exchanges.  Solved and sorted on local
// scalars, a struct only at the return: exchanging struct members made the compiler repeat a comparison in the backward.
template <bool DESCENDING>
__device__ __forceinline__ Eig3 eigen_sorted(const Sym3d& a) {
  double a00 = a.m00, a01 = a.m01, a02 = a.m02, a11 = a.m11, a12 = a.m12, a22 = a.m22;
  double v00, v01, v02, v10, v11, v12, v20, v21, v22;
  jacobi_solve3(a00, a01, a02, a11, a12, a22, v00, v01, v02, v10, v11, v12, v20, v21, v22);
  if (DESCENDING ? a00 < a11 : a00 > a11) swap_pair(a00, a11, v00, v10, v20, v01, v11, v21);
  if (DESCENDING ? a11 < a22 : a11 > a22) swap_pair(a11, a22, v01, v11, v21, v02, v12, v22);
  if (DESCENDING ? a00 < a11 : a00 > a11) swap_pair(a00, a11, v00, v10, v20, v01, v11, v21);
  return {a00, a11, a22, {v00, v01, v02, v10, v11, v12, v20, v21, v22}};
}

// the eigenpairs of P^T P, descending: l0 = sigma_1^2
__device__ __forceinline__ Eig3 gram_eigen_desc(const Mat3d& p) { return eigen_sorted<true>(gram(p)); }

// R = argmax over SO(3) of tr(R^T P) from the eigenpairs of P^T P (descending): u1 = P v1 / sigma1, u2 = P v2 made
// orthonormal to u1, u3 = u1 x u2, v3 = v1 x v2 (w below), R = sum u_k v_k^T
__device__ __forceinline__ Mat3d shape_rotation(const Mat3d& p, const Eig3& e) {
  const Mat3d& v = e.v;
  const double is1 = 1.0 / sqrt(e.l0);
  const double u10 = (p.m00 * v.m00 + p.m01 * v.m10 + p.m02 * v.m20) * is1;
  const double u11 = (p.m10 * v.m00 + p.m11 * v.m10 + p.m12 * v.m20) * is1;
  const double u12 = (p.m20 * v.m00 + p.m21 * v.m10 + p.m22 * v.m20) * is1;
  double u20 = p.m00 * v.m01 + p.m01 * v.m11 + p.m02 * v.m21, u21 = p.m10 * v.m01 + p.m11 * v.m11 + p.m12 * v.m21;
  double u22 = p.m20 * v.m01 + p.m21 * v.m11 + p.m22 * v.m21;
  const double dot = u10 * u20 + u11 * u21 + u12 * u22;
  u20 -= dot * u10; u21 -= dot * u11; u22 -= dot * u12;
  const double in2 = 1.0 / sqrt(u20 * u20 + u21 * u21 + u22 * u22);
  u20 *= in2; u21 *= in2; u22 *= in2;
  const double u30 = u11 * u22 - u12 * u21, u31 = u12 * u20 - u10 * u22, u32 = u10 * u21 - u11 * u20;
  const double w0 = v.m10 * v.m21 - v.m20 * v.m11, w1 = v.m20 * v.m01 - v.m00 * v.m21, w2 = v.m00 * v.m11 - v.m10 * v.m01;
  return {u10 * v.m00 + u20 * v.m01 + u30 * w0, u10 * v.m10 + u20 * v.m11 + u30 * w1, u10 * v.m20 + u20 * v.m21 + u30 * w2,
          u11 * v.m00 + u21 * v.m01 + u31 * w0, u11 * v.m10 + u21 * v.m11 + u31 * w1, u11 * v.m20 + u21 * v.m21 + u31 * w2,
          u12 * v.m00 + u22 * v.m01 + u32 * w0, u12 * v.m10 + u22 * v.m11 + u32 * w1, u12 * v.m20 + u22 * v.m21 + u32 * w2};
}

// the unit quaternion (w, x, y, z) of a proper rotation matrix, by the largest of the four pivots
__device__ __forceinline__ Quatd rotmat_to_quat(const Mat3d& r) {
  const double tr = r.m00 + r.m11 + r.m22;
  Quatd q;
  if (tr > 0.0) {
    const double s = 2.0 * sqrt(tr + 1.0);
    q.w = 0.25 * s; q.x = (r.m21 - r.m12) / s; q.y = (r.m02 - r.m20) / s; q.z = (r.m10 - r.m01) / s;
  } else if (r.m00 > r.m11 && r.m00 > r.m22) {
    const double s = 2.0 * sqrt(1.0 + r.m00 - r.m11 - r.m22);
    q.w = (r.m21 - r.m12) / s; q.x = 0.25 * s; q.y = (r.m01 + r.m10) / s; q.z = (r.m02 + r.m20) / s;
  } else if (r.m11 > r.m22) {
    const double s = 2.0 * sqrt(1.0 + r.m11 - r.m00 - r.m22);
    q.w = (r.m02 - r.m20) / s; q.x = (r.m01 + r.m10) / s; q.y = 0.25 * s; q.z = (r.m12 + r.m21) / s;
  } else {
    const double s = 2.0 * sqrt(1.0 + r.m22 - r.m00 - r.m11);
    q.w = (r.m10 - r.m01) / s; q.x = (r.m02 + r.m20) / s; q.y = (r.m12 + r.m21) / s; q.z = 0.25 * s;
  }
  return q;
}

// a (x) b scaled to unit length; inv receives 1 / |a (x) b|
__device__ __forceinline__ Quatd quat_mul_normalised(const Quatd& a, const Quatd& b, double& inv) {
  const double ow = a.w * b.w - a.x * b.x - a.y * b.y - a.z * b.z, ox = a.w * b.x + a.x * b.w + a.y * b.z - a.z * b.y;
  const double oy = a.w * b.y - a.x * b.z + a.y * b.w + a.z * b.x, oz = a.w * b.z + a.x * b.y - a.y * b.x + a.z * b.w;
  inv = 1.0 / sqrt(ow * ow + ox * ox + oy * oy + oz * oz);
  return {ow * inv, ox * inv, oy * inv, oz * inv};
}

}  // namespace mgs
#endif
#endif  // MGS_DEFORM_SHAPE_H_
