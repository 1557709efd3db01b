// deform.hip -- Gaussians that follow simulated particles (include/mgs_deform.h), gfx950: bind once, move per frame.
//
// deform_knn_kernel (the hot path of the bind).  hinge_nn_kernel's structure: a workgroup of kDeformGroup threads keeps one
// Gaussian mean per thread in registers and streams the particle set through LDS in tiles of kDeformTile float4 entries;
// every lane of a wave reads the same entry, so the ds_read_b128 is a broadcast.  Each thread keeps its 8 best (d2, j)
// pairs sorted in two fully unrolled arrays (registers: every index is a compile-time constant).  The common case of a
// pair is the distance (3 subtractions, 1 multiply, 2 fma) and ONE compare against the current 8th; the insertion -- the
// new pair written over the 8th, then seven compare-and-exchange steps towards the front, each moving on a strict "less"
// only, so that a tie stays behind the lower index that came first -- runs under that branch, which a thread takes about
// 8 ln(m / 8) times in all.  A non-finite particle is staged as +inf and an ineligible Gaussian walks as NaN: neither is
// ever below the 8th.  The particle set is NOT split across workgroups: one workgroup walks all of it, so the lists need
// no merge pass (a scene of few Gaussians leaves compute units idle; the bind runs once per object).
//
// deform_bind_kernel.  One thread per Gaussian, fp64 on the fp32 inputs: weights, centroid, weighted offsets, the moment
// matrix Q, its eigenvalues (jacobi3.h) and its inverse by cofactors; every stored value is rounded to fp32 once.
//
// deform_apply_kernel (every frame).  One thread per Gaussian.  The neighbour-major binding arrays make every streamed
// load coalesced; the 8 gathers of current particle positions are the only random access.  c and P are fp32 fma chains
// of differences to the anchor x_0; the rotation and the deformed covariance are solved in fp64 with the same Jacobi.
// Its SH instantiation (include/mgs_deform_sh.h) then turns the lane's SH rows by the rotation it found, in fp32 registers
// (sh_rotate.h), rows of 16 coefficients staged through LDS (sh_staging.h); the instantiation without SH is untouched by it.
//
// deform_apply_bwd_kernel and deform_scatter_kernel (include/mgs_deform_bwd.h): the rigid mode's backward, one thread per
// Gaussian into a neighbour-major workspace, then one wave per particle that adds its referents' rows in a fixed order.
//
// The shape matching itself -- gather, P, the eigenpairs of P^T P, the rotation, the quaternion product -- is in
// deform_shape.h, once: the forward and the backward call the same functions, which is what makes the backward's R the
// forward's.  The kernels below hold what differs: the branches, the affine covariance, the SH phase, the gradient chain.
#include "mgs_common.h"
#include "jacobi3.h"
#include "deform_shape.h"
#include "sh_staging.h"
#include "sh_rotate.h"
#include "../../include/mgs_deform.h"
#include "../../include/mgs_deform_sh.h"
#include "../../include/mgs_deform_bwd.h"

#include <float.h>
#include <math.h>

namespace mgs {
namespace {

constexpr int kDeformGroup = 256;         // threads of a workgroup (all three kernels)
constexpr int kDeformTile = 1024;         // T: particles per LDS tile (16 KiB)
constexpr int kDeformShGroup = 64;        // threads of a workgroup of the apply's SH instantiation: one wave
constexpr int kRestRows = 12;             // (kK, the 8 neighbours, is deform_shape.h's)
constexpr double kDegenerate = 1e-3;      // the flat / thin threshold on eigenvalue (bind) and singular-value (apply) ratios

enum { kFlagUnbound = 1, kFlagFlat = 2, kFlagThin = 4 };
enum { kStatusUnbound = 1, kStatusFallback = 2, kStatusThin = 4, kStatusNonFinite = 8 };

__global__ __launch_bounds__(kDeformGroup) void deform_knn_kernel(int n, const float* __restrict__ means,
                                                                 const uint8_t* __restrict__ select, int m,
                                                                 const float* __restrict__ parts,
                                                                 int32_t* __restrict__ idx, float* __restrict__ d2) {
  __shared__ float4 tile[kDeformTile];
  const int t = (int)threadIdx.x;
  const long long i = (long long)blockIdx.x * kDeformGroup + t;
  const float inf = __builtin_inff(), nan = __builtin_nanf("");

  float qx = nan, qy = nan, qz = nan;               // ineligible: every distance is a NaN, which is below nothing
  if (i < n && (!select || select[i])) {
    qx = means[3 * i + 0];
    qy = means[3 * i + 1];
    qz = means[3 * i + 2];
    if (!finite3(qx, qy, qz)) qx = nan;
  }
  float bd[kK];
  int bi[kK];
#pragma unroll
  for (int k = 0; k < kK; ++k) { bd[k] = inf; bi[k] = -1; }
  // a workgroup without one eligible Gaussian (the unselected part of a spatially ordered scene) walks nothing
  const int n_walk = __syncthreads_or(qx == qx) ? m : 0;

  const int n_tiles = (int)(((long long)n_walk + kDeformTile - 1) / kDeformTile);
  for (int tl = 0; tl < n_tiles; ++tl) {
    const long long obase = (long long)tl * kDeformTile;
    const int count = m - obase < kDeformTile ? (int)(m - obase) : kDeformTile;
    __syncthreads();                                // the walk of the previous tile is over
    for (int e = t; e < count; e += kDeformGroup) {
      const long long j = obase + e;
      float4 p = make_float4(parts[3 * j + 0], parts[3 * j + 1], parts[3 * j + 2], 0.f);
      if (!finite3(p.x, p.y, p.z)) p = make_float4(inf, inf, inf, 0.f);      // nobody's neighbour
      tile[e] = p;
    }
    __syncthreads();
#pragma unroll 4
    for (int j = 0; j < count; ++j) {
      const float4 p = tile[j];                     // the same address in every lane: a broadcast
      const float dx = qx - p.x, dy = qy - p.y, dz = qz - p.z;
      const float d = __builtin_fmaf(dz, dz, __builtin_fmaf(dy, dy, dx * dx));
      if (d < bd[kK - 1]) {                         // rare: j ascends, so an equal d2 (a higher index) stays out
        bd[kK - 1] = d;
        bi[kK - 1] = (int)obase + j;
#pragma unroll
        for (int k = kK - 1; k >= 1; --k) {
          const bool up = bd[k] < bd[k - 1];        // strict: behind every equal d2 of a lower index
          const float dl = up ? bd[k] : bd[k - 1], dh = up ? bd[k - 1] : bd[k];
          const int il = up ? bi[k] : bi[k - 1], ih = up ? bi[k - 1] : bi[k];
          bd[k - 1] = dl; bd[k] = dh;
          bi[k - 1] = il; bi[k] = ih;
        }
      }
    }
  }
  if (i < n) {
#pragma unroll
    for (int k = 0; k < kK; ++k) {
      idx[(size_t)k * n + i] = bi[k];
      d2[(size_t)k * n + i] = bd[k];
    }
  }
}

__global__ __launch_bounds__(kDeformGroup) void deform_bind_kernel(int n, const float* __restrict__ means,
                                                                  const uint8_t* __restrict__ select,
                                                                  const float* __restrict__ parts, float max_distance,
                                                                  const float* __restrict__ d2, int32_t* __restrict__ idx,
                                                                  float* __restrict__ w, float* __restrict__ p,
                                                                  float* __restrict__ rest, uint8_t* __restrict__ flags) {
  const long long i = (long long)blockIdx.x * kDeformGroup + threadIdx.x;
  if (i >= n) return;
  const size_t N = (size_t)n;
  int id[kK];
  float dd[kK];
#pragma unroll
  for (int k = 0; k < kK; ++k) { id[k] = idx[k * N + i]; dd[k] = d2[k * N + i]; }
  const float mx = means[3 * i + 0], my = means[3 * i + 1], mz = means[3 * i + 2];
  const bool bound = (!select || select[i]) && finite3(mx, my, mz) && id[kK - 1] >= 0 && !(sqrtf(dd[0]) > max_distance);
  if (!bound) {
#pragma unroll
    for (int k = 0; k < kK; ++k) {
      idx[k * N + i] = -1;
      w[k * N + i] = 0.f;
      p[(3 * k + 0) * N + i] = 0.f; p[(3 * k + 1) * N + i] = 0.f; p[(3 * k + 2) * N + i] = 0.f;
    }
#pragma unroll
    for (int r = 0; r < kRestRows; ++r) rest[r * N + i] = 0.f;
    flags[i] = kFlagUnbound;
    return;
  }

  const double h2 = (double)dd[kK - 1];
  double wt[kK], X[kK][3], sum = 0.0;
#pragma unroll
  for (int k = 0; k < kK; ++k) {
    wt[k] = h2 > 0.0 ? exp(-(double)dd[k] / h2) : 1.0;
    sum += wt[k];
    const size_t j = (size_t)id[k];
    X[k][0] = (double)parts[3 * j + 0]; X[k][1] = (double)parts[3 * j + 1]; X[k][2] = (double)parts[3 * j + 2];
  }
  double cx = 0.0, cy = 0.0, cz = 0.0;
#pragma unroll
  for (int k = 0; k < kK; ++k) {
    wt[k] /= sum;
    cx += wt[k] * X[k][0]; cy += wt[k] * X[k][1]; cz += wt[k] * X[k][2];
  }
  double q00 = 0.0, q01 = 0.0, q02 = 0.0, q11 = 0.0, q12 = 0.0, q22 = 0.0;
#pragma unroll
  for (int k = 0; k < kK; ++k) {
    const double rx = X[k][0] - cx, ry = X[k][1] - cy, rz = X[k][2] - cz, wk = wt[k];
    w[k * N + i] = (float)wk;
    p[(3 * k + 0) * N + i] = (float)(wk * rx);
    p[(3 * k + 1) * N + i] = (float)(wk * ry);
    p[(3 * k + 2) * N + i] = (float)(wk * rz);
    q00 += wk * rx * rx; q01 += wk * rx * ry; q02 += wk * rx * rz;
    q11 += wk * ry * ry; q12 += wk * ry * rz; q22 += wk * rz * rz;
  }

  double a00 = q00, a01 = q01, a02 = q02, a11 = q11, a12 = q12, a22 = q22;
  double v00, v01, v02, v10, v11, v12, v20, v21, v22;
  jacobi_solve3(a00, a01, a02, a11, a12, a22, v00, v01, v02, v10, v11, v12, v20, v21, v22);
  double l0 = a00, l1 = a11, l2 = a22, tmp;          // ascending
  if (l0 > l1) { tmp = l0; l0 = l1; l1 = tmp; }
  if (l1 > l2) { tmp = l1; l1 = l2; l2 = tmp; }
  if (l0 > l1) { tmp = l0; l0 = l1; l1 = tmp; }
  const bool flat = l0 < kDegenerate * l2;
  const bool thin = l1 < kDegenerate * l2 || !(l2 > 0.0);

  double i00 = 0.0, i01 = 0.0, i02 = 0.0, i11 = 0.0, i12 = 0.0, i22 = 0.0;
  if (!flat && l2 > 0.0) {                           // the inverse by cofactors (Q is symmetric, so is its inverse)
    const double c00 = q11 * q22 - q12 * q12, c01 = q02 * q12 - q01 * q22, c02 = q01 * q12 - q02 * q11;
    const double inv = 1.0 / (q00 * c00 + q01 * c01 + q02 * c02);
    i00 = c00 * inv; i01 = c01 * inv; i02 = c02 * inv;
    i11 = (q00 * q22 - q02 * q02) * inv;
    i12 = (q01 * q02 - q00 * q12) * inv;
    i22 = (q00 * q11 - q01 * q01) * inv;
  }
  rest[0 * N + i] = (float)((double)mx - cx);
  rest[1 * N + i] = (float)((double)my - cy);
  rest[2 * N + i] = (float)((double)mz - cz);
  rest[3 * N + i] = (float)i00; rest[4 * N + i] = (float)i01; rest[5 * N + i] = (float)i02;
  rest[6 * N + i] = (float)i11; rest[7 * N + i] = (float)i12; rest[8 * N + i] = (float)i22;
  rest[9 * N + i] = dd[kK - 1];
  rest[10 * N + i] = l2 > 0.0 ? (float)(l1 / l2) : 0.f;
  rest[11 * N + i] = l2 > 0.0 ? (float)(l0 / l2) : 0.f;
  flags[i] = (uint8_t)((flat ? kFlagFlat : 0) | (thin ? kFlagThin : 0));
}

// What the SH phase does with a lane's row: nothing (an unbound Gaussian, unless asked to copy), copy it through (bound
// but not turning: thin, a non-finite neighbour) or rotate it.
enum { kRowUnbound = 0, kRowCopy = 1, kRowRotate = 2 };

// the SH phase's copy of R, rounded to fp32 once (row-major, as sh_rotate.h takes it)
__device__ __forceinline__ void round_rotation(const Mat3d& r, float (&Rf)[9]) {
  Rf[0] = (float)r.m00; Rf[1] = (float)r.m01; Rf[2] = (float)r.m02; Rf[3] = (float)r.m10; Rf[4] = (float)r.m11;
  Rf[5] = (float)r.m12; Rf[6] = (float)r.m20; Rf[7] = (float)r.m21; Rf[8] = (float)r.m22;
}

// SH = false: the geometry alone, kDeformGroup threads, no LDS -- what mgs_deform_apply launches.
// SH = true: one wave per workgroup (kDeformShGroup; the staging area of a wave is 13,312 B of LDS, so twelve resident
// waves of a CU hold 159,744 of its 163,840 B however they are grouped, and a workgroup of one wave makes the two
// barriers free).  After the geometry is written the wave turns the SH rows of its rotating lanes (sh_rotate.h).  Rows of
// 16 coefficients go through LDS (sh_staging.h: the HBM side is lane-linear) and only rows some lane has to write are
// fetched; shorter rows are read per lane.  Nobody leaves before the last barrier: a lane past n has nothing to write.
template <bool SH, bool STAGED>
__global__ __launch_bounds__(SH ? kDeformShGroup : kDeformGroup) void deform_apply_kernel(
    int n, const float* __restrict__ means, const float* __restrict__ quats, const float* __restrict__ scales,
    const int32_t* __restrict__ idx, const float* __restrict__ w, const float* __restrict__ p,
    const float* __restrict__ rest, const uint8_t* __restrict__ flags, int mode, int m, const float* __restrict__ now,
    float* __restrict__ out_means, float* __restrict__ out_quats, float* __restrict__ out_scales,
    uint8_t* __restrict__ status, int sh_degree, int stride_f, const float* __restrict__ sh_in,
    float* __restrict__ sh_out, int copy_unbound) {
  constexpr int kGroup = SH ? kDeformShGroup : kDeformGroup;
  const long long i = (long long)blockIdx.x * kGroup + threadIdx.x;
  const bool live = i < n;
  if constexpr (!SH) {
    if (!live) return;
  }
  int row = kRowUnbound;                  // what the SH phase does with this lane's row
  float Rf[9];                            // R rounded to fp32, row-major, where row == kRowRotate
  if (SH ? live : true) {
    row = kRowCopy;
    const size_t N = (size_t)n;
    float mu0 = means[3 * i + 0], mu1 = means[3 * i + 1], mu2 = means[3 * i + 2];
    float4 q = reinterpret_cast<const float4*>(quats)[i];           // (w, x, y, z)
    float s0 = scales[3 * i + 0], s1 = scales[3 * i + 1], s2 = scales[3 * i + 2];
    const unsigned fl = flags[i];
    unsigned st = 0u;

    if (fl & kFlagUnbound) {
      st = kStatusUnbound;
      row = kRowUnbound;
    } else {
      float x[kK][3], wk[kK], pk[kK][3];            // (wk and pk are the backward's: not touched here)
      if (!gather_neighbours<true>(idx, N, i, m, now, x)) {
        st = kStatusNonFinite;
      } else {
        const Moment mo = moment_P<true>(x, w, p, N, i, wk, pk);
        const Mat3f& P = mo.P;
        const float xb0 = x[0][0] + mo.c0, xb1 = x[0][1] + mo.c1, xb2 = x[0][2] + mo.c2;
        const float d00 = rest[0 * N + i], d01 = rest[1 * N + i], d02 = rest[2 * N + i];
        const Mat3d Pd = widen(P);
        const Eig3 eg = gram_eigen_desc(Pd);
        // sigma_mid < 1e-3 sigma_max  <=>  lambda_mid < 1e-6 lambda_max
        const bool thin = (fl & kFlagThin) || !(eg.l0 > 0.0) || eg.l1 < kDegenerate * kDegenerate * eg.l0;

        bool rigid = mode == 0;
        Mat3f A = {};
        if (thin) {
          st = kStatusThin;
          mu0 = xb0 + d00; mu1 = xb1 + d01; mu2 = xb2 + d02;
        } else if (!rigid) {
          if (fl & kFlagFlat) {
            rigid = true;
          } else {                                    // A = P Q^-1 in fp32
            const float ixx = rest[3 * N + i], ixy = rest[4 * N + i], ixz = rest[5 * N + i];
            const float iyy = rest[6 * N + i], iyz = rest[7 * N + i], izz = rest[8 * N + i];
            A.m00 = __builtin_fmaf(P.m02, ixz, __builtin_fmaf(P.m01, ixy, P.m00 * ixx));
            A.m01 = __builtin_fmaf(P.m02, iyz, __builtin_fmaf(P.m01, iyy, P.m00 * ixy));
            A.m02 = __builtin_fmaf(P.m02, izz, __builtin_fmaf(P.m01, iyz, P.m00 * ixz));
            A.m10 = __builtin_fmaf(P.m12, ixz, __builtin_fmaf(P.m11, ixy, P.m10 * ixx));
            A.m11 = __builtin_fmaf(P.m12, iyz, __builtin_fmaf(P.m11, iyy, P.m10 * ixy));
            A.m12 = __builtin_fmaf(P.m12, izz, __builtin_fmaf(P.m11, iyz, P.m10 * ixz));
            A.m20 = __builtin_fmaf(P.m22, ixz, __builtin_fmaf(P.m21, ixy, P.m20 * ixx));
            A.m21 = __builtin_fmaf(P.m22, iyz, __builtin_fmaf(P.m21, iyy, P.m20 * ixy));
            A.m22 = __builtin_fmaf(P.m22, izz, __builtin_fmaf(P.m21, iyz, P.m20 * ixz));
            const double det = (double)A.m00 * ((double)A.m11 * A.m22 - (double)A.m12 * A.m21)
                               - (double)A.m01 * ((double)A.m10 * A.m22 - (double)A.m12 * A.m20)
                               + (double)A.m02 * ((double)A.m10 * A.m21 - (double)A.m11 * A.m20);
            if (!(det > 0.0)) rigid = true;
          }
          if (rigid) st = kStatusFallback;
        }

        if (!thin && rigid) {
          const Mat3d R = shape_rotation(Pd, eg);
          if constexpr (SH) { round_rotation(R, Rf); row = kRowRotate; }
          mu0 = (float)((double)xb0 + (R.m00 * d00 + R.m01 * d01 + R.m02 * d02));
          mu1 = (float)((double)xb1 + (R.m10 * d00 + R.m11 * d01 + R.m12 * d02));
          mu2 = (float)((double)xb2 + (R.m20 * d00 + R.m21 * d01 + R.m22 * d02));
          double inv;
          const Quatd o = quat_mul_normalised(rotmat_to_quat(R), Quatd{q.x, q.y, q.z, q.w}, inv);
          q = make_float4((float)o.w, (float)o.x, (float)o.y, (float)o.z);
        } else if (!thin) {
          if constexpr (SH) {                         // the colour field turns with the neighbourhood's rotation, it does not shear
            round_rotation(shape_rotation(Pd, eg), Rf);
            row = kRowRotate;
          }
          mu0 = xb0 + __builtin_fmaf(A.m02, d02, __builtin_fmaf(A.m01, d01, A.m00 * d00));
          mu1 = xb1 + __builtin_fmaf(A.m12, d02, __builtin_fmaf(A.m11, d01, A.m10 * d00));
          mu2 = xb2 + __builtin_fmaf(A.m22, d02, __builtin_fmaf(A.m21, d01, A.m20 * d00));
          // M = A R(q) diag(s), Sigma' = M M^T
          double bw = q.x, bx = q.y, by = q.z, bz = q.w;
          const double inv = 1.0 / sqrt(bw * bw + bx * bx + by * by + bz * bz);
          bw *= inv; bx *= inv; by *= inv; bz *= inv;
          const double g00 = 1.0 - 2.0 * (by * by + bz * bz), g01 = 2.0 * (bx * by - bw * bz), g02 = 2.0 * (bx * bz + bw * by);
          const double g10 = 2.0 * (bx * by + bw * bz), g11 = 1.0 - 2.0 * (bx * bx + bz * bz), g12 = 2.0 * (by * bz - bw * bx);
          const double g20 = 2.0 * (bx * bz - bw * by), g21 = 2.0 * (by * bz + bw * bx), g22 = 1.0 - 2.0 * (bx * bx + by * by);
          const double t0 = s0, t1 = s1, t2 = s2;
          const Mat3d M = {((double)A.m00 * g00 + (double)A.m01 * g10 + (double)A.m02 * g20) * t0,
                           ((double)A.m00 * g01 + (double)A.m01 * g11 + (double)A.m02 * g21) * t1,
                           ((double)A.m00 * g02 + (double)A.m01 * g12 + (double)A.m02 * g22) * t2,
                           ((double)A.m10 * g00 + (double)A.m11 * g10 + (double)A.m12 * g20) * t0,
                           ((double)A.m10 * g01 + (double)A.m11 * g11 + (double)A.m12 * g21) * t1,
                           ((double)A.m10 * g02 + (double)A.m11 * g12 + (double)A.m12 * g22) * t2,
                           ((double)A.m20 * g00 + (double)A.m21 * g10 + (double)A.m22 * g20) * t0,
                           ((double)A.m20 * g01 + (double)A.m21 * g11 + (double)A.m22 * g21) * t1,
                           ((double)A.m20 * g02 + (double)A.m21 * g12 + (double)A.m22 * g22) * t2};
          Eig3 es = eigen_sorted<false>(gram(transposed(M)));       // ascending; its columns are the new axes
          Mat3d& z = es.v;
          const double detz = z.m00 * (z.m11 * z.m22 - z.m12 * z.m21) - z.m01 * (z.m10 * z.m22 - z.m12 * z.m20)
                              + z.m02 * (z.m10 * z.m21 - z.m11 * z.m20);
          if (detz < 0.0) { z.m02 = -z.m02; z.m12 = -z.m12; z.m22 = -z.m22; }
          const Quatd a = rotmat_to_quat(z);
          const double qn = 1.0 / sqrt(a.w * a.w + a.x * a.x + a.y * a.y + a.z * a.z);
          q = make_float4((float)(a.w * qn), (float)(a.x * qn), (float)(a.y * qn), (float)(a.z * qn));
          s0 = fmaxf((float)sqrt(fmax(es.l0, 0.0)), FLT_MIN);
          s1 = fmaxf((float)sqrt(fmax(es.l1, 0.0)), FLT_MIN);
          s2 = fmaxf((float)sqrt(fmax(es.l2, 0.0)), FLT_MIN);
        }
      }
    }
    out_means[3 * i + 0] = mu0; out_means[3 * i + 1] = mu1; out_means[3 * i + 2] = mu2;
    reinterpret_cast<float4*>(out_quats)[i] = q;
    out_scales[3 * i + 0] = s0; out_scales[3 * i + 1] = s1; out_scales[3 * i + 2] = s2;
    if (status) status[i] = (uint8_t)st;
  }
  if constexpr (SH) {
    __shared__ float4 lds[STAGED ? kShWaveSlots : 1];
    const bool turn = row == kRowRotate && sh_degree >= 1;
    // rows of bound Gaussians are always written, rotated or copied; rows of unbound ones only on request
    const bool wr = live && (row != kRowUnbound || copy_unbound);
    const unsigned long long need = ballot(wr);
    if (need == 0ull) return;                                    // the whole workgroup: it is one wave
    const int g0 = (int)((long long)blockIdx.x * kGroup);
    const int kc = (sh_degree + 1) * (sh_degree + 1) - 1;        // coefficients above the DC term
    float* rowp;                                                 // this lane's 16 x rgb (or shorter) row
    if constexpr (STAGED) {
      sh_rows_to_lds(sh_in, g0, n, need, lds);
      __syncthreads();
      rowp = reinterpret_cast<float*>(lds + threadIdx.x * kShPitchF4);
    } else {
      rowp = const_cast<float*>(sh_in) + (size_t)(live ? i : 0) * stride_f;
    }
    float c[15 * 3], o[15 * 3];
#pragma unroll
    for (int k = 0; k < 45; ++k) c[k] = (wr && k < kc * 3) ? rowp[3 + k] : 0.f;
#pragma unroll
    for (int k = 0; k < 45; ++k) o[k] = c[k];
    if (turn) {
      // degree 1: coefficients 1..3 (c[0..8]), degree 2: 4..8 (c[9..23]), degree 3: 9..15 (c[24..44])
      sh_rotate_band1(Rf, c, o);
      if (sh_degree >= 2) sh_rotate_band<2>(Rf, c + 9, o + 9);
      if (sh_degree >= 3) sh_rotate_band<3>(Rf, c + 24, o + 24);
    }
    if constexpr (STAGED) {
      if (turn) {
#pragma unroll
        for (int k = 0; k < 45; ++k)
          if (k < kc * 3) rowp[3 + k] = o[k];
      }
      __syncthreads();
      // lane-linear write-back of the rows that were fetched
      float4* dst = reinterpret_cast<float4*>(sh_out + (size_t)g0 * 48);
#pragma unroll
      for (int r = 0; r < kShRowF4; ++r) {
        const unsigned f = r * kShWave + threadIdx.x, owner = f / kShRowF4;
        if (((need >> owner) & 1ull) && g0 + (int)owner < n) dst[f] = lds[owner * kShPitchF4 + (f - owner * kShRowF4)];
      }
    } else if (wr) {
      float* dst = sh_out + (size_t)i * stride_f;
#pragma unroll
      for (int ch = 0; ch < 3; ++ch) dst[ch] = rowp[ch];         // the DC term
#pragma unroll
      for (int k = 0; k < 45; ++k)
        if (k < kc * 3) dst[3 + k] = o[k];
      for (int k = 3 + kc * 3; k < stride_f; ++k) dst[k] = rowp[k];   // coefficients above the active degree
    }
  }
}

// deform_apply_bwd_kernel (include/mgs_deform_bwd.h, launch 1).  One thread per Gaussian.  P, the eigenpairs of P^T P,
// R and q' come from the same functions deform_apply_kernel calls (deform_shape.h; c has no part in the gradient, only
// its weights, so moment_P leaves it out), on the same inputs: the forward's R and q' bit for bit.  The branch is the
// forward's status, not a second decision.  The chain v_omega -> y = G^-1 R^T v_omega -> v_P = R [y]x runs in
// fp64 on named scalars; w and p stay in registers from the forward part to the 24 contributions at the end.  The
// contributions go to the neighbour-major workspace ws [8][3][N] (coalesced), a pass-through row's as zeros.
__global__ __launch_bounds__(kDeformGroup) void deform_apply_bwd_kernel(
    int n, const float* __restrict__ quats, const int32_t* __restrict__ idx, const float* __restrict__ w,
    const float* __restrict__ p, const float* __restrict__ rest, const uint8_t* __restrict__ flags, int m,
    const float* __restrict__ now, const uint8_t* __restrict__ status, const float* __restrict__ ct_means,
    const float* __restrict__ ct_quats, const float* __restrict__ ct_scales, float* __restrict__ v_means,
    float* __restrict__ v_quats, float* __restrict__ v_scales, uint8_t* __restrict__ bwd_status, float* __restrict__ ws) {
  const long long i = (long long)blockIdx.x * kDeformGroup + threadIdx.x;
  if (i >= n) return;
  const size_t N = (size_t)n;
  float cm0 = 0.f, cm1 = 0.f, cm2 = 0.f, cs0 = 0.f, cs1 = 0.f, cs2 = 0.f;
  float4 cq = make_float4(0.f, 0.f, 0.f, 0.f);
  if (ct_means) { cm0 = ct_means[3 * i + 0]; cm1 = ct_means[3 * i + 1]; cm2 = ct_means[3 * i + 2]; }
  if (ct_quats) cq = reinterpret_cast<const float4*>(ct_quats)[i];
  if (ct_scales) { cs0 = ct_scales[3 * i + 0]; cs1 = ct_scales[3 * i + 1]; cs2 = ct_scales[3 * i + 2]; }
  float vm0 = cm0, vm1 = cm1, vm2 = cm2;             // v_means = v_d0: the cotangent itself unless the row turned
  float4 vq = cq;
  float vx[kK][3];                                   // the 24 contributions (constant indices only: registers)
#pragma unroll
  for (int k = 0; k < kK; ++k) { vx[k][0] = 0.f; vx[k][1] = 0.f; vx[k][2] = 0.f; }
  unsigned bst = 0u;

  const unsigned st = status[i];
  if (!((flags[i] & kFlagUnbound) || (st & (kStatusUnbound | kStatusNonFinite)))) {
    float x[kK][3];
    const bool in_range = gather_neighbours<false>(idx, N, i, m, now, x);
    if (in_range) {                                  // (a status that is not this frame's: nothing is followed out of range)
      float wk[kK], pk[kK][3];
      const Mat3d P = widen(moment_P<false>(x, w, p, N, i, wk, pk).P);
      // v_P, zero unless the row turned and the guard let the rotation's gradient through
      double g00 = 0., g01 = 0., g02 = 0., g10 = 0., g11 = 0., g12 = 0., g20 = 0., g21 = 0., g22 = 0.;
      if (!(st & kStatusThin)) {
        const Eig3 eg = gram_eigen_desc(P);
        const Mat3d R = shape_rotation(P, eg);
        const double r00 = R.m00, r01 = R.m01, r02 = R.m02, r10 = R.m10, r11 = R.m11, r12 = R.m12, r20 = R.m20, r21 = R.m21,
                     r22 = R.m22;
        const double p00 = P.m00, p01 = P.m01, p02 = P.m02, p10 = P.m10, p11 = P.m11, p12 = P.m12, p20 = P.m20, p21 = P.m21,
                     p22 = P.m22;
        const double d0 = rest[0 * N + i], d1 = rest[1 * N + i], d2 = rest[2 * N + i];
        const double m0 = cm0, m1 = cm1, m2 = cm2;
        vm0 = (float)(r00 * m0 + r10 * m1 + r20 * m2);                      // v_d0 = R^T ct_mu
        vm1 = (float)(r01 * m0 + r11 * m1 + r21 * m2);
        vm2 = (float)(r02 * m0 + r12 * m1 + r22 * m2);
        // S = R^T P (symmetric; the two triangles are averaged) and the guard on G's smallest eigenvalue, tr(S) - sigma_1
        const double s00 = r00 * p00 + r10 * p10 + r20 * p20, s11 = r01 * p01 + r11 * p11 + r21 * p21;
        const double s22 = r02 * p02 + r12 * p12 + r22 * p22;
        const double s01 = 0.5 * ((r00 * p01 + r10 * p11 + r20 * p21) + (r01 * p00 + r11 * p10 + r21 * p20));
        const double s02 = 0.5 * ((r00 * p02 + r10 * p12 + r20 * p22) + (r02 * p00 + r12 * p10 + r22 * p20));
        const double s12 = 0.5 * ((r01 * p02 + r11 * p12 + r21 * p22) + (r02 * p01 + r12 * p11 + r22 * p21));
        const double tr = s00 + s11 + s22, sig1 = sqrt(eg.l0);
        if (tr - sig1 < kDegenerate * sig1) {
          bst = 1u;                                  // guarded: v_P = 0, v_q = ct_q
        } else {
          const Quatd a = rotmat_to_quat(R);
          const float4 q = reinterpret_cast<const float4*>(quats)[i];
          double inv;
          const Quatd o = quat_mul_normalised(a, Quatd{q.x, q.y, q.z, q.w}, inv);   // q'
          const double aw = a.w, ax = a.x, ay = a.y, az = a.z, ow = o.w, ox = o.x, oy = o.y, oz = o.z;
          const double tw = cq.x, tx = cq.y, ty = cq.z, tz = cq.w;
          // v_q = conj(q_R) (x) (ct_q - <ct_q, q'> q') / |q_R (x) q|
          const double dq = tw * ow + tx * ox + ty * oy + tz * oz;
          const double uw = (tw - dq * ow) * inv, ux = (tx - dq * ox) * inv, uy = (ty - dq * oy) * inv, uz = (tz - dq * oz) * inv;
          vq = make_float4((float)(aw * uw + ax * ux + ay * uy + az * uz), (float)(aw * ux - ax * uw - ay * uz + az * uy),
                           (float)(aw * uy + ax * uz - ay * uw - az * ux), (float)(aw * uz - ax * uy + ay * ux - az * uw));
          // v_omega = (R d0) x ct_mu + 1/2 sum_k e_k <ct_q, (0, e_k) (x) q'>
          const double h0 = r00 * d0 + r01 * d1 + r02 * d2, h1 = r10 * d0 + r11 * d1 + r12 * d2;
          const double h2 = r20 * d0 + r21 * d1 + r22 * d2;
          const double o0 = (h1 * m2 - h2 * m1) + 0.5 * (tx * ow - tw * ox + tz * oy - ty * oz);
          const double o1 = (h2 * m0 - h0 * m2) + 0.5 * (ty * ow - tw * oy + tx * oz - tz * ox);
          const double o2 = (h0 * m1 - h1 * m0) + 0.5 * (tz * ow - tw * oz + ty * ox - tx * oy);
          // y = G^-1 R^T v_omega, G = tr(S) I - S, by cofactors
          const double z0 = r00 * o0 + r10 * o1 + r20 * o2, z1 = r01 * o0 + r11 * o1 + r21 * o2;
          const double z2 = r02 * o0 + r12 * o1 + r22 * o2;
          const double G00 = tr - s00, G11 = tr - s11, G22 = tr - s22, G01 = -s01, G02 = -s02, G12 = -s12;
          const double c00 = G11 * G22 - G12 * G12, c01 = G02 * G12 - G01 * G22, c02 = G01 * G12 - G02 * G11;
          const double c11 = G00 * G22 - G02 * G02, c12 = G01 * G02 - G00 * G12, c22 = G00 * G11 - G01 * G01;
          const double idet = 1.0 / (G00 * c00 + G01 * c01 + G02 * c02);
          const double y0 = (c00 * z0 + c01 * z1 + c02 * z2) * idet, y1 = (c01 * z0 + c11 * z1 + c12 * z2) * idet;
          const double y2 = (c02 * z0 + c12 * z1 + c22 * z2) * idet;
          // v_P = R [y]x,  [y]x = (0 -y2 y1 | y2 0 -y0 | -y1 y0 0)
          g00 = r01 * y2 - r02 * y1; g01 = r02 * y0 - r00 * y2; g02 = r00 * y1 - r01 * y0;
          g10 = r11 * y2 - r12 * y1; g11 = r12 * y0 - r10 * y2; g12 = r10 * y1 - r11 * y0;
          g20 = r21 * y2 - r22 * y1; g21 = r22 * y0 - r20 * y2; g22 = r20 * y1 - r21 * y0;
        }
      }
      // v_x_k = w_k ct_mu + v_P p_k (k = 1..7), v_x_0 = ct_mu - sum_k v_x_k: fp64, each rounded to fp32 once
      double a0 = cm0, a1 = cm1, a2 = cm2;
#pragma unroll
      for (int k = 1; k < kK; ++k) {
        const double wd = wk[k], q0 = pk[k][0], q1 = pk[k][1], q2 = pk[k][2];
        const double t0 = wd * (double)cm0 + (g00 * q0 + g01 * q1 + g02 * q2);
        const double t1 = wd * (double)cm1 + (g10 * q0 + g11 * q1 + g12 * q2);
        const double t2 = wd * (double)cm2 + (g20 * q0 + g21 * q1 + g22 * q2);
        a0 -= t0; a1 -= t1; a2 -= t2;
        vx[k][0] = (float)t0; vx[k][1] = (float)t1; vx[k][2] = (float)t2;
      }
      vx[0][0] = (float)a0; vx[0][1] = (float)a1; vx[0][2] = (float)a2;
    }
  }
#pragma unroll
  for (int k = 0; k < kK; ++k) {
    ws[(3 * k + 0) * N + i] = vx[k][0]; ws[(3 * k + 1) * N + i] = vx[k][1]; ws[(3 * k + 2) * N + i] = vx[k][2];
  }
  if (v_means) {
    v_means[3 * i + 0] = vm0; v_means[3 * i + 1] = vm1; v_means[3 * i + 2] = vm2;
    reinterpret_cast<float4*>(v_quats)[i] = vq;
    v_scales[3 * i + 0] = cs0; v_scales[3 * i + 1] = cs1; v_scales[3 * i + 2] = cs2;
  }
  if (bwd_status) bwd_status[i] = (uint8_t)bst;
}

// deform_scatter_kernel (launch 2).  One wave per particle: lane l adds the contributions of the entries t_start[j] + l,
// + 64, ... of its particle in ascending order, then a fixed xor tree.  An entry e = k N + i names ws[(3 k + c) N + i].
__global__ __launch_bounds__(kDeformGroup) void deform_scatter_kernel(int n, int m, const int32_t* __restrict__ t_start,
                                                                     const int32_t* __restrict__ t_entry,
                                                                     const float* __restrict__ ws,
                                                                     float* __restrict__ v_particles) {
  const int lane = (int)(threadIdx.x & 63u);
  const long long j = (long long)blockIdx.x * (kDeformGroup / 64) + (threadIdx.x >> 6);
  if (j >= m) return;                                // (the whole wave)
  const long long total = (long long)kK * n;
  float s0 = 0.f, s1 = 0.f, s2 = 0.f;
  if (n > 0) {
    long long lo = t_start[j], hi = t_start[j + 1];
    lo = lo < 0 ? 0 : lo;
    hi = hi > total ? total : hi;
    const size_t N = (size_t)n;
    for (long long t = lo + lane; t < hi; t += 64) {
      const long long e = t_entry[t];
      if (e >= 0 && e < total) {
        const size_t k = (size_t)(e / n), at = (size_t)e + 2 * k * N;       // (3 k) N + i
        s0 += ws[at]; s1 += ws[at + N]; s2 += ws[at + 2 * N];
      }
    }
  }
#pragma unroll
  for (int d = 32; d >= 1; d >>= 1) {
    s0 += __shfl_xor(s0, d); s1 += __shfl_xor(s1, d); s2 += __shfl_xor(s2, d);
  }
  if (lane == 0) { v_particles[3 * j + 0] = s0; v_particles[3 * j + 1] = s1; v_particles[3 * j + 2] = s2; }
}

size_t bind_workspace_bytes(int n) {
  Bump b(1);
  b.take(sizeof(float) * (size_t)kK * (size_t)n);      // d2 [8][n]: the sorted squared distances between the two launches
  return b.total;
}

constexpr int kBwdMaxN = (1 << 28) - 1;               // t_entry holds k n + i < 8 n in an int32

size_t apply_bwd_workspace_bytes(int n) {
  Bump b(1);
  b.take(sizeof(float) * 3 * (size_t)kK * (size_t)n);  // ws [8][3][n]: the contributions between the two launches
  return b.total;
}

// what mgs_deform_apply and mgs_deform_apply_sh hand to deform_apply_kernel, in its parameter order
struct ApplyArgs {
  int n; const float *means, *quats, *scales; const int32_t* idx; const float *w, *p, *rest; const uint8_t* flags;
  int mode, m; const float* now; float *out_means, *out_quats, *out_scales; uint8_t* status;
  int sh_degree, coeff_stride; const float* sh_in; float* sh_out; int copy_unbound;
};

// The argument checks of the two entry points in their one order (the first failing check decides the message); sh: the
// SH entry point, whose own checks stand where it makes them.  n == 0 ends the list early: nothing is dereferenced.
int check_apply(const char* name, const ApplyArgs& a, bool sh) {
  MGS_REQUIRE(a.n >= 0, "%s: n %d is negative", name, a.n);
  MGS_REQUIRE(a.m >= kK, "%s: m %d particles, at least %d needed", name, a.m, kK);
  MGS_REQUIRE(a.mode == 0 || a.mode == 1, "%s: mode %d is neither 0 (rigid) nor 1 (affine)", name, a.mode);
  if (sh) {
    MGS_REQUIRE(a.sh_degree >= 0 && a.sh_degree <= 3, "%s: sh_degree %d is outside 0..3", name, a.sh_degree);
    MGS_REQUIRE(a.coeff_stride >= (a.sh_degree + 1) * (a.sh_degree + 1),
                "%s: rows of %d coefficients cannot hold the %d of degree %d", name, a.coeff_stride,
                (a.sh_degree + 1) * (a.sh_degree + 1), a.sh_degree);
  }
  if (a.n == 0) return MGS_OK;
  MGS_REQUIRE(a.means && a.quats && a.scales, "%s: means, quats or scales is null", name);
  MGS_REQUIRE(a.idx && a.w && a.p && a.rest && a.flags, "%s: a binding array (idx, w, p, rest, flags) is null", name);
  MGS_REQUIRE(a.now, "%s: particles_now is null", name);
  MGS_REQUIRE(a.out_means && a.out_quats && a.out_scales, "%s: an output is null", name);
  if (sh) {
    MGS_REQUIRE(a.sh_in && a.sh_out, "%s: sh_coeffs or out_sh is null", name);
    MGS_REQUIRE(a.sh_out != a.sh_in, "%s: out_sh is sh_coeffs (the rest rows must survive: every frame turns them anew)", name);
  }
  return MGS_OK;
}

template <bool SH, bool STAGED>
int launch_apply(const char* name, const ApplyArgs& a, mgs_stream_t stream) {
  constexpr int kGroup = SH ? kDeformShGroup : kDeformGroup;
  hipLaunchKernelGGL((deform_apply_kernel<SH, STAGED>), dim3(div_up((unsigned)a.n, (unsigned)kGroup)), dim3(kGroup), 0,
                     (hipStream_t)stream, a.n, a.means, a.quats, a.scales, a.idx, a.w, a.p, a.rest, a.flags, a.mode, a.m, a.now,
                     a.out_means, a.out_quats, a.out_scales, a.status, a.sh_degree, a.coeff_stride * 3, a.sh_in, a.sh_out,
                     a.copy_unbound);
  return check_launch(name);
}

}  // namespace
}  // namespace mgs

using namespace mgs;

extern "C" size_t mgs_deform_bind_workspace_bytes(int n, int m) {
  if (n <= 0 || m < kK) return 0;
  return bind_workspace_bytes(n);
}

extern "C" int mgs_deform_bind(int n, const float* means, const uint8_t* select, int m, const float* particles_rest,
                               float max_distance, void* workspace, size_t workspace_bytes, int32_t* idx, float* w, float* p,
                               float* rest, uint8_t* flags, mgs_stream_t stream) {
  MGS_REQUIRE(n >= 0, "deform_bind: n %d is negative", n);
  MGS_REQUIRE(m >= kK, "deform_bind: m %d particles, at least %d needed", m, kK);
  MGS_REQUIRE(max_distance > 0.f, "deform_bind: max_distance %g is not a positive number", (double)max_distance);
  if (n == 0) return MGS_OK;
  MGS_REQUIRE(means && particles_rest, "deform_bind: means or particles_rest is null");
  MGS_REQUIRE(idx && w && p && rest && flags, "deform_bind: an output (idx, w, p, rest, flags) is null");
  MGS_REQUIRE(workspace, "deform_bind: workspace is null");
  const size_t need = bind_workspace_bytes(n);
  MGS_REQUIRE(workspace_bytes >= need, "deform_bind: workspace of %zu bytes, %zu needed", workspace_bytes, need);
  hipStream_t s = (hipStream_t)stream;
  float* d2 = static_cast<float*>(workspace);
  const dim3 grid(div_up((unsigned)n, (unsigned)kDeformGroup)), block(kDeformGroup);
  hipLaunchKernelGGL(deform_knn_kernel, grid, block, 0, s, n, means, select, m, particles_rest, idx, d2);
  int rc = check_launch("deform_bind");
  if (rc) return rc;
  hipLaunchKernelGGL(deform_bind_kernel, grid, block, 0, s, n, means, select, particles_rest, max_distance,
                     (const float*)d2, idx, w, p, rest, flags);
  return check_launch("deform_bind");
}

extern "C" int mgs_deform_apply(int n, const float* means, const float* quats, const float* scales, const int32_t* idx,
                                const float* w, const float* p, const float* rest, const uint8_t* flags, int mode, int m,
                                const float* particles_now, float* out_means, float* out_quats, float* out_scales,
                                uint8_t* status, mgs_stream_t stream) {
  const ApplyArgs a = {n, means, quats, scales, idx, w, p, rest, flags, mode, m, particles_now, out_means, out_quats,
                       out_scales, status, 0, 0, nullptr, nullptr, 0};
  const int rc = check_apply("deform_apply", a, false);
  if (rc || n == 0) return rc;
  return launch_apply<false, false>("deform_apply", a, stream);
}

extern "C" int mgs_deform_apply_sh(int n, const float* means, const float* quats, const float* scales, const int32_t* idx,
                                   const float* w, const float* p, const float* rest, const uint8_t* flags, int mode, int m,
                                   const float* particles_now, float* out_means, float* out_quats, float* out_scales,
                                   uint8_t* status, int sh_degree, int coeff_stride, const float* sh_coeffs, float* out_sh,
                                   int copy_unbound, mgs_stream_t stream) {
  const ApplyArgs a = {n, means, quats, scales, idx, w, p, rest, flags, mode, m, particles_now, out_means, out_quats,
                       out_scales, status, sh_degree, coeff_stride, sh_coeffs, out_sh, copy_unbound != 0};
  int rc = check_apply("deform_apply_sh", a, true);
  if (rc || n == 0) return rc;
  with_bool(coeff_stride == 16, [&](auto staged) {                // rows of 16 coefficients go through LDS
    rc = launch_apply<true, decltype(staged)::value>("deform_apply_sh", a, stream);
  });
  return rc;
}

extern "C" size_t mgs_deform_apply_bwd_workspace_bytes(int n) {
  if (n <= 0) return 0;
  return apply_bwd_workspace_bytes(n);
}

extern "C" int mgs_deform_apply_bwd(int n, const float* quats, const int32_t* idx, const float* w, const float* p,
                                    const float* rest, const uint8_t* flags, int m, const float* particles_now,
                                    const uint8_t* status, const float* ct_means, const float* ct_quats,
                                    const float* ct_scales, const int32_t* t_start, const int32_t* t_entry, float* v_means,
                                    float* v_quats, float* v_scales, float* v_particles, uint8_t* bwd_status,
                                    void* workspace, size_t workspace_bytes, mgs_stream_t stream) {
  MGS_REQUIRE(n >= 0, "deform_apply_bwd: n %d is negative", n);
  MGS_REQUIRE(n <= kBwdMaxN, "deform_apply_bwd: n %d, at most %d (t_entry is int32)", n, kBwdMaxN);
  MGS_REQUIRE(m >= kK, "deform_apply_bwd: m %d particles, at least %d needed", m, kK);
  MGS_REQUIRE(v_particles, "deform_apply_bwd: v_particles is null");
  const bool rest_grads = v_means || v_quats || v_scales;
  MGS_REQUIRE(!rest_grads || (v_means && v_quats && v_scales),
              "deform_apply_bwd: rest gradients given only in part (v_means, v_quats, v_scales)");
  hipStream_t s = (hipStream_t)stream;
  float* ws = static_cast<float*>(workspace);
  if (n > 0) {
    MGS_REQUIRE(quats, "deform_apply_bwd: quats is null");
    MGS_REQUIRE(idx && w && p && rest && flags, "deform_apply_bwd: a binding array (idx, w, p, rest, flags) is null");
    MGS_REQUIRE(particles_now, "deform_apply_bwd: particles_now is null");
    MGS_REQUIRE(status, "deform_apply_bwd: status is null (the forward's status is a required input)");
    MGS_REQUIRE(t_start && t_entry, "deform_apply_bwd: the transposed binding (t_start, t_entry) is null");
    MGS_REQUIRE(workspace, "deform_apply_bwd: workspace is null");
    const size_t need = apply_bwd_workspace_bytes(n);
    MGS_REQUIRE(workspace_bytes >= need, "deform_apply_bwd: workspace of %zu bytes, %zu needed", workspace_bytes, need);
    hipLaunchKernelGGL(deform_apply_bwd_kernel, dim3(div_up((unsigned)n, (unsigned)kDeformGroup)), dim3(kDeformGroup), 0, s,
                       n, quats, idx, w, p, rest, flags, m, particles_now, status, ct_means, ct_quats, ct_scales, v_means,
                       v_quats, v_scales, bwd_status, ws);
    int rc = check_launch("deform_apply_bwd");
    if (rc) return rc;
  }
  hipLaunchKernelGGL(deform_scatter_kernel, dim3(div_up((unsigned)m, (unsigned)(kDeformGroup / 64))), dim3(kDeformGroup), 0,
                     s, n, m, t_start, t_entry, (const float*)ws, v_particles);
  return check_launch("deform_apply_bwd");
}
