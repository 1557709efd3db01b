// sh_rotate.h -- rotating one Gaussian's SH rows by a 3x3 rotation R that exists only in this lane's registers
// (deform.hip: every Gaussian has its own R, new every frame, so there is no host-made matrix to read).
//
// The rule (include/mgs_deform_sh.h): band l becomes c'_l = M_l(R) c_l with sum_k Y_k(d) c'_k = sum_k Y_k(R^T d) c_k for
// every d, Y the renderer's real basis (gaussians._sh_basis_np).  M_l is never formed:
//   band 1  M_1 = Pi R Pi^T with Pi (x, y, z) -> (-y, z, -x):  v = (-c_3, -c_1, c_2),  u = R v as three fma chains
//           u_a = fma(R_a2, v_2, fma(R_a1, v_1, R_a0 v_0)),  c' = (-u_y, u_z, -u_x).
//   band l = 2, 3  the old colour field is evaluated at 2l+1 fixed directions d_k turned by R^T and multiplied by a
//           constant inverse.  Per direction: t = R^T d_k, t_a = fma(R_2a, d_z, fma(R_1a, d_y, R_0a d_x)); the band's
//           basis at t in its HOMOGENEOUS form (so that nothing assumes |t| = 1: the identity B c' = F below then holds for
//           the fp32 d_k as they are), sh_band_eval; F_k = sum_j Y_j(t) c_j as a product and 2l fma in order of j.  Then
//           c'_m = sum_k W_mk F_k, a product and 2l fma in order of k, with W = B^-1, B_kj = Y_j(d_k), inverted in fp64
//           and rounded to fp32 once (kInv).  The directions were chosen for cond(B) = 1.55 (band 2) and 1.74 (band 3).
// Everything is fp32 on the fp32-rounded R, every index a compile-time constant after unrolling.
// tests/deform_sh_ref.py counts the roundings of exactly this order and emulates it in NumPy.
#ifndef MGS_SH_ROTATE_H_
#define MGS_SH_ROTATE_H_

#include <hip/hip_runtime.h>

namespace mgs {

template <int L>
struct ShBandTables;

template <>
struct ShBandTables<2> {
  static constexpr float kDir[5][3] = {
      {-0.0929295272f, -0.633738637f, -0.767944932f},
      {-0.774724364f, -0.570928991f, -0.271739185f},
      {0.783877194f, -0.222405255f, 0.579717577f},
      {-0.245348543f, 0.967244864f, 0.0651267916f},
      {-0.87374717f, 0.416757822f, 0.250756472f},
  };
  static constexpr float kInv[5][5] = {
      {-0.311748266f, 0.999968708f, -0.754944861f, -0.486155838f, -0.67107451f},
      {-1.50644398f, -0.52165401f, 0.0544496477f, -0.042092558f, -0.875915647f},
      {0.708834708f, -1.23159504f, 0.085220404f, -1.11682403f, -0.694307685f},
      {-0.359342128f, -0.337558359f, -1.52822745f, -0.523446441f, 0.604655564f},
      {-0.0888386071f, 0.322537482f, 0.290210783f, -1.11344433f, 0.964102924f},
  };
};

template <>
struct ShBandTables<3> {
  static constexpr float kDir[7][3] = {
      {-0.417904168f, 0.844621181f, 0.334620893f},
      {0.318835586f, 0.669778705f, -0.670626879f},
      {-0.879883766f, 0.450533539f, 0.151076302f},
      {0.718422353f, -0.162688896f, -0.676314771f},
      {-0.839191675f, -0.421071529f, 0.344174534f},
      {0.218622223f, 0.964782119f, -0.146286547f},
      {-0.391046286f, 0.853818178f, -0.343623877f},
  };
  static constexpr float kInv[7][7] = {
      {0.470981687f, 0.363199443f, -0.719052494f, 0.282423735f, 0.527682543f, 0.537814975f, -0.0464269146f},
      {-0.912837505f, -0.809263647f, -0.0020709422f, 0.199792415f, 0.542839706f, -0.427095413f, 0.236389518f},
      {0.275092542f, -0.787595212f, 0.723100424f, -0.033327885f, -0.26558277f, 1.15743411f, 0.293308556f},
      {-0.589331508f, 0.514258206f, -0.3652291f, 0.539360762f, -1.02323461f, 0.325800836f, 0.645242631f},
      {-0.105386272f, -0.693895161f, -0.902415693f, -1.05752885f, -0.579934835f, -0.0244206898f, -0.108907416f},
      {-0.0497046635f, 0.391980469f, 0.492073178f, -0.858498812f, 0.442980111f, 0.125597f, 0.850681245f},
      {-0.816556513f, -0.048958499f, 0.236496404f, 0.208457962f, 0.133054197f, 0.543285906f, -0.916839898f},
  };
};

// the band's 2l+1 basis functions at t = (x, y, z), homogeneous of degree l; one rounding per operation, fma where written
template <int L>
__device__ __forceinline__ void sh_band_eval(float x, float y, float z, float (&Y)[2 * L + 1]) {
  const float yy = y * y, zz = z * z;
  const float s = __builtin_fmaf(x, x, yy);          // (written as an fma: the compiler would contract xx + yy anyway)
  if constexpr (L == 2) {
    constexpr float K1 = 1.092548430592079f, K2 = 0.31539156525252f, K3 = 0.5462742152960395f;
    Y[0] = K1 * (x * y);
    Y[1] = -K1 * (y * z);
    Y[2] = K2 * __builtin_fmaf(2.f, zz, -s);
    Y[3] = -K1 * (x * z);
    Y[4] = K3 * __builtin_fmaf(x, x, -yy);
  } else {
    constexpr float K4 = 0.5900435899266435f, K5 = 2.890611442640554f, K6 = 0.4570457994644658f;
    constexpr float K7 = 0.3731763325901154f, K8 = 1.445305721320277f;
    const float xx = x * x, q = __builtin_fmaf(4.f, zz, -s);
    Y[0] = K4 * (y * __builtin_fmaf(-3.f, xx, yy));
    Y[1] = K5 * ((x * y) * z);
    Y[2] = -K6 * (y * q);
    Y[3] = K7 * (z * __builtin_fmaf(2.f, zz, -(3.f * s)));
    Y[4] = -K6 * (x * q);
    Y[5] = K8 * (z * __builtin_fmaf(x, x, -yy));
    Y[6] = -K4 * (x * __builtin_fmaf(-3.f, yy, xx));
  }
}

// band 1: c and o hold 3 coefficients x rgb, coefficient-major (c[3 k + channel]); R row-major
__device__ __forceinline__ void sh_rotate_band1(const float (&R)[9], const float* c, float* o) {
#pragma unroll
  for (int ch = 0; ch < 3; ++ch) {
    const float v0 = -c[6 + ch], v1 = -c[ch], v2 = c[3 + ch];
    const float ux = __builtin_fmaf(R[2], v2, __builtin_fmaf(R[1], v1, R[0] * v0));
    const float uy = __builtin_fmaf(R[5], v2, __builtin_fmaf(R[4], v1, R[3] * v0));
    const float uz = __builtin_fmaf(R[8], v2, __builtin_fmaf(R[7], v1, R[6] * v0));
    o[ch] = -uy;
    o[3 + ch] = uz;
    o[6 + ch] = -ux;
  }
}

// band L = 2, 3: c and o hold 2L+1 coefficients x rgb, coefficient-major
template <int L>
__device__ __forceinline__ void sh_rotate_band(const float (&R)[9], const float* c, float* o) {
  constexpr int M = 2 * L + 1;
  float F[M][3];
#pragma unroll
  for (int k = 0; k < M; ++k) {
    const float dx = ShBandTables<L>::kDir[k][0], dy = ShBandTables<L>::kDir[k][1], dz = ShBandTables<L>::kDir[k][2];
    const float x = __builtin_fmaf(R[6], dz, __builtin_fmaf(R[3], dy, R[0] * dx));
    const float y = __builtin_fmaf(R[7], dz, __builtin_fmaf(R[4], dy, R[1] * dx));
    const float z = __builtin_fmaf(R[8], dz, __builtin_fmaf(R[5], dy, R[2] * dx));
    float Y[M];
    sh_band_eval<L>(x, y, z, Y);
#pragma unroll
    for (int ch = 0; ch < 3; ++ch) {
      float acc = Y[0] * c[ch];
#pragma unroll
      for (int j = 1; j < M; ++j) acc = __builtin_fmaf(Y[j], c[3 * j + ch], acc);
      F[k][ch] = acc;
    }
  }
#pragma unroll
  for (int m = 0; m < M; ++m) {
#pragma unroll
    for (int ch = 0; ch < 3; ++ch) {
      float acc = ShBandTables<L>::kInv[m][0] * F[0][ch];
#pragma unroll
      for (int k = 1; k < M; ++k) acc = __builtin_fmaf(ShBandTables<L>::kInv[m][k], F[k][ch], acc);
      o[3 * m + ch] = acc;
    }
  }
}

}  // namespace mgs
#endif
