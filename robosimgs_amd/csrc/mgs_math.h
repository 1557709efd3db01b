// mgs_math.h -- per-Gaussian math of the projection / colour stage, forward and backward.
//
// Plain scalar functions, usable from HIP device code and (for the logic tests under
// tests/host_harness) from a host compiler: MGS_HD expands to `__host__ __device__` under
// hipcc and to nothing under g++.  Semantics: SURVEY.md Appendix A.2 steps 1-6 (the
// gsplat 1.x "classic" projection the reference's Nerfstudio dependency uses; the
// reference itself holds no implementation, README.md:75).
#ifndef MGS_MATH_H_
#define MGS_MATH_H_

#include <math.h>
#include <stdint.h>

#if defined(__HIPCC__)
#define MGS_HD __host__ __device__ __forceinline__
#else
#define MGS_HD inline
#endif

// First statement of project_gaussian and of every helper it calls: multiply-adds are fused where ONE source expression
// holds both (the language's own rule, decided before inlining) and nowhere else.  hipcc's default for HIP is
// -ffp-contract=fast-honor-pragmas: without a pragma the back end fuses across statements as it sees fit in each kernel the
// function is inlined into, and mgs_projection_fwd and mgs_project_color_fwd then rounded conics and compensation differently
// in the last bits (18 and 10 of 257 rows); with this pragma they are the same instructions in both
// (tests/test_gpu_project_color_fwd.py::test_projection_fwd_is_the_fused_kernel_bit_for_bit).  The fused multiply-adds
// themselves stay.  Do NOT add a literal -ffp-contract=fast to the build flags: that form overrides the pragma, the back end
// fuses globally again and the agreement is lost.
#if defined(__clang__)
#define MGS_FP_CONTRACT_IN_EXPRESSION _Pragma("clang fp contract(on)")
#else
#define MGS_FP_CONTRACT_IN_EXPRESSION
#endif

namespace mgs {

struct CameraParams {  // one camera, row-major viewmat (OpenCV world-to-camera)
  float R[9];
  float t[3];
  float fx, fy, cx, cy;
  // the lens models only (the floats behind K in the camera's 16-float row), zero otherwise:
  //   MGS_CAMERA_FISHEYE_KB  k1..k4 in k[0..3] and theta_max^2 (floats 9..13)
  //   MGS_CAMERA_PINHOLE_BC  k1 k2 p1 p2 k3 in k[0..4] and the radial fold u_max (floats 9..14)
  float k[5], u_max;
};

// CAM: the camera model of the caller's instantiation -- only the two lens models read past K[8]
template <int CAM = 0>
MGS_HD CameraParams load_camera(const float* viewmat, const float* K) {
  CameraParams c;
  c.R[0] = viewmat[0]; c.R[1] = viewmat[1]; c.R[2] = viewmat[2];  c.t[0] = viewmat[3];
  c.R[3] = viewmat[4]; c.R[4] = viewmat[5]; c.R[5] = viewmat[6];  c.t[1] = viewmat[7];
  c.R[6] = viewmat[8]; c.R[7] = viewmat[9]; c.R[8] = viewmat[10]; c.t[2] = viewmat[11];
  c.fx = K[0]; c.cx = K[2]; c.fy = K[4]; c.cy = K[5];
  if constexpr (CAM == 3) {   // MGS_CAMERA_FISHEYE_KB
    c.k[0] = K[9]; c.k[1] = K[10]; c.k[2] = K[11]; c.k[3] = K[12]; c.u_max = K[13];
    c.k[4] = 0.f;
  } else if constexpr (CAM == 4) {   // MGS_CAMERA_PINHOLE_BC
    c.k[0] = K[9]; c.k[1] = K[10]; c.k[2] = K[11]; c.k[3] = K[12]; c.k[4] = K[13]; c.u_max = K[14];
  } else {
    c.k[0] = c.k[1] = c.k[2] = c.k[3] = c.k[4] = 0.f; c.u_max = 0.f;
  }
  return c;
}

// camera centre in world space: -R^T t
MGS_HD void camera_position(const CameraParams& c, float pos[3]) {
  pos[0] = -(c.R[0] * c.t[0] + c.R[3] * c.t[1] + c.R[6] * c.t[2]);
  pos[1] = -(c.R[1] * c.t[0] + c.R[4] * c.t[1] + c.R[7] * c.t[2]);
  pos[2] = -(c.R[2] * c.t[0] + c.R[5] * c.t[1] + c.R[8] * c.t[2]);
}

// The raw parameter form (include/mgs.h MGS_PARAMS_RAW): what an optimiser owns are log-scales and opacity logits;
// the project-colour kernels activate them in registers right after the load, s = exp(log_s), o = 1 / (1 + exp(-x)),
// with the accurate expf (about 1 ulp; the forward gate's margins are made for exactly rounded activations, not for
// the fast intrinsic's).  Backward: d s / d log_s = s, d o / d x = o (1 - o).
MGS_HD float activate_scale(float log_s) { return expf(log_s); }
MGS_HD float activate_opacity(float logit) { return 1.0f / (1.0f + expf(-logit)); }
MGS_HD float activate_opacity_grad(float o) { return o * (1.0f - o); }

#ifndef MGS_PROJ_FACTORED
// project_gaussian: 0 = cov2d in the textbook order of A.2 steps 2-4 (the reference's, and what every parity statement is made
// on); 1 = from the 2 x 3 factor J R Rq S (measurement, MGS_EXTRA_FLAGS=-DMGS_PROJ_FACTORED=1: profiles/r6/00_experiments.md 9)
#define MGS_PROJ_FACTORED 0
#endif

// a b - c d with one rounding's worth of error (Kahan): the product c d is rounded, its error recovered by an FMA
MGS_HD float diff_of_products(float a, float b, float c, float d) {
  MGS_FP_CONTRACT_IN_EXPRESSION
  const float w = c * d;
  const float e = fmaf(-c, d, w);     // w - c d exactly
  const float f = fmaf(a, b, -w);
  return f + e;
}

// C = A * B, all 3x3 row-major
MGS_HD void mat3_mul(const float* A, const float* B, float* C) {
  MGS_FP_CONTRACT_IN_EXPRESSION
  for (int i = 0; i < 3; ++i)
    for (int j = 0; j < 3; ++j)
      C[i * 3 + j] = A[i * 3 + 0] * B[0 * 3 + j] + A[i * 3 + 1] * B[1 * 3 + j] +
                     A[i * 3 + 2] * B[2 * 3 + j];
}
// C = A * B^T
MGS_HD void mat3_mul_bt(const float* A, const float* B, float* C) {
  MGS_FP_CONTRACT_IN_EXPRESSION
  for (int i = 0; i < 3; ++i)
    for (int j = 0; j < 3; ++j)
      C[i * 3 + j] = A[i * 3 + 0] * B[j * 3 + 0] + A[i * 3 + 1] * B[j * 3 + 1] +
                     A[i * 3 + 2] * B[j * 3 + 2];
}
// C = A^T * B
MGS_HD void mat3_mul_at(const float* A, const float* B, float* C) {
  for (int i = 0; i < 3; ++i)
    for (int j = 0; j < 3; ++j)
      C[i * 3 + j] = A[0 * 3 + i] * B[0 * 3 + j] + A[1 * 3 + i] * B[1 * 3 + j] +
                     A[2 * 3 + i] * B[2 * 3 + j];
}

// A.2 step 1: normalised wxyz quaternion -> rotation
MGS_HD void quat_to_rotmat(const float q[4], float R[9]) {
  MGS_FP_CONTRACT_IN_EXPRESSION
  float inv = 1.0f / sqrtf(q[0] * q[0] + q[1] * q[1] + q[2] * q[2] + q[3] * q[3]);
  float w = q[0] * inv, x = q[1] * inv, y = q[2] * inv, z = q[3] * inv;
  // (each entry one expression: its multiply-adds are fused under MGS_FP_CONTRACT_IN_EXPRESSION)
  R[0] = 1.f - 2.f * (y * y + z * z); R[1] = 2.f * (x * y - w * z);       R[2] = 2.f * (x * z + w * y);
  R[3] = 2.f * (x * y + w * z);       R[4] = 1.f - 2.f * (x * x + z * z); R[5] = 2.f * (y * z - w * x);
  R[6] = 2.f * (x * z - w * y);       R[7] = 2.f * (y * z + w * x);       R[8] = 1.f - 2.f * (x * x + y * y);
}

struct Projected {
  float mean2d[2];
  float depth;
  float conic[3];
  float compensation;
  int radius;    // 0 = culled; the extent along x under the per-axis rule
  int radius_y;  // == radius under the classic rule
};

// The radius rule is a compile-time policy: every kernel passes it as a template constant.
//   MGS_RADIUS_CLASSIC        gsplat 1.4 (A.2 step 5): one radius ceil(3 sqrt(lambda_1)), the square mean +- radius
//   MGS_RADIUS_OPACITY_AWARE  gsplat >= 1.5: per-axis extents ceil(e sqrt(Sigma_xx)), ceil(e sqrt(Sigma_yy)) with
//                             e = min(3.33, sqrt(2 ln(255 opacity))) -- the bounding box of the alpha >= 1/255 ellipse,
//                             capped at 3.33 sigma; Gaussians of opacity < 1/255 are culled; opacity is multiplied by
//                             the compensation in "antialiased" mode; without opacities e = 3.33
#define MGS_RADIUS_CLASSIC 0
#define MGS_RADIUS_OPACITY_AWARE 1

// The camera model is a compile-time policy like the radius rule (include/mgs.h MGS_CAMERA_*).  It changes the projected
// mean, the 2 x 3 Jacobian J of cov2d = J Sigma_c J^T and the frustum clamp (camera point p = (x, y, z), OpenCV axes):
//   MGS_CAMERA_PINHOLE  mean (fx x/z + cx, fy y/z + cy); J of that map with x/z, y/z clamped to 1.3 x the half field of view
//   MGS_CAMERA_ORTHO    mean (fx x + cx, fy y + cy); J = [[fx, 0, 0], [0, fy, 0]]; no clamp
//   MGS_CAMERA_FISHEYE  ideal equidistant lens, r = f theta: rho = |(x, y)|, theta = atan2(rho, z), s = theta / rho,
//                       mean (fx s x + cx, fy s y + cy); J is the (dense) Jacobian of that map; no clamp
//   MGS_CAMERA_FISHEYE_KB  that lens with OpenCV's fisheye polynomial: theta_d = theta P(theta^2) (fisheye_kb_terms below);
//                       culled where theta^2 >= cam.u_max, the end of the polynomial's monotonic range
//   MGS_CAMERA_PINHOLE_BC  the pinhole camera with OpenCV's radial / tangential lens (pinhole_bc_terms below): dense J, no
//                       clamp; culled past the radial fold, where det Jd <= 0, and outside the pinhole's clamp box
// Depth is camera z and near / far cull on it under every model.
#ifndef MGS_CAMERA_PINHOLE
#define MGS_CAMERA_PINHOLE 0
#define MGS_CAMERA_ORTHO 1
#define MGS_CAMERA_FISHEYE 2
#endif
#ifndef MGS_CAMERA_FISHEYE_KB
#define MGS_CAMERA_FISHEYE_KB 3
#endif
#ifndef MGS_CAMERA_PINHOLE_BC
#define MGS_CAMERA_PINHOLE_BC 4
#endif

// Below t = rho^2 / z^2 = 0.1 the fisheye terms come from their series in t (nine terms: truncation < 1e-8 relative):
// the closed forms are 0/0 on the optical axis and lose digits to cancellation near it.
#define MGS_FISHEYE_SERIES_T 0.1f

// Equidistant fisheye at camera point (x, y, z), with q = rho^2 and r2 = q + z^2:
//   s = theta / rho                     -> 1/z on the axis
//   a = (z / r2 - s) / q = ds/dq / ...  -> -2 / (3 z^3)   (ds/dx = a x, ds/dy = a y, ds/dz = -1 / r2)
//   b = da/dq = (-z / r2^2 - 3a/2) / q  -> 4 / (5 z^5)    (da/dx = 2 x b, da/dy = 2 y b, da/dz = 2 / r2^2; backward only)
//   ir2 = 1 / r2
// Series with t = q / z^2:  s z = sum (-t)^n / (2n+1);  a z^3 = sum (-1)^(n+1) 2(n+1)/(2n+3) t^n;  b z^5 = d(a z^3)/dt.
template <bool WITH_B>
MGS_HD void fisheye_terms(float x, float y, float z, float& s, float& a, float& b, float& ir2) {
  MGS_FP_CONTRACT_IN_EXPRESSION
  const float q = x * x + y * y;
  ir2 = 1.0f / (q + z * z);
  if (z > 0.f && q < MGS_FISHEYE_SERIES_T * (z * z)) {
    const float rz = 1.0f / z, rz2 = rz * rz, t = q * rz2;
    s = rz * (1.f + t * (-1.f / 3.f + t * (1.f / 5.f + t * (-1.f / 7.f + t * (1.f / 9.f + t * (-1.f / 11.f +
        t * (1.f / 13.f + t * (-1.f / 15.f + t * (1.f / 17.f)))))))));
    a = rz * rz2 * (-2.f / 3.f + t * (4.f / 5.f + t * (-6.f / 7.f + t * (8.f / 9.f + t * (-10.f / 11.f +
        t * (12.f / 13.f + t * (-14.f / 15.f + t * (16.f / 17.f + t * (-18.f / 19.f)))))))));
    if (WITH_B)
      b = rz2 * rz2 * rz * (4.f / 5.f + t * (-12.f / 7.f + t * (24.f / 9.f + t * (-40.f / 11.f + t * (60.f / 13.f +
          t * (-84.f / 15.f + t * (112.f / 17.f + t * (-144.f / 19.f + t * (180.f / 21.f)))))))));
  } else {
    const float rho = sqrtf(q);
    s = atan2f(rho, z) / rho;
    a = (z * ir2 - s) / q;
    if (WITH_B) b = (-z * ir2 * ir2 - 1.5f * a) / q;
  }
}

// The Kannala-Brandt polynomial on top of the equidistant terms (s, a, ir2 of fisheye_terms at the same point; q = rho^2):
//   u = theta^2 = s^2 q,  P(u) = 1 + k1 u + k2 u^2 + k3 u^3 + k4 u^4,  theta_d = theta P
//   S = s P                       (the mean is (fx S x + cx, fy S y + cy))
//   A = a P + 2 s^2 z P' / r2     (dS/dx = A x, dS/dy = A y)
//   D = P + 2 u P' = d theta_d / d theta     (dS/dz = -D / r2)
// so J is the equidistant J with s -> S, a -> A and its third column times D.  No new singularity on the axis: u, P, P'
// are polynomials in what the series branch yields.  du/d(x, y, z) = (2 s z x, 2 s z y, -2 s q) / r2.
struct FisheyeKb {
  float u, P, P1, P2;   // P1 = P', P2 = P''
  float S, A, D;
};
template <bool WITH_P2>
MGS_HD FisheyeKb fisheye_kb_terms(const float k[4], float q, float z, float s, float a, float ir2) {
  MGS_FP_CONTRACT_IN_EXPRESSION
  FisheyeKb t;
  const float u = s * s * q;
  t.u = u;
  t.P = 1.f + u * (k[0] + u * (k[1] + u * (k[2] + u * k[3])));
  t.P1 = k[0] + u * (2.f * k[1] + u * (3.f * k[2] + u * (4.f * k[3])));
  t.P2 = WITH_P2 ? 2.f * k[1] + u * (6.f * k[2] + u * (12.f * k[3])) : 0.f;
  t.S = s * t.P;
  t.A = a * t.P + 2.f * s * s * z * t.P1 * ir2;
  t.D = t.P + 2.f * u * t.P1;
  return t;
}

// OpenCV's radial / tangential (Brown-Conrady) lens at the normalised point (a, b) = (x/z, y/z), include/mgs_lens_pinhole.h;
// k = (k1, k2, p1, p2, k3), u = a^2 + b^2:
//   Rad = 1 + k1 u + k2 u^2 + k3 u^3,  R1 = Rad',  R2 = Rad''  (backward only)
//   xd = a Rad + 2 p1 a b + p2 (u + 2 a^2),  yd = b Rad + p1 (u + 2 b^2) + 2 p2 a b
//   Jd = d(xd, yd)/d(a, b) = [[d00, d01], [d01, d11]]
struct PinholeBc {
  float u, R1, R2;
  float xd, yd;
  float d00, d01, d11;
};
template <bool WITH_R2>
MGS_HD PinholeBc pinhole_bc_terms(const float k[5], float a, float b) {
  MGS_FP_CONTRACT_IN_EXPRESSION
  PinholeBc t;
  const float aa = a * a, bb = b * b, ab = a * b, u = aa + bb;
  const float p1 = k[2], p2 = k[3];
  const float Rad = 1.f + u * (k[0] + u * (k[1] + u * k[4]));
  t.u = u;
  t.R1 = k[0] + u * (2.f * k[1] + u * (3.f * k[4]));
  t.R2 = WITH_R2 ? 2.f * k[1] + u * (6.f * k[4]) : 0.f;
  t.xd = a * Rad + 2.f * p1 * ab + p2 * (u + 2.f * aa);
  t.yd = b * Rad + p1 * (u + 2.f * bb) + 2.f * p2 * ab;
  t.d00 = Rad + 2.f * aa * t.R1 + 2.f * p1 * b + 6.f * p2 * a;
  t.d01 = 2.f * ab * t.R1 + 2.f * p1 * a + 2.f * p2 * b;
  t.d11 = Rad + 2.f * bb * t.R1 + 6.f * p1 * b + 2.f * p2 * a;
  return t;
}

// A.2 steps 1-5.  Returns radius == 0 for culled Gaussians (all other fields zeroed).
template <int CAM = MGS_CAMERA_PINHOLE>
MGS_HD Projected project_gaussian(const float mean[3], const float quat[4],
                                  const float scale[3], const CameraParams& cam, float W,
                                  float H, float eps2d, float near_plane, float far_plane,
                                  float radius_clip, int radius_rule = MGS_RADIUS_CLASSIC,
                                  bool has_opacity = false, float opacity = 1.f, bool antialiased = false) {
  MGS_FP_CONTRACT_IN_EXPRESSION
  Projected out;
  out.mean2d[0] = out.mean2d[1] = out.depth = 0.f;
  out.conic[0] = out.conic[1] = out.conic[2] = 0.f;
  out.compensation = 0.f;
  out.radius = 0;
  out.radius_y = 0;

  const float* R = cam.R;
  float x = R[0] * mean[0] + R[1] * mean[1] + R[2] * mean[2] + cam.t[0];
  float y = R[3] * mean[0] + R[4] * mean[1] + R[5] * mean[2] + cam.t[1];
  float z = R[6] * mean[0] + R[7] * mean[1] + R[8] * mean[2] + cam.t[2];
  if (!(z >= near_plane) || !(z <= far_plane)) return out;

  // J = [[j00, j01, j02], [j10, j11, j12]]; j01 = j10 = 0 except under the fisheye model
  float j00, j01 = 0.f, j02, j10 = 0.f, j11, j12, rz, fs = 0.f;
  [[maybe_unused]] float bcx = 0.f, bcy = 0.f;     // MGS_CAMERA_PINHOLE_BC: the distorted normalised point
  if constexpr (CAM == MGS_CAMERA_PINHOLE) {
    rz = 1.0f / z;
    float rz2 = rz * rz;
    float tanx = 0.5f * W / cam.fx, tany = 0.5f * H / cam.fy;
    float lim_xp = (W - cam.cx) / cam.fx + 0.3f * tanx, lim_xn = cam.cx / cam.fx + 0.3f * tanx;
    float lim_yp = (H - cam.cy) / cam.fy + 0.3f * tany, lim_yn = cam.cy / cam.fy + 0.3f * tany;
    float tx = z * fminf(lim_xp, fmaxf(-lim_xn, x * rz));
    float ty = z * fminf(lim_yp, fmaxf(-lim_yn, y * rz));
    j00 = cam.fx * rz; j02 = -cam.fx * tx * rz2;
    j11 = cam.fy * rz; j12 = -cam.fy * ty * rz2;
  } else if constexpr (CAM == MGS_CAMERA_ORTHO) {
    rz = 1.f;
    j00 = cam.fx; j02 = 0.f;
    j11 = cam.fy; j12 = 0.f;
  } else if constexpr (CAM == MGS_CAMERA_FISHEYE) {
    float fa, fb, ir2;
    fisheye_terms<false>(x, y, z, fs, fa, fb, ir2);
    rz = 1.f;
    const float xya = x * y * fa;
    j00 = cam.fx * (fs + x * x * fa); j01 = cam.fx * xya; j02 = -cam.fx * x * ir2;
    j10 = cam.fy * xya; j11 = cam.fy * (fs + y * y * fa); j12 = -cam.fy * y * ir2;
  } else if constexpr (CAM == MGS_CAMERA_PINHOLE_BC) {
    rz = 1.0f / z;
    const float pa = x * rz, pb = y * rz;
    const PinholeBc bc = pinhole_bc_terms<false>(cam.k, pa, pb);
    if (!(bc.u < cam.u_max)) return out;                                  // past the radial fold
    if (!(diff_of_products(bc.d00, bc.d11, bc.d01, bc.d01) > 0.f)) return out;   // the lens map folds (det Jd <= 0)
    // the pinhole's clamp box, here a cull on the distorted point: the frame plus 0.3 of the half field
    float tanx = 0.5f * W / cam.fx, tany = 0.5f * H / cam.fy;
    float lim_xp = (W - cam.cx) / cam.fx + 0.3f * tanx, lim_xn = cam.cx / cam.fx + 0.3f * tanx;
    float lim_yp = (H - cam.cy) / cam.fy + 0.3f * tany, lim_yn = cam.cy / cam.fy + 0.3f * tany;
    if (!(bc.xd <= lim_xp && bc.xd >= -lim_xn && bc.yd <= lim_yp && bc.yd >= -lim_yn)) return out;
    bcx = bc.xd; bcy = bc.yd;
    j00 = cam.fx * bc.d00 * rz; j01 = cam.fx * bc.d01 * rz; j02 = -cam.fx * rz * (bc.d00 * pa + bc.d01 * pb);
    j10 = cam.fy * bc.d01 * rz; j11 = cam.fy * bc.d11 * rz; j12 = -cam.fy * rz * (bc.d01 * pa + bc.d11 * pb);
  } else {
    static_assert(CAM == MGS_CAMERA_FISHEYE_KB, "camera model");
    float es, ea, eb, ir2;
    fisheye_terms<false>(x, y, z, es, ea, eb, ir2);
    const FisheyeKb kb = fisheye_kb_terms<false>(cam.k, x * x + y * y, z, es, ea, ir2);
    if (!(kb.u < cam.u_max)) return out;      // past the lens's monotonic range: culled like the near plane
    rz = 1.f;
    fs = kb.S;
    const float xya = x * y * kb.A, dr = kb.D * ir2;
    j00 = cam.fx * (fs + x * x * kb.A); j01 = cam.fx * xya; j02 = -cam.fx * x * dr;
    j10 = cam.fy * xya; j11 = cam.fy * (fs + y * y * kb.A); j12 = -cam.fy * y * dr;
  }
  float Rq[9];
  quat_to_rotmat(quat, Rq);
#if MGS_PROJ_FACTORED
  // cov2d = M2 M2^T with M2 = J R Rq diag(scale), a 2 x 3 matrix -- the same matrix as J (R (Rq S S Rq^T) R^T) J^T of A.2 steps
  // 2-4 without ever forming a covariance: a, c are sums of squares and det(cov2d) is the sum of M2's squared 2 x 2 minors
  // (Cauchy-Binet).  The textbook order's det = a c - b^2 cancels for a needle-like Gaussian (relative conic error up to 5e-3
  // at 300 : 1, this order's 2e-6) -- but that error scales the WHOLE conic, which the blend forgives; what sigma = 1/2 d^T conic d
  // does not forgive is independent noise in the three entries, and there the two orders differ by a factor of two
  // (profiles/r6/00_experiments.md section 9: half the pixels over tolerance over 59 clustered scenes, worse on 10 of them).
  float RR[9];
  mat3_mul(R, Rq, RR);
  float m0[3], m1[3];
  for (int k = 0; k < 3; ++k) {
    if constexpr (CAM == MGS_CAMERA_FISHEYE || CAM == MGS_CAMERA_FISHEYE_KB || CAM == MGS_CAMERA_PINHOLE_BC) {
      m0[k] = (j00 * RR[k] + j01 * RR[3 + k] + j02 * RR[6 + k]) * scale[k];
      m1[k] = (j10 * RR[k] + j11 * RR[3 + k] + j12 * RR[6 + k]) * scale[k];
    } else {
      m0[k] = (j00 * RR[k] + j02 * RR[6 + k]) * scale[k];
      m1[k] = (j11 * RR[3 + k] + j12 * RR[6 + k]) * scale[k];
    }
  }
  float a = m0[0] * m0[0] + m0[1] * m0[1] + m0[2] * m0[2];
  float b = m0[0] * m1[0] + m0[1] * m1[1] + m0[2] * m1[2];
  float c = m1[0] * m1[0] + m1[1] * m1[1] + m1[2] * m1[2];
  const float d01 = diff_of_products(m0[0], m1[1], m0[1], m1[0]);
  const float d02 = diff_of_products(m0[0], m1[2], m0[2], m1[0]);
  const float d12 = diff_of_products(m0[1], m1[2], m0[2], m1[1]);
  float det0 = d01 * d01 + d02 * d02 + d12 * d12;
  float det = det0 + eps2d * (a + c) + eps2d * eps2d;       // det(cov2d + eps2d I): positive terms only
  a += eps2d;
  c += eps2d;
#else
  float M[9], cov[9], tmp[9], covc[9];
  for (int i = 0; i < 3; ++i)
    for (int j = 0; j < 3; ++j) M[i * 3 + j] = Rq[i * 3 + j] * scale[j];
  mat3_mul_bt(M, M, cov);       // Sigma = M M^T
  mat3_mul(R, cov, tmp);        // R Sigma
  mat3_mul_bt(tmp, R, covc);    // R Sigma R^T
  float a, b, c;
  if constexpr (CAM == MGS_CAMERA_FISHEYE || CAM == MGS_CAMERA_FISHEYE_KB || CAM == MGS_CAMERA_PINHOLE_BC) {
    // cov2d = J covc J^T with a dense J: T = J covc (2 x 3), then T J^T
    float t0[3], t1[3];
    for (int k = 0; k < 3; ++k) {
      t0[k] = j00 * covc[k] + j01 * covc[3 + k] + j02 * covc[6 + k];
      t1[k] = j10 * covc[k] + j11 * covc[3 + k] + j12 * covc[6 + k];
    }
    a = t0[0] * j00 + t0[1] * j01 + t0[2] * j02;
    b = t0[0] * j10 + t0[1] * j11 + t0[2] * j12;
    c = t1[0] * j10 + t1[1] * j11 + t1[2] * j12;
  } else {
    // cov2d = J covc J^T with J = [[j00,0,j02],[0,j11,j12]]
    a = j00 * (j00 * covc[0] + j02 * covc[6]) + j02 * (j00 * covc[2] + j02 * covc[8]);
    b = j00 * (j11 * covc[1] + j12 * covc[2]) + j02 * (j11 * covc[7] + j12 * covc[8]);
    c = j11 * (j11 * covc[4] + j12 * covc[7]) + j12 * (j11 * covc[5] + j12 * covc[8]);
  }
  float det0 = a * c - b * b;
  a += eps2d;
  c += eps2d;
  float det = a * c - b * b;
  if constexpr (CAM == MGS_CAMERA_FISHEYE_KB || CAM == MGS_CAMERA_PINHOLE_BC) {
    // (MGS_CAMERA_PINHOLE_BC: the same towards its folds, where det Jd -> 0 squashes the splat along one axis.)
    // Towards theta_max the lens squashes a splat radially by D -> 0: cov2d turns needle-like whatever the Gaussian's own
    // shape, and a c - b^2 cancels (the compensation factor was off by 3e-3 relative within a few degrees of the fold).
    // So this model alone takes det(cov2d) as the sum of the squared 2 x 2 minors of M2 = J R Rq S (Cauchy-Binet, positive
    // terms only, as under MGS_PROJ_FACTORED) and the blurred determinant from it; a, b, c keep the textbook order.
    float RR[9], m0[3], m1[3];
    mat3_mul(R, Rq, RR);
    for (int k = 0; k < 3; ++k) {
      m0[k] = (j00 * RR[k] + j01 * RR[3 + k] + j02 * RR[6 + k]) * scale[k];
      m1[k] = (j10 * RR[k] + j11 * RR[3 + k] + j12 * RR[6 + k]) * scale[k];
    }
    const float d01 = diff_of_products(m0[0], m1[1], m0[1], m1[0]);
    const float d02 = diff_of_products(m0[0], m1[2], m0[2], m1[0]);
    const float d12 = diff_of_products(m0[1], m1[2], m0[2], m1[1]);
    det0 = d01 * d01 + d02 * d02 + d12 * d12;
    det = det0 + eps2d * (a + c) - eps2d * eps2d;        // det(cov2d + eps2d I), a and c already blurred
  }
#endif
  float mx, my;
  if constexpr (CAM == MGS_CAMERA_PINHOLE) {
    mx = cam.fx * x * rz + cam.cx; my = cam.fy * y * rz + cam.cy;
  } else if constexpr (CAM == MGS_CAMERA_ORTHO) {
    mx = cam.fx * x + cam.cx; my = cam.fy * y + cam.cy;
  } else if constexpr (CAM == MGS_CAMERA_PINHOLE_BC) {
    mx = cam.fx * bcx + cam.cx; my = cam.fy * bcy + cam.cy;
  } else {
    mx = cam.fx * (fs * x) + cam.cx; my = cam.fy * (fs * y) + cam.cy;
  }

  if (!(det > 0.f)) return out;
  float inv_det = 1.0f / det;

  float radius, radius_y;
  if (radius_rule == MGS_RADIUS_OPACITY_AWARE) {
    float extent = 3.33f;
    if (has_opacity) {
      const float op = antialiased ? opacity * sqrtf(fmaxf(0.f, det0 * inv_det)) : opacity;
      if (!(op >= 1.0f / 255.0f)) return out;
      extent = fminf(extent, sqrtf(2.f * logf(op * 255.0f)));
    }
    radius = ceilf(extent * sqrtf(a));
    radius_y = ceilf(extent * sqrtf(c));
    if (!(radius > radius_clip) && !(radius_y > radius_clip)) return out;
    if (!(radius > 0.f) || !(radius_y > 0.f)) return out;            // an extent of exactly zero reaches no pixel
  } else {
    float m = 0.5f * (a + c);
    float lam = m + sqrtf(fmaxf(0.01f, m * m - det));
    radius = ceilf(3.f * sqrtf(lam));
    radius_y = radius;
    if (!(radius > radius_clip)) return out;
  }
  if (mx + radius <= 0.f || mx - radius >= W || my + radius_y <= 0.f || my - radius_y >= H)
    return out;

  out.mean2d[0] = mx;
  out.mean2d[1] = my;
  out.depth = z;
  out.conic[0] = c * inv_det;
  out.conic[1] = -b * inv_det;
  out.conic[2] = a * inv_det;
  out.compensation = sqrtf(fmaxf(0.f, det0 * inv_det));
  out.radius = (int)radius;
  out.radius_y = (int)radius_y;
  return out;
}

// ---- A.2 step 6: real SH basis (gsplat ordering / signs) --------------------------------
#define MGS_SH_C0 0.2820947917738781f
#define MGS_SH_C1 0.48860251190292f

// Y[0..(deg+1)^2) for a UNIT direction.
MGS_HD void sh_basis(int deg, float x, float y, float z, float* Y) {
  Y[0] = MGS_SH_C0;
  if (deg < 1) return;
  Y[1] = -MGS_SH_C1 * y;
  Y[2] = MGS_SH_C1 * z;
  Y[3] = -MGS_SH_C1 * x;
  if (deg < 2) return;
  float z2 = z * z, fC1 = x * x - y * y, fS1 = 2.f * x * y;
  float t = -1.092548430592079f * z;
  Y[4] = 0.5462742152960395f * fS1;
  Y[5] = t * y;
  Y[6] = 0.9461746957575601f * z2 - 0.3153915652525201f;
  Y[7] = t * x;
  Y[8] = 0.5462742152960395f * fC1;
  if (deg < 3) return;
  float u = -2.285228997322329f * z2 + 0.4570457994644658f;
  float w = 1.445305721320277f * z;
  float fC2 = x * fC1 - y * fS1, fS2 = x * fS1 + y * fC1;
  Y[9] = -0.5900435899266435f * fS2;
  Y[10] = w * fS1;
  Y[11] = u * y;
  Y[12] = z * (1.865881662950577f * z2 - 1.119528997770346f);
  Y[13] = u * x;
  Y[14] = w * fC1;
  Y[15] = -0.5900435899266435f * fC2;
}

// Colour of one Gaussian: evaluate sum_k Y_k(dir) * coeff_k for KC = (DEG+1)^2 coefficients held in registers.
template <int DEG>
MGS_HD void sh_dot(const float dir[3], const float* c /*[KC*3]*/, float rgb[3]) {
  constexpr int KC = (DEG + 1) * (DEG + 1);
  float n2 = dir[0] * dir[0] + dir[1] * dir[1] + dir[2] * dir[2];
  float inv = n2 > 0.f ? 1.0f / sqrtf(n2) : 0.f;
  float Y[KC];
  sh_basis(DEG, dir[0] * inv, dir[1] * inv, dir[2] * inv, Y);
  float r = 0.f, g = 0.f, b = 0.f;
#pragma unroll
  for (int k = 0; k < KC; ++k) {
    r += Y[k] * c[3 * k + 0];
    g += Y[k] * c[3 * k + 1];
    b += Y[k] * c[3 * k + 2];
  }
  rgb[0] = r; rgb[1] = g; rgb[2] = b;
}

// dY/dx, dY/dy, dY/dz of the polynomial basis above (treating x,y,z as independent).
MGS_HD void sh_basis_grad(int deg, float x, float y, float z, float* Yx, float* Yy, float* Yz) {
  Yx[0] = Yy[0] = Yz[0] = 0.f;
  if (deg < 1) return;
  Yx[1] = 0.f;        Yy[1] = -MGS_SH_C1; Yz[1] = 0.f;
  Yx[2] = 0.f;        Yy[2] = 0.f;        Yz[2] = MGS_SH_C1;
  Yx[3] = -MGS_SH_C1; Yy[3] = 0.f;        Yz[3] = 0.f;
  if (deg < 2) return;
  const float c2a = 0.5462742152960395f, c2b = -1.092548430592079f, c2c = 0.9461746957575601f;
  float z2 = z * z, fC1 = x * x - y * y, fS1 = 2.f * x * y;
  // fS1_x = 2y, fS1_y = 2x; fC1_x = 2x, fC1_y = -2y
  Yx[4] = c2a * 2.f * y; Yy[4] = c2a * 2.f * x; Yz[4] = 0.f;
  Yx[5] = 0.f;           Yy[5] = c2b * z;       Yz[5] = c2b * y;
  Yx[6] = 0.f;           Yy[6] = 0.f;           Yz[6] = c2c * 2.f * z;
  Yx[7] = c2b * z;       Yy[7] = 0.f;           Yz[7] = c2b * x;
  Yx[8] = c2a * 2.f * x; Yy[8] = -c2a * 2.f * y; Yz[8] = 0.f;
  if (deg < 3) return;
  const float c3a = -0.5900435899266435f, c3w = 1.445305721320277f;
  const float c3u1 = -2.285228997322329f, c3u0 = 0.4570457994644658f;
  const float c3z1 = 1.865881662950577f, c3z0 = 1.119528997770346f;
  float u = c3u1 * z2 + c3u0, w = c3w * z;
  float u_z = c3u1 * 2.f * z;
  // fC2 = x fC1 - y fS1 ; fS2 = x fS1 + y fC1
  float fC2_x = fC1 + x * 2.f * x - y * 2.f * y;   // = 3x^2 - 3y^2
  float fC2_y = x * (-2.f * y) - fS1 - y * 2.f * x; // = -6xy
  float fS2_x = fS1 + x * 2.f * y + y * 2.f * x;   // = 6xy
  float fS2_y = x * 2.f * x + fC1 + y * (-2.f * y); // = 3x^2 - 3y^2
  Yx[9] = c3a * fS2_x;   Yy[9] = c3a * fS2_y;   Yz[9] = 0.f;
  Yx[10] = w * 2.f * y;  Yy[10] = w * 2.f * x;  Yz[10] = c3w * fS1;
  Yx[11] = 0.f;          Yy[11] = u;            Yz[11] = u_z * y;
  Yx[12] = 0.f;          Yy[12] = 0.f;          Yz[12] = (c3z1 * z2 - c3z0) + z * c3z1 * 2.f * z;
  Yx[13] = u;            Yy[13] = 0.f;          Yz[13] = u_z * x;
  Yx[14] = w * 2.f * x;  Yy[14] = -w * 2.f * y; Yz[14] = c3w * fC1;
  Yx[15] = c3a * fC2_x;  Yy[15] = c3a * fC2_y;  Yz[15] = 0.f;
}


// =========================================================================================
// Backward (vector-Jacobian products) of the functions above
// =========================================================================================

// v_q (un-normalised wxyz) from the cotangent G (row-major 3x3) of R(q/|q|)
MGS_HD void quat_to_rotmat_vjp(const float q[4], const float G[9], float v_q[4]) {
  float inv = 1.0f / sqrtf(q[0] * q[0] + q[1] * q[1] + q[2] * q[2] + q[3] * q[3]);
  float w = q[0] * inv, x = q[1] * inv, y = q[2] * inv, z = q[3] * inv;
  float vn[4];
  vn[0] = 2.f * (x * (G[7] - G[5]) + y * (G[2] - G[6]) + z * (G[3] - G[1]));
  vn[1] = 2.f * (y * (G[1] + G[3]) + z * (G[2] + G[6]) + w * (G[7] - G[5]) - 2.f * x * (G[4] + G[8]));
  vn[2] = 2.f * (x * (G[1] + G[3]) + z * (G[5] + G[7]) + w * (G[2] - G[6]) - 2.f * y * (G[0] + G[8]));
  vn[3] = 2.f * (x * (G[2] + G[6]) + y * (G[5] + G[7]) + w * (G[3] - G[1]) - 2.f * z * (G[0] + G[4]));
  float d = vn[0] * w + vn[1] * x + vn[2] * y + vn[3] * z;
  v_q[0] = (vn[0] - d * w) * inv;
  v_q[1] = (vn[1] - d * x) * inv;
  v_q[2] = (vn[2] - d * y) * inv;
  v_q[3] = (vn[3] - d * z) * inv;
}

struct ProjectedGrad {
  float v_mean[3];
  float v_quat[4];
  float v_scale[3];
  float v_R[9];   // d/d viewmat rotation (row-major)
  float v_t[3];   // d/d viewmat translation
};

// VJP of project_gaussian for a VISIBLE Gaussian (radius > 0).  `conic` is the forward
// output; v_comp is the cotangent of the compensation factor (0 unless antialiased).
template <int CAM = MGS_CAMERA_PINHOLE>
MGS_HD ProjectedGrad project_gaussian_vjp(const float mean[3], const float quat[4],
                                          const float scale[3], const CameraParams& cam, float W,
                                          float H, float eps2d, const float conic[3],
                                          float compensation, const float v_mean2d[2],
                                          float v_depth, const float v_conic[3], float v_comp) {
  ProjectedGrad g;
  const float* R = cam.R;
  float x = R[0] * mean[0] + R[1] * mean[1] + R[2] * mean[2] + cam.t[0];
  float y = R[3] * mean[0] + R[4] * mean[1] + R[5] * mean[2] + cam.t[1];
  float z = R[6] * mean[0] + R[7] * mean[1] + R[8] * mean[2] + cam.t[2];

  // recompute Sigma_c and J
  float Rq[9], M[9], cov[9], tmp[9], covc[9];
  quat_to_rotmat(quat, Rq);
  for (int i = 0; i < 3; ++i)
    for (int j = 0; j < 3; ++j) M[i * 3 + j] = Rq[i * 3 + j] * scale[j];
  mat3_mul_bt(M, M, cov);
  mat3_mul(R, cov, tmp);
  mat3_mul_bt(tmp, R, covc);
  // (the pinhole model's J and clamp state; the other models' code after it leaves the pinhole build unchanged)
  float tanx = 0.5f * W / cam.fx, tany = 0.5f * H / cam.fy;
  float lim_xp = (W - cam.cx) / cam.fx + 0.3f * tanx, lim_xn = cam.cx / cam.fx + 0.3f * tanx;
  float lim_yp = (H - cam.cy) / cam.fy + 0.3f * tany, lim_yn = cam.cy / cam.fy + 0.3f * tany;
  float rz = 1.0f / z, rz2 = rz * rz, rz3 = rz2 * rz;
  float xr = x * rz, yr = y * rz;
  bool x_in = xr <= lim_xp && xr >= -lim_xn, y_in = yr <= lim_yp && yr >= -lim_yn;
  float tx = z * fminf(lim_xp, fmaxf(-lim_xn, xr));
  float ty = z * fminf(lim_yp, fmaxf(-lim_yn, yr));
  float j00 = cam.fx * rz, j02 = -cam.fx * tx * rz2, j11 = cam.fy * rz, j12 = -cam.fy * ty * rz2;
  float j01 = 0.f, j10 = 0.f, fs = 0.f, fa = 0.f, fb = 0.f, ir2 = 0.f;   // fisheye: s, a, b, 1 / r2 (fisheye_terms)
  if constexpr (CAM == MGS_CAMERA_ORTHO) {
    j00 = cam.fx; j02 = 0.f; j11 = cam.fy; j12 = 0.f;
  } else if constexpr (CAM == MGS_CAMERA_FISHEYE) {
    fisheye_terms<true>(x, y, z, fs, fa, fb, ir2);
    const float xya = x * y * fa;
    j00 = cam.fx * (fs + x * x * fa); j01 = cam.fx * xya; j02 = -cam.fx * x * ir2;
    j10 = cam.fy * xya; j11 = cam.fy * (fs + y * y * fa); j12 = -cam.fy * y * ir2;
  }
  [[maybe_unused]] FisheyeKb kb;
  if constexpr (CAM == MGS_CAMERA_FISHEYE_KB) {
    fisheye_terms<true>(x, y, z, fs, fa, fb, ir2);     // the equidistant s, a, b; the lens's S, A, D in kb
    kb = fisheye_kb_terms<true>(cam.k, x * x + y * y, z, fs, fa, ir2);
    const float xya = x * y * kb.A, dr = kb.D * ir2;
    j00 = cam.fx * (kb.S + x * x * kb.A); j01 = cam.fx * xya; j02 = -cam.fx * x * dr;
    j10 = cam.fy * xya; j11 = cam.fy * (kb.S + y * y * kb.A); j12 = -cam.fy * y * dr;
  }
  [[maybe_unused]] PinholeBc bc;
  if constexpr (CAM == MGS_CAMERA_PINHOLE_BC) {
    bc = pinhole_bc_terms<true>(cam.k, xr, yr);
    j00 = cam.fx * bc.d00 * rz; j01 = cam.fx * bc.d01 * rz; j02 = -cam.fx * rz * (bc.d00 * xr + bc.d01 * yr);
    j10 = cam.fy * bc.d01 * rz; j11 = cam.fy * bc.d11 * rz; j12 = -cam.fy * rz * (bc.d01 * xr + bc.d11 * yr);
  }
  static_assert(CAM == MGS_CAMERA_PINHOLE || CAM == MGS_CAMERA_ORTHO || CAM == MGS_CAMERA_FISHEYE ||
                    CAM == MGS_CAMERA_FISHEYE_KB || CAM == MGS_CAMERA_PINHOLE_BC, "camera model");

  // conic = inv(cov2d + eps I):  G2 = -conic * Vc * conic, Vc = [[va, vb/2],[vb/2, vc]]
  float ca = conic[0], cb = conic[1], cc = conic[2];
  float va = v_conic[0], vb = 0.5f * v_conic[1], vc = v_conic[2];
  // P = conic * Vc
  float p00 = ca * va + cb * vb, p01 = ca * vb + cb * vc;
  float p10 = cb * va + cc * vb, p11 = cb * vb + cc * vc;
  float g00 = -(p00 * ca + p01 * cb), g01 = -(p00 * cb + p01 * cc);
  float g10 = -(p10 * ca + p11 * cb), g11 = -(p10 * cb + p11 * cc);
  if (v_comp != 0.f) {   // compensation = sqrt(max(0, det(C)/det(C+eps I)))
    float det_conic = ca * cc - cb * cb;
    float v_sqr = v_comp * 0.5f / (compensation + 1e-6f);
    float om = 1.f - compensation * compensation;
    g00 += v_sqr * (om * ca - eps2d * det_conic);
    g01 += v_sqr * (om * cb);
    g10 += v_sqr * (om * cb);
    g11 += v_sqr * (om * cc - eps2d * det_conic);
  }
  // cov2d = J covc J^T ;  v_covc = J^T G2 J ;  v_J = (G2 + G2^T) J covc
  float J[6] = {j00, j01, j02, j10, j11, j12};
  float G2[4] = {g00, g01, g10, g11};
  float GJ[6];    // G2 * J (2x3)
  for (int c = 0; c < 3; ++c) {
    GJ[c] = G2[0] * J[c] + G2[1] * J[3 + c];
    GJ[3 + c] = G2[2] * J[c] + G2[3] * J[3 + c];
  }
  float v_covc[9];
  for (int r = 0; r < 3; ++r)
    for (int c = 0; c < 3; ++c) v_covc[r * 3 + c] = J[r] * GJ[c] + J[3 + r] * GJ[3 + c];
  float Gs[4] = {2.f * g00, g01 + g10, g01 + g10, 2.f * g11};
  float GsJ[6];
  for (int c = 0; c < 3; ++c) {
    GsJ[c] = Gs[0] * J[c] + Gs[1] * J[3 + c];
    GsJ[3 + c] = Gs[2] * J[c] + Gs[3] * J[3 + c];
  }
  float vJ00 = 0.f, vJ02 = 0.f, vJ11 = 0.f, vJ12 = 0.f;   // only the non-constant entries of a pinhole J
  for (int k = 0; k < 3; ++k) {
    vJ00 += GsJ[k] * covc[k * 3 + 0];
    vJ02 += GsJ[k] * covc[k * 3 + 2];
    vJ11 += GsJ[3 + k] * covc[k * 3 + 1];
    vJ12 += GsJ[3 + k] * covc[k * 3 + 2];
  }
  // camera-space mean
  float vx = cam.fx * rz * v_mean2d[0];
  float vy = cam.fy * rz * v_mean2d[1];
  float vz = -(cam.fx * x * v_mean2d[0] + cam.fy * y * v_mean2d[1]) * rz2 + v_depth;
  if constexpr (CAM == MGS_CAMERA_PINHOLE) {
    if (x_in) vx += -cam.fx * rz2 * vJ02; else vz += -cam.fx * rz3 * vJ02 * tx;
    if (y_in) vy += -cam.fy * rz2 * vJ12; else vz += -cam.fy * rz3 * vJ12 * ty;
    vz += -cam.fx * rz2 * vJ00 - cam.fy * rz2 * vJ11 + 2.f * cam.fx * tx * rz3 * vJ02 +
          2.f * cam.fy * ty * rz3 * vJ12;
  } else if constexpr (CAM == MGS_CAMERA_ORTHO) {
    // J is constant: the mean alone depends on the camera point
    vx = cam.fx * v_mean2d[0];
    vy = cam.fy * v_mean2d[1];
    vz = v_depth;
  } else if constexpr (CAM == MGS_CAMERA_PINHOLE_BC) {
    // Everything is a function of (a, b, rz) = (x/z, y/z, 1/z): with D = Jd,
    //   J[r][0] = f_r D[r][0] rz,  J[r][1] = f_r D[r][1] rz,  J[r][2] = -f_r rz (D[r][0] a + D[r][1] b)
    // so rz dJ/drz = J, and the cotangents of D's three entries and the direct ones of a, b follow from w = f_r vJ.
    //   dd00/da = 6 a R1 + 4 a^3 R2 + 6 p2           dd00/db = dd01/da = Ta = 2 b R1 + 4 a^2 b R2 + 2 p1
    //   dd11/db = 6 b R1 + 4 b^3 R2 + 6 p1           dd01/db = dd11/da = Tb = 2 a R1 + 4 a b^2 R2 + 2 p2
    float vJ[6];
    for (int r = 0; r < 2; ++r)
      for (int c = 0; c < 3; ++c)
        vJ[r * 3 + c] = GsJ[r * 3] * covc[c] + GsJ[r * 3 + 1] * covc[3 + c] + GsJ[r * 3 + 2] * covc[6 + c];
    const float a = xr, b = yr, p1 = cam.k[2], p2 = cam.k[3];
    const float w00 = cam.fx * vJ[0], w01 = cam.fx * vJ[1], w02 = cam.fx * vJ[2];
    const float w10 = cam.fy * vJ[3], w11 = cam.fy * vJ[4], w12 = cam.fy * vJ[5];
    const float gd00 = rz * (w00 - a * w02);
    const float gd01 = rz * ((w01 - b * w02) + (w10 - a * w12));
    const float gd11 = rz * (w11 - b * w12);
    const float Ta = 2.f * b * bc.R1 + 4.f * a * a * b * bc.R2 + 2.f * p1;
    const float Tb = 2.f * a * bc.R1 + 4.f * a * b * b * bc.R2 + 2.f * p2;
    const float Haaa = 6.f * a * bc.R1 + 4.f * a * a * a * bc.R2 + 6.f * p2;
    const float Hbbb = 6.f * b * bc.R1 + 4.f * b * b * b * bc.R2 + 6.f * p1;
    const float vxd = cam.fx * v_mean2d[0], vyd = cam.fy * v_mean2d[1];
    const float va_ = bc.d00 * vxd + bc.d01 * vyd + gd00 * Haaa + gd01 * Ta + gd11 * Tb -
                      rz * (w02 * bc.d00 + w12 * bc.d01);
    const float vb_ = bc.d01 * vxd + bc.d11 * vyd + gd00 * Ta + gd01 * Tb + gd11 * Hbbb -
                      rz * (w02 * bc.d01 + w12 * bc.d11);
    const float vJJ = vJ[0] * j00 + vJ[1] * j01 + vJ[2] * j02 + vJ[3] * j10 + vJ[4] * j11 + vJ[5] * j12;
    vx = rz * va_;
    vy = rz * vb_;
    vz = -rz * (a * va_ + b * vb_ + vJJ) + v_depth;
  } else if constexpr (CAM == MGS_CAMERA_FISHEYE_KB) {
    // as the equidistant branch below, with S, A, D for s, a, 1.  With c = 2 s z / r2 (du/dx = c x, du/dy = c y) and
    // uz = du/dz = -2 s q / r2:
    //   dA/dx = x B, dA/dy = y B,  B = 2 b P + a P' c + (2 z / r2) (2 s a P' + s^2 P'' c - 2 s^2 P' / r2)
    //   dA/dz = Az = 2 P / r2^2 + a P' uz + (2 s^2 / r2) (P' (1 - 2 z^2 / r2) + z P'' uz) - 4 s z P' / r2^2
    //   dD/du = Du = 3 P' + 2 u P''
    vx = j00 * v_mean2d[0] + j10 * v_mean2d[1];
    vy = j01 * v_mean2d[0] + j11 * v_mean2d[1];
    vz = j02 * v_mean2d[0] + j12 * v_mean2d[1] + v_depth;
    float vJ[6];
    for (int r = 0; r < 2; ++r)
      for (int c = 0; c < 3; ++c)
        vJ[r * 3 + c] = GsJ[r * 3] * covc[c] + GsJ[r * 3 + 1] * covc[3 + c] + GsJ[r * 3 + 2] * covc[6 + c];
    const float ir4 = ir2 * ir2, xx = x * x, yy = y * y, xy = x * y, q = xx + yy;
    const float ss = fs * fs, cz = 2.f * fs * z * ir2, uz = -2.f * fs * q * ir2;
    const float B = 2.f * fb * kb.P + fa * kb.P1 * cz +
                    2.f * z * ir2 * (2.f * fs * fa * kb.P1 + ss * kb.P2 * cz - 2.f * ss * kb.P1 * ir2);
    const float Az = 2.f * ir4 * kb.P + fa * kb.P1 * uz +
                     2.f * ss * ir2 * (kb.P1 * (1.f - 2.f * z * z * ir2) + z * kb.P2 * uz) - 4.f * fs * z * kb.P1 * ir4;
    const float Du = 3.f * kb.P1 + 2.f * kb.u * kb.P2;
    const float A = kb.A, dr = kb.D * ir2;
    const float E = 2.f * kb.D * ir4 - Du * cz * ir2;              // d(D / r2): -(x, y) E in x, y
    const float Fz = 2.f * z * kb.D * ir4 - Du * uz * ir2;         //            -Fz in z
    const float wx = cam.fx * vJ[0], w01 = cam.fx * vJ[1], w02 = cam.fx * vJ[2];
    const float w10 = cam.fy * vJ[3], wy = cam.fy * vJ[4], w12 = cam.fy * vJ[5];
    const float wxy = w01 + w10;
    // J00 = fx (S + x^2 A),  J11 = fy (S + y^2 A)
    vx += wx * x * (3.f * A + xx * B) + wy * x * (A + yy * B);
    vy += wx * y * (A + xx * B) + wy * y * (3.f * A + yy * B);
    vz += wx * (xx * Az - dr) + wy * (yy * Az - dr);
    // J01 = fx x y A,  J10 = fy x y A
    vx += wxy * y * (A + xx * B);
    vy += wxy * x * (A + yy * B);
    vz += wxy * xy * Az;
    // J02 = -fx x D / r2,  J12 = -fy y D / r2
    vx += w02 * (xx * E - dr) + w12 * xy * E;
    vy += w02 * xy * E + w12 * (yy * E - dr);
    vz += (w02 * x + w12 * y) * Fz;
  } else {
    // J is the Jacobian of the mean map: the mean's share is J^T v_mean2d
    vx = j00 * v_mean2d[0] + j10 * v_mean2d[1];
    vy = j01 * v_mean2d[0] + j11 * v_mean2d[1];
    vz = j02 * v_mean2d[0] + j12 * v_mean2d[1] + v_depth;
    float vJ[6];          // all six entries of J depend on the camera point
    for (int r = 0; r < 2; ++r)
      for (int c = 0; c < 3; ++c)
        vJ[r * 3 + c] = GsJ[r * 3] * covc[c] + GsJ[r * 3 + 1] * covc[3 + c] + GsJ[r * 3 + 2] * covc[6 + c];
    // closed-form dJ/d(x, y, z) from ds = (a x, a y, -1/r2), da = (2 x b, 2 y b, 2/r2^2), d(1/r2) = -2 (x, y, z)/r2^2
    const float ir4 = ir2 * ir2, xx = x * x, yy = y * y, xy = x * y;
    const float wx = cam.fx * vJ[0], w01 = cam.fx * vJ[1], w02 = cam.fx * vJ[2];
    const float w10 = cam.fy * vJ[3], wy = cam.fy * vJ[4], w12 = cam.fy * vJ[5];
    const float wxy = w01 + w10;      // J01 and J10 share x y a
    // J00 = fx (s + x^2 a),  J11 = fy (s + y^2 a)
    vx += wx * x * (3.f * fa + 2.f * xx * fb) + wy * x * (fa + 2.f * yy * fb);
    vy += wx * y * (fa + 2.f * xx * fb) + wy * y * (3.f * fa + 2.f * yy * fb);
    vz += wx * (2.f * xx * ir4 - ir2) + wy * (2.f * yy * ir4 - ir2);
    // J01 = fx x y a,  J10 = fy x y a
    vx += wxy * y * (fa + 2.f * xx * fb);
    vy += wxy * x * (fa + 2.f * yy * fb);
    vz += wxy * 2.f * xy * ir4;
    // J02 = -fx x / r2,  J12 = -fy y / r2
    vx += w02 * (2.f * xx * ir4 - ir2) + w12 * 2.f * xy * ir4;
    vy += w02 * 2.f * xy * ir4 + w12 * (2.f * yy * ir4 - ir2);
    vz += (w02 * x + w12 * y) * 2.f * z * ir4;
  }
  // world mean, view matrix
  g.v_mean[0] = R[0] * vx + R[3] * vy + R[6] * vz;
  g.v_mean[1] = R[1] * vx + R[4] * vy + R[7] * vz;
  g.v_mean[2] = R[2] * vx + R[5] * vy + R[8] * vz;
  g.v_t[0] = vx; g.v_t[1] = vy; g.v_t[2] = vz;
  float vcs[9];   // symmetrised v_covc
  for (int r = 0; r < 3; ++r)
    for (int c = 0; c < 3; ++c) vcs[r * 3 + c] = v_covc[r * 3 + c] + v_covc[c * 3 + r];
  // covc = R cov R^T : v_R = (v_covc + v_covc^T) R cov ; v_cov = R^T v_covc R
  float Rcov[9];
  mat3_mul(R, cov, Rcov);
  mat3_mul(vcs, Rcov, g.v_R);
  g.v_R[0] += vx * mean[0]; g.v_R[1] += vx * mean[1]; g.v_R[2] += vx * mean[2];
  g.v_R[3] += vy * mean[0]; g.v_R[4] += vy * mean[1]; g.v_R[5] += vy * mean[2];
  g.v_R[6] += vz * mean[0]; g.v_R[7] += vz * mean[1]; g.v_R[8] += vz * mean[2];
  float t2[9], v_cov[9];
  mat3_mul_at(R, v_covc, t2);
  mat3_mul(t2, R, v_cov);
  // cov = M M^T : v_M = (v_cov + v_cov^T) M ; M = Rq diag(s)
  float vs[9], v_M[9];
  for (int r = 0; r < 3; ++r)
    for (int c = 0; c < 3; ++c) vs[r * 3 + c] = v_cov[r * 3 + c] + v_cov[c * 3 + r];
  mat3_mul(vs, M, v_M);
  float v_Rq[9];
  for (int j = 0; j < 3; ++j) {
    g.v_scale[j] = Rq[0 * 3 + j] * v_M[0 * 3 + j] + Rq[1 * 3 + j] * v_M[1 * 3 + j] +
                   Rq[2 * 3 + j] * v_M[2 * 3 + j];
    for (int i = 0; i < 3; ++i) v_Rq[i * 3 + j] = v_M[i * 3 + j] * scale[j];
  }
  quat_to_rotmat_vjp(quat, v_Rq, g.v_quat);
  return g;
}

// VJP of colour = sum_k Y_k(normalize(dir)) coeff_k.  Writes v_coeff[KC*3] and v_dir[3].
template <int DEG>
MGS_HD void sh_vjp(const float dir[3], const float* coeff, const float v_rgb[3], float* v_coeff,
                   float v_dir[3]) {
  constexpr int KC = (DEG + 1) * (DEG + 1);
  float n2 = dir[0] * dir[0] + dir[1] * dir[1] + dir[2] * dir[2];
  float inv = n2 > 0.f ? 1.0f / sqrtf(n2) : 0.f;
  float x = dir[0] * inv, y = dir[1] * inv, z = dir[2] * inv;
  float Y[KC], Yx[KC], Yy[KC], Yz[KC];
  sh_basis(DEG, x, y, z, Y);
  sh_basis_grad(DEG, x, y, z, Yx, Yy, Yz);
  float vx = 0.f, vy = 0.f, vz = 0.f;
  for (int k = 0; k < KC; ++k) {
    v_coeff[3 * k + 0] = Y[k] * v_rgb[0];
    v_coeff[3 * k + 1] = Y[k] * v_rgb[1];
    v_coeff[3 * k + 2] = Y[k] * v_rgb[2];
    float s = coeff[3 * k + 0] * v_rgb[0] + coeff[3 * k + 1] * v_rgb[1] + coeff[3 * k + 2] * v_rgb[2];
    vx += Yx[k] * s; vy += Yy[k] * s; vz += Yz[k] * s;
  }
  float d = vx * x + vy * y + vz * z;
  v_dir[0] = (vx - d * x) * inv;
  v_dir[1] = (vy - d * y) * inv;
  v_dir[2] = (vz - d * z) * inv;
}

}  // namespace mgs
#endif  // MGS_MATH_H_
