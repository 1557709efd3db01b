// Host build (g++) of the pinhole-lens instantiation of robosimgs_amd/csrc/mgs_math.h
// (project_gaussian<MGS_CAMERA_PINHOLE_BC>, project_gaussian_vjp<MGS_CAMERA_PINHOLE_BC>), so the lens math can be checked
// against the fp64 reference (tests/pinhole_lens_ref.py) without a GPU.  Test-only: never linked into libmgs.so.  `row` is
// the camera's 16-float row of include/mgs_lens_pinhole.h: K | k1 k2 p1 p2 k3 | u_max | 0.
// With -DPINHOLE_LENS_MAIN the file is a stand-alone program for a host -fsanitize=address,undefined build: it runs both
// functions over points on the optical axis, across the frame, at the clamp box's border, up to and past the radial fold
// and behind the camera, and fails on a non-finite output or a wrong cull.
#include "../../robosimgs_amd/csrc/mgs_math.h"

#include <float.h>
#include <stdio.h>
#include <stdlib.h>

using namespace mgs;

extern "C" int hh_pinhole_lens_project(int n, const float* means, const float* quats, const float* scales,
                                       const float* viewmat, const float* row, int W, int H, float eps2d, float near_plane,
                                       float far_plane, float radius_clip, int radius_rule, const float* opacities,
                                       int antialiased, int* radii, int* radii_y, float* means2d, float* depths,
                                       float* conics, float* comps) {
  CameraParams cam = load_camera<MGS_CAMERA_PINHOLE_BC>(viewmat, row);
  for (int g = 0; g < n; ++g) {
    Projected p = project_gaussian<MGS_CAMERA_PINHOLE_BC>(means + 3 * g, quats + 4 * g, scales + 3 * g, cam, (float)W, (float)H,
                                                          eps2d, near_plane, far_plane, radius_clip, radius_rule,
                                                          opacities != nullptr, opacities ? opacities[g] : 1.f,
                                                          antialiased != 0);
    radii[g] = p.radius;
    radii_y[g] = p.radius_y;
    means2d[2 * g] = p.mean2d[0]; means2d[2 * g + 1] = p.mean2d[1];
    depths[g] = p.depth;
    for (int k = 0; k < 3; ++k) conics[3 * g + k] = p.conic[k];
    comps[g] = p.compensation;
  }
  return 0;
}

// per-Gaussian gradients (v_R / v_t per Gaussian too: [n,9] / [n,3], so single rows can be compared)
extern "C" int hh_pinhole_lens_vjp(int n, const float* means, const float* quats, const float* scales, const float* viewmat,
                                   const float* row, int W, int H, float eps2d, const int* radii, const float* conics,
                                   const float* comps, const float* v_means2d, const float* v_depths, const float* v_conics,
                                   const float* v_comps, float* v_means, float* v_quats, float* v_scales, float* v_R,
                                   float* v_t) {
  CameraParams cam = load_camera<MGS_CAMERA_PINHOLE_BC>(viewmat, row);
  for (int g = 0; g < n; ++g) {
    ProjectedGrad r{};
    if (radii[g] > 0)
      r = project_gaussian_vjp<MGS_CAMERA_PINHOLE_BC>(means + 3 * g, quats + 4 * g, scales + 3 * g, cam, (float)W, (float)H,
                                                      eps2d, conics + 3 * g, comps[g], v_means2d + 2 * g, v_depths[g],
                                                      v_conics + 3 * g, v_comps ? v_comps[g] : 0.f);
    for (int k = 0; k < 3; ++k) { v_means[3 * g + k] = r.v_mean[k]; v_scales[3 * g + k] = r.v_scale[k]; v_t[3 * g + k] = r.v_t[k]; }
    for (int k = 0; k < 4; ++k) v_quats[4 * g + k] = r.v_quat[k];
    for (int k = 0; k < 9; ++k) v_R[9 * g + k] = r.v_R[k];
  }
  return 0;
}

#ifdef PINHOLE_LENS_MAIN
int main() {
  const int W = 112, H = 80;
  // k1 k2 p1 p2 k3 u_max f: a mild lens without a fold in reach, and one whose radial fold (u = 1 / 1.05) is in the frame
  const float lenses[2][7] = {{-0.12f, 0.03f, 0.002f, -0.0015f, -0.004f, 4.2989f, 90.f},
                              {-0.35f, 0.f, 0.003f, -0.002f, 0.f, 0.95238f, 50.f}};
  const float viewmat[16] = {1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1};
  // |(x', y')| of the points: the axis, across the frame, around the second lens's fold (0.9759), far outside
  const float radii_n[] = {0.f, 1e-6f, 1e-3f, 0.2f, 0.5f, 0.8f, 0.95f, 0.975f, 0.977f, 1.2f, 30.f};
  const int NT = sizeof(radii_n) / sizeof(radii_n[0]), N = NT * 3 + 1;
  float* means = (float*)malloc(sizeof(float) * 3 * N);
  float* quats = (float*)malloc(sizeof(float) * 4 * N);
  float* scales = (float*)malloc(sizeof(float) * 3 * N);
  for (int i = 0; i < N; ++i) {
    const float z = i < NT ? 0.5f : (i < 2 * NT ? 2.f : 7.f), t = radii_n[i % NT], phi = 0.7f * i;
    means[3 * i] = z * t * cosf(phi); means[3 * i + 1] = z * t * sinf(phi); means[3 * i + 2] = z;
    quats[4 * i] = 0.9f; quats[4 * i + 1] = 0.1f * i; quats[4 * i + 2] = -0.3f; quats[4 * i + 3] = 0.2f;
    scales[3 * i] = 0.02f + 0.001f * i; scales[3 * i + 1] = 0.05f; scales[3 * i + 2] = 0.03f;
  }
  means[3 * (N - 1) + 2] = -1.f;      // behind the camera
  int* radii = (int*)malloc(sizeof(int) * N);
  int* radii_y = (int*)malloc(sizeof(int) * N);
  float* m2d = (float*)malloc(sizeof(float) * 2 * N);
  float* dep = (float*)malloc(sizeof(float) * N);
  float* con = (float*)malloc(sizeof(float) * 3 * N);
  float* comp = (float*)malloc(sizeof(float) * N);
  float* cot = (float*)malloc(sizeof(float) * 3 * N);
  float* out = (float*)malloc(sizeof(float) * 22 * N);
  for (int i = 0; i < 3 * N; ++i) cot[i] = 0.25f * (float)((i * 7) % 11) - 1.f;
  int bad = 0, visible = 0;
  for (int l = 0; l < 2; ++l) {
    const float f = lenses[l][6];
    float row[16] = {f, 0, 57.5f, 0, f, 39.f, 0, 0, 1, lenses[l][0], lenses[l][1], lenses[l][2], lenses[l][3], lenses[l][4],
                     lenses[l][5], 0};
    for (int rule = 0; rule < 2; ++rule) {
      hh_pinhole_lens_project(N, means, quats, scales, viewmat, row, W, H, 0.3f, 0.01f, 1e10f, 0.f, rule, nullptr, rule, radii,
                              radii_y, m2d, dep, con, comp);
      hh_pinhole_lens_vjp(N, means, quats, scales, viewmat, row, W, H, 0.3f, radii, con, comp, cot, cot, cot, cot, out,
                          out + 3 * N, out + 7 * N, out + 10 * N, out + 19 * N);
      for (int i = 0; i < N; ++i) visible += radii[i] > 0;
      for (int i = 0; i < 2 * N; ++i) bad += !isfinite(m2d[i]);
      for (int i = 0; i < 3 * N; ++i) bad += !isfinite(con[i]);
      for (int i = 0; i < 22 * N; ++i) bad += !isfinite(out[i]);
      if (radii[N - 1] != 0) ++bad;                                 // the point behind the camera
      if (radii[0] == 0 || radii[3] == 0) ++bad;                    // the axis and 0.2 are inside under both lenses
      if (radii[9] != 0 || radii[10] != 0) ++bad;                   // 1.2 and 30: past the box (first lens) / the fold (second)
      if (l == 1 && (radii[8] != 0 || radii[6] == 0)) ++bad;        // 0.977 lies past the radial fold, 0.95 inside
    }
  }
  free(means); free(quats); free(scales); free(radii); free(radii_y); free(m2d); free(dep); free(con); free(comp); free(cot); free(out);
  printf("pinhole lens harness: %d visible, %d bad\n", visible, bad);
  return bad ? 1 : 0;
}
#endif
