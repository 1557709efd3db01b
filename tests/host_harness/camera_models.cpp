// Host build (g++) of the camera-model instantiations of robosimgs_amd/csrc/mgs_math.h (project_gaussian<CAM>,
// project_gaussian_vjp<CAM>), so the orthographic and fisheye math can be checked against the fp64 reference without a
// GPU.  Test-only: never linked into libmgs.so.  camera_model: MGS_CAMERA_*; -1 = the default call (no template
// argument), which must be the pinhole instantiation.
#include "../../robosimgs_amd/csrc/mgs_math.h"

using namespace mgs;

template <int CAM>
static Projected project_one(const float* m, const float* q, const float* s, const CameraParams& cam, int W, int H,
                             float eps2d, float near_plane, float far_plane, float radius_clip, int rule,
                             const float* opacity, int antialiased) {
  return project_gaussian<CAM>(m, q, s, cam, (float)W, (float)H, eps2d, near_plane, far_plane, radius_clip, rule,
                               opacity != nullptr, opacity ? *opacity : 1.f, antialiased != 0);
}

extern "C" int hh_project_model(int camera_model, int n, const float* means, const float* quats, const float* scales,
                                const float* viewmat, const float* K, int W, int H, float eps2d, float near_plane,
                                float far_plane, float radius_clip, int radius_rule, const float* opacities,
                                int antialiased, int* radii, int* radii_y, float* means2d, float* depths, float* conics,
                                float* comps) {
  CameraParams cam = load_camera(viewmat, K);
  for (int g = 0; g < n; ++g) {
    const float* op = opacities ? opacities + g : nullptr;
    Projected p;
    switch (camera_model) {
      case -1:
        p = project_gaussian(means + 3 * g, quats + 4 * g, scales + 3 * g, cam, (float)W, (float)H, eps2d, near_plane,
                             far_plane, radius_clip, radius_rule, op != nullptr, op ? *op : 1.f, antialiased != 0);
        break;
      case MGS_CAMERA_PINHOLE:
        p = project_one<MGS_CAMERA_PINHOLE>(means + 3 * g, quats + 4 * g, scales + 3 * g, cam, W, H, eps2d, near_plane,
                                            far_plane, radius_clip, radius_rule, op, antialiased);
        break;
      case MGS_CAMERA_ORTHO:
        p = project_one<MGS_CAMERA_ORTHO>(means + 3 * g, quats + 4 * g, scales + 3 * g, cam, W, H, eps2d, near_plane,
                                          far_plane, radius_clip, radius_rule, op, antialiased);
        break;
      case MGS_CAMERA_FISHEYE:
        p = project_one<MGS_CAMERA_FISHEYE>(means + 3 * g, quats + 4 * g, scales + 3 * g, cam, W, H, eps2d, near_plane,
                                            far_plane, radius_clip, radius_rule, op, antialiased);
        break;
      default:
        return -1;
    }
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
extern "C" int hh_project_vjp_model(int camera_model, int n, const float* means, const float* quats,
                                    const float* scales, const float* viewmat, const float* K, int W, int H, float eps2d,
                                    const int* radii, const float* conics, const float* comps, const float* v_means2d,
                                    const float* v_depths, const float* v_conics, const float* v_comps, float* v_means,
                                    float* v_quats, float* v_scales, float* v_R, float* v_t) {
  CameraParams cam = load_camera(viewmat, K);
  for (int g = 0; g < n; ++g) {
    ProjectedGrad r{};
    if (radii[g] > 0) {
      const float* m = means + 3 * g;
      const float* q = quats + 4 * g;
      const float* s = scales + 3 * g;
      const float vc = v_comps ? v_comps[g] : 0.f;
      switch (camera_model) {
        case -1:
          r = project_gaussian_vjp(m, q, s, cam, (float)W, (float)H, eps2d, conics + 3 * g, comps[g], v_means2d + 2 * g,
                                   v_depths[g], v_conics + 3 * g, vc);
          break;
        case MGS_CAMERA_PINHOLE:
          r = project_gaussian_vjp<MGS_CAMERA_PINHOLE>(m, q, s, cam, (float)W, (float)H, eps2d, conics + 3 * g, comps[g],
                                                       v_means2d + 2 * g, v_depths[g], v_conics + 3 * g, vc);
          break;
        case MGS_CAMERA_ORTHO:
          r = project_gaussian_vjp<MGS_CAMERA_ORTHO>(m, q, s, cam, (float)W, (float)H, eps2d, conics + 3 * g, comps[g],
                                                     v_means2d + 2 * g, v_depths[g], v_conics + 3 * g, vc);
          break;
        case MGS_CAMERA_FISHEYE:
          r = project_gaussian_vjp<MGS_CAMERA_FISHEYE>(m, q, s, cam, (float)W, (float)H, eps2d, conics + 3 * g, comps[g],
                                                       v_means2d + 2 * g, v_depths[g], v_conics + 3 * g, vc);
          break;
        default:
          return -1;
      }
    }
    for (int k = 0; k < 3; ++k) { v_means[3 * g + k] = r.v_mean[k]; v_scales[3 * g + k] = r.v_scale[k]; v_t[3 * g + k] = r.v_t[k]; }
    for (int k = 0; k < 4; ++k) v_quats[4 * g + k] = r.v_quat[k];
    for (int k = 0; k < 9; ++k) v_R[9 * g + k] = r.v_R[k];
  }
  return 0;
}
