// Host build (g++) of the per-Gaussian arithmetic of project_color_fwd_kernel (robosimgs_amd/csrc/projection.hip), chained
// as the kernel chains it: the raw activations, project_gaussian<CAM> under either radius rule, the view direction from
// camera_position, sh_dot<DEG> and the + 0.5 clamp, all from robosimgs_amd/csrc/mgs_math.h.  Test-only: never linked into
// libmgs.so.  What is NOT here is the kernel's own logic -- the `active` mask's wave ballot, the SH rows' way through LDS, the
// nullable outputs, the records: tests/test_gpu_project_color_fwd.py holds those on the GPU.
// camera_model: MGS_CAMERA_* (3: `K` is the camera's 16-float row); params: bit 0 raw, bit 1 anti-aliased.
#include "../../robosimgs_amd/csrc/mgs_math.h"

using namespace mgs;

namespace {

template <int CAM, int DEG>
void run(int n, const float* means, const float* quats, const float* scales, const float* opacities, int stride,
         const float* coeffs, const float* viewmat, const float* K, int W, int H, float eps2d, float near_plane,
         float far_plane, float radius_clip, int rule, bool raw, bool aa, int* radii, int* radii_y, float* means2d,
         float* depths, float* conics, float* comps, float* opac_out, float* pre, float* feats) {
  CameraParams cam = load_camera<CAM>(viewmat, K);
  for (int g = 0; g < n; ++g) {
    float m[3] = {means[3 * g], means[3 * g + 1], means[3 * g + 2]};
    float s[3] = {scales[3 * g], scales[3 * g + 1], scales[3 * g + 2]};
    float o = opacities ? opacities[g] : 1.f;
    if (raw) {
      s[0] = activate_scale(s[0]); s[1] = activate_scale(s[1]); s[2] = activate_scale(s[2]);
      o = activate_opacity(o);
    }
    Projected p;
    if (rule == MGS_RADIUS_CLASSIC)
      p = project_gaussian<CAM>(m, quats + 4 * g, s, cam, (float)W, (float)H, eps2d, near_plane, far_plane, radius_clip);
    else
      p = project_gaussian<CAM>(m, quats + 4 * g, s, cam, (float)W, (float)H, eps2d, near_plane, far_plane, radius_clip, rule,
                                opacities != nullptr, o, aa);
    radii[g] = p.radius;
    radii_y[g] = p.radius_y;
    means2d[2 * g] = p.mean2d[0]; means2d[2 * g + 1] = p.mean2d[1];
    depths[g] = p.depth;
    for (int k = 0; k < 3; ++k) conics[3 * g + k] = p.conic[k];
    comps[g] = p.compensation;
    opac_out[g] = aa ? o * p.compensation : o;
    float rgb[3] = {0.f, 0.f, 0.f}, raw_rgb[3] = {0.f, 0.f, 0.f};
    if (p.radius > 0) {
      float campos[3], d[3];
      camera_position(cam, campos);
      d[0] = m[0] - campos[0]; d[1] = m[1] - campos[1]; d[2] = m[2] - campos[2];
      sh_dot<DEG>(d, coeffs + (size_t)g * stride * 3, raw_rgb);
      for (int k = 0; k < 3; ++k) {
        raw_rgb[k] += 0.5f;
        rgb[k] = fmaxf(raw_rgb[k], 0.f);
      }
    }
    for (int k = 0; k < 3; ++k) { pre[3 * g + k] = raw_rgb[k]; feats[4 * g + k] = rgb[k]; }
    feats[4 * g + 3] = p.depth;
  }
}

template <int CAM, typename... A>
int by_degree(int deg, A... a) {
  switch (deg) {
    case 0: run<CAM, 0>(a...); return 0;
    case 1: run<CAM, 1>(a...); return 0;
    case 2: run<CAM, 2>(a...); return 0;
    case 3: run<CAM, 3>(a...); return 0;
  }
  return -1;
}

}  // namespace

// pre [n,3]: the colour before the clamp (zeros on culled rows); feats [n,4]: clamped colour and depth
extern "C" int hh_project_color_fwd(int camera_model, int deg, int n, const float* means, const float* quats,
                                    const float* scales, const float* opacities, int stride, const float* coeffs,
                                    const float* viewmat, const float* K, int W, int H, float eps2d, float near_plane,
                                    float far_plane, float radius_clip, int rule, int params, int* radii, int* radii_y,
                                    float* means2d, float* depths, float* conics, float* comps, float* opac_out, float* pre,
                                    float* feats) {
  const bool raw = params & 1, aa = params & 2;
  switch (camera_model) {
    case MGS_CAMERA_PINHOLE:
      return by_degree<MGS_CAMERA_PINHOLE>(deg, n, means, quats, scales, opacities, stride, coeffs, viewmat, K, W, H, eps2d,
                                           near_plane, far_plane, radius_clip, rule, raw, aa, radii, radii_y, means2d, depths,
                                           conics, comps, opac_out, pre, feats);
    case MGS_CAMERA_ORTHO:
      return by_degree<MGS_CAMERA_ORTHO>(deg, n, means, quats, scales, opacities, stride, coeffs, viewmat, K, W, H, eps2d,
                                         near_plane, far_plane, radius_clip, rule, raw, aa, radii, radii_y, means2d, depths, conics,
                                         comps, opac_out, pre, feats);
    case MGS_CAMERA_FISHEYE:
      return by_degree<MGS_CAMERA_FISHEYE>(deg, n, means, quats, scales, opacities, stride, coeffs, viewmat, K, W, H, eps2d,
                                           near_plane, far_plane, radius_clip, rule, raw, aa, radii, radii_y, means2d, depths,
                                           conics, comps, opac_out, pre, feats);
    case MGS_CAMERA_FISHEYE_KB:
      return by_degree<MGS_CAMERA_FISHEYE_KB>(deg, n, means, quats, scales, opacities, stride, coeffs, viewmat, K, W, H, eps2d,
                                              near_plane, far_plane, radius_clip, rule, raw, aa, radii, radii_y, means2d,
                                              depths, conics, comps, opac_out, pre, feats);
  }
  return -1;
}
