/* mgs_lens_pinhole.h -- the pinhole-lens part of libmgs.so's C ABI: the fifth camera model, MGS_CAMERA_PINHOLE_BC (the
 * pinhole camera with OpenCV's radial / tangential "Brown-Conrady" distortion, cv2.calibrateCamera's distCoeffs
 * (k1, k2, p1, p2, k3), nerfstudio's camera_model "OPENCV"), and the flag bits that select it where a call takes its camera
 * model as a flag.  Compiled into the same libmgs.so / libmgs_debug.so and bound by the conventions at the top of mgs.h.
 * MGS_VERSION is mgs.h's: this header adds one camera_model value and two bits, no entry point, and changes no parameter
 * list.
 *
 * The model.  Camera point (x, y, z) in OpenCV axes, the near / far cull on z of every model, then
 *   x' = x/z   y' = y/z   u = x'^2 + y'^2
 *   Rad = 1 + k1 u + k2 u^2 + k3 u^3          Rad1 = dRad/du
 *   xd = x' Rad + 2 p1 x' y' + p2 (u + 2 x'^2)
 *   yd = y' Rad + p1 (u + 2 y'^2) + 2 p2 x' y'
 *   mean = (fx xd + cx, fy yd + cy)
 *   Jd = d(xd, yd)/d(x', y') = [[Rad + 2 x'^2 Rad1 + 2 p1 y' + 6 p2 x',   2 x' y' Rad1 + 2 p1 x' + 2 p2 y'],
 *                               [the same off-diagonal,                   Rad + 2 y'^2 Rad1 + 6 p1 y' + 2 p2 x']]
 *   J  = diag(fx, fy) Jd [[1/z, 0, -x/z^2], [0, 1/z, -y/z^2]]     (dense 2 x 3, like the fisheye's)
 * J is not clamped.  Instead a Gaussian is culled (radius 0, every output zero, no gradient) when
 *   1. u >= u_max, where u_max is the smallest positive real root of 1 + 3 k1 u + 5 k2 u^2 + 7 k3 u^3 (there the radial map
 *      r Rad stops growing), FLT_MAX without one.  The caller computes it; the kernels solve nothing;
 *   2. det Jd <= 0: with tangential terms the map folds slightly before the radial fold;
 *   3. (xd, yd) lies outside [-lim_xn, lim_xp] x [-lim_yn, lim_yp], the box MGS_CAMERA_PINHOLE clamps x/z, y/z to (the frame
 *      plus 0.3 of the half field), taken here in DISTORTED normalised coordinates, where the frame lives.  This is the one
 *      difference from MGS_CAMERA_PINHOLE besides the lens: a Gaussian centred outside that box is dropped, where the plain
 *      pinhole keeps it with a clamped J.
 * All five coefficients zero give the pinhole map; callers then select MGS_CAMERA_PINHOLE itself.
 *
 * Under the model every `K` / `Ks` pointer addresses MGS_LENS_ROW_FLOATS floats per camera (camera c at Ks + 16 c):
 * K row-major in 0..8, k1 k2 p1 p2 k3 (OpenCV's distCoeffs order) in 9..13, u_max in 14, zero in 15.  The rules of the other
 * camera bits hold: at most one MGS_BIN_CAMERA_* / MGS_FRAMES_CAMERA_* bit per word (MGS_ERR_INVALID_ARGUMENT otherwise), the
 * backward must be given the forward's bit, and dataset output (ds_rgba / ds_distance) stays plain-pinhole-only
 * (MGS_ERR_UNSUPPORTED).  mgs_projection_fwd / _bwd and mgs_project_color_bwd take the model as camera_model =
 * MGS_CAMERA_PINHOLE_BC (the latter optionally | MGS_PARAMS_RAW).  Those three calls take the value only together with the
 * row: with K == NULL they return MGS_ERR_INVALID_ARGUMENT before anything else, for n == 0 too, where every other model's
 * empty call is MGS_OK.  (4 was not a camera model before this header; an empty call that probes for an unknown model with
 * it is answered as it always was.) */
#ifndef MGS_LENS_PINHOLE_H_
#define MGS_LENS_PINHOLE_H_

#include "mgs.h"
#include "mgs_lens.h"

#define MGS_CAMERA_PINHOLE_BC 4

#define MGS_LENS_PINHOLE_ROW_K1 9     /* k1 k2 p1 p2 k3 at 9..13 */
#define MGS_LENS_PINHOLE_ROW_UMAX 14

/* mgs_project_color_fwd bin_flags: MGS_CAMERA_PINHOLE_BC instead of MGS_CAMERA_PINHOLE */
#define MGS_BIN_CAMERA_PINHOLE_BC 512
/* mgs_render_frames / _labeled / _train / _backward flags: project with MGS_CAMERA_PINHOLE_BC */
#define MGS_FRAMES_CAMERA_PINHOLE_BC 512

#endif /* MGS_LENS_PINHOLE_H_ */
