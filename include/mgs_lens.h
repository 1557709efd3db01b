/* mgs_lens.h -- the lens-distortion part of libmgs.so's C ABI: the flag bits that select MGS_CAMERA_FISHEYE_KB
 * (include/mgs.h, at MGS_CAMERA_*: the equidistant fisheye with OpenCV's k1..k4 polynomial) where a call takes its camera
 * model as a flag rather than as a camera_model argument.  Compiled into the same libmgs.so / libmgs_debug.so and bound by
 * the conventions at the top of mgs.h.  MGS_VERSION is mgs.h's: this header adds two bits and no entry point, and changes
 * no parameter list.
 *
 * Under either bit the call's `K` / `Ks` pointer addresses MGS_LENS_ROW_FLOATS floats per camera (camera c at
 * Ks + 16 c): K row-major in 0..8, k1..k4 in 9..12, u_max = theta_max^2 in 13, zero in 14..15 (mgs.h says what
 * theta_max is).  The rules of the other camera bits hold: at most one MGS_BIN_CAMERA_* / MGS_FRAMES_CAMERA_* bit per
 * word (MGS_ERR_INVALID_ARGUMENT otherwise), the backward must be given the forward's bit, and dataset output
 * (ds_rgba / ds_distance) stays pinhole-only (MGS_ERR_UNSUPPORTED).  mgs_projection_fwd / _bwd and mgs_project_color_bwd
 * take the model as camera_model = MGS_CAMERA_FISHEYE_KB (the latter optionally | MGS_PARAMS_RAW). */
#ifndef MGS_LENS_H_
#define MGS_LENS_H_

#include "mgs.h"

#define MGS_LENS_ROW_FLOATS 16
#define MGS_LENS_ROW_K1 9     /* k1..k4 at 9..12 */
#define MGS_LENS_ROW_UMAX 13

/* mgs_project_color_fwd bin_flags: MGS_CAMERA_FISHEYE_KB instead of MGS_CAMERA_PINHOLE */
#define MGS_BIN_CAMERA_FISHEYE_KB 256
/* mgs_render_frames / _labeled / _train / _backward flags: project with MGS_CAMERA_FISHEYE_KB */
#define MGS_FRAMES_CAMERA_FISHEYE_KB 256

#endif /* MGS_LENS_H_ */
