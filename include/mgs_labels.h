/* mgs_labels.h -- C ABI of the part-label output of libmgs.so: which class of Gaussians every pixel of a frame shows.
 * Compiled into the same libmgs.so / libmgs_debug.so as include/mgs.h's render path and bound by the same conventions
 * (see the top of mgs.h): device pointers unless marked "host", the caller owns every buffer, all work is enqueued on
 * `stream`, nothing synchronises or reads a count back, every call is capturable in a hipGraph, and the return value is
 * 0, <0 MGS_ERR_* or >0 a hipError_t from a launch.  MGS_VERSION is mgs.h's: this header adds entry points and changes no
 * parameter list.
 *
 * A label frame.  class_ids[n] int32 gives every Gaussian one class, n_classes = K with 1 <= K <= MGS_LABELS_MAX_CLASSES.
 * For pixel p and class k
 *     W_k(p) = sum over the Gaussians i of p's tile list with class_ids[i] == k of w_i(p),
 * where w_i(p) is exactly the weight the frame itself blends Gaussian i with at p (mgs_rasterize_fwd on the same lists,
 * SURVEY.md A.2 step 9): alpha = min(0.999, opacity exp(-sigma)), counted iff sigma >= 0 and alpha >= 1/255;
 * w = alpha T; the Gaussian at which T (1 - alpha) <= 1e-4 closes the pixel and neither it nor anything behind it is
 * counted.  `opacity` is what the frame's raster reads (the packed record's, anti-aliased where the frame is).
 *   labels[p]        = the k with the largest W_k(p), ties to the lowest k; MGS_LABEL_NONE where no counted Gaussian has
 *                      a class in 0..K-1
 *   label_weights[p] = max_k W_k(p), 0 where the label is MGS_LABEL_NONE (nullable)
 * A Gaussian whose class lies outside 0..K-1 (-1, say) occludes as usual and is reported for no class.
 * Labels are not differentiable: there is no backward. */
#ifndef MGS_LABELS_H_
#define MGS_LABELS_H_

#include "mgs.h"

#ifdef __cplusplus
extern "C" {
#endif

#define MGS_LABEL_NONE 255
#define MGS_LABELS_MAX_CLASSES 32

/* One camera, on the list arguments of mgs_rasterize_fwd (tile size 16; tile_offsets[tile_w * tile_h + 1], flatten_ids,
 * tile_group_order nullable: a launch order, never a result).  labels[height * width] uint8, label_weights[height * width].
 * MGS_ERR_INVALID_ARGUMENT, before any launch: n_classes outside 1..MGS_LABELS_MAX_CLASSES; class_ids or labels NULL;
 * neither `splats` nor all of means2d / conics / opacities given.  One launch. */
int mgs_raster_labels(int n, const float *means2d, const float *conics, const float *opacities,
                      const float *splats,            /* nullable; when given the three above are not read */
                      const int32_t *class_ids, int n_classes, int width, int height, int tile_w, int tile_h,
                      const int32_t *tile_offsets, const int32_t *flatten_ids,
                      const int32_t *tile_group_order /* nullable */,
                      uint8_t *labels, float *label_weights /* nullable */, mgs_stream_t stream);

/* mgs_render_frames with a label frame per camera: per camera projection, binning, the raster and mgs_raster_labels on
 * that camera's records and lists while they sit in the shared workspace.  Every other parameter, the workspace size and
 * the frames written are mgs_render_frames'; labels[n_cams * height * width], label_weights likewise (nullable).
 * The label arguments are checked as above before any launch. */
int mgs_render_frames_labeled(int n, const float *means, const float *quats, const float *scales, const float *opacities,
                              int sh_degree, int coeff_stride, const float *sh_coeffs, int n_cams, const float *viewmats,
                              const float *Ks, int width, int height, float eps2d, float near_plane, float far_plane,
                              float radius_clip, int antialiased, int channels, int flags, const float *backgrounds,
                              uint32_t isect_capacity, float *render, float *alphas, uint32_t *n_isect, uint32_t *status,
                              uint8_t *ds_rgba, void *ds_distance, int ds_distance_type, const double *ds_Kinv_host,
                              const int32_t *class_ids, int n_classes, uint8_t *labels /* [C,H,W] */,
                              float *label_weights /* [C,H,W], nullable */, void *workspace, size_t *workspace_bytes,
                              mgs_stream_t stream);

#ifdef __cplusplus
}
#endif
#endif /* MGS_LABELS_H_ */
