/* mgs_tsdf.h -- C ABI of fusing depth frames into a truncated signed distance (TSDF) volume and extracting its isosurface
 * as a triangle mesh (csrc/tsdf.hip, csrc/tsdf_tets.h).  Compiled into the same libmgs.so / libmgs_debug.so as include/mgs.h's
 * render path and bound by the same conventions (see the top of mgs.h): device pointers unless marked "host", the caller owns
 * every buffer, all work is enqueued on `stream`, nothing synchronises or reads a value back, and the return value is 0, <0
 * MGS_ERR_* or >0 a hipError_t from a launch.  The version is mgs.h's: this header adds entry points and changes no parameter
 * list.
 *
 * The volume.  nx x ny x nz samples, x fastest; sample (i, j, k) sits at origin + (i + 0.5, j + 0.5, k + 0.5) voxel_size in
 * world coordinates.  tsdf and weight are fp32 [nz,ny,nx]; color (nullable) is planar fp32 [3,nz,ny,nx].  An empty volume is
 * all zeros.  At most 2^31 - 1 samples.
 *
 * Integration, per sample p and camera c in the call's camera order:
 *     q = R_c p + t_c, skipped if q.z <= near;  u = fx q.x / q.z + cx, v alike; the pixel is (floor u, floor v), skipped
 *     outside the frame;  d the z-depth there, skipped if not finite, if d <= 0 or, where alphas are given, if alpha <
 *     alpha_min (a select: what a skipped pixel holds, NaN included, changes nothing);  s = d - q.z, skipped if s < -trunc;
 *     t = min(1, s / trunc);  tsdf <- (tsdf w + t) / (w + 1), each colour plane alike with the pixel's colour;
 *     w <- min(w + 1, max_weight).
 * One launch for all cameras: the volume is read and written once per call.  No atomics; a sample's updates are applied in
 * camera order, so C views in one call give the bytes of any chunking of them into several calls.
 *
 * Extraction: marching tetrahedra on the Kuhn split of every cell (csrc/tsdf_tets.h states the split, the cases and the
 * winding).  A cell is emitted iff its eight weights are >= min_weight; a corner is inside iff tsdf < level.  One vertex per
 * crossed tetrahedron edge of an emitted cell, ordered by the edge's lower grid point (x fastest), then edge type 0..6; faces
 * by cell (x fastest), then tetrahedron 0..5; the normal (B - A) x (C - A) points towards increasing tsdf.  A value exactly on
 * `level` gives zero-area triangles, which are kept.  The output is a function of the volume alone. */
#ifndef MGS_TSDF_H_
#define MGS_TSDF_H_

#include "mgs.h"

#ifdef __cplusplus
extern "C" {
#endif

typedef struct mgs_tsdf_volume {
  int nx, ny, nz;
  float origin[3];
  float voxel_size;
  float trunc;          /* truncation distance, world units (integration only) */
  float max_weight;     /* the weight's cap, >= 1 (integration only) */
  float *tsdf;          /* [nz,ny,nx] */
  float *weight;        /* [nz,ny,nx] */
  float *color;         /* nullable [3,nz,ny,nx] */
} mgs_tsdf_volume;

/* mgs_tsdf_extract_emit's status word */
#define MGS_TSDF_STATUS_OVERFLOW 1u

/* Fuses n_cams frames of height x width into the volume.  frame_channels 4: frames is the renderer's [C,H,W,4] RGB+ED frame
 * (colour in channels 0..2, expected z-depth in channel 3), read in place; frame_channels 1: frames is a [C,H,W] depth image
 * and the colour planes, if any, are left as they are.  alphas: nullable [C,H,W].  viewmats [C,4,4] world-to-camera, Ks
 * [C,3,3]; camera_model must be MGS_CAMERA_PINHOLE.
 * MGS_ERR_INVALID_ARGUMENT, before any launch: vol, frames, viewmats, Ks, vol->tsdf or vol->weight NULL; a dimension < 1 or
 * more than 2^31 - 1 samples; voxel_size or trunc not finite or <= 0; max_weight not >= 1; n_cams < 1; height or width < 1;
 * frame_channels other than 1 or 4; any other camera_model.  One launch. */
int mgs_tsdf_integrate(const mgs_tsdf_volume *vol, int n_cams, int height, int width, const float *frames,
                       int frame_channels, const float *alphas /* nullable */, float alpha_min, float near_plane,
                       const float *viewmats, const float *Ks, int camera_model, mgs_stream_t stream);

/* Passes (a) to (c) of the extraction: a byte per emitted cell, per grid point the owned edges that carry a vertex and per
 * cell its triangles, and exclusive scans of both counts.  counts [2] uint64 receives the number of vertices and of faces
 * and stays on the device.  workspace NULL: only *workspace_bytes is written (host), nothing is launched; otherwise
 * *workspace_bytes is the size given, the workspace is 256-byte aligned, and it must reach mgs_tsdf_extract_emit as this call
 * left it, with the same volume, level and min_weight.
 * MGS_ERR_INVALID_ARGUMENT, before any launch: the volume's refusals above (trunc and max_weight are not read); level or
 * min_weight not finite; counts or workspace_bytes NULL; MGS_ERR_WORKSPACE_TOO_SMALL for a workspace that is.  Three
 * launches. */
int mgs_tsdf_extract_count(const mgs_tsdf_volume *vol, float level, float min_weight, uint64_t *counts, void *workspace,
                           size_t *workspace_bytes /* host, in/out */, mgs_stream_t stream);

/* Pass (d): writes vertices [*,3] fp32, colors [*,3] fp32 (nullable; needs vol->color) and faces [*,3] int32 in the order
 * stated above.  Nothing is ever written at or past a capacity: vertex v is written iff v < vertex_capacity, face f iff f <
 * face_capacity, and where a count exceeds its capacity *status becomes MGS_TSDF_STATUS_OVERFLOW (0 otherwise; written by
 * every call).  Capacities are rows, at most 2^31 - 1.
 * MGS_ERR_INVALID_ARGUMENT, before any launch: as mgs_tsdf_extract_count; vertices, faces, status or workspace NULL; colors
 * without vol->color; a negative capacity or one above 2^31 - 1.  One launch. */
int mgs_tsdf_extract_emit(const mgs_tsdf_volume *vol, float level, float min_weight, const uint64_t *counts,
                          const void *workspace, size_t workspace_bytes, float *vertices, float *colors /* nullable */,
                          int64_t vertex_capacity, int32_t *faces, int64_t face_capacity, uint32_t *status,
                          mgs_stream_t stream);

#ifdef __cplusplus
}
#endif
#endif /* MGS_TSDF_H_ */
