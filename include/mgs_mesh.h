/* mgs_mesh.h -- C ABI of the triangle-mesh rasteriser (csrc/mesh.hip, csrc/mesh_raster.h): the opaque foreground of a hybrid
 * frame, as a stand-alone operator.  Compiled into the same libmgs.so / libmgs_debug.so as include/mgs.h's render path and
 * bound by the same conventions (see the top of mgs.h): device pointers unless marked "host", the caller owns every
 * buffer, all work is enqueued on `stream`, and the return value is 0, <0 MGS_ERR_* or >0 a hipError_t from a launch.  The
 * version is mgs.h's: this header adds entry points and changes no parameter list.
 *
 * Inside every mgs_mesh_* / mgs_rasterize_mesh call there are kernel launches and nothing else: no memset, no allocation,
 * no host read-back and no host-to-device copy.  The only atomics are a 64-bit unsigned minimum on the visibility buffer
 * and an integer add on a counter per camera, both of which the clear kernel initialises; no floating-point atomic, and the
 * same inputs give the same bytes in every run.
 *
 * Semantics: tests/mesh_ref.py's docstring, to the evaluation order.  vertices float [V,3], faces int32 [F,3], link_ids
 * int32 [V] (nullable), per-link rotations float [L,3,3] (row-major), translations float [L,3], scales float [L] (nullable:
 * 1) in the convention of mgs_transform_gaussians (x' = s R x + t), viewmats float [C,4,4] (row-major, world to camera),
 * Ks float [C,3,3] of an OpenCV pinhole camera.  A vertex whose link id is outside 0 .. L-1 is static: it is copied.
 *
 * Stages, all over C = n_cams cameras:
 *   vertices  verts_cam float [C,V,3] = V (s R x + t) + t_view, in the fma order of the statement's "Vertex stage".
 *   raster    clear: the visibility buffer (uint64 [C,H,W], first field of the workspace) is set to all-ones and the per-
 *             camera counters to 0, by a kernel.  faces: per face the statement's setup and drop rules -- a vertex index
 *             outside 0 .. V-1 is checked before any vertex is loaded; non-finite; det = 0; with cull_backfaces det >= 0; a
 *             pixel box (the projections clipped to z = near_plane, widened by one pixel, three for a face that crosses the
 *             near plane) that misses the image -- then a walk of the 8 x 8 pixel blocks the box touches, one pixel per
 *             lane, and at each inside pixel with near <= z <= far a 64-bit minimum of (float_bits(z) << 32) | face.  A face
 *             whose box touches more than 15 blocks is appended to the camera's list (room for F records: a bound by
 *             construction; the slot is still checked before the store) and a second launch spreads the blocks of all
 *             listed faces over a fixed grid of 2048 waves per camera.
 *   resolve   per pixel from the winning key: depth float [C,H,W] (0 where uncovered), face_ids int32 [C,H,W] (-1), rgb
 *             float [C,H,W,3] from the barycentrics recomputed for the winning face in the same order -- vertex_colors
 *             float [V,3], else face_colors float [F,3], else 0.7 grey; with headlight times ambient + (1 - ambient) |cos|
 *             of the angle between the face normal and the pixel's ray -- (0, 0, 0) where uncovered; normals (nullable)
 *             float [C,H,W,3], the unit normal (b - a) x (c - a) turned toward the camera.
 *
 * Workspace: 256-byte aligned; fields in this order, each rounded up to 256 bytes:
 *     visibility  uint64 [C,H,W]        8 C H W bytes
 *     counters    uint32 [C]            4 C bytes      (faces in the camera's list)
 *     large       64-byte records [C,F] 64 C F bytes   (the list of faces for the fixed grid)
 * Nothing in it need be initialised; mgs_mesh_resolve reads the visibility buffer mgs_mesh_raster left.
 *
 * Limits, refused with MGS_ERR_INVALID_ARGUMENT and a message before any launch: n_cams < 1; V < 1; F < 1 (F is an int:
 * below 2^31); width or height outside 1 .. 16368; near_plane <= 0 or NaN; far_plane < near_plane or NaN; ambient outside
 * 0 .. 1; a null pointer that is not marked nullable; L < 0, or L > 0 without rotations and translations; a workspace that
 * is too small.  Every product of C H W or C V is formed in 64 bits.
 *
 * Textured meshes (per-corner uvs, base-colour textures, wrap modes, mipmaps) are mgs_mesh_texture.h's: entry points of
 * their own beside these, which they leave as they are. */
#ifndef MGS_MESH_H_
#define MGS_MESH_H_

#include "mgs.h"

#define MGS_MESH_MAX_SIDE 16368
#define MGS_MESH_LARGE_BLOCKS 15

#ifdef __cplusplus
extern "C" {
#endif

/* Bytes of the workspace for n_cams cameras, V vertices, F faces and width x height images. */
int mgs_mesh_workspace_bytes(int n_cams, int V, int F, int width, int height, size_t *bytes /* host */);

/* One launch. */
int mgs_mesh_vertices(int n_cams, int V, const float *vertices, const int32_t *link_ids /* nullable */, int L,
                      const float *rotations /* nullable iff L == 0 */, const float *translations /* nullable iff L == 0 */,
                      const float *scales /* nullable */, const float *viewmats, float *verts_cam, mgs_stream_t stream);

/* Clear + faces: three launches.  cull_backfaces: 0 or 1. */
int mgs_mesh_raster(int n_cams, int V, const float *verts_cam, int F, const int32_t *faces, const float *Ks, int width,
                    int height, float near_plane, float far_plane, int cull_backfaces, void *workspace,
                    size_t workspace_bytes, mgs_stream_t stream);

/* One launch.  headlight: 0 or 1. */
int mgs_mesh_resolve(int n_cams, int V, const float *verts_cam, int F, const int32_t *faces,
                     const float *vertex_colors /* nullable */, const float *face_colors /* nullable */, const float *Ks,
                     int width, int height, int headlight, float ambient, const void *workspace, size_t workspace_bytes,
                     float *rgb, float *depth, int32_t *face_ids, float *normals /* nullable */, mgs_stream_t stream);

/* The four stages: five launches. */
int mgs_rasterize_mesh(int n_cams, int V, const float *vertices, const int32_t *link_ids /* nullable */, int L,
                       const float *rotations, const float *translations, const float *scales /* nullable */,
                       const float *viewmats, const float *Ks, int F, const int32_t *faces,
                       const float *vertex_colors /* nullable */, const float *face_colors /* nullable */, int width,
                       int height, float near_plane, float far_plane, int cull_backfaces, int headlight, float ambient,
                       void *workspace, size_t workspace_bytes, float *verts_cam, float *rgb, float *depth,
                       int32_t *face_ids, float *normals /* nullable */, mgs_stream_t stream);

#ifdef __cplusplus
}
#endif
#endif /* MGS_MESH_H_ */
