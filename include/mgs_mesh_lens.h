/* mgs_mesh_lens.h -- C ABI of the triangle-mesh rasteriser under a lens (csrc/mesh_lens.hip, csrc/mesh_lens_raster.h): the
 * operator of mgs_mesh.h for the cameras of mgs_lens.h (MGS_CAMERA_FISHEYE_KB; all k zero: the ideal fisheye) and
 * mgs_lens_pinhole.h (MGS_CAMERA_PINHOLE_BC), so that a mesh layer registers with a splat frame rendered under the same
 * lens.  Compiled into the same libmgs.so / libmgs_debug.so and bound by the conventions at the top of mgs.h.  The version
 * is mgs.h's: this header adds entry points and changes no parameter list; mgs_mesh.h's calls are as they were.
 *
 * The raster of mgs_mesh.h is homogeneous: the pixel enters the edge test only through its ray.  Under a lens the triangle is
 * unchanged and the ray of pixel (px, py) is (x_u, y_u, 1), with (x_u, y_u) the preimage under the lens's distortion map of
 * d = ((px + 0.5 - cx) / fx, (py + 0.5 - cy) / fy).  Nothing is tessellated, approximated by straight edges or resampled:
 * the same edge test runs at another point.  Semantics: tests/mesh_lens_ref.py.
 *
 * lens_rows float [C,16]: the camera rows of mgs_lens.h / mgs_lens_pinhole.h (K row-major in 0..8, the coefficients from
 * 9, u_max at 13 / 14), in place of every Ks.  The kernels solve no polynomial for u_max; they read it from the row.
 *
 * Stages:
 *   rays      mgs_mesh_lens_rays, three launches: per pixel the ray (x_u, y_u), NaN in both components where the pixel has
 *             none.  MGS_CAMERA_PINHOLE_BC: 12 Newton steps on D(q) = d from q = d; valid iff u < u_max, det Jd > 0 and the
 *             fp32 residual max|D(q) - d| is within twice the counted bound of one fp32 evaluation of D at q.
 *             MGS_CAMERA_FISHEYE_KB: 12 Newton steps on theta P(theta^2) = |d| from theta = |d|; valid iff theta^2 < u_max,
 *             the residual is within its bound and cos(theta) > 0 as evaluated; q = d sin(theta) / (cos(theta) |d|), q = d
 *             at d = 0 (a ray at 90 degrees or beyond sees nothing: the raster refuses z < near_plane).  Then per 8 x 8 pixel
 *             block the rectangle (min x_u, min y_u, max x_u, max y_u) over the valid rays of the block and of the one-pixel
 *             ring around it, (+inf, +inf, -inf, -inf) where the block has no valid pixel of its own, and the join of those
 *             rectangles per superblock of 8 x 8 blocks.
 *   raster    mgs_mesh_raster_lens, three launches: mgs_mesh_raster with the planes set up under fx = fy = 1, cx = cy = 0
 *             and each pixel's (dx, dy) loaded from the ray map; a pixel without a ray is never inside.  A face's box is
 *             taken in ray space, where its outline is straight: x/z, y/z over the vertices with z >= near_plane and the
 *             near-plane crossings, widened by the counted fp32 bound of those quotients, tested against the superblock
 *             rectangles and the block rectangles of each overlapping superblock; bx0, by0, nbx, nby is the bounding box
 *             in block indices of all overlapping blocks.  The 15-block threshold, the list, the fixed grid of 2048 waves
 *             and the 64-bit minimum are mgs_mesh.h's.
 *   resolve   mgs_mesh_resolve_lens, one launch: mgs_mesh_resolve at the pixel's ray; the headlight's ray is (x_u, y_u, 1)
 *             normalised; a pixel without a ray is uncovered (depth 0, face id -1, rgb 0).  depth is the camera z.
 * mgs_rasterize_mesh_lens runs vertices, rays, raster and resolve: eight launches.  It builds the ray map in every call,
 * because callers overwrite lens_rows in place between frames.
 *
 * Lens workspace (lens_workspace): 256-byte aligned; fields in this order, each rounded up to 256 bytes, with
 * BX = ceil(W / 8), BY = ceil(H / 8), SX = ceil(BX / 8), SY = ceil(BY / 8):
 *     rays         float [C,H,W,2]     8 C H W bytes
 *     blocks       float [C,BY,BX,4]   16 C BY BX bytes
 *     superblocks  float [C,SY,SX,4]   16 C SY SX bytes
 * Nothing in it need be initialised; the raster and the resolve read what mgs_mesh_lens_rays left.  `workspace` is
 * mgs_mesh.h's (mgs_mesh_workspace_bytes), unchanged.
 *
 * Inside every call there are kernel launches and nothing else; no floating-point atomic; the same inputs give the same
 * bytes in every run.  Refused with a message before any launch: what mgs_mesh.h refuses; a camera_model that is neither
 * MGS_CAMERA_FISHEYE_KB nor MGS_CAMERA_PINHOLE_BC (MGS_CAMERA_ORTHO, whose rays are parallel and have no ray map of this
 * form, and MGS_CAMERA_PINHOLE / MGS_CAMERA_FISHEYE, which have no row: MGS_ERR_UNSUPPORTED; any other value:
 * MGS_ERR_INVALID_ARGUMENT); lens_rows == NULL; a lens workspace that is null, misaligned or too small.  Textured meshes
 * under a lens are not built: the texture's level of detail needs the ray map's derivatives. */
#ifndef MGS_MESH_LENS_H_
#define MGS_MESH_LENS_H_

#include "mgs_lens_pinhole.h"
#include "mgs_mesh.h"

#define MGS_MESH_LENS_NEWTON_STEPS 12
#define MGS_MESH_LENS_SUPERBLOCK 8

#ifdef __cplusplus
extern "C" {
#endif

/* Bytes of the lens workspace for n_cams cameras and width x height images. */
int mgs_mesh_lens_workspace_bytes(int n_cams, int width, int height, size_t *bytes /* host */);

/* Rays, block rectangles, superblock rectangles: three launches. */
int mgs_mesh_lens_rays(int n_cams, int camera_model, const float *lens_rows, int width, int height, void *lens_workspace,
                       size_t lens_workspace_bytes, mgs_stream_t stream);

/* mgs_mesh_raster on the ray map mgs_mesh_lens_rays left: three launches. */
int mgs_mesh_raster_lens(int n_cams, int V, const float *verts_cam, int F, const int32_t *faces, int camera_model,
                         const float *lens_rows, int width, int height, float near_plane, float far_plane,
                         int cull_backfaces, void *workspace, size_t workspace_bytes, const void *lens_workspace,
                         size_t lens_workspace_bytes, mgs_stream_t stream);

/* mgs_mesh_resolve on the same ray map: one launch. */
int mgs_mesh_resolve_lens(int n_cams, int V, const float *verts_cam, int F, const int32_t *faces,
                          const float *vertex_colors /* nullable */, const float *face_colors /* nullable */,
                          int camera_model, const float *lens_rows, int width, int height, int headlight, float ambient,
                          const void *workspace, size_t workspace_bytes, const void *lens_workspace,
                          size_t lens_workspace_bytes, float *rgb, float *depth, int32_t *face_ids,
                          float *normals /* nullable */, mgs_stream_t stream);

/* Vertices, rays, raster, resolve: eight launches. */
int mgs_rasterize_mesh_lens(int n_cams, int V, const float *vertices, const int32_t *link_ids /* nullable */, int L,
                            const float *rotations, const float *translations, const float *scales /* nullable */,
                            const float *viewmats, int camera_model, const float *lens_rows, int F, const int32_t *faces,
                            const float *vertex_colors /* nullable */, const float *face_colors /* nullable */, int width,
                            int height, float near_plane, float far_plane, int cull_backfaces, int headlight,
                            float ambient, void *workspace, size_t workspace_bytes, void *lens_workspace,
                            size_t lens_workspace_bytes, float *verts_cam, float *rgb, float *depth, int32_t *face_ids,
                            float *normals /* nullable */, mgs_stream_t stream);

#ifdef __cplusplus
}
#endif
#endif /* MGS_MESH_LENS_H_ */
