/* mgs_mesh_texture.h -- C ABI of textured triangle meshes (csrc/mesh_texture.hip, csrc/mesh_texture.h): base-colour
 * textures with per-corner uvs, wrap modes and mipmaps in the resolve stage of the mesh rasteriser.  An addition to
 * mgs_mesh.h in the way mgs_deform_sh.h adds to mgs_deform.h: the same libraries, the same conventions (device pointers
 * unless marked "host", the caller owns every buffer, work is enqueued on `stream`, 0 / <0 MGS_ERR_* / >0 hipError_t), the
 * version is mgs.h's, and no parameter list of mgs_mesh.h changes.  A mesh without textures keeps to mgs_mesh.h's entry
 * points: their kernels are not touched by this header's.
 *
 * Inside every call there are kernel launches and nothing else: no memset, no allocation, no host read-back, no copy, no
 * atomics (beyond mgs_mesh_raster's own), no workspace beyond mgs_mesh.h's.  The same inputs give the same bytes.
 *
 * Semantics: tests/texture_ref.py's docstring, to the evaluation order.
 *   texels       one little-endian 32-bit word per texel, byte 0 red .. byte 3 alpha (carried, ignored: the layer is
 *                opaque), row-major, row 0 at the top.  Values are used as they are, byte / 255: colours here are display-
 *                referred, nothing is linearised, and mip levels average in that same space.
 *   texture set  T textures, all levels of all textures in one array of `texel_count` words: texture 0's level 0, its level
 *                1, .. , texture 1's level 0, .. without gaps.  Level l is max(1, w >> l) x max(1, h >> l); there are
 *                1 + floor(log2(max(w, h))) levels.
 *   descriptor   20 int32 words per texture: w, h, levels, wrap (wrap_s | wrap_t << 8, each MGS_MESH_WRAP_*), then 16
 *                unsigned words: the index of each level's first texel in the array (0 past `levels`).
 *                mgs_mesh_texture_layout writes them on the host; the caller copies them to the device for the resolve.
 *   mips         texel (x, y) of level l+1 is per byte (s00 + s01 + s10 + s11 + 2) >> 2 of level l's texels at columns
 *                min(2x, w_l - 1), min(2x + 1, w_l - 1) and rows likewise.  One launch per level and texture.
 *   face_uvs     float [F,3,2]: one (u, v) per corner; the origin is the image's top-left corner and v points down.
 *   face_textures int32 [F]: the face's texture; a value outside 0 .. T-1 means "not textured" (checked before any
 *                descriptor is read).
 *   resolve      mgs_mesh_resolve's outputs.  rgb of a textured pixel = texel x tint x shade: (u, v) interpolated with the
 *                winning face's barycentrics, wrapped in floating point (repeat u - floor u; mirror 1 - |u - 2 floor(u / 2)
 *                - 1|; clamp), sampled bilinearly at level 0 (MGS_MESH_FILTER_BILINEAR) or trilinearly at the analytic
 *                level of detail log2 of the longer of the two screen-space derivative vectors of (w u, h v), clamped to
 *                0 .. levels - 1 (MGS_MESH_FILTER_TRILINEAR); tint = the interpolated vertex colour, the face colour, or 1.
 *                A pixel whose face is not textured, or whose u, v or (trilinear) derivatives are not finite, gets
 *                mgs_mesh_resolve's bits.  Every texel index is wrapped or clamped into its level and held below
 *                texel_count before the load; depth, face ids and normals are mgs_mesh_resolve's bits everywhere.
 *
 * Limits, refused with MGS_ERR_INVALID_ARGUMENT and a message before any launch: n_textures outside 1 .. 4096; a side
 * outside 1 .. 16384; a wrap mode that is none of the three; the texels of all levels reaching 2^31; descriptors (host, for
 * mgs_mesh_build_mips) that are not the layout of their own sizes, or a texel_count that is not their total; filter not 0
 * or 1; a null or misaligned pointer; and everything mgs_mesh.h's entry points of the same stages refuse. */
#ifndef MGS_MESH_TEXTURE_H_PUBLIC_
#define MGS_MESH_TEXTURE_H_PUBLIC_

#include "mgs_mesh.h"

#define MGS_MESH_TEXTURE_MAX_SIDE 16384
#define MGS_MESH_MAX_TEXTURES 4096
#define MGS_MESH_TEXTURE_DESC_WORDS 20
#define MGS_MESH_WRAP_REPEAT 0 /* glTF 10497 */
#define MGS_MESH_WRAP_CLAMP 1  /* glTF 33071 */
#define MGS_MESH_WRAP_MIRROR 2 /* glTF 33648 */
#define MGS_MESH_FILTER_BILINEAR 0
#define MGS_MESH_FILTER_TRILINEAR 1

#ifdef __cplusplus
extern "C" {
#endif

/* Host only, no launch.  sizes host int32 [T,2] = (w, h); wraps host int32 [T,2] = (wrap_s, wrap_t), nullable: repeat;
 * descriptors host int32 [T,20], nullable: only the count is wanted. */
int mgs_mesh_texture_layout(int n_textures, const int32_t *sizes /* host */, const int32_t *wraps /* host, nullable */,
                            int32_t *descriptors /* host, nullable */, size_t *texel_count /* host */);

/* Levels 1 .. of every texture from its level 0, which the caller has stored: one launch per level and texture. */
int mgs_mesh_build_mips(int n_textures, const int32_t *descriptors /* host */, void *texels, size_t texel_count,
                        mgs_stream_t stream);

/* mgs_mesh_resolve with textures: one launch.  filter: MGS_MESH_FILTER_*. */
int mgs_mesh_resolve_textured(int n_cams, int V, const float *verts_cam, int F, const int32_t *faces,
                              const float *vertex_colors /* nullable */, const float *face_colors /* nullable */,
                              const float *Ks, int width, int height, int headlight, float ambient, const void *workspace,
                              size_t workspace_bytes, float *rgb, float *depth, int32_t *face_ids,
                              float *normals /* nullable */, const float *face_uvs, const int32_t *face_textures,
                              int n_textures, const int32_t *descriptors, const void *texels, size_t texel_count, int filter,
                              mgs_stream_t stream);

/* mgs_rasterize_mesh with the textured resolve: five launches. */
int mgs_rasterize_mesh_textured(int n_cams, int V, const float *vertices, const int32_t *link_ids /* nullable */, int L,
                                const float *rotations, const float *translations, const float *scales /* nullable */,
                                const float *viewmats, const float *Ks, int F, const int32_t *faces,
                                const float *vertex_colors /* nullable */, const float *face_colors /* nullable */, int width,
                                int height, float near_plane, float far_plane, int cull_backfaces, int headlight,
                                float ambient, void *workspace, size_t workspace_bytes, float *verts_cam, float *rgb,
                                float *depth, int32_t *face_ids, float *normals /* nullable */, const float *face_uvs,
                                const int32_t *face_textures, int n_textures, const int32_t *descriptors, const void *texels,
                                size_t texel_count, int filter, mgs_stream_t stream);

#ifdef __cplusplus
}
#endif
#endif /* MGS_MESH_TEXTURE_H_PUBLIC_ */
