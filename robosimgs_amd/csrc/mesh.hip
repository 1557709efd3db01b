// mesh.hip -- the triangle-mesh rasteriser (include/mgs_mesh.h), gfx950.  Every expression that decides an index or a value
// is mesh_raster.h's, shared with the host harness (tests/host_harness/mesh_harness.cpp); the launch shape of the raster and
// resolve stages is mesh_kernels.h's, shared with the lens path (mesh_lens.hip), instantiated here for PinholeViews: a
// pixel's ray is (px + 0.5 - cx, py + 0.5 - cy) and a face's planes and box are set up under the camera's K.
//
// mesh_vertices_kernel               one thread per (camera, vertex).
// mesh_clear_kernel                  mesh_kernels.h
// mesh_faces_kernel<PinholeViews>    mesh_kernels.h
// mesh_large_kernel<PinholeViews>    mesh_kernels.h
// mesh_resolve_kernel<PinholeViews>  mesh_kernels.h
#include "mgs_common.h"
#include "../../include/mgs_mesh.h"

#define MGS_MESH_HD __host__ __device__ __forceinline__
#include "mesh_raster.h"
#include "mesh_checks.h"
#include "mesh_kernels.h"

namespace mgs {
namespace {

using namespace mesh;
static_assert(kLargeBlocks == MGS_MESH_LARGE_BLOCKS && kMaxSide == MGS_MESH_MAX_SIDE, "mesh_raster.h and mgs_mesh.h disagree");

__global__ __launch_bounds__(kGroup) void mesh_vertices_kernel(int V, const float* __restrict__ vertices,
                                                              const int32_t* __restrict__ link_ids, int L,
                                                              const float* __restrict__ rotations,
                                                              const float* __restrict__ translations,
                                                              const float* __restrict__ scales,
                                                              const float* __restrict__ viewmats, float* __restrict__ verts_cam) {
  const int c = (int)blockIdx.y;
  const long long v = (long long)blockIdx.x * kGroup + threadIdx.x;
  if (v >= V) return;
  const float x[3] = {vertices[3 * v + 0], vertices[3 * v + 1], vertices[3 * v + 2]};
  float cam[3];
  vertex_to_camera(x, link_ids ? link_ids[v] : -1, L, rotations, translations, scales, viewmats + 16 * (size_t)c, cam);
  float* o = verts_cam + vertex_index(c, V, (int)v);
  o[0] = cam[0]; o[1] = cam[1]; o[2] = cam[2];
}

}  // namespace
}  // namespace mgs

using namespace mgs;

extern "C" int mgs_mesh_workspace_bytes(int n_cams, int V, int F, int width, int height, size_t* bytes) {
  MGS_TRY(check_sizes("mesh_workspace_bytes", n_cams, V, F, width, height));
  MGS_REQUIRE(bytes, "mesh_workspace_bytes: bytes is null");
  *bytes = workspace_layout(n_cams, F, width, height).total;
  return MGS_OK;
}

extern "C" int mgs_mesh_vertices(int n_cams, int V, const float* vertices, const int32_t* link_ids, int L,
                                 const float* rotations, const float* translations, const float* scales,
                                 const float* viewmats, float* verts_cam, mgs_stream_t stream) {
  MGS_TRY(check_sizes("mesh_vertices", n_cams, V, 1, 1, 1));
  MGS_TRY(check_links("mesh_vertices", L, rotations, translations));
  MGS_REQUIRE(vertices && viewmats && verts_cam, "mesh_vertices: vertices, viewmats or verts_cam is null");
  const dim3 grid(div_up((unsigned)V, (unsigned)kGroup), (unsigned)n_cams), block(kGroup);
  hipLaunchKernelGGL(mesh_vertices_kernel, grid, block, 0, (hipStream_t)stream, V, vertices, link_ids, L, rotations,
                     translations, scales, viewmats, verts_cam);
  return check_launch("mesh_vertices");
}

extern "C" int mgs_mesh_raster(int n_cams, int V, const float* verts_cam, int F, const int32_t* faces, const float* Ks,
                               int width, int height, float near_plane, float far_plane, int cull_backfaces, void* workspace,
                               size_t workspace_bytes, mgs_stream_t stream) {
  MGS_TRY(check_sizes("mesh_raster", n_cams, V, F, width, height));
  MGS_TRY(check_planes("mesh_raster", near_plane, far_plane));
  MGS_REQUIRE(verts_cam && faces && Ks, "mesh_raster: verts_cam, faces or Ks is null");
  const Layout l = workspace_layout(n_cams, F, width, height);
  MGS_TRY(check_workspace("mesh_raster", "workspace", workspace, workspace_bytes, l.total));
  return launch_raster("mesh_raster", PinholeViews{Ks}, n_cams, V, verts_cam, F, faces, width, height, near_plane, far_plane,
                       cull_backfaces, workspace, l, (hipStream_t)stream);
}

extern "C" int mgs_mesh_resolve(int n_cams, int V, const float* verts_cam, int F, const int32_t* faces,
                                const float* vertex_colors, const float* face_colors, const float* Ks, int width, int height,
                                int headlight, float ambient, const void* workspace, size_t workspace_bytes, float* rgb,
                                float* depth, int32_t* face_ids, float* normals, mgs_stream_t stream) {
  MGS_TRY(check_sizes("mesh_resolve", n_cams, V, F, width, height));
  MGS_TRY(check_ambient("mesh_resolve", ambient));
  MGS_REQUIRE(verts_cam && faces && Ks, "mesh_resolve: verts_cam, faces or Ks is null");
  MGS_REQUIRE(rgb && depth && face_ids, "mesh_resolve: an output (rgb, depth, face_ids) is null");
  const Layout l = workspace_layout(n_cams, F, width, height);
  MGS_TRY(check_workspace("mesh_resolve", "workspace", workspace, workspace_bytes, l.total));
  return launch_resolve("mesh_resolve", PinholeViews{Ks}, n_cams, V, verts_cam, F, faces, vertex_colors, face_colors, width, height,
                        headlight, ambient, workspace, l, rgb, depth, face_ids, normals, (hipStream_t)stream);
}

extern "C" int mgs_rasterize_mesh(int n_cams, int V, const float* vertices, const int32_t* link_ids, int L,
                                  const float* rotations, const float* translations, const float* scales,
                                  const float* viewmats, const float* Ks, int F, const int32_t* faces,
                                  const float* vertex_colors, const float* face_colors, int width, int height,
                                  float near_plane, float far_plane, int cull_backfaces, int headlight, float ambient,
                                  void* workspace, size_t workspace_bytes, float* verts_cam, float* rgb, float* depth,
                                  int32_t* face_ids, float* normals, mgs_stream_t stream) {
  // every argument is checked before the first launch
  MGS_TRY(check_sizes("rasterize_mesh", n_cams, V, F, width, height));
  MGS_TRY(check_planes("rasterize_mesh", near_plane, far_plane));
  MGS_TRY(check_links("rasterize_mesh", L, rotations, translations));
  MGS_TRY(check_ambient("rasterize_mesh", ambient));
  MGS_REQUIRE(vertices && viewmats && Ks && faces, "rasterize_mesh: vertices, viewmats, Ks or faces is null");
  MGS_REQUIRE(verts_cam && rgb && depth && face_ids, "rasterize_mesh: an output (verts_cam, rgb, depth, face_ids) is null");
  MGS_TRY(check_workspace("rasterize_mesh", "workspace", workspace, workspace_bytes,
                          workspace_layout(n_cams, F, width, height).total));
  MGS_TRY(mgs_mesh_vertices(n_cams, V, vertices, link_ids, L, rotations, translations, scales, viewmats, verts_cam, stream));
  MGS_TRY(mgs_mesh_raster(n_cams, V, verts_cam, F, faces, Ks, width, height, near_plane, far_plane, cull_backfaces, workspace,
                          workspace_bytes, stream));
  return mgs_mesh_resolve(n_cams, V, verts_cam, F, faces, vertex_colors, face_colors, Ks, width, height, headlight, ambient,
                          workspace, workspace_bytes, rgb, depth, face_ids, normals, stream);
}
