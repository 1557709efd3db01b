// Host build (g++) of the mesh rasteriser's arithmetic in robosimgs_amd/csrc/mesh_raster.h: the five launches of csrc/mesh.hip
// as mesh_walk.h walks them for the pinhole's views, on the caller's outputs.  Test-only: never linked into libmgs.so.
#define MGS_MESH_HD inline
#include "mesh_walk.h"

using namespace mgs::mesh;

// stats (nullable) int64 [C,2]: the faces each camera's list received, and the keys formed for it.  Returns 0, or 1 where an
// allocation failed.
extern "C" int mh_rasterize(int n_cams, int V, const float* vertices, const int32_t* link_ids, int L, const float* rotations,
                            const float* translations, const float* scales, const float* viewmats, const float* Ks, int F,
                            const int32_t* faces, const float* vertex_colors, const float* face_colors, int width, int height,
                            float near_plane, float far_plane, int cull, int headlight, float ambient, float* verts_cam,
                            float* rgb, float* depth, int32_t* face_ids, float* normals, int64_t* stats) {
  mesh_walk::vertices(n_cams, V, vertices, link_ids, L, rotations, translations, scales, viewmats, verts_cam);
  return mesh_walk::render(PinholeViews{Ks}, n_cams, V, verts_cam, F, faces, vertex_colors, face_colors, width, height, near_plane,
                           far_plane, cull, headlight, ambient, rgb, depth, face_ids, normals, stats, mesh_walk::Extras());
}

// the workspace layout of include/mgs_mesh.h: out = {visibility, counters, large, total}
extern "C" void mh_workspace_layout(int n_cams, int F, int width, int height, size_t* out) {
  const Layout l = workspace_layout(n_cams, F, width, height);
  out[0] = l.vis; out[1] = l.counters; out[2] = l.large; out[3] = l.total;
}
