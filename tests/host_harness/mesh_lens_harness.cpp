// Host build (g++) of the mesh rasteriser under a lens: robosimgs_amd/csrc/mesh_lens_raster.h over mesh_raster.h.  The ray
// stage of csrc/mesh_lens.hip is walked here, serially, on heap buffers of exactly the sizes include/mgs_mesh_lens.h gives the
// lens workspace's fields; the other launches are mesh_walk.h's, for LensView.  Test-only: never linked into libmgs.so.
#include <cstring>

#define MGS_MESH_HD inline
#include "../../robosimgs_amd/csrc/mesh_lens_raster.h"
#include "mesh_walk.h"

using namespace mgs::mesh;

namespace {

// mesh_rays_kernel, mesh_lens_blocks_kernel, mesh_lens_supers_kernel
void ray_stage(int n_cams, int camera_model, const float* rows, int width, int height, Ray* rays, Rect* blocks, Rect* supers,
               bool solve) {
  const int nbx = blocks_of(width), nby = blocks_of(height), nsx = supers_of(width), nsy = supers_of(height);
  for (int c = 0; c < n_cams; ++c) {
    for (int py = 0; py < height && solve; ++py)
      for (int px = 0; px < width; ++px)
        rays[pixel_index(c, width, height, px, py)] = pixel_ray(camera_model, rows + kLensRowFloats * (size_t)c, px, py);
    for (int by = 0; by < nby; ++by)
      for (int bx = 0; bx < nbx; ++bx) blocks[rect_index(c, nbx, nby, bx, by)] = block_rect(rays, c, width, height, bx, by);
    for (int sy = 0; sy < nsy; ++sy)
      for (int sx = 0; sx < nsx; ++sx) supers[rect_index(c, nsx, nsy, sx, sy)] = super_rect(blocks, c, nbx, nby, sx, sy);
  }
}

}  // namespace

// The ray stage alone: rays float [C,H,W,2], blocks float [C,BY,BX,4], supers float [C,SY,SX,4] (caller's buffers of the
// layout's sizes).
extern "C" void mlh_rays(int n_cams, int camera_model, const float* rows, int width, int height, float* rays, float* blocks,
                         float* supers) {
  ray_stage(n_cams, camera_model, rows, width, height, reinterpret_cast<Ray*>(rays), reinterpret_cast<Rect*>(blocks),
            reinterpret_cast<Rect*>(supers), true);
}

// The fused call.  rays_in (nullable) float [C,H,W,2]: a ray map to rasterise on instead of the harness's own (the block
// tables are then built from it).  every_block != 0: every face that has planes walks every block of the image, through no
// box at all -- what a box may never differ from.  rays_out (nullable) receives the map used.  stats (nullable) int64 [C,2]:
// the faces each camera's list received and the keys formed; face_blocks (nullable) int32 [C,F]: the blocks of each face's
// box, 0 where the face is dropped.  Returns 0, or 1 where an allocation failed.
extern "C" int mlh_rasterize(int n_cams, int V, const float* vertices, const int32_t* link_ids, int L, const float* rotations,
                             const float* translations, const float* scales, const float* viewmats, int camera_model,
                             const float* rows, int F, const int32_t* faces, const float* vertex_colors,
                             const float* face_colors, int width, int height, float near_plane, float far_plane, int cull,
                             int headlight, float ambient, const float* rays_in, int every_block, float* verts_cam, float* rgb,
                             float* depth, int32_t* face_ids, float* normals, float* rays_out, int64_t* stats,
                             int32_t* face_blocks) {
  // the three fields of the lens workspace, each a heap block of its exact size
  Ray* rays = static_cast<Ray*>(malloc(ray_bytes(n_cams, width, height)));
  Rect* blocks = static_cast<Rect*>(malloc(block_rect_bytes(n_cams, width, height)));
  Rect* supers = static_cast<Rect*>(malloc(super_rect_bytes(n_cams, width, height)));
  if (!rays || !blocks || !supers) { free(rays); free(blocks); free(supers); return 1; }
  mesh_walk::vertices(n_cams, V, vertices, link_ids, L, rotations, translations, scales, viewmats, verts_cam);
  if (rays_in) memcpy(rays, rays_in, ray_bytes(n_cams, width, height));
  ray_stage(n_cams, camera_model, rows, width, height, rays, blocks, supers, rays_in == nullptr);
  if (rays_out) memcpy(rays_out, rays, ray_bytes(n_cams, width, height));
  mesh_walk::Extras extras;
  extras.every_block = every_block != 0;
  extras.face_blocks = face_blocks;
  const int rc = mesh_walk::render(LensView{rays, blocks, supers}, n_cams, V, verts_cam, F, faces, vertex_colors, face_colors, width,
                                   height, near_plane, far_plane, cull, headlight, ambient, rgb, depth, face_ids, normals, stats,
                                   extras);
  free(rays); free(blocks); free(supers);
  return rc;
}

// the lens workspace layout of include/mgs_mesh_lens.h: out = {rays, blocks, superblocks, total}
extern "C" void mlh_workspace_layout(int n_cams, int width, int height, size_t* out) {
  const LensLayout l = lens_layout(n_cams, width, height);
  out[0] = l.rays; out[1] = l.blocks; out[2] = l.supers; out[3] = l.total;
}

// one evaluation of the forward map in fp32, as the kernels evaluate it: out = {xd, yd, bound} (pinhole lens) or
// {theta_d, 0, bound} (fisheye, a = theta)
extern "C" void mlh_distort(int camera_model, const float* k, float a, float b, float* out) {
  if (camera_model == kModelPinholeBc) {
    const Distorted D = distort_bc(k, a, b);
    out[0] = D.xd; out[1] = D.yd; out[2] = D.bound;
  } else {
    const Radial R = distort_kb(k, a);
    out[0] = R.td; out[1] = 0.0f; out[2] = R.bound;
  }
}
