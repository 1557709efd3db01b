// mesh_lens.hip -- the triangle-mesh rasteriser under a lens (include/mgs_mesh_lens.h), gfx950.  Every expression that
// decides an index or a value is mesh_raster.h's or mesh_lens_raster.h's, shared with the host harness
// (tests/host_harness/mesh_lens_harness.cpp); what is here is the ray stage and the entry points.
//
// mesh_rays_kernel         one thread per (camera, pixel): the Newton solve of the pixel's ray, one 8-byte store.
// mesh_lens_blocks_kernel  one thread per (camera, 8 x 8 block): the rectangle over the block's 10 x 10 pixels.
// mesh_lens_supers_kernel  one thread per (camera, superblock): the join of its 64 block rectangles.
// mesh_clear_kernel, mesh_faces_kernel<LensView>, mesh_large_kernel<LensView>, mesh_resolve_kernel<LensView>
//                          mesh_kernels.h's, the one text the pinhole path (mesh.hip) runs as well, on LensView: a lane tests
//                          its face's box in ray space against the camera's superblock rectangles (the same address in every
//                          lane: scalar loads) and the blocks of each overlapping one, and a pixel's ray is one 8-byte load
//                          in place of (px + 0.5 - cx, py + 0.5 - cy).  profiles/mesh_refactor/README.md holds the kernels of
//                          both paths to what they were as texts of their own: registers, opcodes and time.
#include "mgs_common.h"
#include "../../include/mgs_mesh_lens.h"

#define MGS_MESH_HD __host__ __device__ __forceinline__
#include "mesh_lens_raster.h"
#include "mesh_checks.h"
#include "mesh_kernels.h"

namespace mgs {
namespace {

using namespace mesh;
static_assert(sizeof(Ray) == 8 && sizeof(Rect) == 16, "record sizes of include/mgs_mesh_lens.h");
static_assert(kModelFisheyeKb == MGS_CAMERA_FISHEYE_KB && kModelPinholeBc == MGS_CAMERA_PINHOLE_BC &&
                  kLensRowFloats == MGS_LENS_ROW_FLOATS && kNewtonSteps == MGS_MESH_LENS_NEWTON_STEPS &&
                  kSuperSide == MGS_MESH_LENS_SUPERBLOCK,
              "mesh_lens_raster.h and the public headers disagree");

__global__ __launch_bounds__(kGroup) void mesh_rays_kernel(int camera_model, const float* __restrict__ lens_rows, int width,
                                                          int height, Ray* __restrict__ rays) {
  const int c = (int)blockIdx.y;
  const long long p = (long long)blockIdx.x * kGroup + threadIdx.x;
  if (p >= (long long)width * height) return;
  const int px = (int)(p % width), py = (int)(p / width);
  rays[pixel_index(c, width, height, px, py)] = pixel_ray(camera_model, lens_rows + kLensRowFloats * (size_t)c, px, py);
}

__global__ __launch_bounds__(kGroup) void mesh_lens_blocks_kernel(int width, int height, const Ray* __restrict__ rays,
                                                                 Rect* __restrict__ blocks) {
  const int c = (int)blockIdx.y, nbx = blocks_of(width), nby = blocks_of(height);
  const long long b = (long long)blockIdx.x * kGroup + threadIdx.x;
  if (b >= (long long)nbx * nby) return;
  const int bx = (int)(b % nbx), by = (int)(b / nbx);
  blocks[rect_index(c, nbx, nby, bx, by)] = block_rect(rays, c, width, height, bx, by);
}

__global__ __launch_bounds__(kGroup) void mesh_lens_supers_kernel(int width, int height, const Rect* __restrict__ blocks,
                                                                 Rect* __restrict__ supers) {
  const int c = (int)blockIdx.y, nsx = supers_of(width), nsy = supers_of(height);
  const long long s = (long long)blockIdx.x * kGroup + threadIdx.x;
  if (s >= (long long)nsx * nsy) return;
  const int sx = (int)(s % nsx), sy = (int)(s / nsx);
  supers[rect_index(c, nsx, nsy, sx, sy)] = super_rect(blocks, c, blocks_of(width), blocks_of(height), sx, sy);
}

int check_model(const char* fn, int camera_model, const float* lens_rows) {
  if (camera_model == MGS_CAMERA_ORTHO)
    return set_error(MGS_ERR_UNSUPPORTED, "%s: MGS_CAMERA_ORTHO has parallel rays and no ray map: the mesh operator has no "
                     "orthographic camera", fn);
  if (camera_model == MGS_CAMERA_PINHOLE || camera_model == MGS_CAMERA_FISHEYE)
    return set_error(MGS_ERR_UNSUPPORTED, "%s: camera_model %d has no lens row: the plain pinhole is mgs_mesh.h's, the ideal "
                     "fisheye is MGS_CAMERA_FISHEYE_KB with all k zero", fn, camera_model);
  MGS_REQUIRE(camera_model == MGS_CAMERA_FISHEYE_KB || camera_model == MGS_CAMERA_PINHOLE_BC,
              "%s: camera_model %d is not a camera model", fn, camera_model);
  MGS_REQUIRE(lens_rows, "%s: lens_rows is null", fn);
  return MGS_OK;
}

LensView lens_view(const void* lens_workspace, const LensLayout& l) {
  const char* ws = static_cast<const char*>(lens_workspace);
  return {reinterpret_cast<const Ray*>(ws + l.rays), reinterpret_cast<const Rect*>(ws + l.blocks),
          reinterpret_cast<const Rect*>(ws + l.supers)};
}

}  // namespace
}  // namespace mgs

using namespace mgs;

extern "C" int mgs_mesh_lens_workspace_bytes(int n_cams, int width, int height, size_t* bytes) {
  MGS_TRY(check_sizes("mesh_lens_workspace_bytes", n_cams, 1, 1, width, height));
  MGS_REQUIRE(bytes, "mesh_lens_workspace_bytes: bytes is null");
  *bytes = lens_layout(n_cams, width, height).total;
  return MGS_OK;
}

extern "C" int mgs_mesh_lens_rays(int n_cams, int camera_model, const float* lens_rows, int width, int height,
                                  void* lens_workspace, size_t lens_workspace_bytes, mgs_stream_t stream) {
  MGS_TRY(check_sizes("mesh_lens_rays", n_cams, 1, 1, width, height));
  MGS_TRY(check_model("mesh_lens_rays", camera_model, lens_rows));
  const LensLayout l = lens_layout(n_cams, width, height);
  MGS_TRY(check_workspace("mesh_lens_rays", "lens_workspace", lens_workspace, lens_workspace_bytes, l.total));
  char* ws = static_cast<char*>(lens_workspace);
  Ray* rays = reinterpret_cast<Ray*>(ws + l.rays);
  Rect* blocks = reinterpret_cast<Rect*>(ws + l.blocks);
  Rect* supers = reinterpret_cast<Rect*>(ws + l.supers);
  hipStream_t s = (hipStream_t)stream;
  const dim3 block(kGroup);
  const size_t n_px = (size_t)width * (size_t)height;                        // <= 16368^2 < 2^28
  const size_t n_blocks_ = (size_t)blocks_of(width) * (size_t)blocks_of(height);
  const size_t n_supers = (size_t)supers_of(width) * (size_t)supers_of(height);
  hipLaunchKernelGGL(mesh_rays_kernel, dim3((unsigned)((n_px + kGroup - 1) / kGroup), (unsigned)n_cams), block, 0, s,
                     camera_model, lens_rows, width, height, rays);
  MGS_TRY(check_launch("mesh_lens_rays (rays)"));
  hipLaunchKernelGGL(mesh_lens_blocks_kernel, dim3((unsigned)((n_blocks_ + kGroup - 1) / kGroup), (unsigned)n_cams), block, 0, s,
                     width, height, (const Ray*)rays, blocks);
  MGS_TRY(check_launch("mesh_lens_rays (blocks)"));
  hipLaunchKernelGGL(mesh_lens_supers_kernel, dim3((unsigned)((n_supers + kGroup - 1) / kGroup), (unsigned)n_cams), block, 0, s,
                     width, height, (const Rect*)blocks, supers);
  return check_launch("mesh_lens_rays (superblocks)");
}

extern "C" int mgs_mesh_raster_lens(int n_cams, int V, const float* verts_cam, int F, const int32_t* faces, int camera_model,
                                    const float* lens_rows, int width, int height, float near_plane, float far_plane,
                                    int cull_backfaces, void* workspace, size_t workspace_bytes, const void* lens_workspace,
                                    size_t lens_workspace_bytes, mgs_stream_t stream) {
  MGS_TRY(check_sizes("mesh_raster_lens", n_cams, V, F, width, height));
  MGS_TRY(check_planes("mesh_raster_lens", near_plane, far_plane));
  MGS_TRY(check_model("mesh_raster_lens", camera_model, lens_rows));
  MGS_REQUIRE(verts_cam && faces, "mesh_raster_lens: verts_cam or faces is null");
  const Layout l = workspace_layout(n_cams, F, width, height);
  const LensLayout ll = lens_layout(n_cams, width, height);
  MGS_TRY(check_workspace("mesh_raster_lens", "workspace", workspace, workspace_bytes, l.total));
  MGS_TRY(check_workspace("mesh_raster_lens", "lens_workspace", lens_workspace, lens_workspace_bytes, ll.total));
  return launch_raster("mesh_raster_lens", lens_view(lens_workspace, ll), n_cams, V, verts_cam, F, faces, width, height, near_plane,
                       far_plane, cull_backfaces, workspace, l, (hipStream_t)stream);
}

extern "C" int mgs_mesh_resolve_lens(int n_cams, int V, const float* verts_cam, int F, const int32_t* faces,
                                     const float* vertex_colors, const float* face_colors, int camera_model,
                                     const float* lens_rows, int width, int height, int headlight, float ambient,
                                     const void* workspace, size_t workspace_bytes, const void* lens_workspace,
                                     size_t lens_workspace_bytes, float* rgb, float* depth, int32_t* face_ids, float* normals,
                                     mgs_stream_t stream) {
  MGS_TRY(check_sizes("mesh_resolve_lens", n_cams, V, F, width, height));
  MGS_TRY(check_ambient("mesh_resolve_lens", ambient));
  MGS_TRY(check_model("mesh_resolve_lens", camera_model, lens_rows));
  MGS_REQUIRE(verts_cam && faces, "mesh_resolve_lens: verts_cam or faces is null");
  MGS_REQUIRE(rgb && depth && face_ids, "mesh_resolve_lens: an output (rgb, depth, face_ids) is null");
  const Layout l = workspace_layout(n_cams, F, width, height);
  const LensLayout ll = lens_layout(n_cams, width, height);
  MGS_TRY(check_workspace("mesh_resolve_lens", "workspace", workspace, workspace_bytes, l.total));
  MGS_TRY(check_workspace("mesh_resolve_lens", "lens_workspace", lens_workspace, lens_workspace_bytes, ll.total));
  return launch_resolve("mesh_resolve_lens", lens_view(lens_workspace, ll), n_cams, V, verts_cam, F, faces, vertex_colors,
                        face_colors, width, height, headlight, ambient, workspace, l, rgb, depth, face_ids, normals,
                        (hipStream_t)stream);
}

extern "C" int mgs_rasterize_mesh_lens(int n_cams, int V, const float* vertices, const int32_t* link_ids, int L,
                                       const float* rotations, const float* translations, const float* scales,
                                       const float* viewmats, int camera_model, const float* lens_rows, int F,
                                       const int32_t* faces, const float* vertex_colors, const float* face_colors, int width,
                                       int height, float near_plane, float far_plane, int cull_backfaces, int headlight,
                                       float ambient, void* workspace, size_t workspace_bytes, void* lens_workspace,
                                       size_t lens_workspace_bytes, float* verts_cam, float* rgb, float* depth,
                                       int32_t* face_ids, float* normals, mgs_stream_t stream) {
  // every argument is checked before the first launch
  MGS_TRY(check_sizes("rasterize_mesh_lens", n_cams, V, F, width, height));
  MGS_TRY(check_planes("rasterize_mesh_lens", near_plane, far_plane));
  MGS_TRY(check_links("rasterize_mesh_lens", L, rotations, translations));
  MGS_TRY(check_ambient("rasterize_mesh_lens", ambient));
  MGS_TRY(check_model("rasterize_mesh_lens", camera_model, lens_rows));
  MGS_REQUIRE(vertices && viewmats && faces, "rasterize_mesh_lens: vertices, viewmats or faces is null");
  MGS_REQUIRE(verts_cam && rgb && depth && face_ids, "rasterize_mesh_lens: an output (verts_cam, rgb, depth, face_ids) is null");
  MGS_TRY(check_workspace("rasterize_mesh_lens", "workspace", workspace, workspace_bytes,
                          workspace_layout(n_cams, F, width, height).total));
  MGS_TRY(check_workspace("rasterize_mesh_lens", "lens_workspace", lens_workspace, lens_workspace_bytes,
                          lens_layout(n_cams, width, height).total));
  MGS_TRY(mgs_mesh_vertices(n_cams, V, vertices, link_ids, L, rotations, translations, scales, viewmats, verts_cam, stream));
  MGS_TRY(mgs_mesh_lens_rays(n_cams, camera_model, lens_rows, width, height, lens_workspace, lens_workspace_bytes, stream));
  MGS_TRY(mgs_mesh_raster_lens(n_cams, V, verts_cam, F, faces, camera_model, lens_rows, width, height, near_plane, far_plane,
                               cull_backfaces, workspace, workspace_bytes, lens_workspace, lens_workspace_bytes, stream));
  return mgs_mesh_resolve_lens(n_cams, V, verts_cam, F, faces, vertex_colors, face_colors, camera_model, lens_rows, width,
                               height, headlight, ambient, workspace, workspace_bytes, lens_workspace, lens_workspace_bytes, rgb,
                               depth, face_ids, normals, stream);
}
