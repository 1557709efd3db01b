// mesh_lens.hip -- the triangle-mesh rasteriser under a lens (include/mgs_mesh_lens.h), gfx950.  Every expression that
// decides an index or a value is mesh_raster.h's or mesh_lens_raster.h's, shared with the host harness
// (tests/host_harness/mesh_lens_harness.cpp); what is here is the launch shape, which is mesh.hip's.
//
// mesh_rays_kernel         one thread per (camera, pixel): the Newton solve of the pixel's ray, one 8-byte store.
// mesh_lens_blocks_kernel  one thread per (camera, 8 x 8 block): the rectangle over the block's 10 x 10 pixels.
// mesh_lens_supers_kernel  one thread per (camera, superblock): the join of its 64 block rectangles.
// mesh_lens_clear_kernel   mesh.hip's clear.
// mesh_lens_faces_kernel   mesh_faces_kernel with face_setup_lens -- a lane tests its face's box in ray space against the
//                          camera's superblock rectangles (the same address in every lane: scalar loads) and the blocks of each
//                          overlapping one -- and one 8-byte load of the pixel's ray in place of (px + 0.5 - cx, py + 0.5 - cy).
// mesh_lens_large_kernel   mesh_large_kernel on the ray map.
// mesh_lens_resolve_kernel mesh_resolve_kernel on the ray map.
//
// The pinhole path keeps kernels of its own (mesh.hip, untouched by this file): sharing them through a ray policy was not
// measured against it, and its kernels are what profiles/mesh cites.
#include "mgs_common.h"
#include "../../include/mgs_mesh_lens.h"

#define MGS_MESH_HD __host__ __device__ __forceinline__
#include "mesh_lens_raster.h"

namespace mgs {
namespace {

using namespace mesh;
static_assert(sizeof(FaceRec) == 64 && sizeof(Ray) == 8 && sizeof(Rect) == 16, "record sizes of include/mgs_mesh_lens.h");
static_assert(kModelFisheyeKb == MGS_CAMERA_FISHEYE_KB && kModelPinholeBc == MGS_CAMERA_PINHOLE_BC &&
                  kLensRowFloats == MGS_LENS_ROW_FLOATS && kNewtonSteps == MGS_MESH_LENS_NEWTON_STEPS &&
                  kSuperSide == MGS_MESH_LENS_SUPERBLOCK,
              "mesh_lens_raster.h and the public headers disagree");

constexpr unsigned kClearBlocks = 2048;

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

__global__ __launch_bounds__(kGroup) void mesh_lens_clear_kernel(size_t n_keys, unsigned long long* __restrict__ vis, int n_cams,
                                                                uint32_t* __restrict__ counters) {
  const size_t stride = (size_t)gridDim.x * kGroup, n_pairs = n_keys / 2;
  ulonglong2* vis2 = reinterpret_cast<ulonglong2*>(vis);                     // the field starts on a 256-byte boundary
  for (size_t i = (size_t)blockIdx.x * kGroup + threadIdx.x; i < n_pairs; i += stride)
    vis2[i] = make_ulonglong2(kEmptyKey, kEmptyKey);
  if (blockIdx.x == 0) {
    if (threadIdx.x == 0 && (n_keys & 1)) vis[n_keys - 1] = kEmptyKey;
    for (int c = (int)threadIdx.x; c < n_cams; c += kGroup) counters[c] = 0u;
  }
}

// block (bxi, byi) of face r's box: the lane's pixel, its ray, its key, and the minimum on the visibility buffer of camera c
__device__ __forceinline__ void walk_block(const FaceRec& r, int bxi, int byi, int lane, const Ray* __restrict__ rays, int c,
                                           int width, int height, float near_plane, float far_plane,
                                           unsigned long long* __restrict__ vis) {
  int px, py;
  uint64_t key;
  if (!block_pixel(r, bxi, byi, lane, width, height, px, py)) return;
  const size_t at = pixel_index(c, width, height, px, py);
  if (pixel_key_lens(r, rays[at], near_plane, far_plane, key)) atomicMin(vis + at, (unsigned long long)key);
}

__global__ __launch_bounds__(kGroup) void mesh_lens_faces_kernel(int V, const float* __restrict__ verts_cam, int F, int per_wave,
                                                                const int32_t* __restrict__ faces, const Ray* __restrict__ rays,
                                                                const Rect* __restrict__ blocks, const Rect* __restrict__ supers,
                                                                int width, int height, float near_plane, float far_plane,
                                                                int cull, unsigned long long* __restrict__ vis,
                                                                uint32_t* __restrict__ counters, FaceRec* __restrict__ large) {
  __shared__ FaceRec recs[kGroup];
  const int c = (int)blockIdx.y, t = (int)threadIdx.x, lane = t & (kWave - 1), base = t - lane;
  const long long f = face_of_lane((long long)blockIdx.x * (kGroup / kWave) + (t >> 6), per_wave, lane, F);
  FaceRec r;
  bool live = f >= 0 && face_setup_lens(verts_cam + vertex_index(c, V, 0), V, faces, (int)f, near_plane, blocks, supers, c, width,
                                        height, cull != 0, r);
  if (live && n_blocks(r) > kLargeBlocks) {
    const uint32_t slot = atomicAdd(&counters[c], 1u);
    if (large_slot_ok(slot, F)) large[large_index(c, F, slot)] = r;
    live = false;
  }
  if (live) recs[t] = r;
  __syncthreads();                                          // nobody has left: every thread reaches it
  unsigned long long todo = ballot(live);
  while (todo) {
    const int j = __builtin_ctzll(todo);
    todo &= todo - 1;
    const FaceRec q = recs[base + j];                       // the same address in every lane: a broadcast
    for (int byi = 0; byi < q.nby; ++byi)                   // at most kLargeBlocks blocks
      for (int bxi = 0; bxi < q.nbx; ++bxi) walk_block(q, bxi, byi, lane, rays, c, width, height, near_plane, far_plane, vis);
  }
}

__global__ __launch_bounds__(kGroup) void mesh_lens_large_kernel(int F, const Ray* __restrict__ rays, int width, int height,
                                                                float near_plane, float far_plane,
                                                                unsigned long long* __restrict__ vis,
                                                                const uint32_t* __restrict__ counters,
                                                                const FaceRec* __restrict__ large) {
  const int c = (int)blockIdx.y, t = (int)threadIdx.x, lane = t & (kWave - 1);
  const int w = (int)blockIdx.x * (kGroup / kWave) + (t >> 6);              // 0 .. kLargeWaves - 1
  const uint32_t listed = counters[c];
  const uint32_t n = listed < (uint32_t)F ? listed : (uint32_t)F;
  if (n == 0u) return;
  int offset = 0;                                                           // blocks of the faces before, modulo kLargeWaves
  for (uint32_t i0 = 0; i0 < n; i0 += kWave) {
    const uint32_t mine = i0 + (uint32_t)lane;                              // one list entry per lane
    int nb = 0;
    if (mine < n) {
      const FaceRec* p = large + large_index(c, F, mine);
      nb = p->nbx * p->nby;
    }
    int before = nb;                                                        // inclusive prefix sum over the lanes: < 2^30
    for (int d = 1; d < kWave; d <<= 1) {
      const int up = __shfl_up(before, d);
      if (lane >= d) before += up;
    }
    const int total = __shfl(before, kWave - 1);
    before -= nb;
    const int k0 = first_block_of_wave(next_offset(offset, before, kLargeWaves), w, kLargeWaves);
    unsigned long long todo = ballot(k0 < nb);                              // the entries wave w has a block of
    while (todo) {
      const int j = __builtin_ctzll(todo);
      todo &= todo - 1;
      const FaceRec q = large[large_index(c, F, i0 + (uint32_t)j)];
      const int nq = n_blocks(q);
      for (int k = __shfl(k0, j); k < nq; k += kLargeWaves) {
        int bxi, byi;
        div_mod(k, q.nbx, byi, bxi);
        walk_block(q, bxi, byi, lane, rays, c, width, height, near_plane, far_plane, vis);
      }
    }
    offset = next_offset(offset, total, kLargeWaves);
  }
}

__global__ __launch_bounds__(kGroup) void mesh_lens_resolve_kernel(int V, const float* __restrict__ verts_cam, int F,
                                                                  const int32_t* __restrict__ faces,
                                                                  const float* __restrict__ vertex_colors,
                                                                  const float* __restrict__ face_colors,
                                                                  const Ray* __restrict__ rays, int width, int height,
                                                                  int headlight, float ambient,
                                                                  const unsigned long long* __restrict__ vis,
                                                                  float* __restrict__ rgb, float* __restrict__ depth,
                                                                  int32_t* __restrict__ face_ids, float* __restrict__ normals) {
  const int c = (int)blockIdx.y;
  const long long p = (long long)blockIdx.x * kGroup + threadIdx.x;
  if (p >= (long long)width * height) return;
  const int px = (int)(p % width), py = (int)(p / width);
  const size_t at = pixel_index(c, width, height, px, py);
  const Shaded s = resolve_pixel_lens(vis[at], verts_cam + vertex_index(c, V, 0), V, faces, F, vertex_colors, face_colors,
                                      rays[at], headlight != 0, ambient);
  rgb[3 * at + 0] = s.rgb[0]; rgb[3 * at + 1] = s.rgb[1]; rgb[3 * at + 2] = s.rgb[2];
  depth[at] = s.depth;
  face_ids[at] = s.face;
  if (normals) { normals[3 * at + 0] = s.normal[0]; normals[3 * at + 1] = s.normal[1]; normals[3 * at + 2] = s.normal[2]; }
}

// ---- argument checks shared by the entry points (each returns MGS_OK or has set the error) ---------------------------------
int check_sizes(const char* fn, int n_cams, int V, int F, int width, int height) {
  MGS_REQUIRE(n_cams >= 1, "%s: n_cams %d, at least 1 needed", fn, n_cams);
  MGS_REQUIRE(V >= 1, "%s: V %d vertices, at least 1 needed", fn, V);
  MGS_REQUIRE(F >= 1, "%s: F %d faces, at least 1 needed", fn, F);
  MGS_REQUIRE(width >= 1 && width <= kMaxSide && height >= 1 && height <= kMaxSide,
              "%s: image %d x %d, each side must be in 1 .. %d", fn, width, height, kMaxSide);
  MGS_REQUIRE(n_cams <= 65535, "%s: n_cams %d is above 65535", fn, n_cams);
  return MGS_OK;
}

int check_planes(const char* fn, float near_plane, float far_plane) {
  MGS_REQUIRE(near_plane > 0.f, "%s: near_plane %g is not a positive number", fn, (double)near_plane);
  MGS_REQUIRE(far_plane >= near_plane, "%s: far_plane %g is not a number at or above near_plane %g", fn, (double)far_plane,
              (double)near_plane);
  return MGS_OK;
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

int check_workspace(const char* fn, const char* what, const void* workspace, size_t workspace_bytes, size_t need) {
  MGS_REQUIRE(workspace, "%s: %s is null", fn, what);
  MGS_REQUIRE(((uintptr_t)workspace & 255u) == 0, "%s: %s is not 256-byte aligned", fn, what);
  MGS_REQUIRE(workspace_bytes >= need, "%s: %s of %zu bytes, %zu needed", fn, what, workspace_bytes, need);
  return MGS_OK;
}

int check_links(const char* fn, int L, const float* rotations, const float* translations) {
  MGS_REQUIRE(L >= 0, "%s: L %d links is negative", fn, L);
  MGS_REQUIRE(L == 0 || (rotations && translations), "%s: %d links but rotations or translations is null", fn, L);
  return MGS_OK;
}

#define MGS_TRY(expr)        \
  do {                       \
    const int rc_ = (expr);  \
    if (rc_) return rc_;     \
  } while (0)

struct LensFields { const Ray* rays; const Rect* blocks; const Rect* supers; };
LensFields lens_fields(const void* lens_workspace, const LensLayout& l) {
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
  char* ws = static_cast<char*>(workspace);
  unsigned long long* vis = reinterpret_cast<unsigned long long*>(ws + l.vis);
  uint32_t* counters = reinterpret_cast<uint32_t*>(ws + l.counters);
  FaceRec* large = reinterpret_cast<FaceRec*>(ws + l.large);
  const LensFields lf = lens_fields(lens_workspace, ll);
  hipStream_t s = (hipStream_t)stream;
  const size_t n_keys = (size_t)n_cams * (size_t)height * (size_t)width;
  const size_t clear_groups = (n_keys / 2 + kGroup - 1) / kGroup;
  const dim3 block(kGroup);
  hipLaunchKernelGGL(mesh_lens_clear_kernel,
                     dim3(clear_groups < kClearBlocks ? (unsigned)(clear_groups ? clear_groups : 1) : kClearBlocks), block, 0, s,
                     n_keys, vis, n_cams, counters);
  MGS_TRY(check_launch("mesh_raster_lens (clear)"));
  const int per_wave = faces_per_wave(F);
  const long long face_waves = ((long long)F + per_wave - 1) / per_wave;                // <= 2^25
  hipLaunchKernelGGL(mesh_lens_faces_kernel,
                     dim3((unsigned)((face_waves + kGroup / kWave - 1) / (kGroup / kWave)), (unsigned)n_cams), block, 0, s, V,
                     verts_cam, F, per_wave, faces, lf.rays, lf.blocks, lf.supers, width, height, near_plane, far_plane,
                     cull_backfaces, vis, counters, large);
  MGS_TRY(check_launch("mesh_raster_lens (faces)"));
  hipLaunchKernelGGL(mesh_lens_large_kernel, dim3(kLargeWaves / (kGroup / kWave), (unsigned)n_cams), block, 0, s, F, lf.rays,
                     width, height, near_plane, far_plane, vis, (const uint32_t*)counters, (const FaceRec*)large);
  return check_launch("mesh_raster_lens (large faces)");
}

extern "C" int mgs_mesh_resolve_lens(int n_cams, int V, const float* verts_cam, int F, const int32_t* faces,
                                     const float* vertex_colors, const float* face_colors, int camera_model,
                                     const float* lens_rows, int width, int height, int headlight, float ambient,
                                     const void* workspace, size_t workspace_bytes, const void* lens_workspace,
                                     size_t lens_workspace_bytes, float* rgb, float* depth, int32_t* face_ids, float* normals,
                                     mgs_stream_t stream) {
  MGS_TRY(check_sizes("mesh_resolve_lens", n_cams, V, F, width, height));
  MGS_REQUIRE(ambient >= 0.f && ambient <= 1.f, "mesh_resolve_lens: ambient %g is outside 0 .. 1", (double)ambient);
  MGS_TRY(check_model("mesh_resolve_lens", camera_model, lens_rows));
  MGS_REQUIRE(verts_cam && faces, "mesh_resolve_lens: verts_cam or faces is null");
  MGS_REQUIRE(rgb && depth && face_ids, "mesh_resolve_lens: an output (rgb, depth, face_ids) is null");
  const Layout l = workspace_layout(n_cams, F, width, height);
  const LensLayout ll = lens_layout(n_cams, width, height);
  MGS_TRY(check_workspace("mesh_resolve_lens", "workspace", workspace, workspace_bytes, l.total));
  MGS_TRY(check_workspace("mesh_resolve_lens", "lens_workspace", lens_workspace, lens_workspace_bytes, ll.total));
  const unsigned long long* vis = reinterpret_cast<const unsigned long long*>(static_cast<const char*>(workspace) + l.vis);
  const LensFields lf = lens_fields(lens_workspace, ll);
  const size_t n_px = (size_t)width * (size_t)height;                        // <= 16368^2 < 2^28
  hipLaunchKernelGGL(mesh_lens_resolve_kernel, dim3((unsigned)((n_px + kGroup - 1) / kGroup), (unsigned)n_cams), dim3(kGroup), 0,
                     (hipStream_t)stream, V, verts_cam, F, faces, vertex_colors, face_colors, lf.rays, width, height, headlight,
                     ambient, vis, rgb, depth, face_ids, normals);
  return check_launch("mesh_resolve_lens");
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
  MGS_REQUIRE(ambient >= 0.f && ambient <= 1.f, "rasterize_mesh_lens: ambient %g is outside 0 .. 1", (double)ambient);
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
