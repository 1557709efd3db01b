// mesh.hip -- the triangle-mesh rasteriser (include/mgs_mesh.h), gfx950.  Every expression that decides an index or a value
// is mesh_raster.h's, shared with the host harness (tests/host_harness/mesh_harness.cpp); what is here is the launch shape.
//
// mesh_clear_kernel     grid-stride, 16-byte stores: the visibility buffer to all-ones, the per-camera counters to 0.
// mesh_vertices_kernel  one thread per (camera, vertex).
// mesh_faces_kernel     a wave sets up faces_per_wave(F) faces at once, one per lane (64 for a large mesh, down to 8 for a
//                       small one, so that a mesh of 25 k faces still makes 3 k waves: a wave walks its faces one after
//                       the other, and that serial walk is the kernel's critical path).  A face of more than
//                       kLargeBlocks blocks is appended to the camera's list (capacity F, slot checked).  The others go
//                       through LDS: the wave takes its live faces in turn (a ballot, lowest bit first), every lane reads
//                       the same record (a broadcast) and the wave walks the face's 8 x 8 blocks, one pixel per lane.
//                       Nobody leaves before the barrier.
// mesh_large_kernel     a fixed grid of kLargeWaves waves per camera.  Every wave walks the camera's list 64 entries at a
//                       time -- one block count per lane, a prefix sum over the lanes -- numbering the blocks of all faces
//                       through; block g is the wave's iff g mod kLargeWaves is its number, so one full-image face and a
//                       thousand middling ones are both spread evenly.  A wave fetches a face's record only where it has
//                       a block of it (a ballot).
// mesh_resolve_kernel   one thread per (camera, pixel).
//
// The visibility update is global_atomic_umin_x2 without a returned value and without a plain load in front of it: a
// load of the current key that skips the atomic where it cannot win was measured and cost 40-60 % more time in the face
// kernel (profiles/mesh/README.md): the wave then waits for the load, where the atomic is fire-and-forget.
#include "mgs_common.h"
#include "../../include/mgs_mesh.h"

#define MGS_MESH_HD __host__ __device__ __forceinline__
#include "mesh_raster.h"

namespace mgs {
namespace {

using namespace mesh;
static_assert(sizeof(FaceRec) == 64, "the large-face record is 16 dwords (include/mgs_mesh.h)");
static_assert(kLargeBlocks == MGS_MESH_LARGE_BLOCKS && kMaxSide == MGS_MESH_MAX_SIDE, "mesh_raster.h and mgs_mesh.h disagree");

constexpr unsigned kClearBlocks = 2048;

__global__ __launch_bounds__(kGroup) void mesh_clear_kernel(size_t n_keys, unsigned long long* __restrict__ vis, int n_cams,
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

// block (bxi, byi) of face r's box: the lane's pixel, its key, and the minimum on the visibility buffer of camera c
__device__ __forceinline__ void walk_block(const FaceRec& r, int bxi, int byi, int lane, Cam cam, int c, int width, int height,
                                           float near_plane, float far_plane, unsigned long long* __restrict__ vis) {
  int px, py;
  uint64_t key;
  if (block_pixel(r, bxi, byi, lane, width, height, px, py) && pixel_key(r, cam, px, py, near_plane, far_plane, key))
    atomicMin(vis + pixel_index(c, width, height, px, py), (unsigned long long)key);
}

__global__ __launch_bounds__(kGroup) void mesh_faces_kernel(int V, const float* __restrict__ verts_cam, int F, int per_wave,
                                                           const int32_t* __restrict__ faces, const float* __restrict__ Ks,
                                                           int width, int height, float near_plane, float far_plane, int cull,
                                                           unsigned long long* __restrict__ vis, uint32_t* __restrict__ counters,
                                                           FaceRec* __restrict__ large) {
  __shared__ FaceRec recs[kGroup];
  const int c = (int)blockIdx.y, t = (int)threadIdx.x, lane = t & (kWave - 1), base = t - lane;
  const long long f = face_of_lane((long long)blockIdx.x * (kGroup / kWave) + (t >> 6), per_wave, lane, F);
  const Cam cam = load_cam(Ks + 9 * (size_t)c);
  FaceRec r;
  bool live = f >= 0 && face_setup(verts_cam + vertex_index(c, V, 0), V, faces, (int)f, cam, near_plane, width, height, cull != 0, r);
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
      for (int bxi = 0; bxi < q.nbx; ++bxi) walk_block(q, bxi, byi, lane, cam, c, width, height, near_plane, far_plane, vis);
  }
}

__global__ __launch_bounds__(kGroup) void mesh_large_kernel(int F, const float* __restrict__ Ks, int width, int height,
                                                           float near_plane, float far_plane,
                                                           unsigned long long* __restrict__ vis,
                                                           const uint32_t* __restrict__ counters,
                                                           const FaceRec* __restrict__ large) {
  const int c = (int)blockIdx.y, t = (int)threadIdx.x, lane = t & (kWave - 1);
  const int w = (int)blockIdx.x * (kGroup / kWave) + (t >> 6);              // 0 .. kLargeWaves - 1
  const uint32_t listed = counters[c];
  const uint32_t n = listed < (uint32_t)F ? listed : (uint32_t)F;
  if (n == 0u) return;
  const Cam cam = load_cam(Ks + 9 * (size_t)c);
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
        walk_block(q, bxi, byi, lane, cam, c, width, height, near_plane, far_plane, vis);
      }
    }
    offset = next_offset(offset, total, kLargeWaves);
  }
}

__global__ __launch_bounds__(kGroup) void mesh_resolve_kernel(int V, const float* __restrict__ verts_cam, int F,
                                                             const int32_t* __restrict__ faces,
                                                             const float* __restrict__ vertex_colors,
                                                             const float* __restrict__ face_colors, const float* __restrict__ Ks,
                                                             int width, int height, int headlight, float ambient,
                                                             const unsigned long long* __restrict__ vis, float* __restrict__ rgb,
                                                             float* __restrict__ depth, int32_t* __restrict__ face_ids,
                                                             float* __restrict__ normals) {
  const int c = (int)blockIdx.y;
  const long long p = (long long)blockIdx.x * kGroup + threadIdx.x;
  if (p >= (long long)width * height) return;
  const int px = (int)(p % width), py = (int)(p / width);
  const size_t at = pixel_index(c, width, height, px, py);
  const Shaded s = resolve_pixel(vis[at], verts_cam + vertex_index(c, V, 0), V, faces, F, vertex_colors, face_colors,
                                 load_cam(Ks + 9 * (size_t)c), px, py, headlight != 0, ambient);
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

int check_workspace(const char* fn, const void* workspace, size_t workspace_bytes, const Layout& l) {
  MGS_REQUIRE(workspace, "%s: workspace is null", fn);
  MGS_REQUIRE(((uintptr_t)workspace & 255u) == 0, "%s: workspace is not 256-byte aligned", fn);
  MGS_REQUIRE(workspace_bytes >= l.total, "%s: workspace of %zu bytes, %zu needed", fn, workspace_bytes, l.total);
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
  MGS_TRY(check_workspace("mesh_raster", workspace, workspace_bytes, l));
  char* ws = static_cast<char*>(workspace);
  unsigned long long* vis = reinterpret_cast<unsigned long long*>(ws + l.vis);
  uint32_t* counters = reinterpret_cast<uint32_t*>(ws + l.counters);
  FaceRec* large = reinterpret_cast<FaceRec*>(ws + l.large);
  hipStream_t s = (hipStream_t)stream;
  const size_t n_keys = (size_t)n_cams * (size_t)height * (size_t)width;
  const size_t clear_groups = (n_keys / 2 + kGroup - 1) / kGroup;
  const dim3 block(kGroup);
  hipLaunchKernelGGL(mesh_clear_kernel, dim3(clear_groups < kClearBlocks ? (unsigned)(clear_groups ? clear_groups : 1) : kClearBlocks),
                     block, 0, s, n_keys, vis, n_cams, counters);
  MGS_TRY(check_launch("mesh_raster (clear)"));
  const int per_wave = faces_per_wave(F);
  const long long face_waves = ((long long)F + per_wave - 1) / per_wave;                // <= 2^25
  hipLaunchKernelGGL(mesh_faces_kernel, dim3((unsigned)((face_waves + kGroup / kWave - 1) / (kGroup / kWave)), (unsigned)n_cams),
                     block, 0, s, V, verts_cam, F, per_wave, faces, Ks, width, height, near_plane, far_plane, cull_backfaces, vis,
                     counters, large);
  MGS_TRY(check_launch("mesh_raster (faces)"));
  hipLaunchKernelGGL(mesh_large_kernel, dim3(kLargeWaves / (kGroup / kWave), (unsigned)n_cams), block, 0, s, F, Ks, width, height,
                     near_plane, far_plane, vis, (const uint32_t*)counters, (const FaceRec*)large);
  return check_launch("mesh_raster (large faces)");
}

extern "C" int mgs_mesh_resolve(int n_cams, int V, const float* verts_cam, int F, const int32_t* faces,
                                const float* vertex_colors, const float* face_colors, const float* Ks, int width, int height,
                                int headlight, float ambient, const void* workspace, size_t workspace_bytes, float* rgb,
                                float* depth, int32_t* face_ids, float* normals, mgs_stream_t stream) {
  MGS_TRY(check_sizes("mesh_resolve", n_cams, V, F, width, height));
  MGS_REQUIRE(ambient >= 0.f && ambient <= 1.f, "mesh_resolve: ambient %g is outside 0 .. 1", (double)ambient);
  MGS_REQUIRE(verts_cam && faces && Ks, "mesh_resolve: verts_cam, faces or Ks is null");
  MGS_REQUIRE(rgb && depth && face_ids, "mesh_resolve: an output (rgb, depth, face_ids) is null");
  const Layout l = workspace_layout(n_cams, F, width, height);
  MGS_TRY(check_workspace("mesh_resolve", workspace, workspace_bytes, l));
  const unsigned long long* vis = reinterpret_cast<const unsigned long long*>(static_cast<const char*>(workspace) + l.vis);
  const size_t n_px = (size_t)width * (size_t)height;                        // <= 16368^2 < 2^28
  hipLaunchKernelGGL(mesh_resolve_kernel, dim3((unsigned)((n_px + kGroup - 1) / kGroup), (unsigned)n_cams), dim3(kGroup), 0,
                     (hipStream_t)stream, V, verts_cam, F, faces, vertex_colors, face_colors, Ks, width, height, headlight,
                     ambient, vis, rgb, depth, face_ids, normals);
  return check_launch("mesh_resolve");
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
  MGS_REQUIRE(ambient >= 0.f && ambient <= 1.f, "rasterize_mesh: ambient %g is outside 0 .. 1", (double)ambient);
  MGS_REQUIRE(vertices && viewmats && Ks && faces, "rasterize_mesh: vertices, viewmats, Ks or faces is null");
  MGS_REQUIRE(verts_cam && rgb && depth && face_ids, "rasterize_mesh: an output (verts_cam, rgb, depth, face_ids) is null");
  MGS_TRY(check_workspace("rasterize_mesh", workspace, workspace_bytes, workspace_layout(n_cams, F, width, height)));
  MGS_TRY(mgs_mesh_vertices(n_cams, V, vertices, link_ids, L, rotations, translations, scales, viewmats, verts_cam, stream));
  MGS_TRY(mgs_mesh_raster(n_cams, V, verts_cam, F, faces, Ks, width, height, near_plane, far_plane, cull_backfaces, workspace,
                          workspace_bytes, stream));
  return mgs_mesh_resolve(n_cams, V, verts_cam, F, faces, vertex_colors, face_colors, Ks, width, height, headlight, ambient,
                          workspace, workspace_bytes, rgb, depth, face_ids, normals, stream);
}
