// mesh_kernels.h -- the launch shape of the mesh rasteriser, once, for every camera the raster knows: the device code that
// mesh.hip (the pinhole, PinholeViews) and mesh_lens.hip (a lens, LensView) instantiate.  A kernel takes its cameras as the
// three __restrict__ pointers of a `Views` (mesh_raster.h, mesh_lens_raster.h; v0, v1, v2 below) and puts them together
// with Views::from: camera(c) is the view of camera c, and the view answers where the planes are set up, what a face's box
// is and what a pixel's ray is.  Every expression that decides an index or a value is the arithmetic headers', shared with
// the host walk (tests/host_harness/mesh_walk.h).
//
// mesh_clear_kernel          grid-stride, 16-byte stores: the visibility buffer to all-ones, the per-camera counters to 0.
// mesh_faces_kernel<Views>   a wave sets up faces_per_wave(F) faces at once, one per lane (64 for a large mesh, down to 8 for
//                            a small one, so that a mesh of 25 k faces still makes 3 k waves: a wave walks its faces one
//                            after the other, and that serial walk is the kernel's critical path).  A face of more than
//                            kLargeBlocks blocks is appended to the camera's list (capacity F, slot checked).  The others
//                            go through LDS: the wave takes its live faces in turn (a ballot, lowest bit first), every lane
//                            reads the same record (a broadcast) and the wave walks the face's 8 x 8 blocks, one pixel per
//                            lane.  Nobody leaves before the barrier.
// mesh_large_kernel<Views>   a fixed grid of kLargeWaves waves per camera.  Every wave walks the camera's list 64 entries at
//                            a time -- one block count per lane, a prefix sum over the lanes -- numbering the blocks of all
//                            faces through; block g is the wave's iff g mod kLargeWaves is its number, so one full-image
//                            face and a thousand middling ones are both spread evenly.  A wave fetches a face's record only
//                            where it has a block of it (a ballot).
// mesh_resolve_kernel<Views> one thread per (camera, pixel).
//
// The visibility update is global_atomic_umin_x2 without a returned value and without a plain load in front of it: a
// load of the current key that skips the atomic where it cannot win was measured and cost 40-60 % more time in the face
// kernel (profiles/mesh/README.md): the wave then waits for the load, where the atomic is fire-and-forget.
#ifndef MGS_MESH_KERNELS_H_
#define MGS_MESH_KERNELS_H_

#include "mgs_common.h"
#include "mesh_checks.h"
#include "mesh_raster.h"

namespace mgs {
namespace {                                   // one text, a copy with internal linkage in each translation unit

using namespace mesh;
static_assert(sizeof(FaceRec) == 64, "the large-face record is 16 dwords (include/mgs_mesh.h)");

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

// block (bxi, byi) of face r's box: the lane's pixel, its key, and the minimum on the visibility buffer of camera c
template <class View>
__device__ __forceinline__ void walk_block(const View& view, const FaceRec& r, int bxi, int byi, int lane, int c, int width,
                                           int height, float near_plane, float far_plane,
                                           unsigned long long* __restrict__ vis) {
  int px, py;
  uint64_t key;
  if (!block_pixel(r, bxi, byi, lane, width, height, px, py)) return;
  const size_t at = pixel_index(c, width, height, px, py);
  if (pixel_key(view, r, at, px, py, near_plane, far_plane, key)) atomicMin(vis + at, (unsigned long long)key);
}

template <class Views>
__global__ __launch_bounds__(kGroup) void mesh_faces_kernel(const typename Views::P0* __restrict__ v0,
                                                           const typename Views::P1* __restrict__ v1,
                                                           const typename Views::P2* __restrict__ v2, int V,
                                                           const float* __restrict__ verts_cam, int F, int per_wave,
                                                           const int32_t* __restrict__ faces, int width, int height,
                                                           float near_plane, float far_plane, int cull,
                                                           unsigned long long* __restrict__ vis, uint32_t* __restrict__ counters,
                                                           FaceRec* __restrict__ large) {
  __shared__ FaceRec recs[kGroup];
  const int c = (int)blockIdx.y, t = (int)threadIdx.x, lane = t & (kWave - 1), base = t - lane;
  const long long f = face_of_lane((long long)blockIdx.x * (kGroup / kWave) + (t >> 6), per_wave, lane, F);
  const auto view = Views::from(v0, v1, v2).camera(c);
  FaceRec r;
  bool live = f >= 0 && face_setup(view, verts_cam + vertex_index(c, V, 0), V, faces, (int)f, near_plane, c, width, height,
                                   cull != 0, r);
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
      for (int bxi = 0; bxi < q.nbx; ++bxi) walk_block(view, q, bxi, byi, lane, c, width, height, near_plane, far_plane, vis);
  }
}

template <class Views>
__global__ __launch_bounds__(kGroup) void mesh_large_kernel(const typename Views::P0* __restrict__ v0,
                                                           const typename Views::P1* __restrict__ v1,
                                                           const typename Views::P2* __restrict__ v2, int F, int width, int height,
                                                           float near_plane, float far_plane,
                                                           unsigned long long* __restrict__ vis,
                                                           const uint32_t* __restrict__ counters,
                                                           const FaceRec* __restrict__ large) {
  const int c = (int)blockIdx.y, t = (int)threadIdx.x, lane = t & (kWave - 1);
  const int w = (int)blockIdx.x * (kGroup / kWave) + (t >> 6);              // 0 .. kLargeWaves - 1
  const uint32_t listed = counters[c];
  const uint32_t n = listed < (uint32_t)F ? listed : (uint32_t)F;
  if (n == 0u) return;
  const auto view = Views::from(v0, v1, v2).camera(c);
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
        walk_block(view, q, bxi, byi, lane, c, width, height, near_plane, far_plane, vis);
      }
    }
    offset = next_offset(offset, total, kLargeWaves);
  }
}

template <class Views>
__global__ __launch_bounds__(kGroup) void mesh_resolve_kernel(const typename Views::P0* __restrict__ v0,
                                                             const typename Views::P1* __restrict__ v1,
                                                             const typename Views::P2* __restrict__ v2, int V,
                                                             const float* __restrict__ verts_cam, int F,
                                                             const int32_t* __restrict__ faces,
                                                             const float* __restrict__ vertex_colors,
                                                             const float* __restrict__ face_colors, int width, int height,
                                                             int headlight, float ambient,
                                                             const unsigned long long* __restrict__ vis, float* __restrict__ rgb,
                                                             float* __restrict__ depth, int32_t* __restrict__ face_ids,
                                                             float* __restrict__ normals) {
  const int c = (int)blockIdx.y;
  const long long p = (long long)blockIdx.x * kGroup + threadIdx.x;
  if (p >= (long long)width * height) return;
  const int px = (int)(p % width), py = (int)(p / width);
  const size_t at = pixel_index(c, width, height, px, py);
  store_shaded(resolve_pixel(Views::from(v0, v1, v2).camera(c), vis[at], verts_cam + vertex_index(c, V, 0), V, faces, F, vertex_colors,
                             face_colors, at, px, py, headlight != 0, ambient),
               at, rgb, depth, face_ids, normals);
}

inline int check_stage(const char* fn, const char* stage) {
  const hipError_t e = hipGetLastError();
  if (e != hipSuccess) return set_error((int)e, "%s (%s): launch failed: %s", fn, stage, hipGetErrorString(e));
  return MGS_OK;
}

// The raster stage for the cameras of `views`: clear, then the faces, then the large faces, on the workspace laid out by l.
// The caller has checked every argument.
template <class Views>
int launch_raster(const char* fn, Views views, int n_cams, int V, const float* verts_cam, int F, const int32_t* faces, int width,
                  int height, float near_plane, float far_plane, int cull_backfaces, void* workspace, const Layout& l,
                  hipStream_t s) {
  char* ws = static_cast<char*>(workspace);
  unsigned long long* vis = reinterpret_cast<unsigned long long*>(ws + l.vis);
  uint32_t* counters = reinterpret_cast<uint32_t*>(ws + l.counters);
  FaceRec* large = reinterpret_cast<FaceRec*>(ws + l.large);
  const size_t n_keys = (size_t)n_cams * (size_t)height * (size_t)width;
  const size_t clear_groups = (n_keys / 2 + kGroup - 1) / kGroup;
  const int per_wave = faces_per_wave(F);
  const long long face_waves = ((long long)F + per_wave - 1) / per_wave;                // <= 2^25
  const dim3 block(kGroup), face_grid((unsigned)((face_waves + kGroup / kWave - 1) / (kGroup / kWave)), (unsigned)n_cams);
  hipLaunchKernelGGL(mesh_clear_kernel, dim3(clear_groups < kClearBlocks ? (unsigned)(clear_groups ? clear_groups : 1) : kClearBlocks),
                     block, 0, s, n_keys, vis, n_cams, counters);
  MGS_TRY(check_stage(fn, "clear"));
  hipLaunchKernelGGL((mesh_faces_kernel<Views>), face_grid, block, 0, s, views.p0(), views.p1(), views.p2(), V, verts_cam, F,
                     per_wave, faces, width, height, near_plane, far_plane, cull_backfaces, vis, counters, large);
  MGS_TRY(check_stage(fn, "faces"));
  hipLaunchKernelGGL((mesh_large_kernel<Views>), dim3(kLargeWaves / (kGroup / kWave), (unsigned)n_cams), block, 0, s, views.p0(),
                     views.p1(), views.p2(), F, width, height, near_plane, far_plane, vis, (const uint32_t*)counters,
                     (const FaceRec*)large);
  return check_stage(fn, "large faces");
}

// The resolve stage for the cameras of `views`.  The caller has checked every argument.
template <class Views>
int launch_resolve(const char* fn, Views views, int n_cams, int V, const float* verts_cam, int F, const int32_t* faces,
                   const float* vertex_colors, const float* face_colors, int width, int height, int headlight, float ambient,
                   const void* workspace, const Layout& l, float* rgb, float* depth, int32_t* face_ids, float* normals,
                   hipStream_t s) {
  const unsigned long long* vis = reinterpret_cast<const unsigned long long*>(static_cast<const char*>(workspace) + l.vis);
  const size_t n_px = (size_t)width * (size_t)height;                        // <= 16368^2 < 2^28
  hipLaunchKernelGGL((mesh_resolve_kernel<Views>), dim3((unsigned)((n_px + kGroup - 1) / kGroup), (unsigned)n_cams), dim3(kGroup), 0,
                     s, views.p0(), views.p1(), views.p2(), V, verts_cam, F, faces, vertex_colors, face_colors, width, height,
                     headlight, ambient, vis, rgb, depth, face_ids, normals);
  return check_launch(fn);
}

}  // namespace
}  // namespace mgs
#endif  // MGS_MESH_KERNELS_H_
