// tsdf.hip -- depth frames into a truncated signed distance volume, and its isosurface as a triangle mesh
// (include/mgs_tsdf.h), gfx950.
//
// tsdf_integrate_kernel (the hot path).  One thread per sample, lanes along x, ONE launch for all cameras: a sample's tsdf,
// weight and colour are loaded once, updated in registers camera by camera in the call's order, and stored once (only where
// some camera updated them), so the volume crosses HBM once per call however many views are fused.  The camera index is
// wave-uniform, so its matrices are scalar loads; every lane projects its sample (nine fmas and two divisions, nothing
// beside the frame gathers), and where no lane of the wave lands in front of the camera and inside its frame the wave skips
// the camera: a uniform branch around every memory access.  No atomics: nobody else touches a thread's sample.
//
// Extraction, marching tetrahedra on the Kuhn split (tsdf_tets.h holds the tables and the per-point logic, shared with a g++
// harness).  (a) tsdf_cells_kernel: a byte per emitted cell.  (b) tsdf_count_kernel: per grid point the 7-bit set of owned
// edges that carry a vertex, per cell its triangles; a workgroup covers kItems points, scans both counts through LDS (packed
// in one word: each stays below 2^16 inside a workgroup) and leaves 16-bit local offsets and its two sums.  (c)
// tsdf_scan_blocks_kernel, ONE workgroup: the sums become 64-bit exclusive offsets, kBlock per round with a carry, and the
// two totals.  (d) tsdf_emit_kernel: a vertex's index is its workgroup's offset + its point's local offset + its rank in the
// point's edge set, which is also how a face finds the vertices of its edges; every store is guarded by its capacity.
// Reduce-then-scan as in refine.hip; no rocPRIM.
#include "mgs_common.h"
#define MGS_TETS_HD __host__ __device__ __forceinline__
#include "tsdf_tets.h"
#include "../../include/mgs_tsdf.h"

#include <math.h>

namespace mgs {
namespace {

constexpr int kBlock = 256;
constexpr int kPerThread = 4;
constexpr int kItems = kBlock * kPerThread;      // grid points per workgroup of the count pass
constexpr uint64_t kMaxSamples = 0x7fffffffull;

struct IntegrateArgs {
  int nx, ny;
  uint32_t n;
  float ox, oy, oz, voxel, trunc, max_weight;
  float* tsdf;
  float* weight;
  float* color;
  int n_cams, height, width;
  const float* frames;
  const float* alphas;
  float alpha_min, near_plane;
  const float* viewmats;
  const float* Ks;
};

template <bool kRgbd, bool kColor>
__global__ __launch_bounds__(kBlock) void tsdf_integrate_kernel(const IntegrateArgs a) {
  const uint32_t p = blockIdx.x * (uint32_t)kBlock + threadIdx.x;
  if (p >= a.n) return;
  const uint32_t row = p / (uint32_t)a.nx;
  const int i = (int)(p - row * (uint32_t)a.nx), j = (int)(row % (uint32_t)a.ny), k = (int)(row / (uint32_t)a.ny);
  const float px = __builtin_fmaf((float)i + 0.5f, a.voxel, a.ox);
  const float py = __builtin_fmaf((float)j + 0.5f, a.voxel, a.oy);
  const float pz = __builtin_fmaf((float)k + 0.5f, a.voxel, a.oz);
  const float fw = (float)a.width, fh = (float)a.height;

  float f = a.tsdf[p], w = a.weight[p], col[3] = {0.f, 0.f, 0.f};
  if (kColor) {
#pragma unroll
    for (int c = 0; c < 3; ++c) col[c] = a.color[(size_t)c * a.n + p];
  }
  bool touched = false;
  for (int cam = 0; cam < a.n_cams; ++cam) {
    const float* V = a.viewmats + 16 * (size_t)cam;      // wave-uniform: scalar loads
    const float* K = a.Ks + 9 * (size_t)cam;
    const float qx = __builtin_fmaf(V[2], pz, __builtin_fmaf(V[1], py, __builtin_fmaf(V[0], px, V[3])));
    const float qy = __builtin_fmaf(V[6], pz, __builtin_fmaf(V[5], py, __builtin_fmaf(V[4], px, V[7])));
    const float qz = __builtin_fmaf(V[10], pz, __builtin_fmaf(V[9], py, __builtin_fmaf(V[8], px, V[11])));
    const float u = __builtin_fmaf(K[0], qx / qz, K[2]), v = __builtin_fmaf(K[4], qy / qz, K[5]);
    // in front of the camera and inside its frame (a NaN compares false); floor(u) in [0, W) is u in [0, W)
    const bool vis = qz > a.near_plane && u >= 0.f && u < fw && v >= 0.f && v < fh;
    if (ballot(vis) == 0ull) continue;                   // this camera sees none of the wave's samples
    if (!vis) continue;
    const size_t pix = ((size_t)cam * a.height + (size_t)(int)v) * a.width + (size_t)(int)u;
    const float d = kRgbd ? a.frames[4 * pix + 3] : a.frames[pix];
    const float s = d - qz;
    if (!(isfinite(d) && d > 0.f && s >= -a.trunc)) continue;
    // the alpha is gathered only by the lanes the depth lets through: most samples lie behind the surface
    if (a.alphas && !(a.alphas[pix] >= a.alpha_min)) continue;
    const float t = __builtin_fminf(1.f, s / a.trunc), w1 = w + 1.f;
    f = __builtin_fmaf(f, w, t) / w1;
    if (kColor) {
#pragma unroll
      for (int c = 0; c < 3; ++c) col[c] = __builtin_fmaf(col[c], w, a.frames[4 * pix + c]) / w1;
    }
    w = __builtin_fminf(w1, a.max_weight);
    touched = true;
  }
  if (touched) {
    a.tsdf[p] = f;
    a.weight[p] = w;
    if (kColor) {
#pragma unroll
      for (int c = 0; c < 3; ++c) a.color[(size_t)c * a.n + p] = col[c];
    }
  }
}

// ---- extraction ---------------------------------------------------------------------------------------------------------
struct ExtractLayout {
  size_t cell_flags, edge_mask, vloc, tloc, block_sums, voff, toff, total;
  uint32_t blocks;
};

ExtractLayout extract_layout(size_t n) {
  Bump b(1);
  ExtractLayout L;
  L.blocks = (uint32_t)((n + kItems - 1) / kItems);
  L.cell_flags = b.take(n);
  L.edge_mask = b.take(n);
  L.vloc = b.take(sizeof(uint16_t) * n);
  L.tloc = b.take(sizeof(uint16_t) * n);
  L.block_sums = b.take(sizeof(uint32_t) * L.blocks);
  L.voff = b.take(sizeof(uint64_t) * L.blocks);
  L.toff = b.take(sizeof(uint64_t) * L.blocks);
  L.total = b.total;
  return L;
}

struct Workspace {
  uint8_t* cell_flags;
  uint8_t* edge_mask;
  uint16_t* vloc;
  uint16_t* tloc;
  uint32_t* block_sums;      // vertices | triangles << 16 of a workgroup's kItems points
  uint64_t* voff;
  uint64_t* toff;
};

Workspace workspace_of(void* base, const ExtractLayout& L) {
  char* ws = static_cast<char*>(base);
  return Workspace{reinterpret_cast<uint8_t*>(ws + L.cell_flags), reinterpret_cast<uint8_t*>(ws + L.edge_mask),
                   reinterpret_cast<uint16_t*>(ws + L.vloc), reinterpret_cast<uint16_t*>(ws + L.tloc),
                   reinterpret_cast<uint32_t*>(ws + L.block_sums), reinterpret_cast<uint64_t*>(ws + L.voff),
                   reinterpret_cast<uint64_t*>(ws + L.toff)};
}

__device__ __forceinline__ void point_ijk(const tets::Grid& g, uint32_t p, int& i, int& j, int& k) {
  const uint32_t row = p / (uint32_t)g.nx;
  i = (int)(p - row * (uint32_t)g.nx);
  j = (int)(row % (uint32_t)g.ny);
  k = (int)(row / (uint32_t)g.ny);
}

__global__ __launch_bounds__(kBlock) void tsdf_cells_kernel(const tets::Grid g, uint32_t n, uint8_t* __restrict__ cell_flags) {
  const uint32_t p = blockIdx.x * (uint32_t)kBlock + threadIdx.x;
  if (p >= n) return;
  int i, j, k;
  point_ijk(g, p, i, j, k);
  cell_flags[p] = tets::cell_emitted(g, i, j, k, p) ? 1 : 0;
}

// Inclusive scan of one value per thread over the workgroup (Hillis-Steele through LDS).  Returns the exclusive value;
// `total` the workgroup's.  Ends with a barrier: lds may be reused at once.
template <class T> __device__ __forceinline__ T block_scan_exclusive(T v, T* lds, T& total) {
  const int t = threadIdx.x;
  lds[t] = v;
  __syncthreads();
  for (int d = 1; d < kBlock; d <<= 1) {
    T add = T();
    if (t >= d) add = lds[t - d];
    __syncthreads();
    if (t >= d) lds[t] = add + lds[t];
    __syncthreads();
  }
  const T excl = t ? lds[t - 1] : T();
  total = lds[kBlock - 1];
  __syncthreads();
  return excl;
}

__global__ __launch_bounds__(kBlock) void tsdf_count_kernel(const tets::Grid g, uint32_t n, const Workspace ws) {
  __shared__ uint32_t lds[kBlock];
  const uint32_t at = blockIdx.x * (uint32_t)kItems + threadIdx.x * (uint32_t)kPerThread;
  uint32_t counts[kPerThread], mine = 0u;      // vertices | triangles << 16
#pragma unroll
  for (int e = 0; e < kPerThread; ++e) {
    const uint32_t p = at + e;
    counts[e] = 0u;
    if (p < n) {
      int i, j, k;
      point_ijk(g, p, i, j, k);
      const int mask = tets::point_edge_mask(g, ws.cell_flags, i, j, k, p);
      ws.edge_mask[p] = (uint8_t)mask;
      const int tris = ws.cell_flags[p] ? tets::cell_triangle_count(tets::cell_inside_bits(g, p)) : 0;
      counts[e] = (uint32_t)__builtin_popcount((unsigned)mask) | ((uint32_t)tris << 16);
    }
    mine += counts[e];
  }
  uint32_t total;
  uint32_t run = block_scan_exclusive(mine, lds, total);
#pragma unroll
  for (int e = 0; e < kPerThread; ++e) {
    const uint32_t p = at + e;
    if (p < n) {
      ws.vloc[p] = (uint16_t)(run & 0xffffu);
      ws.tloc[p] = (uint16_t)(run >> 16);
    }
    run += counts[e];
  }
  if (threadIdx.x == 0) ws.block_sums[blockIdx.x] = total;
}

struct Pair64 {
  uint64_t v, t;
};
__device__ __forceinline__ Pair64 operator+(const Pair64& a, const Pair64& b) { return {a.v + b.v, a.t + b.t}; }

__global__ __launch_bounds__(kBlock) void tsdf_scan_blocks_kernel(uint32_t n_blocks, const Workspace ws,
                                                                 uint64_t* __restrict__ counts) {
  __shared__ Pair64 lds[kBlock];
  Pair64 carry{0ull, 0ull};
  for (uint32_t base = 0; base < n_blocks; base += kBlock) {
    const uint32_t b = base + threadIdx.x;
    Pair64 mine{0ull, 0ull};
    if (b < n_blocks) mine = Pair64{ws.block_sums[b] & 0xffffu, ws.block_sums[b] >> 16};
    Pair64 total;
    const Pair64 excl = block_scan_exclusive(mine, lds, total);
    if (b < n_blocks) {
      ws.voff[b] = carry.v + excl.v;
      ws.toff[b] = carry.t + excl.t;
    }
    carry = carry + total;
  }
  if (threadIdx.x == 0) {
    counts[0] = carry.v;
    counts[1] = carry.t;
  }
}

__global__ __launch_bounds__(kBlock) void tsdf_emit_kernel(const tets::Grid g, uint32_t n, const Workspace ws,
                                                          const uint64_t* __restrict__ counts, float* __restrict__ vertices,
                                                          float* __restrict__ colors, uint64_t vertex_capacity,
                                                          int32_t* __restrict__ faces, uint64_t face_capacity,
                                                          uint32_t* __restrict__ status) {
  const uint32_t p = blockIdx.x * (uint32_t)kBlock + threadIdx.x;
  if (p >= n) return;
  if (p == 0u) *status = (counts[0] > vertex_capacity || counts[1] > face_capacity) ? MGS_TSDF_STATUS_OVERFLOW : 0u;
  int i, j, k;
  point_ijk(g, p, i, j, k);
  const int mask = ws.edge_mask[p];
  if (mask) {
    uint64_t at = ws.voff[p / kItems] + ws.vloc[p];
    for (int t = 0; t < tets::kEdgeTypes; ++t) {
      if (!((mask >> t) & 1)) continue;
      if (at < vertex_capacity) {                         // never a store at or past the capacity
        float xyz[3], rgb[3] = {0.f, 0.f, 0.f};
        tets::edge_vertex(g, i, j, k, p, t, xyz, rgb);
#pragma unroll
        for (int c = 0; c < 3; ++c) {
          vertices[3 * at + c] = xyz[c];
          if (colors) colors[3 * at + c] = rgb[c];
        }
      }
      ++at;
    }
  }
  if (!ws.cell_flags[p]) return;
  const int inside = tets::cell_inside_bits(g, p);
  if (inside == 0 || inside == 255) return;
  uint64_t at = ws.toff[p / kItems] + ws.tloc[p];
  for (int tet = 0; tet < 6; ++tet) {
    int pairs[2][3];
    const int nt = tets::tet_triangles(tet, tets::tet_case(tet, inside), pairs);
    for (int tri = 0; tri < nt; ++tri, ++at) {
      if (at >= face_capacity) continue;
#pragma unroll
      for (int c = 0; c < 3; ++c) {
        const int oa = tets::tet_corner(tet, pairs[tri][c] & 3), ob = tets::tet_corner(tet, pairs[tri][c] >> 2);
        const size_t owner = p + tets::offset_step(g, oa);
        const uint64_t vid = ws.voff[owner / kItems] + ws.vloc[owner]
                             + (uint64_t)tets::bits_below(ws.edge_mask[owner], tets::type_of_offset(ob ^ oa));
        faces[3 * at + c] = (int32_t)vid;
      }
    }
  }
}

// the refusals every entry point shares; integration also reads trunc and max_weight
int check_volume(const char* fn, const mgs_tsdf_volume* vol, bool integration) {
  MGS_REQUIRE(vol, "%s: vol is null", fn);
  MGS_REQUIRE(vol->tsdf && vol->weight, "%s: vol->tsdf or vol->weight is null", fn);
  MGS_REQUIRE(vol->nx >= 1 && vol->ny >= 1 && vol->nz >= 1, "%s: dims %d x %d x %d: every dimension must be >= 1", fn, vol->nx,
              vol->ny, vol->nz);
  const uint64_t n = (uint64_t)vol->nx * (uint64_t)vol->ny * (uint64_t)vol->nz;
  MGS_REQUIRE(n <= kMaxSamples, "%s: dims %d x %d x %d are %llu samples, more than 2^31 - 1", fn, vol->nx, vol->ny, vol->nz,
              (unsigned long long)n);
  MGS_REQUIRE(isfinite(vol->voxel_size) && vol->voxel_size > 0.f, "%s: voxel_size %g is not a finite positive number", fn,
              (double)vol->voxel_size);
  MGS_REQUIRE(isfinite(vol->origin[0]) && isfinite(vol->origin[1]) && isfinite(vol->origin[2]), "%s: origin is not finite", fn);
  if (integration) {
    MGS_REQUIRE(isfinite(vol->trunc) && vol->trunc > 0.f, "%s: trunc %g is not a finite positive number", fn, (double)vol->trunc);
    MGS_REQUIRE(vol->max_weight >= 1.f, "%s: max_weight %g is not >= 1", fn, (double)vol->max_weight);
  }
  return MGS_OK;
}

tets::Grid grid_of(const mgs_tsdf_volume* vol, float level, float min_weight) {
  return tets::Grid{vol->nx, vol->ny, vol->nz, vol->tsdf, vol->weight, vol->color, vol->origin[0], vol->origin[1],
                    vol->origin[2], vol->voxel_size, level, min_weight};
}

}  // namespace
}  // namespace mgs

using namespace mgs;

extern "C" int mgs_tsdf_integrate(const mgs_tsdf_volume* vol, int n_cams, int height, int width, const float* frames,
                                  int frame_channels, const float* alphas, float alpha_min, float near_plane,
                                  const float* viewmats, const float* Ks, int camera_model, mgs_stream_t stream) {
  if (int rc = check_volume("tsdf_integrate", vol, true)) return rc;
  MGS_REQUIRE(camera_model == MGS_CAMERA_PINHOLE, "tsdf_integrate: camera_model %d: only MGS_CAMERA_PINHOLE is fused",
              camera_model);
  MGS_REQUIRE(n_cams >= 1, "tsdf_integrate: n_cams %d must be >= 1", n_cams);
  MGS_REQUIRE(height >= 1 && width >= 1, "tsdf_integrate: a frame of %d x %d", width, height);
  MGS_REQUIRE(frame_channels == 1 || frame_channels == 4, "tsdf_integrate: frame_channels %d is neither 1 nor 4",
              frame_channels);
  MGS_REQUIRE(frames, "tsdf_integrate: frames is null");
  MGS_REQUIRE(viewmats && Ks, "tsdf_integrate: viewmats or Ks is null");
  MGS_REQUIRE(!isnan(alpha_min) && !isnan(near_plane), "tsdf_integrate: alpha_min or near_plane is NaN");
  const uint32_t n = (uint32_t)((uint64_t)vol->nx * vol->ny * vol->nz);
  const IntegrateArgs a{vol->nx, vol->ny, n, vol->origin[0], vol->origin[1], vol->origin[2], vol->voxel_size, vol->trunc,
                        vol->max_weight, vol->tsdf, vol->weight, vol->color, n_cams, height, width, frames, alphas, alpha_min,
                        near_plane, viewmats, Ks};
  const dim3 grid(div_up(n, (unsigned)kBlock)), block(kBlock);
  hipStream_t s = (hipStream_t)stream;
  if (frame_channels == 4 && vol->color) hipLaunchKernelGGL((tsdf_integrate_kernel<true, true>), grid, block, 0, s, a);
  else if (frame_channels == 4) hipLaunchKernelGGL((tsdf_integrate_kernel<true, false>), grid, block, 0, s, a);
  else hipLaunchKernelGGL((tsdf_integrate_kernel<false, false>), grid, block, 0, s, a);
  return check_launch("tsdf_integrate");
}

extern "C" int mgs_tsdf_extract_count(const mgs_tsdf_volume* vol, float level, float min_weight, uint64_t* counts,
                                      void* workspace, size_t* workspace_bytes, mgs_stream_t stream) {
  if (int rc = check_volume("tsdf_extract_count", vol, false)) return rc;
  MGS_REQUIRE(isfinite(level) && isfinite(min_weight), "tsdf_extract_count: level %g or min_weight %g is not finite",
              (double)level, (double)min_weight);
  MGS_REQUIRE(workspace_bytes, "tsdf_extract_count: workspace_bytes is null");
  const uint32_t n = (uint32_t)((uint64_t)vol->nx * vol->ny * vol->nz);
  const ExtractLayout L = extract_layout(n);
  if (!workspace) {
    *workspace_bytes = L.total;
    return MGS_OK;
  }
  MGS_REQUIRE(counts, "tsdf_extract_count: counts is null");
  if (*workspace_bytes < L.total)
    return set_error(MGS_ERR_WORKSPACE_TOO_SMALL, "tsdf_extract_count: workspace of %zu bytes, %zu needed", *workspace_bytes,
                     L.total);
  const Workspace ws = workspace_of(workspace, L);
  const tets::Grid g = grid_of(vol, level, min_weight);
  hipStream_t s = (hipStream_t)stream;
  hipLaunchKernelGGL(tsdf_cells_kernel, dim3(div_up(n, (unsigned)kBlock)), dim3(kBlock), 0, s, g, n, ws.cell_flags);
  if (int rc = check_launch("tsdf_extract_count")) return rc;
  hipLaunchKernelGGL(tsdf_count_kernel, dim3(L.blocks), dim3(kBlock), 0, s, g, n, ws);
  if (int rc = check_launch("tsdf_extract_count")) return rc;
  hipLaunchKernelGGL(tsdf_scan_blocks_kernel, dim3(1), dim3(kBlock), 0, s, L.blocks, ws, counts);
  return check_launch("tsdf_extract_count");
}

extern "C" int mgs_tsdf_extract_emit(const mgs_tsdf_volume* vol, float level, float min_weight, const uint64_t* counts,
                                     const void* workspace, size_t workspace_bytes, float* vertices, float* colors,
                                     int64_t vertex_capacity, int32_t* faces, int64_t face_capacity, uint32_t* status,
                                     mgs_stream_t stream) {
  if (int rc = check_volume("tsdf_extract_emit", vol, false)) return rc;
  MGS_REQUIRE(isfinite(level) && isfinite(min_weight), "tsdf_extract_emit: level %g or min_weight %g is not finite",
              (double)level, (double)min_weight);
  MGS_REQUIRE(counts && workspace, "tsdf_extract_emit: counts or workspace is null");
  MGS_REQUIRE(vertices && faces && status, "tsdf_extract_emit: vertices, faces or status is null");
  MGS_REQUIRE(!colors || vol->color, "tsdf_extract_emit: colors asked of a volume without colour");
  MGS_REQUIRE(vertex_capacity >= 0 && vertex_capacity <= (int64_t)kMaxSamples && face_capacity >= 0 &&
                  face_capacity <= (int64_t)kMaxSamples,
              "tsdf_extract_emit: capacities %lld and %lld must lie in 0 .. 2^31 - 1", (long long)vertex_capacity,
              (long long)face_capacity);
  const uint32_t n = (uint32_t)((uint64_t)vol->nx * vol->ny * vol->nz);
  const ExtractLayout L = extract_layout(n);
  if (workspace_bytes < L.total)
    return set_error(MGS_ERR_WORKSPACE_TOO_SMALL, "tsdf_extract_emit: workspace of %zu bytes, %zu needed", workspace_bytes,
                     L.total);
  const Workspace ws = workspace_of(const_cast<void*>(workspace), L);
  hipLaunchKernelGGL(tsdf_emit_kernel, dim3(div_up(n, (unsigned)kBlock)), dim3(kBlock), 0, (hipStream_t)stream,
                     grid_of(vol, level, min_weight), n, ws, counts, vertices, colors, (uint64_t)vertex_capacity, faces,
                     (uint64_t)face_capacity, status);
  return check_launch("tsdf_extract_emit");
}
