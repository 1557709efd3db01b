// Host build (g++) of the mesh rasteriser's arithmetic in robosimgs_amd/csrc/mesh_raster.h.  The five launches of
// csrc/mesh.hip are walked serially -- workgroup by workgroup, wave by wave, lane by lane -- with the header's own index
// expressions, on heap buffers of exactly the sizes include/mgs_mesh.h gives the workspace fields and the outputs, so that
// an address sanitizer sees every index the kernels would form.  Test-only: never linked into libmgs.so.
#include <cmath>
#include <cstddef>
#include <cstdint>
#include <cstdlib>
#include <cstring>
#include <vector>

#define MGS_MESH_HD inline
#include "../../robosimgs_amd/csrc/mesh_raster.h"

using namespace mgs::mesh;

namespace {

// mesh.hip's walk_block: the minimum on the visibility buffer
void walk_block(const FaceRec& r, int bxi, int byi, int lane, Cam cam, int c, int width, int height, float near_plane, float far_plane,
                uint64_t* vis, int64_t& n_keys) {
  int px, py;
  uint64_t key;
  if (block_pixel(r, bxi, byi, lane, width, height, px, py) && pixel_key(r, cam, px, py, near_plane, far_plane, key)) {
    uint64_t* at = vis + pixel_index(c, width, height, px, py);
    if (key < *at) *at = key;
    ++n_keys;
  }
}

}  // namespace

// stats (nullable) int64 [C,2]: the faces each camera's list received, and the keys formed for it (the (pixel, face) pairs
// that reach the visibility update: the atomics of a kernel without the plain-load test).  Returns 0, or 1 where an
// allocation failed.
extern "C" int mh_rasterize(int n_cams, int V, const float* vertices, const int32_t* link_ids, int L, const float* rotations,
                            const float* translations, const float* scales, const float* viewmats, const float* Ks, int F,
                            const int32_t* faces, const float* vertex_colors, const float* face_colors, int width, int height,
                            float near_plane, float far_plane, int cull, int headlight, float ambient, float* verts_cam,
                            float* rgb, float* depth, int32_t* face_ids, float* normals, int64_t* stats) {
  // the three workspace fields, each a heap block of its exact size
  uint64_t* vis = static_cast<uint64_t*>(malloc(vis_bytes(n_cams, width, height)));
  uint32_t* counters = static_cast<uint32_t*>(malloc(counter_bytes(n_cams)));
  FaceRec* large = static_cast<FaceRec*>(malloc(large_bytes(n_cams, F)));
  if (!vis || !counters || !large) { free(vis); free(counters); free(large); return 1; }
  std::vector<int64_t> formed((size_t)n_cams, 0);

  // ---- mesh_clear_kernel: grid-stride over pairs of keys, the odd one and the counters by workgroup 0
  {
    const size_t n_keys = (size_t)n_cams * (size_t)height * (size_t)width, n_pairs = n_keys / 2;
    for (size_t i = 0; i < n_pairs; ++i) { vis[2 * i] = kEmptyKey; vis[2 * i + 1] = kEmptyKey; }
    if (n_keys & 1) vis[n_keys - 1] = kEmptyKey;
    for (int c = 0; c < n_cams; ++c) counters[c] = 0u;
  }
  // ---- mesh_vertices_kernel
  for (int c = 0; c < n_cams; ++c)
    for (int v = 0; v < V; ++v) {
      const float x[3] = {vertices[3 * (size_t)v + 0], vertices[3 * (size_t)v + 1], vertices[3 * (size_t)v + 2]};
      float cam[3];
      vertex_to_camera(x, link_ids ? link_ids[v] : -1, L, rotations, translations, scales, viewmats + 16 * (size_t)c, cam);
      float* o = verts_cam + vertex_index(c, V, v);
      o[0] = cam[0]; o[1] = cam[1]; o[2] = cam[2];
    }
  // ---- mesh_faces_kernel: workgroups of four waves, each wave setting up faces_per_wave(F) faces, one per lane
  const int per_wave = faces_per_wave(F);
  const long long face_waves = ((long long)F + per_wave - 1) / per_wave;
  const long long face_groups = (face_waves + kGroup / kWave - 1) / (kGroup / kWave);
  for (int c = 0; c < n_cams; ++c) {
    const Cam cam = load_cam(Ks + 9 * (size_t)c);
    for (long long g = 0; g < face_groups; ++g) {
      FaceRec recs[kGroup];
      bool live[kGroup];
      for (int t = 0; t < kGroup; ++t) {
        const int lane = t & (kWave - 1);
        const long long f = face_of_lane(g * (kGroup / kWave) + (t >> 6), per_wave, lane, F);
        FaceRec r;
        live[t] = f >= 0 && face_setup(verts_cam + vertex_index(c, V, 0), V, faces, (int)f, cam, near_plane, width, height,
                                       cull != 0, r);
        if (live[t] && n_blocks(r) > kLargeBlocks) {
          const uint32_t slot = counters[c]++;
          if (large_slot_ok(slot, F)) large[large_index(c, F, slot)] = r;
          live[t] = false;
        }
        if (live[t]) recs[t] = r;
      }
      for (int base = 0; base < kGroup; base += kWave)
        for (int j = 0; j < kWave; ++j) {
          if (!live[base + j]) continue;
          const FaceRec q = recs[base + j];
          for (int byi = 0; byi < q.nby; ++byi)
            for (int bxi = 0; bxi < q.nbx; ++bxi)
              for (int lane = 0; lane < kWave; ++lane)
                walk_block(q, bxi, byi, lane, cam, c, width, height, near_plane, far_plane, vis, formed[(size_t)c]);
        }
    }
  }
  // ---- mesh_large_kernel: kLargeWaves waves per camera, each walking the whole list 64 entries at a time
  for (int c = 0; c < n_cams; ++c) {
    const Cam cam = load_cam(Ks + 9 * (size_t)c);
    const uint32_t listed = counters[c];
    const uint32_t n = listed < (uint32_t)F ? listed : (uint32_t)F;
    if (stats) stats[2 * c] = (int64_t)listed;
    for (int w = 0; w < kLargeWaves && n; ++w) {
      int offset = 0;
      for (uint32_t i0 = 0; i0 < n; i0 += kWave) {
        int nb[kWave], before[kWave], total = 0;
        for (int lane = 0; lane < kWave; ++lane) {                       // one entry per lane, then the prefix sum over the lanes
          const uint32_t mine = i0 + (uint32_t)lane;
          nb[lane] = 0;
          if (mine < n) {
            const FaceRec* p = large + large_index(c, F, mine);
            nb[lane] = p->nbx * p->nby;
          }
          before[lane] = total;
          total += nb[lane];
        }
        for (int j = 0; j < kWave; ++j) {
          const int k0 = first_block_of_wave(next_offset(offset, before[j], kLargeWaves), w, kLargeWaves);
          if (!(k0 < nb[j])) continue;
          const FaceRec q = large[large_index(c, F, i0 + (uint32_t)j)];
          const int nq = n_blocks(q);
          for (int k = k0; k < nq; k += kLargeWaves) {
            int bxi, byi;
            div_mod(k, q.nbx, byi, bxi);
            for (int lane = 0; lane < kWave; ++lane)
              walk_block(q, bxi, byi, lane, cam, c, width, height, near_plane, far_plane, vis, formed[(size_t)c]);
          }
        }
        offset = next_offset(offset, total, kLargeWaves);
      }
    }
  }
  // ---- mesh_resolve_kernel: one thread per (camera, pixel), the tail workgroup's threads past the image included
  const long long n_px = (long long)width * height, px_groups = (n_px + kGroup - 1) / kGroup;
  for (int c = 0; c < n_cams; ++c)
    for (long long p = 0; p < px_groups * kGroup; ++p) {
      if (p >= n_px) continue;
      const int px = (int)(p % width), py = (int)(p / width);
      const size_t at = pixel_index(c, width, height, px, py);
      const Shaded s = resolve_pixel(vis[at], verts_cam + vertex_index(c, V, 0), V, faces, F, vertex_colors, face_colors,
                                     load_cam(Ks + 9 * (size_t)c), px, py, headlight != 0, ambient);
      rgb[3 * at + 0] = s.rgb[0]; rgb[3 * at + 1] = s.rgb[1]; rgb[3 * at + 2] = s.rgb[2];
      depth[at] = s.depth;
      face_ids[at] = s.face;
      if (normals) { normals[3 * at + 0] = s.normal[0]; normals[3 * at + 1] = s.normal[1]; normals[3 * at + 2] = s.normal[2]; }
    }
  for (int c = 0; c < n_cams && stats; ++c) stats[2 * c + 1] = formed[(size_t)c];
  free(vis); free(counters); free(large);
  return 0;
}

// the workspace layout of include/mgs_mesh.h: out = {visibility, counters, large, total}
extern "C" void mh_workspace_layout(int n_cams, int F, int width, int height, size_t* out) {
  const Layout l = workspace_layout(n_cams, F, width, height);
  out[0] = l.vis; out[1] = l.counters; out[2] = l.large; out[3] = l.total;
}
