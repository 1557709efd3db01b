// The launches of csrc/mesh_kernels.h walked serially -- workgroup by workgroup, wave by wave, lane by lane -- for a view
// (PinholeViews of mesh_raster.h, LensView of mesh_lens_raster.h), with the headers' own index expressions, on heap buffers
// of exactly the sizes include/mgs_mesh.h gives the workspace fields, so that an address sanitizer sees every index the
// kernels would form.  mesh_harness.cpp and mesh_lens_harness.cpp instantiate it.  Test-only: never linked into libmgs.so.
#ifndef MGS_TESTS_MESH_WALK_H_
#define MGS_TESTS_MESH_WALK_H_

#include <cstddef>
#include <cstdint>
#include <cstdlib>
#include <vector>

#include "../../robosimgs_amd/csrc/mesh_raster.h"

namespace mesh_walk {

using namespace mgs::mesh;

// What a test may ask beside the render.  every_block: every face that has planes walks every block of the image, through no
// box at all -- what a box may never differ from.  face_blocks (nullable) int32 [C,F]: the blocks of each face's box, 0
// where the face is dropped.
struct Extras {
  bool every_block = false;
  int32_t* face_blocks = nullptr;
};

// mesh_kernels.h's walk_block: the minimum on the visibility buffer; n_keys counts the keys formed
template <class View>
void walk_block(const View& view, const FaceRec& r, int bxi, int byi, int lane, int c, int width, int height, float near_plane,
                float far_plane, uint64_t* vis, int64_t& n_keys) {
  int px, py;
  uint64_t key;
  if (!block_pixel(r, bxi, byi, lane, width, height, px, py)) return;
  const size_t at = pixel_index(c, width, height, px, py);
  if (pixel_key(view, r, at, px, py, near_plane, far_plane, key)) {
    if (key < vis[at]) vis[at] = key;
    ++n_keys;
  }
}

// mesh.hip's mesh_vertices_kernel
inline void vertices(int n_cams, int V, const float* verts, const int32_t* link_ids, int L, const float* rotations,
                     const float* translations, const float* scales, const float* viewmats, float* verts_cam) {
  for (int c = 0; c < n_cams; ++c)
    for (int v = 0; v < V; ++v) {
      const float x[3] = {verts[3 * (size_t)v + 0], verts[3 * (size_t)v + 1], verts[3 * (size_t)v + 2]};
      float cam[3];
      vertex_to_camera(x, link_ids ? link_ids[v] : -1, L, rotations, translations, scales, viewmats + 16 * (size_t)c, cam);
      float* o = verts_cam + vertex_index(c, V, v);
      o[0] = cam[0]; o[1] = cam[1]; o[2] = cam[2];
    }
}

// The clear, faces, large and resolve launches on verts_cam.  stats (nullable) int64 [C,2]: the faces each camera's list
// received, and the keys formed for it (the (pixel, face) pairs that reach the visibility update: the atomics of a kernel
// without the plain-load test).  Returns 0, or 1 where an allocation failed.
template <class Views>
int render(const Views& views, int n_cams, int V, const float* verts_cam, int F, const int32_t* faces, const float* vertex_colors,
           const float* face_colors, int width, int height, float near_plane, float far_plane, int cull, int headlight,
           float ambient, float* rgb, float* depth, int32_t* face_ids, float* normals, int64_t* stats, const Extras& extras) {
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
  // ---- mesh_faces_kernel: workgroups of four waves, each wave setting up faces_per_wave(F) faces, one per lane
  const int per_wave = faces_per_wave(F);
  const long long face_waves = ((long long)F + per_wave - 1) / per_wave;
  const long long face_groups = (face_waves + kGroup / kWave - 1) / (kGroup / kWave);
  const int grid_x = (width + kBlockSide - 1) / kBlockSide, grid_y = (height + kBlockSide - 1) / kBlockSide;
  for (int c = 0; c < n_cams; ++c) {
    const auto view = views.camera(c);
    const float* vc = verts_cam + vertex_index(c, V, 0);
    for (int f = 0; f < F && extras.face_blocks; ++f) extras.face_blocks[(size_t)c * F + f] = 0;
    for (long long g = 0; g < face_groups; ++g) {
      FaceRec recs[kGroup];
      bool live[kGroup];
      for (int t = 0; t < kGroup; ++t) {
        const int lane = t & (kWave - 1);
        const long long f = face_of_lane(g * (kGroup / kWave) + (t >> 6), per_wave, lane, F);
        FaceRec r;
        live[t] = f >= 0 && face_setup(view, vc, V, faces, (int)f, near_plane, c, width, height, cull != 0, r);
        if (live[t] && extras.face_blocks) extras.face_blocks[(size_t)c * F + f] = n_blocks(r);
        if (extras.every_block && f >= 0) {
          // no box: the planes alone decide whether the face exists, and it walks the whole grid
          live[t] = false;
          FaceVerts fv;
          r.face = (int)f; r.pad = 0;
          if (load_face(vc, V, faces, (int)f, fv) && face_planes(fv.a, fv.b, fv.c, view.plane_cam(), cull != 0, r)) {
            r.bx0 = 0; r.by0 = 0; r.nbx = grid_x; r.nby = grid_y;
            for (int byi = 0; byi < grid_y; ++byi)
              for (int bxi = 0; bxi < grid_x; ++bxi)
                for (int l = 0; l < kWave; ++l)
                  walk_block(view, r, bxi, byi, l, c, width, height, near_plane, far_plane, vis, formed[(size_t)c]);
          }
          continue;
        }
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
                walk_block(view, q, bxi, byi, lane, c, width, height, near_plane, far_plane, vis, formed[(size_t)c]);
        }
    }
  }
  // ---- mesh_large_kernel: kLargeWaves waves per camera, each walking the whole list 64 entries at a time
  for (int c = 0; c < n_cams; ++c) {
    const auto view = views.camera(c);
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
              walk_block(view, q, bxi, byi, lane, c, width, height, near_plane, far_plane, vis, formed[(size_t)c]);
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
      store_shaded(resolve_pixel(views.camera(c), vis[at], verts_cam + vertex_index(c, V, 0), V, faces, F, vertex_colors,
                                 face_colors, at, px, py, headlight != 0, ambient),
                   at, rgb, depth, face_ids, normals);
    }
  for (int c = 0; c < n_cams && stats; ++c) stats[2 * c + 1] = formed[(size_t)c];
  free(vis); free(counters); free(large);
  return 0;
}

}  // namespace mesh_walk
#endif  // MGS_TESTS_MESH_WALK_H_
