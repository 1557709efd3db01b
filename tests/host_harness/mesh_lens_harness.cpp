// Host build (g++) of the mesh rasteriser under a lens: robosimgs_amd/csrc/mesh_lens_raster.h over mesh_raster.h.  The
// launches of csrc/mesh_lens.hip are walked serially -- workgroup by workgroup, wave by wave, lane by lane -- with the
// headers' own index expressions, on heap buffers of exactly the sizes include/mgs_mesh_lens.h and include/mgs_mesh.h give
// the workspace fields and the outputs, so that an address sanitizer sees every index the kernels would form.  Test-only:
// never linked into libmgs.so.
#include <cmath>
#include <cstddef>
#include <cstdint>
#include <cstdlib>
#include <cstring>
#include <vector>

#define MGS_MESH_HD inline
#include "../../robosimgs_amd/csrc/mesh_lens_raster.h"

using namespace mgs::mesh;

namespace {

// mesh_lens.hip's walk_block: the minimum on the visibility buffer
void walk_block(const FaceRec& r, int bxi, int byi, int lane, const Ray* rays, int c, int width, int height, float near_plane,
                float far_plane, uint64_t* vis, int64_t& n_keys) {
  int px, py;
  uint64_t key;
  if (!block_pixel(r, bxi, byi, lane, width, height, px, py)) return;
  const size_t at = pixel_index(c, width, height, px, py);
  if (pixel_key_lens(r, rays[at], near_plane, far_plane, key)) {
    if (key < vis[at]) vis[at] = key;
    ++n_keys;
  }
}

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
  // the three workspace fields of mgs_mesh.h and the three of mgs_mesh_lens.h, each a heap block of its exact size
  uint64_t* vis = static_cast<uint64_t*>(malloc(vis_bytes(n_cams, width, height)));
  uint32_t* counters = static_cast<uint32_t*>(malloc(counter_bytes(n_cams)));
  FaceRec* large = static_cast<FaceRec*>(malloc(large_bytes(n_cams, F)));
  Ray* rays = static_cast<Ray*>(malloc(ray_bytes(n_cams, width, height)));
  Rect* blocks = static_cast<Rect*>(malloc(block_rect_bytes(n_cams, width, height)));
  Rect* supers = static_cast<Rect*>(malloc(super_rect_bytes(n_cams, width, height)));
  if (!vis || !counters || !large || !rays || !blocks || !supers) {
    free(vis); free(counters); free(large); free(rays); free(blocks); free(supers);
    return 1;
  }
  std::vector<int64_t> formed((size_t)n_cams, 0);
  const int nbx = blocks_of(width), nby = blocks_of(height);

  // ---- mesh_vertices_kernel
  for (int c = 0; c < n_cams; ++c)
    for (int v = 0; v < V; ++v) {
      const float x[3] = {vertices[3 * (size_t)v + 0], vertices[3 * (size_t)v + 1], vertices[3 * (size_t)v + 2]};
      float cam[3];
      vertex_to_camera(x, link_ids ? link_ids[v] : -1, L, rotations, translations, scales, viewmats + 16 * (size_t)c, cam);
      float* o = verts_cam + vertex_index(c, V, v);
      o[0] = cam[0]; o[1] = cam[1]; o[2] = cam[2];
    }
  // ---- the ray stage
  if (rays_in) memcpy(rays, rays_in, ray_bytes(n_cams, width, height));
  ray_stage(n_cams, camera_model, rows, width, height, rays, blocks, supers, rays_in == nullptr);
  if (rays_out) memcpy(rays_out, rays, ray_bytes(n_cams, width, height));
  // ---- mesh_lens_clear_kernel
  {
    const size_t n_keys = (size_t)n_cams * (size_t)height * (size_t)width, n_pairs = n_keys / 2;
    for (size_t i = 0; i < n_pairs; ++i) { vis[2 * i] = kEmptyKey; vis[2 * i + 1] = kEmptyKey; }
    if (n_keys & 1) vis[n_keys - 1] = kEmptyKey;
    for (int c = 0; c < n_cams; ++c) counters[c] = 0u;
  }
  // ---- mesh_lens_faces_kernel: workgroups of four waves, each wave setting up faces_per_wave(F) faces, one per lane
  const int per_wave = faces_per_wave(F);
  const long long face_waves = ((long long)F + per_wave - 1) / per_wave;
  const long long face_groups = (face_waves + kGroup / kWave - 1) / (kGroup / kWave);
  for (int c = 0; c < n_cams; ++c) {
    for (int f = 0; f < F && face_blocks; ++f) face_blocks[(size_t)c * F + f] = 0;
    for (long long g = 0; g < face_groups; ++g) {
      FaceRec recs[kGroup];
      bool live[kGroup];
      for (int t = 0; t < kGroup; ++t) {
        const int lane = t & (kWave - 1);
        const long long f = face_of_lane(g * (kGroup / kWave) + (t >> 6), per_wave, lane, F);
        FaceRec r;
        live[t] = f >= 0 && face_setup_lens(verts_cam + vertex_index(c, V, 0), V, faces, (int)f, near_plane, blocks, supers, c,
                                            width, height, cull != 0, r);
        if (live[t] && face_blocks) face_blocks[(size_t)c * F + f] = n_blocks(r);
        if (every_block && f >= 0) {
          // no box: the planes alone decide whether the face exists, and it walks the whole grid
          const int32_t i0 = faces[3 * (size_t)f], i1 = faces[3 * (size_t)f + 1], i2 = faces[3 * (size_t)f + 2];
          live[t] = false;
          if (index_ok(i0, V) && index_ok(i1, V) && index_ok(i2, V)) {
            const float* vc = verts_cam + vertex_index(c, V, 0);
            const Cam unit = {1.0f, 1.0f, 0.0f, 0.0f};
            r.face = (int)f; r.pad = 0;
            if (face_planes(vc + 3 * (size_t)i0, vc + 3 * (size_t)i1, vc + 3 * (size_t)i2, unit, cull != 0, r)) {
              r.bx0 = 0; r.by0 = 0; r.nbx = nbx; r.nby = nby;
              for (int byi = 0; byi < nby; ++byi)
                for (int bxi = 0; bxi < nbx; ++bxi)
                  for (int l = 0; l < kWave; ++l)
                    walk_block(r, bxi, byi, l, rays, c, width, height, near_plane, far_plane, vis, formed[(size_t)c]);
            }
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
                walk_block(q, bxi, byi, lane, rays, c, width, height, near_plane, far_plane, vis, formed[(size_t)c]);
        }
    }
  }
  // ---- mesh_lens_large_kernel: kLargeWaves waves per camera, each walking the whole list 64 entries at a time
  for (int c = 0; c < n_cams; ++c) {
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
              walk_block(q, bxi, byi, lane, rays, c, width, height, near_plane, far_plane, vis, formed[(size_t)c]);
          }
        }
        offset = next_offset(offset, total, kLargeWaves);
      }
    }
  }
  // ---- mesh_lens_resolve_kernel: one thread per (camera, pixel), the tail workgroup's threads past the image included
  const long long n_px = (long long)width * height, px_groups = (n_px + kGroup - 1) / kGroup;
  for (int c = 0; c < n_cams; ++c)
    for (long long p = 0; p < px_groups * kGroup; ++p) {
      if (p >= n_px) continue;
      const int px = (int)(p % width), py = (int)(p / width);
      const size_t at = pixel_index(c, width, height, px, py);
      const Shaded s = resolve_pixel_lens(vis[at], verts_cam + vertex_index(c, V, 0), V, faces, F, vertex_colors, face_colors,
                                          rays[at], headlight != 0, ambient);
      rgb[3 * at + 0] = s.rgb[0]; rgb[3 * at + 1] = s.rgb[1]; rgb[3 * at + 2] = s.rgb[2];
      depth[at] = s.depth;
      face_ids[at] = s.face;
      if (normals) { normals[3 * at + 0] = s.normal[0]; normals[3 * at + 1] = s.normal[1]; normals[3 * at + 2] = s.normal[2]; }
    }
  for (int c = 0; c < n_cams && stats; ++c) stats[2 * c + 1] = formed[(size_t)c];
  free(vis); free(counters); free(large); free(rays); free(blocks); free(supers);
  return 0;
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
