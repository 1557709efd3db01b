// Host build (g++) of the texture arithmetic in robosimgs_amd/csrc/mesh_texture.h, beside mesh_harness.cpp (which walks the
// vertex and raster stages and is not changed): the launches of csrc/mesh_texture.hip are walked serially with the header's
// own index expressions on heap buffers of exactly the sizes include/mgs_mesh_texture.h gives them, so that an address
// sanitizer sees every index the kernels would form.  Test-only: never linked into libmgs.so.
#include <cmath>
#include <cstddef>
#include <cstdint>
#include <cstdlib>
#include <cstring>

#define MGS_MESH_HD inline
#include "../../robosimgs_amd/csrc/mesh_texture.h"

using namespace mgs::mesh;

// mgs_mesh_texture_layout: descriptors [T,20] (nullable), returns the texel count, 0 where refused
extern "C" uint64_t mth_layout(int T, const int32_t* sizes, const int32_t* wraps, int32_t* descriptors) {
  return texture_layout(T, sizes, wraps, reinterpret_cast<TexDesc*>(descriptors));
}

// mgs_mesh_build_mips: one "launch" per (texture, level), one "thread" per destination texel, the tail group's threads
// past the level included.  texels: exactly texel_count words.
extern "C" void mth_build_mips(int T, const int32_t* descriptors, uint32_t* texels) {
  const TexDesc* d = reinterpret_cast<const TexDesc*>(descriptors);
  for (int t = 0; t < T; ++t)
    for (int l = 1; l < d[t].levels; ++l) {
      const int sw = level_side(d[t].w, l - 1), sh = level_side(d[t].h, l - 1), dw = level_side(d[t].w, l), dh = level_side(d[t].h, l);
      const uint32_t* src = texels + (size_t)d[t].offset[l - 1];
      uint32_t* dst = texels + (size_t)d[t].offset[l];
      const long long n = (long long)dw * dh, groups = (n + kGroup - 1) / kGroup;
      for (long long i = 0; i < groups * kGroup; ++i) {
        if (i >= n) continue;
        dst[i] = mip_texel(src, sw, sh, (int)(i % dw), (int)(i / dw));
      }
    }
}

// mesh_resolve_textured_kernel on the winners the raster stage left: face_ids_in / depth_in [C,H,W] are the outputs of
// mh_rasterize, from which the visibility keys are put together again bit for bit (key = depth bits << 32 | face).
extern "C" int mth_resolve(int n_cams, int V, const float* verts_cam, int F, const int32_t* faces, const float* vertex_colors,
                           const float* face_colors, const float* Ks, int width, int height, int headlight, float ambient,
                           const int32_t* face_ids_in, const float* depth_in, const float* face_uvs, const int32_t* face_textures,
                           int T, const int32_t* descriptors, const uint32_t* texels, uint64_t texel_count, int filter, float* rgb,
                           float* depth, int32_t* face_ids, float* normals) {
  const size_t n_all = (size_t)n_cams * (size_t)height * (size_t)width;
  uint64_t* vis = static_cast<uint64_t*>(malloc(vis_bytes(n_cams, width, height)));
  if (!vis) return 1;
  for (size_t i = 0; i < n_all; ++i) vis[i] = face_ids_in[i] < 0 ? kEmptyKey : pack_key(depth_in[i], face_ids_in[i]);
  const TexDesc* descs = reinterpret_cast<const TexDesc*>(descriptors);
  const long long n_px = (long long)width * height, px_groups = (n_px + kGroup - 1) / kGroup;
  for (int c = 0; c < n_cams; ++c)
    for (long long p = 0; p < px_groups * kGroup; ++p) {
      const bool inside = p < n_px;
      const int px = inside ? (int)(p % width) : 0, py = inside ? (int)(p / width) : 0;
      const size_t at = pixel_index(c, width, height, px, py);
      const uint64_t key = inside ? vis[at] : kEmptyKey;
      const int32_t tid = key_texture(key, face_textures, F, T);
      const Shaded s = resolve_pixel_textured(key, verts_cam + vertex_index(c, V, 0), V, faces, F, vertex_colors, face_colors,
                                              load_cam(Ks + 9 * (size_t)c), px, py, headlight != 0, ambient, face_uvs, tid >= 0,
                                              descs + (tid >= 0 ? tid : 0), texels, texel_count, filter);
      if (inside) store_shaded(s, at, rgb, depth, face_ids, normals);
    }
  free(vis);
  return 0;
}
