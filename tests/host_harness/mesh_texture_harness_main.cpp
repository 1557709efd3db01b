// A stand-alone program around mesh_harness.cpp and mesh_texture_harness.cpp for tests/test_mesh_texture_host.py, which
// builds the three with g++ -fsanitize=address,undefined and runs it: the hostile inputs of the textured resolve -- texture
// ids T, -7 and 2^31 - 1, uvs NaN, +-inf and +-1e30, a 1 x 1 texture, a face that crosses the near plane -- under every
// wrap mode and both filters, on heap buffers of the exact sizes.  Host code only; prints one line per scene.
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <limits>
#include <vector>

extern "C" int mh_rasterize(int n_cams, int V, const float* vertices, const int32_t* link_ids, int L, const float* rotations,
                            const float* translations, const float* scales, const float* viewmats, const float* Ks, int F,
                            const int32_t* faces, const float* vertex_colors, const float* face_colors, int width, int height,
                            float near_plane, float far_plane, int cull, int headlight, float ambient, float* verts_cam,
                            float* rgb, float* depth, int32_t* face_ids, float* normals, int64_t* stats);
extern "C" uint64_t mth_layout(int T, const int32_t* sizes, const int32_t* wraps, int32_t* descriptors);
extern "C" void mth_build_mips(int T, const int32_t* descriptors, uint32_t* texels);
extern "C" int mth_resolve(int n_cams, int V, const float* verts_cam, int F, const int32_t* faces, const float* vertex_colors,
                           const float* face_colors, const float* Ks, int width, int height, int headlight, float ambient,
                           const int32_t* face_ids_in, const float* depth_in, const float* face_uvs, const int32_t* face_textures,
                           int T, const int32_t* descriptors, const uint32_t* texels, uint64_t texel_count, int filter, float* rgb,
                           float* depth, int32_t* face_ids, float* normals);

namespace {
template <class T> T* heap(const std::vector<T>& v) {              // an exact-size heap copy: an index one past it is caught
  T* p = static_cast<T*>(malloc(v.size() * sizeof(T)));
  for (size_t i = 0; i < v.size(); ++i) p[i] = v[i];
  return p;
}
}  // namespace

int main() {
  const int W = 37, H = 29, C = 1, T = 3;
  const float inf = std::numeric_limits<float>::infinity(), nan = std::numeric_limits<float>::quiet_NaN();
  const std::vector<float> K = {33.3f, 0, 18.75f, 0, 35.4f, 14.375f, 0, 0, 1};
  const std::vector<float> view = {1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1};
  // two triangles that cover the image at z = 4 and 5, a small one in front, one that crosses the near plane
  const std::vector<float> verts = {-40, -30, 4, 40, -30, 4, 0, 50, 4,   -30, -40, 5, 30, -40, 5, 0, 60, 5,
                                    -0.5f, -0.4f, 2, 0.6f, -0.3f, 2.5f, 0.1f, 0.5f, 2.2f,   -0.5f, -0.3f, 2, 0.6f, -0.2f, 2.5f, 0.1f, 0.4f, -1};
  const std::vector<int32_t> faces = {0, 1, 2, 3, 4, 5, 6, 7, 8, 9, 10, 11};
  const int V = 12, F = 4;
  const int32_t sizes[2 * T] = {1, 1, 5, 3, 64, 32};
  const float hostile_uv[] = {nan, inf, -inf, 1e30f, -1e30f, 3.4e38f, -2.5f, 0.0f, 1.0f};
  const int32_t hostile_id[] = {T, -7, 2147483647, 0, 1, 2};
  float* vc_in = heap(verts);
  int32_t* fc = heap(faces);
  float* Kd = heap(K);
  float* vw = heap(view);
  const size_t n_px = (size_t)C * H * W;
  float* verts_cam = static_cast<float*>(malloc(sizeof(float) * 3 * (size_t)C * V));
  float* rgb0 = static_cast<float*>(malloc(sizeof(float) * 3 * n_px));
  float* depth0 = static_cast<float*>(malloc(sizeof(float) * n_px));
  int32_t* ids0 = static_cast<int32_t*>(malloc(sizeof(int32_t) * n_px));
  float* rgb = static_cast<float*>(malloc(sizeof(float) * 3 * n_px));
  float* depth = static_cast<float*>(malloc(sizeof(float) * n_px));
  int32_t* ids = static_cast<int32_t*>(malloc(sizeof(int32_t) * n_px));
  float* normals = static_cast<float*>(malloc(sizeof(float) * 3 * n_px));
  if (mh_rasterize(C, V, vc_in, nullptr, 0, nullptr, nullptr, nullptr, vw, Kd, F, fc, nullptr, nullptr, W, H, 0.5f, 1e10f, 0, 1, 0.3f,
                   verts_cam, rgb0, depth0, ids0, nullptr, nullptr)) return 2;
  int n_scenes = 0;
  for (int wrap = 0; wrap < 3; ++wrap) {
    int32_t wraps[2 * T];
    for (int t = 0; t < T; ++t) { wraps[2 * t] = (wrap + t) % 3; wraps[2 * t + 1] = (wrap + t + 1) % 3; }
    std::vector<int32_t> dv(20 * T);
    const uint64_t count = mth_layout(T, sizes, wraps, dv.data());
    if (count == 0) return 2;
    int32_t* desc = heap(dv);
    uint32_t* texels = static_cast<uint32_t*>(malloc(sizeof(uint32_t) * count));
    for (int t = 0; t < T; ++t) {                                  // level 0: a hash of the position
      const uint32_t at = (uint32_t)desc[20 * t + 4];
      for (int i = 0; i < sizes[2 * t] * sizes[2 * t + 1]; ++i) texels[at + i] = 2654435761u * (uint32_t)(i + 17 * t + 1);
    }
    mth_build_mips(T, desc, texels);
    for (int filter = 0; filter < 2; ++filter)
      for (float bad : hostile_uv)
        for (int32_t id : hostile_id) {
          std::vector<float> uv(6 * F);
          for (int i = 0; i < 6 * F; ++i) uv[i] = -2.0f + 0.37f * (float)i;
          uv[1] = bad; uv[6 + 2] = bad; uv[12 + 5] = -bad; uv[18] = bad;         // one hostile value per face
          const std::vector<int32_t> ft = {id, (int32_t)(((int64_t)id % T + T) % T), 2, id};
          float* uvp = heap(uv);
          int32_t* ftp = heap(ft);
          if (mth_resolve(C, V, verts_cam, F, fc, nullptr, nullptr, Kd, W, H, 1, 0.3f, ids0, depth0, uvp, ftp, T, desc, texels, count,
                          filter, rgb, depth, ids, normals)) return 2;
          double sum = 0.0;
          size_t bad_px = 0;
          for (size_t p = 0; p < n_px; ++p) {
            if (ids[p] != ids0[p] || depth[p] != depth0[p]) ++bad_px;
            for (int j = 0; j < 3; ++j) {
              const float x = rgb[3 * p + j];
              if (!(x >= 0.0f && x <= 1.0f)) ++bad_px;             // every defined outcome is a colour in 0 .. 1
              sum += x;
            }
          }
          if (bad_px) { fprintf(stderr, "scene %d: %zu pixels off\n", n_scenes, bad_px); return 3; }
          if (n_scenes % 27 == 0) printf("scene %3d: wrap %d filter %d id %d: checksum %.6g\n", n_scenes, wrap, filter, id, sum);
          free(uvp); free(ftp);
          ++n_scenes;
        }
    free(desc); free(texels);
  }
  free(vc_in); free(fc); free(Kd); free(vw); free(verts_cam); free(rgb0); free(depth0); free(ids0); free(rgb); free(depth);
  free(ids); free(normals);
  printf("%d scenes, no sanitizer report\n", n_scenes);
  return 0;
}
