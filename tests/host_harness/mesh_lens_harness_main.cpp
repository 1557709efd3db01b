// The stand-alone program of the lens mesh harness (tests/host_harness/mesh_lens_harness.cpp): its own main, host code
// only, built by tests/test_mesh_lens_host.py with -fsanitize=address,undefined and run as it is on hostile inputs -- NaN and
// infinite coefficients, u_max = 0, non-finite vertices, an index equal to V, a 1 x 1 image.  Every buffer is a heap block of
// its exact size, so any index the kernels would form outside one is reported and aborts the run.
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <limits>
#include <vector>

extern "C" int mlh_rasterize(int n_cams, int V, const float* vertices, const int32_t* link_ids, int L, const float* rotations,
                             const float* translations, const float* scales, const float* viewmats, int camera_model,
                             const float* rows, int F, const int32_t* faces, const float* vertex_colors,
                             const float* face_colors, int width, int height, float near_plane, float far_plane, int cull,
                             int headlight, float ambient, const float* rays_in, int every_block, float* verts_cam, float* rgb,
                             float* depth, int32_t* face_ids, float* normals, float* rays_out, int64_t* stats,
                             int32_t* face_blocks);

namespace {

const float kNan = std::numeric_limits<float>::quiet_NaN(), kInf = std::numeric_limits<float>::infinity();

struct Scene {
  const char* name;
  int model, width, height;
  std::vector<float> row, verts;
  std::vector<int32_t> faces;
};

std::vector<float> make_row(int model, float f, float cx, float cy, std::vector<float> k, float u_max) {
  std::vector<float> r(16, 0.0f);
  r[0] = f; r[2] = cx; r[4] = f; r[5] = cy; r[8] = 1.0f;
  for (size_t i = 0; i < k.size(); ++i) r[9 + i] = k[i];
  r[model == 4 ? 14 : 13] = u_max;
  return r;
}

// covered pixels, or -1 where an output breaks the contract of an uncovered pixel
long run(const Scene& s) {
  const int V = (int)s.verts.size() / 3, F = (int)s.faces.size() / 3, W = s.width, H = s.height;
  const float view[16] = {1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1};
  std::vector<float> vc((size_t)3 * V), rgb((size_t)3 * W * H), depth((size_t)W * H), normals((size_t)3 * W * H),
      rays((size_t)2 * W * H), vcol((size_t)3 * V, 0.5f);
  std::vector<int32_t> ids((size_t)W * H), blocks((size_t)F);
  int64_t stats[2] = {0, 0};
  long covered = 0;
  for (int every = 0; every < 2; ++every) {
    if (mlh_rasterize(1, V, s.verts.data(), nullptr, 0, nullptr, nullptr, nullptr, view, s.model, s.row.data(), F, s.faces.data(),
                      vcol.data(), nullptr, W, H, 0.05f, 1e10f, 0, 1, 0.3f, nullptr, every, vc.data(), rgb.data(), depth.data(),
                      ids.data(), normals.data(), rays.data(), stats, blocks.data()))
      return -1;
    covered = 0;
    for (size_t p = 0; p < (size_t)W * H; ++p) {
      const bool has_ray = rays[2 * p] == rays[2 * p] && rays[2 * p + 1] == rays[2 * p + 1];
      if (ids[p] >= F || ids[p] < -1) return -1;
      if (ids[p] < 0 && (depth[p] != 0.0f || rgb[3 * p] != 0.0f)) return -1;
      if (ids[p] >= 0 && (!has_ray || !(depth[p] > 0.0f))) return -1;
      covered += ids[p] >= 0;
    }
  }
  return covered;
}

}  // namespace

int main() {
  const std::vector<float> tri = {-0.5f, -0.4f, 2.0f, 0.6f, -0.3f, 2.5f, 0.1f, 0.5f, 3.0f};
  const std::vector<int32_t> one = {0, 1, 2};
  std::vector<Scene> scenes;
  for (int model : {4, 3}) {
    const std::vector<float> mild = model == 4 ? std::vector<float>{-0.12f, 0.03f, 0.002f, -0.0015f, -0.004f}
                                               : std::vector<float>{-0.04f, 0.012f, -0.006f, 0.0015f};
    const float um = model == 4 ? 4.2989f : 2.4674f;
    scenes.push_back({"honest", model, 37, 29, make_row(model, 30.0f, 18.5f, 14.5f, mild, um), tri, one});
    scenes.push_back({"nan coefficients", model, 37, 29, make_row(model, 30.0f, 18.5f, 14.5f, {kNan, 0.1f, kNan, 0.0f}, um), tri, one});
    scenes.push_back({"infinite coefficients", model, 37, 29, make_row(model, 30.0f, 18.5f, 14.5f, {kInf, -kInf, 0.0f, kInf}, um), tri, one});
    scenes.push_back({"u_max = 0", model, 37, 29, make_row(model, 30.0f, 18.5f, 14.5f, mild, 0.0f), tri, one});
    scenes.push_back({"u_max = nan", model, 37, 29, make_row(model, 30.0f, 18.5f, 14.5f, mild, kNan), tri, one});
    scenes.push_back({"zero focal length", model, 37, 29, make_row(model, 0.0f, 18.5f, 14.5f, mild, um), tri, one});
    scenes.push_back({"non-finite vertices", model, 37, 29, make_row(model, 30.0f, 18.5f, 14.5f, mild, um),
                      {-0.5f, -0.4f, 2.0f, kNan, -0.3f, 2.5f, 0.1f, kInf, 3.0f, 0.3f, 0.3f, -kInf, -0.5f, -0.4f, 2.0f, 0.6f, -0.3f, 2.5f,
                       0.1f, 0.5f, 3.0f},
                      {0, 1, 2, 0, 2, 3, 4, 5, 6}});
    scenes.push_back({"an index equal to V", model, 37, 29, make_row(model, 30.0f, 18.5f, 14.5f, mild, um), tri, {0, 1, 3, 0, 1, 2, -1, 1, 2}});
    scenes.push_back({"1 x 1 image", model, 1, 1, make_row(model, 30.0f, 0.5f, 0.5f, mild, um), tri, one});
    scenes.push_back({"huge face through the eye", model, 16, 70, make_row(model, 30.0f, 8.0f, 35.0f, mild, um),
                      {-1e30f, -1e30f, 1e-30f, 1e30f, -1e30f, 2.0f, 0.0f, 1e30f, -3.0f}, one});
  }
  int bad = 0;
  long total = 0;
  for (const Scene& s : scenes) {
    const long covered = run(s);
    std::printf("%-28s model %d: %ld covered\n", s.name, s.model, covered);
    if (covered < 0) ++bad;
    const bool must_be_empty = std::strstr(s.name, "coefficients") || std::strstr(s.name, "u_max") || std::strstr(s.name, "focal");
    if (must_be_empty && covered != 0) ++bad;
    if (!std::strcmp(s.name, "honest") && covered <= 0) ++bad;
    total += covered > 0 ? covered : 0;
  }
  std::printf("mesh lens harness: %zu scenes, %ld covered, %d bad\n", scenes.size(), total, bad);
  return bad ? 1 : 0;
}
