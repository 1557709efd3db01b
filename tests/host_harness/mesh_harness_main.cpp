// A stand-alone program around tests/host_harness/mesh_harness.cpp for scripts/mesh_host_sanitize.py, which builds both with
// g++ -fsanitize=address,undefined: it reads scenes from the file named on the command line, runs each through
// mh_rasterize on heap buffers of the exact output sizes and prints one line per scene.  Host code only.
//
// A scene: int32 {magic, n_cams, V, F, L, width, height, cull, headlight, has_vertex_colors, has_face_colors, has_links},
// float {near, far, ambient}, then vertices [V,3] f32, faces [F,3] i32, link_ids [V] i32 (if has_links), rotations [L,3,3],
// translations [L,3], scales [L] (if L > 0), viewmats [C,4,4], Ks [C,3,3], vertex_colors [V,3], face_colors [F,3] (if present).
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <vector>

extern "C" int mh_rasterize(int n_cams, int V, const float* vertices, const int32_t* link_ids, int L, const float* rotations,
                            const float* translations, const float* scales, const float* viewmats, const float* Ks, int F,
                            const int32_t* faces, const float* vertex_colors, const float* face_colors, int width, int height,
                            float near_plane, float far_plane, int cull, int headlight, float ambient, float* verts_cam,
                            float* rgb, float* depth, int32_t* face_ids, float* normals, int64_t* stats);

namespace {
constexpr int32_t kMagic = 0x4853454D;

template <class T> T* read_array(FILE* f, size_t n) {
  T* p = static_cast<T*>(malloc(n ? n * sizeof(T) : 1));
  if (!p || fread(p, sizeof(T), n, f) != n) { fprintf(stderr, "short scene file\n"); exit(2); }
  return p;
}
}  // namespace

int main(int argc, char** argv) {
  if (argc != 2) { fprintf(stderr, "usage: %s scenes.bin\n", argv[0]); return 2; }
  FILE* f = fopen(argv[1], "rb");
  if (!f) { perror(argv[1]); return 2; }
  int32_t h[12];
  int n_scenes = 0;
  while (fread(h, sizeof(int32_t), 12, f) == 12) {
    if (h[0] != kMagic) { fprintf(stderr, "scene %d: bad magic\n", n_scenes); return 2; }
    const int C = h[1], V = h[2], F = h[3], L = h[4], W = h[5], H = h[6];
    float* planes = read_array<float>(f, 3);
    float* vertices = read_array<float>(f, 3 * (size_t)V);
    int32_t* faces = read_array<int32_t>(f, 3 * (size_t)F);
    int32_t* links = h[11] ? read_array<int32_t>(f, (size_t)V) : nullptr;
    float* rot = L ? read_array<float>(f, 9 * (size_t)L) : nullptr;
    float* trans = L ? read_array<float>(f, 3 * (size_t)L) : nullptr;
    float* scl = L ? read_array<float>(f, (size_t)L) : nullptr;
    float* viewmats = read_array<float>(f, 16 * (size_t)C);
    float* Ks = read_array<float>(f, 9 * (size_t)C);
    float* vcol = h[9] ? read_array<float>(f, 3 * (size_t)V) : nullptr;
    float* fcol = h[10] ? read_array<float>(f, 3 * (size_t)F) : nullptr;
    const size_t n_px = (size_t)C * H * W;
    float* verts_cam = static_cast<float*>(malloc(sizeof(float) * 3 * (size_t)C * V));
    float* rgb = static_cast<float*>(malloc(sizeof(float) * 3 * n_px));
    float* depth = static_cast<float*>(malloc(sizeof(float) * n_px));
    int32_t* ids = static_cast<int32_t*>(malloc(sizeof(int32_t) * n_px));
    float* normals = static_cast<float*>(malloc(sizeof(float) * 3 * n_px));
    std::vector<int64_t> stats(2 * (size_t)C);
    const int rc = mh_rasterize(C, V, vertices, links, L, rot, trans, scl, viewmats, Ks, F, faces, vcol, fcol, W, H, planes[0],
                                planes[1], h[7], h[8], planes[2], verts_cam, rgb, depth, ids, normals, stats.data());
    if (rc) { fprintf(stderr, "scene %d: mh_rasterize returned %d\n", n_scenes, rc); return 2; }
    size_t covered = 0;
    double sum = 0.0;
    for (size_t p = 0; p < n_px; ++p) {
      covered += ids[p] >= 0;
      sum += depth[p] + rgb[3 * p] + normals[3 * p + 2];
    }
    int64_t listed = 0, keys = 0;
    for (int c = 0; c < C; ++c) { listed += stats[2 * (size_t)c]; keys += stats[2 * (size_t)c + 1]; }
    printf("scene %2d: %d cam %5d x %5d, %6d faces, %6lld on the large-face list, %9lld keys, %8zu pixels covered, checksum %.6g\n",
           n_scenes, C, W, H, F, (long long)listed, (long long)keys, covered, sum);
    free(planes); free(vertices); free(faces); free(links); free(rot); free(trans); free(scl); free(viewmats); free(Ks);
    free(vcol); free(fcol); free(verts_cam); free(rgb); free(depth); free(ids); free(normals);
    ++n_scenes;
  }
  fclose(f);
  printf("%d scenes, no sanitizer report\n", n_scenes);
  return 0;
}
