// The isosurface extractor without a GPU: robosimgs_amd/csrc/tsdf_tets.h -- the tables and per-point logic csrc/tsdf.hip's
// kernels are made of -- walked serially on heap buffers: (a) cell bytes, (b) edge sets and triangle counts, (c) two exclusive
// scans, (d) the emit with its capacity guards.  Built as a shared library for tests/test_tsdf_host.py, or with
// -DTSDF_HARNESS_MAIN as a stand-alone program (a self-check that runs under -fsanitize=address,undefined).
#include <cmath>
#include <cstddef>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <vector>

#define MGS_TETS_HD inline
#include "../../robosimgs_amd/csrc/tsdf_tets.h"

using namespace mgs::tets;

// pairs[6]: lo | hi << 2 of triangle 0's three edges, then triangle 1's; returns the number of triangles
extern "C" int th_tet_triangles(int tet, int c, int* pairs) {
  int p[2][3] = {{0, 0, 0}, {0, 0, 0}};
  const int n = tet_triangles(tet, c, p);
  for (int t = 0; t < 2; ++t)
    for (int k = 0; k < 3; ++k) pairs[3 * t + k] = p[t][k];
  return n;
}

extern "C" void th_tables(int* corners /* [6][4] */, int* offsets /* [7] */) {
  for (int t = 0; t < 6; ++t)
    for (int l = 0; l < 4; ++l) corners[4 * t + l] = tet_corner(t, l);
  for (int t = 0; t < kEdgeTypes; ++t) offsets[t] = offset_of_type(t);
}

// The whole extraction.  counts[2]: vertices and faces found; nothing is written at or past a capacity.  Returns 1 where a
// count exceeds its capacity, else 0.
extern "C" int th_extract(int nx, int ny, int nz, const float* tsdf, const float* weight, const float* color,
                          const float* origin, float voxel, float level, float min_weight, long long vertex_capacity,
                          long long face_capacity, float* vertices, float* colors, int32_t* faces, long long* counts) {
  const Grid g{nx, ny, nz, tsdf, weight, color, origin[0], origin[1], origin[2], voxel, level, min_weight};
  const size_t n = grid_points(g);
  std::vector<uint8_t> cell(n), mask(n);
  std::vector<long long> voff(n), toff(n);
  auto walk = [&](auto&& f) {
    size_t p = 0;
    for (int k = 0; k < nz; ++k)
      for (int j = 0; j < ny; ++j)
        for (int i = 0; i < nx; ++i, ++p) f(i, j, k, p);
  };
  walk([&](int i, int j, int k, size_t p) { cell[p] = cell_emitted(g, i, j, k, p) ? 1 : 0; });
  long long nv = 0, nf = 0;
  walk([&](int i, int j, int k, size_t p) {
    mask[p] = (uint8_t)point_edge_mask(g, cell.data(), i, j, k, p);
    voff[p] = nv;
    toff[p] = nf;
    nv += bits_below(mask[p], kEdgeTypes);
    if (cell[p]) nf += cell_triangle_count(cell_inside_bits(g, p));
  });
  counts[0] = nv;
  counts[1] = nf;
  walk([&](int i, int j, int k, size_t p) {
    long long at = voff[p];
    for (int t = 0; t < kEdgeTypes; ++t) {
      if (!((mask[p] >> t) & 1)) continue;
      if (at < vertex_capacity) {
        float xyz[3], rgb[3] = {0.f, 0.f, 0.f};
        edge_vertex(g, i, j, k, p, t, xyz, rgb);
        for (int c = 0; c < 3; ++c) {
          vertices[3 * at + c] = xyz[c];
          if (colors) colors[3 * at + c] = rgb[c];
        }
      }
      ++at;
    }
    if (!cell[p]) return;
    const int inside = cell_inside_bits(g, p);
    at = toff[p];
    for (int tet = 0; tet < 6; ++tet) {
      int pairs[2][3];
      const int nt = tet_triangles(tet, tet_case(tet, inside), pairs);
      for (int tri = 0; tri < nt; ++tri, ++at) {
        if (at >= face_capacity) continue;
        for (int c = 0; c < 3; ++c) {
          const int oa = tet_corner(tet, pairs[tri][c] & 3), ob = tet_corner(tet, pairs[tri][c] >> 2);
          const size_t owner = p + offset_step(g, oa);
          faces[3 * at + c] = (int32_t)(voff[owner] + bits_below(mask[owner], type_of_offset(ob ^ oa)));
        }
      }
    }
  });
  return (nv > vertex_capacity || nf > face_capacity) ? 1 : 0;
}

#ifdef TSDF_HARNESS_MAIN
// Self-check on volumes with weight holes and values exactly on the level: every face names an emitted vertex, every vertex
// is named, a second run with short capacities leaves the words behind them alone.
int main() {
  unsigned seed = 12345u;
  auto rnd = [&]() { seed = seed * 1664525u + 1013904223u; return (float)(seed >> 8) / 16777216.f; };
  int fails = 0;
  for (int round = 0; round < 4; ++round) {
    const int nx = 9 + round, ny = 8, nz = 7 - round;
    const size_t n = (size_t)nx * ny * nz;
    std::vector<float> f(n), w(n), col(3 * n);
    for (size_t p = 0; p < n; ++p) {
      f[p] = 2.f * rnd() - 1.f;
      if (round >= 1 && rnd() < 0.2f) f[p] = 0.f;             // exactly on the level
      w[p] = (round >= 2 && rnd() < 0.1f) ? 0.f : 1.f;        // weight holes
    }
    for (float& c : col) c = rnd();
    const float origin[3] = {-0.3f, 0.1f, 2.f};
    long long counts[2] = {0, 0};
    th_extract(nx, ny, nz, f.data(), w.data(), col.data(), origin, 0.05f, 0.f, 1.f, 0, 0, nullptr, nullptr, nullptr, counts);
    const long long V = counts[0], F = counts[1];
    std::vector<float> v(3 * V), c(3 * V);
    std::vector<int32_t> faces(3 * F);
    const int over = th_extract(nx, ny, nz, f.data(), w.data(), col.data(), origin, 0.05f, 0.f, 1.f, V, F, v.data(), c.data(),
                                faces.data(), counts);
    std::vector<char> named(V, 0);
    for (int32_t id : faces) {
      if (id < 0 || id >= V) ++fails;
      else named[id] = 1;
    }
    for (char x : named) fails += x ? 0 : 1;
    for (float x : v) fails += std::isfinite(x) ? 0 : 1;
    fails += over;
    // exactly sized heap blocks of short capacities: the sanitizer sees any store past them
    const long long cv = V / 2, cf = F / 3;
    std::vector<float> v2(3 * cv), c2(3 * cv);
    std::vector<int32_t> f2(3 * cf);
    fails += th_extract(nx, ny, nz, f.data(), w.data(), col.data(), origin, 0.05f, 0.f, 1.f, cv, cf, v2.data(), c2.data(),
                        f2.data(), counts) == 1 ? 0 : 1;
    for (size_t e = 0; e < v2.size(); ++e) fails += v2[e] == v[e] ? 0 : 1;
    for (size_t e = 0; e < f2.size(); ++e) fails += f2[e] == faces[e] ? 0 : 1;
    std::printf("round %d: %lld vertices, %lld faces\n", round, V, F);
  }
  for (int tet = 0; tet < 6; ++tet)
    for (int c = 0; c < 16; ++c) {
      int pairs[6];
      fails += th_tet_triangles(tet, c, pairs) == case_triangles(c) ? 0 : 1;
    }
  std::printf(fails ? "FAILED: %d\n" : "OK\n", fails);
  return fails ? 1 : 0;
}
#endif
