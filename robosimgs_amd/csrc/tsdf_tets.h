// tsdf_tets.h -- marching tetrahedra on the Kuhn split of a grid cell: the tables and the per-point / per-cell logic of the
// isosurface extractor (include/mgs_tsdf.h), shared by csrc/tsdf.hip's kernels and a g++ host harness
// (tests/host_harness/tsdf_harness.cpp), as mesh_raster.h and tile_rect.h are.
//
// The split.  Six tetrahedra share the cell's main diagonal, one per permutation pi of the axes in lexicographic order:
// corners v0 = (0,0,0), v1 = v0 + e_pi0, v2 = v1 + e_pi1, v3 = (1,1,1), as bit sets (x = 1, y = 2, z = 4) in kTetCorner.  The
// corners of a tetrahedron are nested, so every edge runs from a grid point to that point plus one of seven offsets: the
// edge's type (x, y, z, xy, xz, yz, xyz = 0..6), and it is owned by that lower point.  The split is the same in every cell, so
// neighbouring cells agree on the diagonals of their shared faces.
//
// The cases.  Bit l of a case is set iff local corner l is inside (tsdf < level).  One corner l alone on its side gives the
// triangle of the edges (l, m), m ascending; two inside corners a < b with outside corners c0 < c1 give the quad (a,c0),
// (a,c1), (b,c1), (b,c0) as the triangles (q0, q1, q2), (q0, q2, q3).  kTetWinding[n] bit `case` says that every triangle
// (A, B, C) of that pair is emitted as (A, C, B), so that (B - A) x (C - A) points towards increasing tsdf.  For one inside
// corner l the unflipped normal points away from v_l iff det[v_m - v_l] > 0, which is the parity of pi times (-1)^l; the
// table is checked exhaustively against a derivation from generic values (tests/tsdf_ref.py, tests/test_tsdf_host.py).
#ifndef MGS_TSDF_TETS_H_
#define MGS_TSDF_TETS_H_

#include <math.h>
#include <stddef.h>
#include <stdint.h>

#ifndef MGS_TETS_HD
#define MGS_TETS_HD __host__ __device__ __forceinline__
#endif

namespace mgs {
namespace tets {

constexpr int kEdgeTypes = 7;
constexpr int kMaxCellTriangles = 12;

// corners 0..3 of tetrahedron n, four bits each (corner l at bits 4l..4l+2): 0, 1 << pi0, that | 1 << pi1, 7
constexpr uint16_t kTetCorner[6] = {0x7310, 0x7510, 0x7320, 0x7620, 0x7540, 0x7640};
constexpr uint16_t kTetWinding[6] = {0x4d24, 0x32da, 0x32da, 0x4d24, 0x4d24, 0x32da};
// edge type of an offset bit set 1..7 (x y xy z xz yz xyz), three bits each from bit 3 * offset; and the offsets of the types
constexpr uint32_t kTypeOfOffset = (0u << 3) | (1u << 6) | (3u << 9) | (2u << 12) | (4u << 15) | (5u << 18) | (6u << 21);
constexpr uint32_t kOffsetOfType = 1u | (2u << 3) | (4u << 6) | (3u << 9) | (5u << 12) | (6u << 15) | (7u << 18);

MGS_TETS_HD int tet_corner(int tet, int l) { return (kTetCorner[tet] >> (4 * l)) & 7; }
MGS_TETS_HD int type_of_offset(int bits) { return (int)((kTypeOfOffset >> (3 * bits)) & 7u); }
MGS_TETS_HD int offset_of_type(int type) { return (int)((kOffsetOfType >> (3 * type)) & 7u); }
MGS_TETS_HD int popcount4(int m) { return (m & 1) + ((m >> 1) & 1) + ((m >> 2) & 1) + ((m >> 3) & 1); }
// triangles of a case: 0, 1 or 2
MGS_TETS_HD int case_triangles(int c) {
  const int n = popcount4(c);
  return n == 2 ? 2 : (n == 1 || n == 3) ? 1 : 0;
}

// The triangles of (tet, case) as emitted: pairs[t][k] = lo | hi << 2, the local corners lo < hi of the edge that carries
// corner k of triangle t.  Returns their number.
MGS_TETS_HD int tet_triangles(int tet, int c, int pairs[2][3]) {
  const int n = popcount4(c);
  if (n == 0 || n == 4) return 0;
  const bool flip = (kTetWinding[tet] >> c) & 1;
  if (n != 2) {
    const int lone_mask = n == 1 ? c : (~c & 15);
    const int l = lone_mask == 1 ? 0 : lone_mask == 2 ? 1 : lone_mask == 4 ? 2 : 3;
    int k = 0, e[3];
    for (int m = 0; m < 4; ++m)
      if (m != l) e[k++] = m < l ? (m | l << 2) : (l | m << 2);
    pairs[0][0] = e[0];
    pairs[0][1] = flip ? e[2] : e[1];
    pairs[0][2] = flip ? e[1] : e[2];
    return 1;
  }
  int in[2], out[2], ki = 0, ko = 0;
  for (int m = 0; m < 4; ++m) {
    if ((c >> m) & 1) in[ki++] = m;
    else out[ko++] = m;
  }
  int q[4];
  const int ab[4] = {in[0], in[0], in[1], in[1]}, cc[4] = {out[0], out[1], out[1], out[0]};
  for (int k = 0; k < 4; ++k) q[k] = ab[k] < cc[k] ? (ab[k] | cc[k] << 2) : (cc[k] | ab[k] << 2);
  pairs[0][0] = q[0]; pairs[0][1] = flip ? q[2] : q[1]; pairs[0][2] = flip ? q[1] : q[2];
  pairs[1][0] = q[0]; pairs[1][1] = flip ? q[3] : q[2]; pairs[1][2] = flip ? q[2] : q[3];
  return 2;
}

// ---- the volume as the extractor reads it -------------------------------------------------------------------------------
struct Grid {
  int nx, ny, nz;
  const float* tsdf;      // [nz,ny,nx]
  const float* weight;    // [nz,ny,nx]
  const float* color;     // [3,nz,ny,nx] or null
  float ox, oy, oz, voxel;
  float level, min_weight;
};

MGS_TETS_HD size_t grid_points(const Grid& g) { return (size_t)g.nx * (size_t)g.ny * (size_t)g.nz; }
// linear step of an offset bit set
MGS_TETS_HD size_t offset_step(const Grid& g, int bits) {
  return (size_t)(bits & 1) + (size_t)((bits >> 1) & 1) * (size_t)g.nx + (size_t)((bits >> 2) & 1) * (size_t)g.nx * (size_t)g.ny;
}

// (a) the cell whose lowest corner is sample (i, j, k) is emitted: it exists and its eight weights are >= min_weight
MGS_TETS_HD bool cell_emitted(const Grid& g, int i, int j, int k, size_t p) {
  if (i + 1 >= g.nx || j + 1 >= g.ny || k + 1 >= g.nz) return false;
  bool ok = true;
  for (int c = 0; c < 8; ++c) ok = ok && g.weight[p + offset_step(g, c)] >= g.min_weight;
  return ok;
}

// (b) the owned edges of sample (i, j, k) that carry a vertex, as a bit per type: the other end exists, the edge is crossed,
// and one of the cells that contain it is emitted.  The cells that contain an edge of offset o from p are p - d for every
// bit set d of the axes o leaves out.
MGS_TETS_HD int point_edge_mask(const Grid& g, const uint8_t* cell_flags, int i, int j, int k, size_t p) {
  const bool in_a = g.tsdf[p] < g.level;
  int mask = 0;
  for (int t = 0; t < kEdgeTypes; ++t) {
    const int o = offset_of_type(t);
    if (i + (o & 1) >= g.nx || j + ((o >> 1) & 1) >= g.ny || k + ((o >> 2) & 1) >= g.nz) continue;
    if ((g.tsdf[p + offset_step(g, o)] < g.level) == in_a) continue;
    bool used = false;
    for (int d = 0; d < 8; ++d) {
      if (d & o) continue;
      if (((d & 1) && i == 0) || ((d & 2) && j == 0) || ((d & 4) && k == 0)) continue;
      used = used || cell_flags[p - offset_step(g, d)] != 0;
    }
    if (used) mask |= 1 << t;
  }
  return mask;
}

// the inside bits of the eight corners of the cell at p (bit c: corner of offset bit set c)
MGS_TETS_HD int cell_inside_bits(const Grid& g, size_t p) {
  int bits = 0;
  for (int c = 0; c < 8; ++c) bits |= (g.tsdf[p + offset_step(g, c)] < g.level ? 1 : 0) << c;
  return bits;
}
MGS_TETS_HD int tet_case(int tet, int inside_bits) {
  int c = 0;
  for (int l = 0; l < 4; ++l) c |= ((inside_bits >> tet_corner(tet, l)) & 1) << l;
  return c;
}
// (b) triangles of an emitted cell, 0..12
MGS_TETS_HD int cell_triangle_count(int inside_bits) {
  int n = 0;
  for (int tet = 0; tet < 6; ++tet) n += case_triangles(tet_case(tet, inside_bits));
  return n;
}

MGS_TETS_HD int bits_below(int mask, int t) {
  int n = 0;
  for (int b = 0; b < t; ++b) n += (mask >> b) & 1;
  return n;
}

// (d) the vertex on the edge of type t owned by sample (i, j, k): position p_a + s (p_b - p_a) with s = (level - f_a) /
// (f_b - f_a), one division and one fma per coordinate; colour with the same s, clamped to [0, 1]
MGS_TETS_HD void edge_vertex(const Grid& g, int i, int j, int k, size_t p, int t, float xyz[3], float rgb[3]) {
  const int o = offset_of_type(t);
  const size_t pb = p + offset_step(g, o);
  const float fa = g.tsdf[p], fb = g.tsdf[pb];
  const float s = (g.level - fa) / (fb - fa);
  xyz[0] = fmaf(s, (o & 1) ? g.voxel : 0.f, fmaf((float)i + 0.5f, g.voxel, g.ox));
  xyz[1] = fmaf(s, (o & 2) ? g.voxel : 0.f, fmaf((float)j + 0.5f, g.voxel, g.oy));
  xyz[2] = fmaf(s, (o & 4) ? g.voxel : 0.f, fmaf((float)k + 0.5f, g.voxel, g.oz));
  if (g.color) {
    const size_t plane = grid_points(g);
    for (int c = 0; c < 3; ++c) {
      const float ca = g.color[c * plane + p], cb = g.color[c * plane + pb];
      const float v = fmaf(s, cb - ca, ca);
      rgb[c] = fminf(1.f, fmaxf(0.f, v));
    }
  }
}

}  // namespace tets
}  // namespace mgs
#endif  // MGS_TSDF_TETS_H_
