// register_grid.h -- the cell arithmetic of register.hip's uniform grid, host and device: what the build kernels (count,
// scatter) and the query kernel both compute, defined once, and what tests/host_harness/register_grid_harness.cpp compiles
// with g++.  Plain C++ and <math.h> only.
//
// The grid covers the bounds [lo, hi] of the finite targets with cubic cells of edge h.  h starts a little above
// max_distance (kRegisterEdgeMargin) and grows by kRegisterEdgeGrowth until nx * ny * nz <= max_cells.  A coordinate maps
// to floor((x - lo) * inv_h), all in fp64: the difference of two floats is exact there, the product is monotone in x, and
// its rounding (2^-53 of a cell index below 2^21) is far inside the margin.  So two coordinates at most max_distance apart
// -- also "at most" as the fp32 difference form sees it, 2^-22 relative -- land in the same or in adjacent cells, and the 27
// cells about a query's cell hold every target within max_distance.  A query outside the bounds is clamped to two cells
// outside the grid (-2 or n + 1): its 3-cell range, cut to 0..n-1, is the outermost cell when it is within h of the grid and
// empty when it is farther.  The extent of a cell index is taken from the same expression at x = hi, so hi itself is in cell n-1.
#ifndef MGS_REGISTER_GRID_H_
#define MGS_REGISTER_GRID_H_

#include <math.h>

#if defined(__HIPCC__)
#define MGS_GRID_HD __host__ __device__ inline
#else
#define MGS_GRID_HD inline
#endif

namespace mgs {

constexpr double kRegisterEdgeMargin = 1.0 + 1.0 / 1024.0;   // h0 = max_distance * this
constexpr double kRegisterEdgeGrowth = 1.25;                 // h grows by this until the cells fit the cap

struct RegisterGrid {
  double ox, oy, oz;     // the low corner: the smallest finite target coordinate per axis
  double h, inv_h;       // cell edge and 1 / h
  int nx, ny, nz;        // cells per axis, nx * ny * nz <= the cap; x is the fastest index
};

// cells along one axis of extent `ext` (>= 0): the index of the far bound, plus one
MGS_GRID_HD double register_axis_cells(double ext, double inv_h) { return floor(ext * inv_h) + 1.0; }

// The grid of targets bounded by lo[3]..hi[3] (fp32 values, lo <= hi, all finite).  max_cells >= 1.
MGS_GRID_HD RegisterGrid register_grid_make(const float* lo, const float* hi, float max_distance, int max_cells) {
  RegisterGrid g;
  g.ox = (double)lo[0]; g.oy = (double)lo[1]; g.oz = (double)lo[2];
  const double ex = (double)hi[0] - g.ox, ey = (double)hi[1] - g.oy, ez = (double)hi[2] - g.oz;
  double h = (double)max_distance * kRegisterEdgeMargin;
  for (;;) {
    const double inv = 1.0 / h;
    const double cells = register_axis_cells(ex, inv) * register_axis_cells(ey, inv) * register_axis_cells(ez, inv);
    if (cells <= (double)max_cells) break;         // also where inv underflowed to 0 (one cell); a NaN cannot arise
    h *= kRegisterEdgeGrowth;
  }
  g.h = h;
  g.inv_h = 1.0 / h;
  g.nx = (int)register_axis_cells(ex, g.inv_h);
  g.ny = (int)register_axis_cells(ey, g.inv_h);
  g.nz = (int)register_axis_cells(ez, g.inv_h);
  return g;
}

// The cell index of coordinate x along an axis of n cells that starts at o, clamped to -2..n+1 (two cells outside).
MGS_GRID_HD int register_cell_coord(double o, double inv_h, int n, float x) {
  double t = floor(((double)x - o) * inv_h);
  t = t >= -2.0 ? t : -2.0;                         // a NaN (a query the transform sent nowhere) goes here too
  t = t > (double)n + 1.0 ? (double)n + 1.0 : t;
  return (int)t;
}

// A target's cell along an axis: inside 0..n-1 by construction, clamped so that no rounding can index outside the table.
MGS_GRID_HD int register_target_coord(double o, double inv_h, int n, float x) {
  const int c = register_cell_coord(o, inv_h, n, x);
  return c < 0 ? 0 : (c > n - 1 ? n - 1 : c);
}

// linear cell index, x fastest
MGS_GRID_HD int register_cell_index(const RegisterGrid& g, int cx, int cy, int cz) { return (cz * g.ny + cy) * g.nx + cx; }

MGS_GRID_HD int register_target_cell(const RegisterGrid& g, float x, float y, float z) {
  return register_cell_index(g, register_target_coord(g.ox, g.inv_h, g.nx, x), register_target_coord(g.oy, g.inv_h, g.ny, y),
                             register_target_coord(g.oz, g.inv_h, g.nz, z));
}

// The cells c-1..c+1 about a query's cell along one axis, cut to 0..n-1: lo > hi where the query is more than a cell outside.
MGS_GRID_HD void register_query_range(double o, double inv_h, int n, float x, int& lo, int& hi) {
  const int c = register_cell_coord(o, inv_h, n, x);
  lo = c - 1 < 0 ? 0 : c - 1;
  hi = c + 1 > n - 1 ? n - 1 : c + 1;
}

}  // namespace mgs
#endif  // MGS_REGISTER_GRID_H_
