// The uniform grid of csrc/register.hip without a GPU: robosimgs_amd/csrc/register_grid.h -- the cell arithmetic its build
// kernels and its query kernel share -- compiled with g++ as a shared library for tests/test_register_host.py.
#include <cstdint>

#include "../../robosimgs_amd/csrc/register_grid.h"

using namespace mgs;

// grid[5]: ox oy oz h inv_h; dims[3]
extern "C" void rg_make(const float* lo, const float* hi, float max_distance, int max_cells, double* grid, int* dims) {
  const RegisterGrid g = register_grid_make(lo, hi, max_distance, max_cells);
  grid[0] = g.ox; grid[1] = g.oy; grid[2] = g.oz; grid[3] = g.h; grid[4] = g.inv_h;
  dims[0] = g.nx; dims[1] = g.ny; dims[2] = g.nz;
}

static RegisterGrid unpack(const double* grid, const int* dims) {
  RegisterGrid g;
  g.ox = grid[0]; g.oy = grid[1]; g.oz = grid[2]; g.h = grid[3]; g.inv_h = grid[4];
  g.nx = dims[0]; g.ny = dims[1]; g.nz = dims[2];
  return g;
}

// ranges[6 * i ..]: x0 x1 y0 y1 z0 z1 of query i
extern "C" void rg_query_ranges(const double* grid, const int* dims, int n, const float* pts, int* ranges) {
  const RegisterGrid g = unpack(grid, dims);
  for (int i = 0; i < n; ++i) {
    int* r = ranges + 6 * (size_t)i;
    register_query_range(g.ox, g.inv_h, g.nx, pts[3 * i + 0], r[0], r[1]);
    register_query_range(g.oy, g.inv_h, g.ny, pts[3 * i + 1], r[2], r[3]);
    register_query_range(g.oz, g.inv_h, g.nz, pts[3 * i + 2], r[4], r[5]);
  }
}

// cells[3 * j ..]: the cell coordinates of target j; linear[j]: its index in the table
extern "C" void rg_target_cells(const double* grid, const int* dims, int n, const float* pts, int* cells, int* linear) {
  const RegisterGrid g = unpack(grid, dims);
  for (int j = 0; j < n; ++j) {
    cells[3 * j + 0] = register_target_coord(g.ox, g.inv_h, g.nx, pts[3 * j + 0]);
    cells[3 * j + 1] = register_target_coord(g.oy, g.inv_h, g.ny, pts[3 * j + 1]);
    cells[3 * j + 2] = register_target_coord(g.oz, g.inv_h, g.nz, pts[3 * j + 2]);
    linear[j] = register_target_cell(g, pts[3 * j + 0], pts[3 * j + 1], pts[3 * j + 2]);
  }
}
