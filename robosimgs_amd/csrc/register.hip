// register.hip -- point-set registration (include/mgs_register.h), gfx950: ICP whose nearest-neighbour search runs on a
// uniform grid over the target.  Nothing is read back to the host and nothing is allocated: one memset node and a linear
// chain of launches on the caller's stream.
//
// The grid, once per call (cell arithmetic: register_grid.h, shared with the query):
//   register_stats_kernel   bounds of the finite targets, the first finite source point, the count of finite sources and
//                           the "a point was non-finite" bit: per-wave reductions, then integer atomics on ordered
//                           encodings (a float orders like enc(bits));
//   register_setup_kernel   one thread: the grid (edge enlarged until the cells fit kRegisterMaxCells), T_0 and the pivots
//                           of the moments: the first finite source point and the low corner of the target's bounds (no
//                           order of the targets changes either);
//   register_count_kernel   table[1 + cell] += 1 per finite target (integer atomic);
//   register_scan_*         exclusive scan of the used cells in three launches (chunk sums, their scan, the chunks);
//   register_scatter_kernel slot = atomicAdd(table[1 + cell], 1): the targets in cell order as float4 {x, y, z, index bits}.
//                           The add turns table[1 + c] from begin(c) into begin(c + 1), so that afterwards table[c] is where
//                           cell c begins and a run of adjacent cells c0..c1 is table[c0] .. table[c1 + 1].  The order inside
//                           a cell depends on the run; no result does, because the query's minimum is over (distance bits,
//                           original index).
// Per iteration, and once more at the end:
//   register_query_kernel   one thread per source point: p' = s R p + t in fp64, rounded to fp32; the 3 x 3 x 3 cells about
//                           it as 9 runs along x; the minimum of (fp32 difference-form distance, index); the inlier test;
//                           c_i and d2_i (last pass only); the 29 fp64 sums of the inliers about the two pivots, each thread
//                           in index order, a wave by a fixed butterfly, the waves in wave order, one row per workgroup;
//   register_solve_kernel   one workgroup: the rows in index order inside eight ranges, the ranges in order, then one thread: rmse, the history row, the collinearity
//                           test (eigenvalues of both covariances, jacobi3.h), R' = argmax tr(R'^T S) (deform_shape.h's
//                           shape_rotation, which never returns a reflection), s', t', the stop rule, the new record.  In
//                           its last launch it writes result[32] instead.
// The host enqueues every iteration; a kernel of an iteration returns at once when the record's `done` word is set.
#include "mgs_common.h"
#include "deform_shape.h"
#include "register_grid.h"
#include "../../include/mgs_register.h"

#include <math.h>

namespace mgs {
namespace {

constexpr int kRegisterGroup = 256;               // G: threads of a workgroup (stats, count, scatter, scan, query)
constexpr int kRegisterMaxCells = 1 << 21;        // the cell table's capacity (128^3): 8 MiB of uint32
constexpr int kRegisterPartBlocks = 1024;         // workgroups of the query kernel, at the most (one row of sums each)
constexpr int kRegisterStatBlocks = 256;          // workgroups of the stats kernel per set, at the most
constexpr int kRegisterMoments = 29;              // n | dp (3) | dq (3) | dq dp^T (9) | dp dp^T (6) | dq dq^T (6) | residual^2
constexpr int kRegisterScanItems = 8;             // table entries per thread of a scan chunk
constexpr int kRegisterScanChunk = kRegisterGroup * kRegisterScanItems;
constexpr int kRegisterScanBlocks = kRegisterMaxCells / kRegisterScanChunk;     // 1024: one workgroup scans the chunk sums
constexpr int kRegisterSolveRanges = 8;           // the solve kernel adds the rows in this many ranges, then the ranges
constexpr int kRegisterSolveGroup = 32 * kRegisterSolveRanges;
constexpr int kRegisterMaxIterations = 256;
constexpr double kRegisterCollinear = 1e-12;      // second eigenvalue <= this x the first: the rotation is undetermined
static_assert(kRegisterMaxCells % kRegisterScanChunk == 0 && kRegisterScanBlocks <= 1024, "the scan's three levels");

// the words the stats pass folds into; the launcher's memset leaves 0 in each, every fold is an atomicMax / Add / Or
enum {
  kHdrMinX = 0,          // ~enc(min) of the finite targets, 3 words (0: no finite target)
  kHdrMaxX = 3,          // enc(max), 3 words
  kHdrFirstSource = 6,   // ~(index of the first finite source point)
  kHdrSourceFinite = 7,  // number of finite source points
  kHdrFlags = 8,         // bit 1: a point of either set was non-finite
  kHdrWords = 64
};

struct RegisterState {
  double T[13];          // R row-major | t | s
  double prev_rmse;
  double pa[3], pb[3];   // the pivots: the first finite source point, the low corner of the target's bounds
  double n_source;       // finite source points
  int done, executed, converged, flags;
  RegisterGrid grid;
};

struct RegisterLayout {
  size_t state, header, table, chunk_sums, sorted, partials, total;
};

RegisterLayout register_layout(int n_s, int n_t) {
  (void)n_s;
  Bump b(1);
  RegisterLayout L;
  L.state = b.take(sizeof(RegisterState));
  L.header = b.take(sizeof(unsigned) * kHdrWords);                       // header and table are one contiguous memset
  L.table = b.take(sizeof(unsigned) * ((size_t)kRegisterMaxCells + 2));
  L.chunk_sums = b.take(sizeof(unsigned) * kRegisterScanBlocks);
  L.sorted = b.take(sizeof(float4) * (size_t)n_t);
  L.partials = b.take(sizeof(double) * kRegisterPartBlocks * kRegisterMoments);
  L.total = b.total;
  return L;
}

// a float's bits as an unsigned that orders like the float; finite values land strictly inside (0, 0xffffffff)
__device__ __forceinline__ unsigned order_bits(float f) {
  const unsigned u = __float_as_uint(f);
  return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}
__device__ __forceinline__ float order_value(unsigned e) {
  return __uint_as_float((e & 0x80000000u) ? (e & 0x7fffffffu) : ~e);
}
__device__ __forceinline__ unsigned wave_max_u32(unsigned v) {
#pragma unroll
  for (int m = 32; m >= 1; m >>= 1) {
    const unsigned o = (unsigned)__shfl_xor((int)v, m);
    v = o > v ? o : v;
  }
  return v;
}

// blocks [0, blocks_t): the target; the rest: the source
__global__ __launch_bounds__(kRegisterGroup) void register_stats_kernel(int n_s, const float* __restrict__ source, int n_t,
                                                                        const float* __restrict__ target, int blocks_t,
                                                                        unsigned* __restrict__ header) {
  const bool is_target = (int)blockIdx.x < blocks_t;
  const int blk = is_target ? (int)blockIdx.x : (int)blockIdx.x - blocks_t;
  const int n_blk = is_target ? blocks_t : (int)gridDim.x - blocks_t;
  const int n = is_target ? n_t : n_s;
  const float* pts = is_target ? target : source;
  unsigned lo0 = 0u, lo1 = 0u, lo2 = 0u, hi0 = 0u, hi1 = 0u, hi2 = 0u, first = 0u, count = 0u;
  bool bad = false;
  for (long long i = (long long)blk * kRegisterGroup + (int)threadIdx.x; i < n; i += (long long)n_blk * kRegisterGroup) {
    const float x = pts[3 * i + 0], y = pts[3 * i + 1], z = pts[3 * i + 2];
    if (finite3(x, y, z)) {
      const unsigned ex = order_bits(x), ey = order_bits(y), ez = order_bits(z), nf = ~(unsigned)i;
      lo0 = ~ex > lo0 ? ~ex : lo0; lo1 = ~ey > lo1 ? ~ey : lo1; lo2 = ~ez > lo2 ? ~ez : lo2;
      hi0 = ex > hi0 ? ex : hi0; hi1 = ey > hi1 ? ey : hi1; hi2 = ez > hi2 ? ez : hi2;
      first = nf > first ? nf : first;
      ++count;
    } else {
      bad = true;
    }
  }
  // a wave folds with shuffles, the workgroup through LDS, and one thread per word goes to memory: the atomics of a call
  // all land on the same ten words, so their number is what they cost
  __shared__ unsigned fold[kRegisterGroup / 64][kHdrFlags + 1];
  const int wave = (int)threadIdx.x >> 6;
  lo0 = wave_max_u32(lo0); lo1 = wave_max_u32(lo1); lo2 = wave_max_u32(lo2);
  hi0 = wave_max_u32(hi0); hi1 = wave_max_u32(hi1); hi2 = wave_max_u32(hi2);
  first = wave_max_u32(first);
  count = wave_sum_u32(count);
  const unsigned any_bad = ballot(bad) != 0ull ? 2u : 0u;
  if (lane_id() == 0u) {
    fold[wave][kHdrMinX + 0] = lo0; fold[wave][kHdrMinX + 1] = lo1; fold[wave][kHdrMinX + 2] = lo2;
    fold[wave][kHdrMaxX + 0] = hi0; fold[wave][kHdrMaxX + 1] = hi1; fold[wave][kHdrMaxX + 2] = hi2;
    fold[wave][kHdrFirstSource] = first; fold[wave][kHdrSourceFinite] = count; fold[wave][kHdrFlags] = any_bad;
  }
  __syncthreads();
  const int word = (int)threadIdx.x;
  if (word > kHdrFlags) return;
  if (is_target ? (word == kHdrFirstSource || word == kHdrSourceFinite) : word < kHdrFirstSource) return;
  unsigned v = 0u;
  for (int w = 0; w < kRegisterGroup / 64; ++w) {
    const unsigned o = fold[w][word];
    v = word == kHdrSourceFinite ? v + o : (word == kHdrFlags ? (v | o) : (o > v ? o : v));
  }
  if (!v) return;                                     // nothing seen: the memset's zero stands
  if (word == kHdrSourceFinite) atomicAdd(header + word, v);
  else if (word == kHdrFlags) atomicOr(header + word, v);
  else atomicMax(header + word, v);
}

__global__ __launch_bounds__(64) void register_setup_kernel(int n_s, const float* __restrict__ source,
                                                            const unsigned* __restrict__ header, float max_distance,
                                                            const double* __restrict__ init,
                                                            RegisterState* __restrict__ state) {
  if (threadIdx.x != 0u) return;
  float lo[3] = {0.f, 0.f, 0.f}, hi[3] = {0.f, 0.f, 0.f};      // no finite target: one empty cell at the origin
  if (header[kHdrMaxX]) {
#pragma unroll
    for (int c = 0; c < 3; ++c) {
      lo[c] = order_value(~header[kHdrMinX + c]);
      hi[c] = order_value(header[kHdrMaxX + c]);
    }
  }
  state->grid = register_grid_make(lo, hi, max_distance, kRegisterMaxCells);
#pragma unroll
  for (int c = 0; c < 13; ++c) state->T[c] = init ? init[c] : ((c == 0 || c == 4 || c == 8 || c == 12) ? 1.0 : 0.0);
  const unsigned fs = ~header[kHdrFirstSource];
#pragma unroll
  for (int c = 0; c < 3; ++c) {
    state->pa[c] = fs < (unsigned)n_s ? (double)source[3 * (size_t)fs + c] : 0.0;
    state->pb[c] = (double)lo[c];
  }
  state->prev_rmse = 0.0;
  state->n_source = (double)header[kHdrSourceFinite];
  state->done = 0;
  state->executed = 0;
  state->converged = 0;
  state->flags = (int)(header[kHdrFlags] & 2u);
}

__global__ __launch_bounds__(kRegisterGroup) void register_count_kernel(int n_t, const float* __restrict__ target,
                                                                        const RegisterState* __restrict__ state,
                                                                        unsigned* __restrict__ table) {
  const long long j = (long long)blockIdx.x * kRegisterGroup + (int)threadIdx.x;
  if (j >= n_t) return;
  const float x = target[3 * j + 0], y = target[3 * j + 1], z = target[3 * j + 2];
  if (!finite3(x, y, z)) return;
  atomicAdd(table + 1 + register_target_cell(state->grid, x, y, z), 1u);
}

// inclusive scan of one value per thread over a workgroup of N threads; lds: N words
template <int N>
__device__ __forceinline__ unsigned block_inclusive_scan(unsigned v, unsigned* lds) {
  const int t = (int)threadIdx.x;
  lds[t] = v;
  __syncthreads();
#pragma unroll
  for (int off = 1; off < N; off <<= 1) {
    const unsigned add = t >= off ? lds[t - off] : 0u;
    __syncthreads();
    lds[t] += add;
    __syncthreads();
  }
  return lds[t];
}

__device__ __forceinline__ int grid_cells(const RegisterState* state) {
  return state->grid.nx * state->grid.ny * state->grid.nz;               // <= kRegisterMaxCells (register_grid_make)
}

// chunk_sums[b] = the sum of the chunk's counts; chunks past the used cells leave at once
__global__ __launch_bounds__(kRegisterGroup) void register_scan_sums_kernel(const RegisterState* __restrict__ state,
                                                                            const unsigned* __restrict__ counts,
                                                                            unsigned* __restrict__ chunk_sums) {
  __shared__ unsigned lds[kRegisterGroup];
  const int cells = grid_cells(state);
  const int base = (int)blockIdx.x * kRegisterScanChunk;
  if (base >= cells) return;
  unsigned v = 0u;
#pragma unroll
  for (int k = 0; k < kRegisterScanItems; ++k) {
    const int c = base + (int)threadIdx.x * kRegisterScanItems + k;
    v += c < cells ? counts[c] : 0u;
  }
  v = block_inclusive_scan<kRegisterGroup>(v, lds);
  if (threadIdx.x == kRegisterGroup - 1) chunk_sums[blockIdx.x] = v;
}

// one workgroup: chunk_sums becomes its own exclusive scan
__global__ __launch_bounds__(kRegisterScanBlocks) void register_scan_chunks_kernel(const RegisterState* __restrict__ state,
                                                                                   unsigned* __restrict__ chunk_sums) {
  __shared__ unsigned lds[kRegisterScanBlocks];
  const int cells = grid_cells(state);
  const bool used = (int)threadIdx.x * kRegisterScanChunk < cells;
  const unsigned v = used ? chunk_sums[threadIdx.x] : 0u;
  const unsigned inc = block_inclusive_scan<kRegisterScanBlocks>(v, lds);
  if (used) chunk_sums[threadIdx.x] = inc - v;
}

// counts[c] becomes the number of targets in the cells before c
__global__ __launch_bounds__(kRegisterGroup) void register_scan_apply_kernel(const RegisterState* __restrict__ state,
                                                                             const unsigned* __restrict__ chunk_sums,
                                                                             unsigned* __restrict__ counts) {
  __shared__ unsigned lds[kRegisterGroup];
  const int cells = grid_cells(state);
  const int base = (int)blockIdx.x * kRegisterScanChunk;
  if (base >= cells) return;
  unsigned item[kRegisterScanItems], v = 0u;
#pragma unroll
  for (int k = 0; k < kRegisterScanItems; ++k) {
    const int c = base + (int)threadIdx.x * kRegisterScanItems + k;
    item[k] = c < cells ? counts[c] : 0u;
    v += item[k];
  }
  unsigned run = block_inclusive_scan<kRegisterGroup>(v, lds) - v + chunk_sums[blockIdx.x];
#pragma unroll
  for (int k = 0; k < kRegisterScanItems; ++k) {
    const int c = base + (int)threadIdx.x * kRegisterScanItems + k;
    if (c < cells) counts[c] = run;
    run += item[k];
  }
}

__global__ __launch_bounds__(kRegisterGroup) void register_scatter_kernel(int n_t, const float* __restrict__ target,
                                                                          const RegisterState* __restrict__ state,
                                                                          unsigned* __restrict__ table,
                                                                          float4* __restrict__ sorted) {
  const long long j = (long long)blockIdx.x * kRegisterGroup + (int)threadIdx.x;
  if (j >= n_t) return;
  const float x = target[3 * j + 0], y = target[3 * j + 1], z = target[3 * j + 2];
  if (!finite3(x, y, z)) return;
  const unsigned slot = atomicAdd(table + 1 + register_target_cell(state->grid, x, y, z), 1u);
  if (slot < (unsigned)n_t) sorted[slot] = make_float4(x, y, z, __int_as_float((int)j));     // always: the counts sum to <= n_t
}

// LAST: the pass after the loop -- it runs whatever `done` says and writes correspondence / distance2 where given
template <bool LAST>
__global__ __launch_bounds__(kRegisterGroup) void register_query_kernel(int n_s, const float* __restrict__ source, int n_t,
                                                                        const float4* __restrict__ sorted,
                                                                        const unsigned* __restrict__ table,
                                                                        const RegisterState* __restrict__ state, float limit2,
                                                                        int n_blk, int32_t* __restrict__ correspondence,
                                                                        float* __restrict__ distance2,
                                                                        double* __restrict__ partials) {
  __shared__ double wave_sums[kRegisterGroup / 64][kRegisterMoments];
  if (!LAST && state->done) return;
  const RegisterGrid g = state->grid;
  const double r00 = state->T[0], r01 = state->T[1], r02 = state->T[2], r10 = state->T[3], r11 = state->T[4], r12 = state->T[5];
  const double r20 = state->T[6], r21 = state->T[7], r22 = state->T[8], tx = state->T[9], ty = state->T[10], tz = state->T[11];
  const double sc = state->T[12];
  const double pax = state->pa[0], pay = state->pa[1], paz = state->pa[2];
  const double pbx = state->pb[0], pby = state->pb[1], pbz = state->pb[2];
  const float inf = __builtin_inff();

  // the workgroup's points: a contiguous range, a multiple of the workgroup long
  const long long per = (((long long)n_s + n_blk - 1) / n_blk + kRegisterGroup - 1) / kRegisterGroup * kRegisterGroup;
  const long long start = (long long)blockIdx.x * per;
  const long long end = start + per < n_s ? start + per : n_s;
  double s[kRegisterMoments];
#pragma unroll
  for (int c = 0; c < kRegisterMoments; ++c) s[c] = 0.0;
  for (long long i = start + (int)threadIdx.x; i < end; i += kRegisterGroup) {
    const float px = source[3 * i + 0], py = source[3 * i + 1], pz = source[3 * i + 2];
    float best = inf, bqx = 0.f, bqy = 0.f, bqz = 0.f;
    int best_j = 0x7fffffff;
    double mx = 0.0, my = 0.0, mz = 0.0;
    if (finite3(px, py, pz)) {
      mx = sc * (r00 * (double)px + r01 * (double)py + r02 * (double)pz) + tx;
      my = sc * (r10 * (double)px + r11 * (double)py + r12 * (double)pz) + ty;
      mz = sc * (r20 * (double)px + r21 * (double)py + r22 * (double)pz) + tz;
      const float fx = (float)mx, fy = (float)my, fz = (float)mz;
      int x0, x1, y0, y1, z0, z1;
      register_query_range(g.ox, g.inv_h, g.nx, fx, x0, x1);
      register_query_range(g.oy, g.inv_h, g.ny, fy, y0, y1);
      register_query_range(g.oz, g.inv_h, g.nz, fz, z0, z1);
      if (x0 <= x1) {
        for (int cz = z0; cz <= z1; ++cz) {
          for (int cy = y0; cy <= y1; ++cy) {
            const int row = (cz * g.ny + cy) * g.nx;
            const unsigned e0 = table[row + x0];                                  // cells x0..x1: one run
            unsigned e1 = table[row + x1 + 1];
            e1 = e1 < (unsigned)n_t ? e1 : (unsigned)n_t;                         // always: the table ends at the finite count
            for (unsigned e = e0; e < e1; ++e) {
              const float4 q = sorted[e];
              const float dx = fx - q.x, dy = fy - q.y, dz = fz - q.z;
              const float d2 = __builtin_fmaf(dz, dz, __builtin_fmaf(dy, dy, dx * dx));
              const int j = __float_as_int(q.w);
              if (d2 < best || (d2 == best && j < best_j)) {
                best = d2; best_j = j; bqx = q.x; bqy = q.y; bqz = q.z;
              }
            }
          }
        }
      }
    }
    const bool inlier = best_j != 0x7fffffff && best <= limit2;
    if (LAST) {
      if (correspondence) correspondence[i] = inlier ? best_j : -1;
      if (distance2) distance2[i] = inlier ? best : inf;
    }
    if (inlier) {
      const double dpx = (double)px - pax, dpy = (double)py - pay, dpz = (double)pz - paz;
      const double dqx = (double)bqx - pbx, dqy = (double)bqy - pby, dqz = (double)bqz - pbz;
      const double rx = mx - (double)bqx, ry = my - (double)bqy, rz = mz - (double)bqz;
      s[0] += 1.0;
      s[1] += dpx; s[2] += dpy; s[3] += dpz;
      s[4] += dqx; s[5] += dqy; s[6] += dqz;
      s[7] += dqx * dpx; s[8] += dqx * dpy; s[9] += dqx * dpz;
      s[10] += dqy * dpx; s[11] += dqy * dpy; s[12] += dqy * dpz;
      s[13] += dqz * dpx; s[14] += dqz * dpy; s[15] += dqz * dpz;
      s[16] += dpx * dpx; s[17] += dpx * dpy; s[18] += dpx * dpz; s[19] += dpy * dpy; s[20] += dpy * dpz; s[21] += dpz * dpz;
      s[22] += dqx * dqx; s[23] += dqx * dqy; s[24] += dqx * dqz; s[25] += dqy * dqy; s[26] += dqy * dqz; s[27] += dqz * dqz;
      s[28] += rx * rx + ry * ry + rz * rz;
    }
  }
  // a wave: the fixed butterfly; the workgroup: its waves in order
#pragma unroll
  for (int c = 0; c < kRegisterMoments; ++c) {
#pragma unroll
    for (int m = 32; m >= 1; m >>= 1) s[c] += __shfl_xor(s[c], m);
  }
  const int wave = (int)threadIdx.x >> 6;
  if ((threadIdx.x & 63u) == 0u) {
#pragma unroll
    for (int c = 0; c < kRegisterMoments; ++c) wave_sums[wave][c] = s[c];
  }
  __syncthreads();
  if (threadIdx.x < (unsigned)kRegisterMoments) {
    double v = 0.0;
    for (int w = 0; w < kRegisterGroup / 64; ++w) v += wave_sums[w][threadIdx.x];
    partials[(size_t)blockIdx.x * kRegisterMoments + threadIdx.x] = v;
  }
}

__device__ __forceinline__ bool finite_mat(const Mat3d& r) {
  return isfinite(r.m00) && isfinite(r.m01) && isfinite(r.m02) && isfinite(r.m10) && isfinite(r.m11) && isfinite(r.m12) &&
         isfinite(r.m20) && isfinite(r.m21) && isfinite(r.m22);
}

// the scatter matrix sum d d^T - n m m^T of one set is collinear (or a point): its second eigenvalue <= 1e-12 x its first
__device__ __forceinline__ bool collinear(const double* ss, double n, double m0, double m1, double m2) {
  const Sym3d c = {ss[0] - n * m0 * m0, ss[1] - n * m0 * m1, ss[2] - n * m0 * m2,
                   ss[3] - n * m1 * m1, ss[4] - n * m1 * m2, ss[5] - n * m2 * m2};
  const Eig3 e = eigen_sorted<true>(c);
  return !(e.l1 > kRegisterCollinear * e.l0);
}

// LAST: the launch after the final query -- result[32] from the record and that pass's sums
template <bool LAST>
__global__ __launch_bounds__(kRegisterSolveGroup) void register_solve_kernel(RegisterState* __restrict__ state,
                                                            const double* __restrict__ partials, int n_blk, int k,
                                                            int with_scale, double tol, double* __restrict__ history,
                                                            double* __restrict__ result) {
  __shared__ double range_sums[kRegisterSolveRanges][kRegisterMoments];
  __shared__ double sums[kRegisterMoments];
  if (!LAST && state->done) return;
  // thread (range, moment): its range of rows in index order; then per moment the ranges in order.  A fixed order, and eight
  // chains of loads in flight per moment instead of one
  const int moment = (int)threadIdx.x & 31, range = (int)threadIdx.x >> 5;
  if (moment < kRegisterMoments) {
    const int rows = (n_blk + kRegisterSolveRanges - 1) / kRegisterSolveRanges;
    const int b0 = range * rows, b1 = b0 + rows < n_blk ? b0 + rows : n_blk;
    double v = 0.0;
#pragma unroll 8
    for (int b = b0; b < b1; ++b) v += partials[(size_t)b * kRegisterMoments + moment];
    range_sums[range][moment] = v;
  }
  __syncthreads();
  if (threadIdx.x < (unsigned)kRegisterMoments) {
    double v = 0.0;
    for (int r = 0; r < kRegisterSolveRanges; ++r) v += range_sums[r][threadIdx.x];
    sums[threadIdx.x] = v;
  }
  __syncthreads();
  if (threadIdx.x != 0u) return;

  const double n = sums[0];
  const double rmse = n > 0.0 ? sqrt(sums[28] / n) : 0.0;
  if (LAST) {
#pragma unroll
    for (int c = 0; c < 13; ++c) result[c] = state->T[c];
    result[13] = rmse;
    result[14] = state->n_source > 0.0 ? n / state->n_source : 0.0;
    result[15] = n;
    result[16] = (double)state->executed;
    result[17] = (double)state->converged;
    result[18] = (double)state->flags;
    result[19] = state->grid.h;
    result[20] = (double)state->grid.nx; result[21] = (double)state->grid.ny; result[22] = (double)state->grid.nz;
#pragma unroll
    for (int c = 23; c < 32; ++c) result[c] = 0.0;
    return;
  }
  if (history) {
    history[4 * (size_t)k + 0] = n; history[4 * (size_t)k + 1] = rmse;
    history[4 * (size_t)k + 2] = state->T[12]; history[4 * (size_t)k + 3] = 0.0;
  }
  state->executed = k + 1;

  bool undetermined = !(n >= 3.0);
  Mat3d R = {1.0, 0.0, 0.0, 0.0, 1.0, 0.0, 0.0, 0.0, 1.0};
  double scale = 1.0, mp0 = 0.0, mp1 = 0.0, mp2 = 0.0, mq0 = 0.0, mq1 = 0.0, mq2 = 0.0;
  if (!undetermined) {
    const double inv_n = 1.0 / n;
    mp0 = sums[1] * inv_n; mp1 = sums[2] * inv_n; mp2 = sums[3] * inv_n;
    mq0 = sums[4] * inv_n; mq1 = sums[5] * inv_n; mq2 = sums[6] * inv_n;
    undetermined = collinear(sums + 16, n, mp0, mp1, mp2) || collinear(sums + 22, n, mq0, mq1, mq2);
  }
  if (!undetermined) {
    const Mat3d S = {sums[7] - n * mq0 * mp0,  sums[8] - n * mq0 * mp1,  sums[9] - n * mq0 * mp2,
                     sums[10] - n * mq1 * mp0, sums[11] - n * mq1 * mp1, sums[12] - n * mq1 * mp2,
                     sums[13] - n * mq2 * mp0, sums[14] - n * mq2 * mp1, sums[15] - n * mq2 * mp2};
    R = shape_rotation(S, gram_eigen_desc(S));
    const double tr = R.m00 * S.m00 + R.m01 * S.m01 + R.m02 * S.m02 + R.m10 * S.m10 + R.m11 * S.m11 + R.m12 * S.m12 +
                      R.m20 * S.m20 + R.m21 * S.m21 + R.m22 * S.m22;
    const double var_p = (sums[16] - n * mp0 * mp0) + (sums[19] - n * mp1 * mp1) + (sums[21] - n * mp2 * mp2);
    if (with_scale) scale = tr / var_p;
    undetermined = !finite_mat(R) || !isfinite(scale);
  }
  if (undetermined) {
    state->flags |= 1;
    state->done = 1;
    return;
  }
  const double pm0 = state->pa[0] + mp0, pm1 = state->pa[1] + mp1, pm2 = state->pa[2] + mp2;
  state->T[0] = R.m00; state->T[1] = R.m01; state->T[2] = R.m02;
  state->T[3] = R.m10; state->T[4] = R.m11; state->T[5] = R.m12;
  state->T[6] = R.m20; state->T[7] = R.m21; state->T[8] = R.m22;
  state->T[9] = (state->pb[0] + mq0) - scale * (R.m00 * pm0 + R.m01 * pm1 + R.m02 * pm2);
  state->T[10] = (state->pb[1] + mq1) - scale * (R.m10 * pm0 + R.m11 * pm1 + R.m12 * pm2);
  state->T[11] = (state->pb[2] + mq2) - scale * (R.m20 * pm0 + R.m21 * pm1 + R.m22 * pm2);
  state->T[12] = scale;
  if (k > 0 && fabs(rmse - state->prev_rmse) <= tol * state->prev_rmse) {
    state->converged = 1;
    state->done = 1;
  }
  state->prev_rmse = rmse;
}

int capped_blocks(int n, int cap) {
  const unsigned b = div_up((unsigned)n, (unsigned)kRegisterGroup);
  return (int)(b < (unsigned)cap ? b : (unsigned)cap);
}

}  // namespace
}  // namespace mgs

using namespace mgs;

extern "C" size_t mgs_register_workspace_bytes(int n_s, int n_t, int iterations) {
  if (n_s <= 0 || n_t <= 0 || iterations < 0 || iterations > kRegisterMaxIterations) return 0;
  return register_layout(n_s, n_t).total;
}

extern "C" int mgs_register_icp(int n_s, const float* source, int n_t, const float* target, float max_distance,
                                int iterations, int with_scale, double tol, const double* init, void* workspace,
                                size_t workspace_bytes, int32_t* correspondence, float* distance2, double* history,
                                double* result, mgs_stream_t stream) {
  MGS_REQUIRE(n_s > 0 && n_t > 0, "register_icp: a point set is empty (n_s %d, n_t %d)", n_s, n_t);
  MGS_REQUIRE(source && target, "register_icp: source or target is null");
  MGS_REQUIRE(result, "register_icp: result is null");
  MGS_REQUIRE(isfinite(max_distance) && max_distance > 0.f, "register_icp: max_distance %g is not a finite positive number",
              (double)max_distance);
  MGS_REQUIRE(isfinite(tol) && tol >= 0.0, "register_icp: tol %g is not a finite non-negative number", tol);
  MGS_REQUIRE(iterations >= 0 && iterations <= kRegisterMaxIterations, "register_icp: iterations %d outside 0..%d", iterations,
              kRegisterMaxIterations);
  MGS_REQUIRE(workspace, "register_icp: workspace is null");
  MGS_REQUIRE((uintptr_t)workspace % 256 == 0, "register_icp: workspace %p is not 256-byte aligned", workspace);
  const RegisterLayout L = register_layout(n_s, n_t);
  MGS_REQUIRE(workspace_bytes >= L.total, "register_icp: workspace of %zu bytes, %zu needed", workspace_bytes, L.total);
  hipStream_t s = (hipStream_t)stream;
  char* ws = static_cast<char*>(workspace);
  RegisterState* state = reinterpret_cast<RegisterState*>(ws + L.state);
  unsigned* header = reinterpret_cast<unsigned*>(ws + L.header);
  unsigned* table = reinterpret_cast<unsigned*>(ws + L.table);
  unsigned* chunk_sums = reinterpret_cast<unsigned*>(ws + L.chunk_sums);
  float4* sorted = reinterpret_cast<float4*>(ws + L.sorted);
  double* partials = reinterpret_cast<double*>(ws + L.partials);
  const float limit2 = max_distance * max_distance;

  hipError_t e = hipMemsetAsync(ws + L.header, 0, L.chunk_sums - L.header, s);         // header and cell table: zeros
  if (e != hipSuccess) return set_error((int)e, "register_icp: memset failed: %s", hipGetErrorString(e));
  const int blocks_t = capped_blocks(n_t, kRegisterStatBlocks), blocks_s = capped_blocks(n_s, kRegisterStatBlocks);
  hipLaunchKernelGGL(register_stats_kernel, dim3(blocks_t + blocks_s), dim3(kRegisterGroup), 0, s, n_s, source, n_t, target,
                     blocks_t, header);
  int rc = check_launch("register_icp");
  if (rc) return rc;
  hipLaunchKernelGGL(register_setup_kernel, dim3(1), dim3(64), 0, s, n_s, source, header, max_distance, init, state);
  if ((rc = check_launch("register_icp"))) return rc;
  const unsigned per_target = div_up((unsigned)n_t, (unsigned)kRegisterGroup);
  hipLaunchKernelGGL(register_count_kernel, dim3(per_target), dim3(kRegisterGroup), 0, s, n_t, target, state, table);
  if ((rc = check_launch("register_icp"))) return rc;
  hipLaunchKernelGGL(register_scan_sums_kernel, dim3(kRegisterScanBlocks), dim3(kRegisterGroup), 0, s, state, table + 1,
                     chunk_sums);
  if ((rc = check_launch("register_icp"))) return rc;
  hipLaunchKernelGGL(register_scan_chunks_kernel, dim3(1), dim3(kRegisterScanBlocks), 0, s, state, chunk_sums);
  if ((rc = check_launch("register_icp"))) return rc;
  hipLaunchKernelGGL(register_scan_apply_kernel, dim3(kRegisterScanBlocks), dim3(kRegisterGroup), 0, s, state, chunk_sums,
                     table + 1);
  if ((rc = check_launch("register_icp"))) return rc;
  hipLaunchKernelGGL(register_scatter_kernel, dim3(per_target), dim3(kRegisterGroup), 0, s, n_t, target, state, table, sorted);
  if ((rc = check_launch("register_icp"))) return rc;

  const int n_blk = capped_blocks(n_s, kRegisterPartBlocks);
  for (int k = 0; k < iterations; ++k) {
    hipLaunchKernelGGL(register_query_kernel<false>, dim3(n_blk), dim3(kRegisterGroup), 0, s, n_s, source, n_t, sorted, table,
                       state, limit2, n_blk, (int32_t*)nullptr, (float*)nullptr, partials);
    if ((rc = check_launch("register_icp"))) return rc;
    hipLaunchKernelGGL(register_solve_kernel<false>, dim3(1), dim3(kRegisterSolveGroup), 0, s, state, partials, n_blk, k, with_scale, tol,
                       history, result);
    if ((rc = check_launch("register_icp"))) return rc;
  }
  hipLaunchKernelGGL(register_query_kernel<true>, dim3(n_blk), dim3(kRegisterGroup), 0, s, n_s, source, n_t, sorted, table,
                     state, limit2, n_blk, correspondence, distance2, partials);
  if ((rc = check_launch("register_icp"))) return rc;
  hipLaunchKernelGGL(register_solve_kernel<true>, dim3(1), dim3(kRegisterSolveGroup), 0, s, state, partials, n_blk, iterations, with_scale, tol,
                     history, result);
  return check_launch("register_icp");
}
