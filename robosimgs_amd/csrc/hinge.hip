// hinge.hip -- the hinge of an articulated part from two point sets (include/mgs_hinge.h), gfx950.
//
// Three kernels behind mgs_hinge_fit, none of which reads anything back to the host:
//
// hinge_nn_kernel (the hot path, once per direction).  A workgroup of kHingeGroup threads keeps kHingeQueries query points
// per thread in registers (query base + thread + k * kHingeGroup: coalesced) and streams a range of the other set
// through LDS in tiles of kHingeTile float4 entries; every thread of a wave reads the same entry, so the ds_read_b128 is
// a broadcast, paid once for the thread's kHingeQueries pairs.  A pair is 3 subtractions, 1 multiply, 2 fma and 1 min:
// 7 vector instructions, 6.5 as built (the unrolled loop folds two entries' mins into one v_min3).  The other set is split over blockIdx.y so that a small query set still fills the chip; the
// splits meet in nn2 with an unsigned atomicMin on the float's bits (a non-negative float orders like its bits, and a
// minimum does not depend on order: the same bits under any tiling, split or launch order).  A non-finite point of the
// other set is staged as +inf (its pairs are +inf and lose every min); a non-finite query never writes, so its nn2 keeps
// the 0xffffffff (a NaN) that the launcher's memset left there, and a NaN is below no limit.  The A-side minimum, the
// index of A's first finite point (the pivot of the moments) and the "every point was finite" bit are folded into three
// words of the workspace with integer atomics, one per wave.
//
// hinge_moments_kernel.  contact = sqrtf(nn2) < sqrtf(min2) + threshold, the contact byte, and per workgroup the fp64
// sums of 1, d and d d^T (d = x - pivot) over its contact points: each thread walks its points in index order, a wave is
// summed with a fixed butterfly and the four waves in wave order.  At most kHingePartBlocks workgroups per set.
//
// hinge_final_kernel (one workgroup).  The partial sums are added in index order, then one thread forms the two means,
// the position, the covariance (n - 1), solves the symmetric 3x3 eigenproblem with cyclic Jacobi sweeps in fp64 (jacobi3.h:
// every index a compile-time constant, no scratch), applies the sign rule and the fallback and writes the 16 doubles.
#include "mgs_common.h"
#include "jacobi3.h"
#include "../../include/mgs_hinge.h"

#include <math.h>

namespace mgs {
namespace {

constexpr int kHingeGroup = 256;          // G: threads of a workgroup (all three kernels)
constexpr int kHingeTile = 1024;          // T: entries of the other set per LDS tile (16 KiB; 256: profiles/hinge/README.md)
constexpr int kHingeQueries = 4;          // query points per thread
constexpr int kHingePartBlocks = 256;     // workgroups of the moments kernel per set, at the most
constexpr int kHingeMoments = 10;         // count, sum d (3), sum d d^T (xx xy xz yy yz zz)
constexpr unsigned kHingeTargetBlocks = 2048;   // the nn launch splits the other set until it has about this many workgroups

// the three words the nn passes fold into (the launcher's memset leaves 0xffffffff in each)
enum { kHdrMin2 = 0, kHdrFirstFinite = 1, kHdrClean = 2 };

struct HingeLayout {
  size_t nn2_a, nn2_b, header, partials, total;
};

HingeLayout hinge_layout(int n_a, int n_b) {
  Bump b(1);
  HingeLayout L;
  L.nn2_a = b.take(sizeof(float) * (size_t)n_a);       // nn2_a, nn2_b and header are one contiguous memset
  L.nn2_b = b.take(sizeof(float) * (size_t)n_b);
  L.header = b.take(256);
  L.partials = b.take(sizeof(double) * 2 * kHingePartBlocks * kHingeMoments);
  L.total = b.total;
  return L;
}

__device__ __forceinline__ bool finite3(float x, float y, float z) {
  return isfinite(x) && isfinite(y) && isfinite(z);
}

__device__ __forceinline__ unsigned wave_min_u32(unsigned v) {
#pragma unroll
  for (int m = 32; m >= 1; m >>= 1) {
    const unsigned o = (unsigned)__shfl_xor((int)v, m);
    v = o < v ? o : v;
  }
  return v;
}

__global__ __launch_bounds__(kHingeGroup) void hinge_nn_kernel(int n_q, const float* __restrict__ q, int n_o,
                                                               const float* __restrict__ o, int tiles_per_split,
                                                               unsigned* __restrict__ nn2, unsigned* __restrict__ header,
                                                               int is_a) {
  __shared__ float4 tile[kHingeTile];
  const int t = (int)threadIdx.x;
  const long long base = (long long)blockIdx.x * (kHingeGroup * kHingeQueries) + t;
  const float inf = __builtin_inff();

  float qx[kHingeQueries], qy[kHingeQueries], qz[kHingeQueries], best[kHingeQueries];
  bool ok[kHingeQueries], bad = false;
#pragma unroll
  for (int k = 0; k < kHingeQueries; ++k) {
    const long long i = base + (long long)k * kHingeGroup;
    qx[k] = qy[k] = qz[k] = 0.f;
    best[k] = inf;
    ok[k] = false;
    if (i < n_q) {
      qx[k] = q[3 * i + 0];
      qy[k] = q[3 * i + 1];
      qz[k] = q[3 * i + 2];
      ok[k] = finite3(qx[k], qy[k], qz[k]);
      bad |= !ok[k];
    }
  }

  const int n_tiles = (int)(((long long)n_o + kHingeTile - 1) / kHingeTile);
  const int tile0 = (int)blockIdx.y * tiles_per_split;
  const int tile1 = tile0 + tiles_per_split < n_tiles ? tile0 + tiles_per_split : n_tiles;
  for (int tl = tile0; tl < tile1; ++tl) {
    const long long obase = (long long)tl * kHingeTile;
    const int count = n_o - obase < kHingeTile ? (int)(n_o - obase) : kHingeTile;
    __syncthreads();                                // the walk of the previous tile is over
    for (int e = t; e < count; e += kHingeGroup) {
      const long long j = obase + e;
      float4 p = make_float4(o[3 * j + 0], o[3 * j + 1], o[3 * j + 2], 0.f);
      if (!finite3(p.x, p.y, p.z)) p = make_float4(inf, inf, inf, 0.f);      // nobody's neighbour
      tile[e] = p;
    }
    __syncthreads();
#pragma unroll 4
    for (int j = 0; j < count; ++j) {
      const float4 p = tile[j];                     // the same address in every lane: a broadcast
#pragma unroll
      for (int k = 0; k < kHingeQueries; ++k) {
        const float dx = qx[k] - p.x, dy = qy[k] - p.y, dz = qz[k] - p.z;
        best[k] = __builtin_fminf(best[k], __builtin_fmaf(dz, dz, __builtin_fmaf(dy, dy, dx * dx)));
      }
    }
  }

  unsigned lo = 0xffffffffu, first = 0xffffffffu;
#pragma unroll
  for (int k = 0; k < kHingeQueries; ++k) {
    if (ok[k]) {
      const long long i = base + (long long)k * kHingeGroup;
      const unsigned bits = __float_as_uint(best[k]);          // >= +0 or +inf: ordered like the float
      atomicMin(nn2 + i, bits);
      lo = bits < lo ? bits : lo;
      first = (unsigned)i < first ? (unsigned)i : first;
    }
  }
  const bool lane0 = lane_id() == 0u;
  if (is_a) {
    lo = wave_min_u32(lo);
    if (lane0 && lo != 0xffffffffu) atomicMin(header + kHdrMin2, lo);
  }
  if (blockIdx.y == 0) {
    if (is_a) {
      first = wave_min_u32(first);
      if (lane0 && first != 0xffffffffu) atomicMin(header + kHdrFirstFinite, first);
    }
    if (ballot(bad) != 0ull && lane0) atomicAnd(header + kHdrClean, ~2u);
  }
}

__global__ __launch_bounds__(kHingeGroup) void hinge_moments_kernel(
    int n_a, const float* __restrict__ pts_a, int n_b, const float* __restrict__ pts_b, const unsigned* __restrict__ nn2_a,
    const unsigned* __restrict__ nn2_b, const unsigned* __restrict__ header, float threshold, int blocks_a, int blocks_b,
    uint8_t* __restrict__ contact_a, uint8_t* __restrict__ contact_b, double* __restrict__ partials) {
  __shared__ double wave_sums[kHingeGroup / 64][kHingeMoments];
  const int side = (int)blockIdx.x >= blocks_a ? 1 : 0;
  const int blk = side ? (int)blockIdx.x - blocks_a : (int)blockIdx.x;
  const int n_blk = side ? blocks_b : blocks_a;
  const int n = side ? n_b : n_a;
  const float* pts = side ? pts_b : pts_a;
  const unsigned* nn2 = side ? nn2_b : nn2_a;
  uint8_t* contact = side ? contact_b : contact_a;

  const unsigned first = header[kHdrFirstFinite];
  double px = 0.0, py = 0.0, pz = 0.0;
  if (first < (unsigned)n_a) {
    px = (double)pts_a[3 * (size_t)first + 0];
    py = (double)pts_a[3 * (size_t)first + 1];
    pz = (double)pts_a[3 * (size_t)first + 2];
  }
  const float limit = sqrtf(__uint_as_float(header[kHdrMin2])) + threshold;      // NaN where no pair was finite

  // the workgroup's points: a contiguous range, a multiple of the workgroup long
  const long long per = (((long long)n + n_blk - 1) / n_blk + kHingeGroup - 1) / kHingeGroup * kHingeGroup;
  const long long start = (long long)blk * per;
  const long long end = start + per < n ? start + per : n;
  double s[kHingeMoments];
#pragma unroll
  for (int c = 0; c < kHingeMoments; ++c) s[c] = 0.0;
  for (long long i = start + (int)threadIdx.x; i < end; i += kHingeGroup) {
    const bool c = sqrtf(__uint_as_float(nn2[i])) < limit;
    if (contact) contact[i] = c ? 1 : 0;
    if (c) {
      const double dx = (double)pts[3 * i + 0] - px, dy = (double)pts[3 * i + 1] - py, dz = (double)pts[3 * i + 2] - pz;
      s[0] += 1.0;
      s[1] += dx; s[2] += dy; s[3] += dz;
      s[4] += dx * dx; s[5] += dx * dy; s[6] += dx * dz;
      s[7] += dy * dy; s[8] += dy * dz; s[9] += dz * dz;
    }
  }
  // a wave: the fixed butterfly; the workgroup: its waves in order
#pragma unroll
  for (int c = 0; c < kHingeMoments; ++c) {
#pragma unroll
    for (int m = 32; m >= 1; m >>= 1) s[c] += __shfl_xor(s[c], m);
  }
  const int wave = (int)threadIdx.x >> 6;
  if ((threadIdx.x & 63u) == 0u) {
#pragma unroll
    for (int c = 0; c < kHingeMoments; ++c) wave_sums[wave][c] = s[c];
  }
  __syncthreads();
  if (threadIdx.x < (unsigned)kHingeMoments) {
    double v = 0.0;
    for (int w = 0; w < kHingeGroup / 64; ++w) v += wave_sums[w][threadIdx.x];
    partials[((size_t)side * kHingePartBlocks + blk) * kHingeMoments + threadIdx.x] = v;
  }
}

__global__ __launch_bounds__(64) void hinge_final_kernel(int n_a, const float* __restrict__ pts_a,
                                                         const unsigned* __restrict__ header,
                                                         const double* __restrict__ partials, int blocks_a, int blocks_b,
                                                         double* __restrict__ joint) {
  __shared__ double sums[2][kHingeMoments];
  if (threadIdx.x < 2u * kHingeMoments) {
    const int side = (int)threadIdx.x / kHingeMoments, c = (int)threadIdx.x % kHingeMoments;
    const int n_blk = side ? blocks_b : blocks_a;
    const double* p = partials + (size_t)side * kHingePartBlocks * kHingeMoments + c;
    double v = 0.0;
    for (int b = 0; b < n_blk; ++b) v += p[(size_t)b * kHingeMoments];       // index order
    sums[side][c] = v;
  }
  __syncthreads();
  if (threadIdx.x != 0u) return;

  const unsigned first = header[kHdrFirstFinite];
  double pvx = 0.0, pvy = 0.0, pvz = 0.0;
  if (first < (unsigned)n_a) {
    pvx = (double)pts_a[3 * (size_t)first + 0];
    pvy = (double)pts_a[3 * (size_t)first + 1];
    pvz = (double)pts_a[3 * (size_t)first + 2];
  }
  const double na = sums[0][0], nb = sums[1][0], n = na + nb;
  const double pos_x = 0.5 * ((pvx + sums[0][1] / na) + (pvx + sums[1][1] / nb));
  const double pos_y = 0.5 * ((pvy + sums[0][2] / na) + (pvy + sums[1][2] / nb));
  const double pos_z = 0.5 * ((pvz + sums[0][3] / na) + (pvz + sums[1][3] / nb));
  const double sx = sums[0][1] + sums[1][1], sy = sums[0][2] + sums[1][2], sz = sums[0][3] + sums[1][3];
  const double inv = n > 1.0 ? 1.0 / (n - 1.0) : 0.0, inv_n = n > 0.0 ? 1.0 / n : 0.0;
  double a00 = ((sums[0][4] + sums[1][4]) - sx * sx * inv_n) * inv;
  double a01 = ((sums[0][5] + sums[1][5]) - sx * sy * inv_n) * inv;
  double a02 = ((sums[0][6] + sums[1][6]) - sx * sz * inv_n) * inv;
  double a11 = ((sums[0][7] + sums[1][7]) - sy * sy * inv_n) * inv;
  double a12 = ((sums[0][8] + sums[1][8]) - sy * sz * inv_n) * inv;
  double a22 = ((sums[0][9] + sums[1][9]) - sz * sz * inv_n) * inv;
  double v00, v01, v02, v10, v11, v12, v20, v21, v22;
  jacobi_solve3(a00, a01, a02, a11, a12, a22, v00, v01, v02, v10, v11, v12, v20, v21, v22);       // jacobi3.h

  // the eigenvalues ascending; the columns 1 and 2 of v follow the first two exchanges, so that the largest
  // eigenvalue's vector ends in column 2 (pairwise exchanges: a three-way choice of column becomes an indexed read of a
  // private array, which is scratch)
  double l0 = a00, l1 = a11, l2 = a22, tmp;
  if (l0 > l1) { tmp = l0; l0 = l1; l1 = tmp; v01 = v00; v11 = v10; v21 = v20; }
  if (l1 > l2) { tmp = l1; l1 = l2; l2 = tmp; v02 = v01; v12 = v11; v22 = v21; }
  if (l0 > l1) { tmp = l0; l0 = l1; l1 = tmp; }
  const double lmax = l2;
  double ax = v02, ay = v12, az = v22;

  const double norm = sqrt(ax * ax + ay * ay + az * az);
  ax /= norm; ay /= norm; az /= norm;
  double big = ax;                                  // the component of largest magnitude is positive; ties: lowest index
  if (fabs(ay) > fabs(big)) big = ay;
  if (fabs(az) > fabs(big)) big = az;
  if (big < 0.0) { ax = -ax; ay = -ay; az = -az; }

  const double total = l0 + l1 + l2;
  double conf = total > 0.0 ? lmax / total : 0.0;
  unsigned flags = (header[kHdrClean] & 2u) ? 0u : 2u;
  if (!(conf >= 0.5)) {                             // also where it is undefined (no contact point at all)
    ax = 1.0; ay = 0.0; az = 0.0;
    flags |= 1u;
  }
  joint[0] = pos_x; joint[1] = pos_y; joint[2] = pos_z;
  joint[3] = ax; joint[4] = ay; joint[5] = az;
  joint[6] = conf;
  joint[7] = (double)sqrtf(__uint_as_float(header[kHdrMin2]));
  joint[8] = na; joint[9] = nb;
  joint[10] = l0; joint[11] = l1; joint[12] = l2;
  joint[13] = (double)flags;
  joint[14] = 0.0; joint[15] = 0.0;
}

int moment_blocks(int n) {
  const unsigned b = div_up((unsigned)n, (unsigned)kHingeGroup);
  return (int)(b < (unsigned)kHingePartBlocks ? b : (unsigned)kHingePartBlocks);
}

int launch_nn(int n_q, const float* q, int n_o, const float* o, unsigned* nn2, unsigned* header, int is_a,
              hipStream_t stream) {
  const unsigned blocks_q = div_up((unsigned)n_q, (unsigned)(kHingeGroup * kHingeQueries));
  const unsigned tiles = div_up((unsigned)n_o, (unsigned)kHingeTile);
  unsigned splits = div_up(kHingeTargetBlocks, blocks_q);
  if (splits > tiles) splits = tiles;
  const unsigned per = div_up(tiles, splits);
  splits = div_up(tiles, per);                      // no empty split; at most kHingeTargetBlocks of them (< 65536)
  hipLaunchKernelGGL(hinge_nn_kernel, dim3(blocks_q, splits), dim3(kHingeGroup), 0, stream, n_q, q, n_o, o, (int)per, nn2,
                     header, is_a);
  return check_launch("hinge_fit");
}

}  // namespace
}  // namespace mgs

using namespace mgs;

extern "C" size_t mgs_hinge_workspace_bytes(int n_a, int n_b) {
  if (n_a <= 0 || n_b <= 0) return 0;
  return hinge_layout(n_a, n_b).total;
}

extern "C" int mgs_hinge_fit(int n_a, const float* pts_a, int n_b, const float* pts_b, float threshold, void* workspace,
                             size_t workspace_bytes, uint8_t* contact_a, uint8_t* contact_b, double* joint,
                             mgs_stream_t stream) {
  MGS_REQUIRE(n_a > 0 && n_b > 0, "hinge_fit: a part is empty (n_a %d, n_b %d)", n_a, n_b);
  MGS_REQUIRE(pts_a && pts_b, "hinge_fit: pts_a or pts_b is null");
  MGS_REQUIRE(joint, "hinge_fit: joint is null");
  MGS_REQUIRE(isfinite(threshold) && threshold > 0.f, "hinge_fit: threshold %g is not a finite positive number",
              (double)threshold);
  MGS_REQUIRE(workspace, "hinge_fit: workspace is null");
  const HingeLayout L = hinge_layout(n_a, n_b);
  MGS_REQUIRE(workspace_bytes >= L.total, "hinge_fit: workspace of %zu bytes, %zu needed", workspace_bytes, L.total);
  hipStream_t s = (hipStream_t)stream;
  char* ws = static_cast<char*>(workspace);
  unsigned* nn2_a = reinterpret_cast<unsigned*>(ws + L.nn2_a);
  unsigned* nn2_b = reinterpret_cast<unsigned*>(ws + L.nn2_b);
  unsigned* header = reinterpret_cast<unsigned*>(ws + L.header);
  double* partials = reinterpret_cast<double*>(ws + L.partials);

  hipError_t e = hipMemsetAsync(ws + L.nn2_a, 0xff, L.partials - L.nn2_a, s);     // nn2_a, nn2_b, header: all ones
  if (e != hipSuccess) return set_error((int)e, "hinge_fit: memset failed: %s", hipGetErrorString(e));
  int rc = launch_nn(n_a, pts_a, n_b, pts_b, nn2_a, header, 1, s);
  if (rc) return rc;
  rc = launch_nn(n_b, pts_b, n_a, pts_a, nn2_b, header, 0, s);
  if (rc) return rc;
  const int blocks_a = moment_blocks(n_a), blocks_b = moment_blocks(n_b);
  hipLaunchKernelGGL(hinge_moments_kernel, dim3(blocks_a + blocks_b), dim3(kHingeGroup), 0, s, n_a, pts_a, n_b, pts_b,
                     nn2_a, nn2_b, header, threshold, blocks_a, blocks_b, contact_a, contact_b, partials);
  rc = check_launch("hinge_fit");
  if (rc) return rc;
  hipLaunchKernelGGL(hinge_final_kernel, dim3(1), dim3(64), 0, s, n_a, pts_a, header, partials, blocks_a, blocks_b, joint);
  return check_launch("hinge_fit");
}
