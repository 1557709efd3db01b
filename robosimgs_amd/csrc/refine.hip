// refine.hip -- the refinement half of the training loop: splatfacto-mcmc's strategy (include/mgs_refine.h) without a
// host read-back.  Three operations:
//   (a) weights + dead list: a reduce-then-scan over blocks of kItems Gaussians (weights_kernel, scan_blocks_kernel,
//       scan_apply_kernel).  The sums of w are fp64 at every level; the scan also compacts the rows of positive weight
//       into (cdf, live) so that the sampler can only ever return one of them, whatever the last bits of the sums do.
//   (b) sample_kernel (one thread per target: a binary search of the compacted cdf, an integer atomic per draw),
//       update_sources_kernel (one thread per Gaussian: the one writer of a drawn source's new opacity and scale, in
//       fp64 -- the alternating sum D has a condition number of 4e4 at r = 51) and copy_rows_kernel (one thread per
//       float of a target row, all groups in one launch).
//   (c) noise_kernel: streaming, four Gaussians per thread so that the 12- and 4-byte rows are whole float4s of the flat
//       arrays (as optim.hip reads its rows).
// Hand-written scans through LDS; no rocPRIM.  Counts stay on the device: grids are sized by n and exit early.
#include <algorithm>
#include <cmath>

#include "mgs_common.h"
#include "mgs_math.h"
#include "../../include/mgs_refine.h"

namespace mgs {
namespace {

constexpr int kBlock = 256;
constexpr int kPerThread = 4;
constexpr int kItems = kBlock * kPerThread;    // Gaussians per workgroup of the scan
constexpr unsigned kMaxBlocks = 2048;          // grid cap of the grid-stride launches
constexpr int kMaxGroups = MGS_REFINE_MAX_GROUPS;
constexpr double kMaxOpacity = 1.0 - 1.1920928955078125e-07;    // 1 - 2^-23
constexpr uint32_t kLeadBit = 0x80000000u;

struct Rec {           // per scan block: its sums (after weights_kernel), then its exclusive offsets (scan_blocks_kernel)
  double sum;
  uint32_t dead, live;
};

struct Part {
  double s;
  uint32_t d, l;
};
__device__ __forceinline__ Part operator+(const Part& a, const Part& b) { return {a.s + b.s, a.d + b.d, a.l + b.l}; }

// Inclusive scan of one Part per thread over the workgroup (Hillis-Steele through LDS: eight steps).  Returns the
// inclusive value; `excl` the exclusive one and `total` the workgroup's.  Ends with a barrier: lds may be reused at once.
__device__ __forceinline__ Part block_scan(Part v, Part* lds, Part& excl, Part& total) {
  const int t = threadIdx.x;
  lds[t] = v;
  __syncthreads();
  for (int d = 1; d < kBlock; d <<= 1) {
    Part add{0.0, 0u, 0u};
    if (t >= d) add = lds[t - d];
    __syncthreads();
    if (t >= d) lds[t] = add + lds[t];        // earlier + later: the order of the indices
    __syncthreads();
  }
  const Part incl = lds[t];
  excl = t ? lds[t - 1] : Part{0.0, 0u, 0u};
  total = lds[kBlock - 1];
  __syncthreads();
  return incl;
}

// four consecutive floats of a flat array of n, zero beyond its end (a float4 where all four exist; p is 16-byte aligned)
__device__ __forceinline__ void load4(const float* p, uint32_t at, uint32_t n, float x[4]) {
  if (at + 4 <= n) {
    const float4 q = *reinterpret_cast<const float4*>(p + at);
    x[0] = q.x, x[1] = q.y, x[2] = q.z, x[3] = q.w;
  } else {
#pragma unroll
    for (int k = 0; k < 4; ++k) x[k] = at + k < n ? p[at + k] : 0.f;
  }
}

// (a) first pass: w and the zeroed draw counts of a block of kItems Gaussians, and the block's sums.
__global__ __launch_bounds__(kBlock) void weights_kernel(uint32_t n, const float* __restrict__ logits, float min_opacity,
                                                         int mode, float* __restrict__ w, uint32_t* __restrict__ draws,
                                                         Rec* __restrict__ recs) {
  __shared__ Part lds[kBlock];
  const uint32_t at = blockIdx.x * (uint32_t)kItems + threadIdx.x * kPerThread;
  float x[4];
  load4(logits, at, n, x);
  Part mine{0.0, 0u, 0u};
  float wv[4];
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    const bool in = at + k < n;
    const float o = activate_opacity(x[k]);
    const bool dead = o <= min_opacity;
    wv[k] = (!in || (dead && mode == MGS_MCMC_RELOCATE)) ? 0.f : o;
    mine.s += (double)wv[k];
    mine.d += (in && dead) ? 1u : 0u;
    mine.l += wv[k] > 0.f ? 1u : 0u;
  }
  if (at + 4 <= n) {
    *reinterpret_cast<float4*>(w + at) = make_float4(wv[0], wv[1], wv[2], wv[3]);
    *reinterpret_cast<uint4*>(draws + at) = make_uint4(0u, 0u, 0u, 0u);
  } else {
#pragma unroll
    for (int k = 0; k < 4; ++k)
      if (at + k < n) w[at + k] = wv[k], draws[at + k] = 0u;
  }
  Part excl, total;
  block_scan(mine, lds, excl, total);
  if (threadIdx.x == 0) recs[blockIdx.x] = Rec{total.s, total.d, total.l};
}

// (a) second pass, ONE workgroup: the block sums become exclusive offsets, kBlock of them per round with a carry.
__global__ __launch_bounds__(kBlock) void scan_blocks_kernel(uint32_t n_blocks, Rec* __restrict__ recs,
                                                             mgs_mcmc_stats* __restrict__ stats) {
  __shared__ Part lds[kBlock];
  Part carry{0.0, 0u, 0u};
  for (uint32_t base = 0; base < n_blocks; base += kBlock) {
    const uint32_t b = base + threadIdx.x;
    Part mine{0.0, 0u, 0u};
    if (b < n_blocks) mine = Part{recs[b].sum, recs[b].dead, recs[b].live};
    Part excl, total;
    block_scan(mine, lds, excl, total);
    if (b < n_blocks) {
      const Part off = carry + excl;
      recs[b] = Rec{off.s, off.d, off.l};
    }
    carry = carry + total;
  }
  if (threadIdx.x == 0) {
    stats->total = carry.s;
    stats->n_dead = (int32_t)carry.d;
    stats->n_live = (int32_t)carry.l;
  }
}

// (a) third pass: the scan inside each block on top of its offsets.  Dead rows (w <= min_opacity: 0 in relocate mode,
// o in add mode) go to dead[] in index order; rows of positive weight go to (cdf, live) in index order.
__global__ __launch_bounds__(kBlock) void scan_apply_kernel(uint32_t n, const float* __restrict__ w, float min_opacity,
                                                            const Rec* __restrict__ recs, int32_t* __restrict__ dead,
                                                            double* __restrict__ cdf, uint32_t* __restrict__ live) {
  __shared__ Part lds[kBlock];
  const uint32_t at = blockIdx.x * (uint32_t)kItems + threadIdx.x * kPerThread;
  float wv[4];
  load4(w, at, n, wv);
  Part mine{0.0, 0u, 0u};
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    const bool in = at + k < n;
    mine.s += (double)wv[k];
    mine.d += (in && wv[k] <= min_opacity) ? 1u : 0u;
    mine.l += wv[k] > 0.f ? 1u : 0u;
  }
  Part excl, total;
  block_scan(mine, lds, excl, total);
  const Rec off = recs[blockIdx.x];
  const double base = off.sum + excl.s;
  uint32_t d = off.dead + excl.d, l = off.live + excl.l;      // < n: every slot written belongs to a row < n
  double run = 0.0;
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    if (at + k >= n) break;
    run += (double)wv[k];
    if (wv[k] <= min_opacity) dead[d++] = (int32_t)(at + k);
    if (wv[k] > 0.f) {
      cdf[l] = base + run;
      live[l++] = at + k;
    }
  }
}

// (b) one thread per target: draw its source.  tsrc[j] = source | kLeadBit for the first draw of that source.
__global__ __launch_bounds__(kBlock) void sample_kernel(int mode, uint32_t max_targets, const mgs_mcmc_stats* __restrict__ stats,
                                                        const float* __restrict__ u, const double* __restrict__ cdf,
                                                        const uint32_t* __restrict__ live, uint32_t* __restrict__ draws,
                                                        uint32_t* __restrict__ tsrc, int32_t* __restrict__ sources) {
  const uint32_t j = blockIdx.x * (uint32_t)kBlock + threadIdx.x;
  const uint32_t targets = mode == MGS_MCMC_RELOCATE ? min((uint32_t)stats->n_dead, max_targets) : max_targets;
  const uint32_t n_live = (uint32_t)stats->n_live;
  const double T = stats->total;
  if (j >= targets || n_live == 0 || !(T > 0.0)) return;
  const double x = (double)u[j] * T;
  uint32_t lo = 0, hi = n_live;                // the smallest k with cdf[k] > x, n_live if there is none
  while (lo < hi) {
    const uint32_t mid = lo + (hi - lo) / 2;
    if (cdf[mid] > x) hi = mid;
    else lo = mid + 1;
  }
  if (lo >= n_live) lo = n_live - 1;           // u T >= T by rounding: the last row of positive weight
  const uint32_t src = live[lo];
  const uint32_t before = atomicAdd(draws + src, 1u);
  tsrc[j] = src | (before == 0 ? kLeadBit : 0u);
  sources[j] = (int32_t)src;
}

// (b) one thread per Gaussian: a drawn source's new opacity and scale, in fp64, stored once.
__global__ __launch_bounds__(kBlock) void update_sources_kernel(uint32_t n, const uint32_t* __restrict__ draws,
                                                                float min_opacity, float* __restrict__ logits,
                                                                float* __restrict__ log_scales) {
  const uint32_t i = blockIdx.x * (uint32_t)kBlock + threadIdx.x;
  if (i >= n) return;
  const uint32_t c = draws[i];
  if (c == 0) return;
  const int r = (int)min(c + 1u, (uint32_t)MGS_MCMC_MAX_RATIO);
  double o = 1.0 / (1.0 + exp(-(double)logits[i]));
  o = fmin(o, kMaxOpacity);
  // 1 - (1 - o)^(1/r) without the cancellation of the plain form at small o
  const double o_new = -expm1(log1p(-o) / (double)r);
  double D = 0.0, binom = 1.0, power = 1.0;    // C(r, k+1) by its recurrence (exact below 2^53 but for one rounding each)
  for (int k = 0; k < r; ++k) {
    binom = binom * (double)(r - k) / (double)(k + 1);
    power *= o_new;
    const double term = binom * power / sqrt((double)(k + 1));
    D += (k & 1) ? -term : term;
  }
  const double kept = fmin(fmax(o_new, (double)min_opacity), kMaxOpacity);
  logits[i] = (float)log(kept / (1.0 - kept));
  const float shift = (float)log(o / D);
  const size_t s = (size_t)3 * i;
  log_scales[s] += shift, log_scales[s + 1] += shift, log_scales[s + 2] += shift;
}

struct CopyGroup {
  float* p;
  float* m;
  float* v;
  uint32_t row, first;     // floats per row; this group's first float within the concatenated row
};
struct CopyArgs {
  CopyGroup grp[kMaxGroups];
  int n_groups;
  uint32_t row_sum;        // floats of one Gaussian over all groups
};

// (b) one thread per float of a target row (all groups concatenated), grid-stride: the row of the source, copied.
__global__ __launch_bounds__(kBlock) void copy_rows_kernel(const CopyArgs a, int mode, uint32_t n, uint32_t max_targets,
                                                           const mgs_mcmc_stats* __restrict__ stats,
                                                           const int32_t* __restrict__ dead, const uint32_t* __restrict__ tsrc) {
  const uint32_t targets = mode == MGS_MCMC_RELOCATE ? min((uint32_t)stats->n_dead, max_targets) : max_targets;
  if (stats->n_live == 0 || !(stats->total > 0.0)) return;
  const uint64_t work = (uint64_t)targets * a.row_sum;
  for (uint64_t e = (uint64_t)blockIdx.x * kBlock + threadIdx.x; e < work; e += (uint64_t)gridDim.x * kBlock) {
    const uint32_t j = (uint32_t)(e / a.row_sum);
    const uint32_t f = (uint32_t)(e - (uint64_t)j * a.row_sum);
    int gi = 0;
    while (gi + 1 < a.n_groups && f >= a.grp[gi + 1].first) ++gi;
    const CopyGroup& G = a.grp[gi];
    const uint32_t k = f - G.first;
    const uint32_t word = tsrc[j];
    const size_t src = (size_t)(word & ~kLeadBit) * G.row + k;
    const size_t dst = (size_t)(mode == MGS_MCMC_RELOCATE ? (uint32_t)dead[j] : n + j) * G.row + k;
    G.p[dst] = G.p[src];
    if (G.m) {
      if (mode == MGS_MCMC_ADD) G.m[dst] = 0.f, G.v[dst] = 0.f;
      else if (word & kLeadBit) G.m[src] = 0.f, G.v[src] = 0.f;
    }
  }
}

// (c) four Gaussians per thread.
struct NoiseArgs {
  float* means;
  const float* quats;
  const float* scales;
  const float* logits;
  const float* z;
  uint32_t n;
  double noise_lr, lr, log_ratio;
  int decay_steps;
  const int32_t* state;
};

__device__ __forceinline__ void noise_one(const float q[4], const float ls[3], float logit, const float z[3], float lambda,
                                          float mean[3]) {
  float R[9];
  quat_to_rotmat(q, R);
  const float rest = 1.0f / (1.0f + expf(logit));                         // 1 - o, without the subtraction
  const float gate = 1.0f / (1.0f + expf(-100.0f * (rest - 0.995f)));
  const float g = gate * lambda;
  const float v[3] = {z[0] * g, z[1] * g, z[2] * g};
  float t[3];
#pragma unroll
  for (int k = 0; k < 3; ++k)                                              // diag(s^2) R^T v
    t[k] = expf(2.0f * ls[k]) * fmaf(R[6 + k], v[2], fmaf(R[3 + k], v[1], R[k] * v[0]));
#pragma unroll
  for (int k = 0; k < 3; ++k)
    mean[k] += fmaf(R[3 * k + 2], t[2], fmaf(R[3 * k + 1], t[1], R[3 * k] * t[0]));
}

__global__ __launch_bounds__(kBlock) void noise_kernel(const NoiseArgs a) {
  double rate = a.lr;
  if (a.state && a.decay_steps > 0)
    rate *= exp(a.log_ratio * ((double)min(max(a.state[0], 0), a.decay_steps) / (double)a.decay_steps));
  const float lambda = (float)(a.noise_lr * rate);
  const uint32_t quads = a.n / 4;
  for (uint32_t i = blockIdx.x * (uint32_t)kBlock + threadIdx.x; i < quads; i += gridDim.x * (uint32_t)kBlock) {
    float m[12], s[12], z[12], q[16], o[4];
    float4* m4 = reinterpret_cast<float4*>(a.means) + (size_t)3 * i;
    const float4* s4 = reinterpret_cast<const float4*>(a.scales) + (size_t)3 * i;
    const float4* z4 = reinterpret_cast<const float4*>(a.z) + (size_t)3 * i;
    const float4* q4 = reinterpret_cast<const float4*>(a.quats) + (size_t)4 * i;
#pragma unroll
    for (int k = 0; k < 3; ++k) {
      const float4 x = m4[k], y = s4[k], w = z4[k];
      m[4 * k] = x.x, m[4 * k + 1] = x.y, m[4 * k + 2] = x.z, m[4 * k + 3] = x.w;
      s[4 * k] = y.x, s[4 * k + 1] = y.y, s[4 * k + 2] = y.z, s[4 * k + 3] = y.w;
      z[4 * k] = w.x, z[4 * k + 1] = w.y, z[4 * k + 2] = w.z, z[4 * k + 3] = w.w;
    }
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      const float4 x = q4[k];
      q[4 * k] = x.x, q[4 * k + 1] = x.y, q[4 * k + 2] = x.z, q[4 * k + 3] = x.w;
    }
    {
      const float4 x = reinterpret_cast<const float4*>(a.logits)[i];
      o[0] = x.x, o[1] = x.y, o[2] = x.z, o[3] = x.w;
    }
#pragma unroll
    for (int k = 0; k < 4; ++k) noise_one(q + 4 * k, s + 3 * k, o[k], z + 3 * k, lambda, m + 3 * k);
#pragma unroll
    for (int k = 0; k < 3; ++k) m4[k] = make_float4(m[4 * k], m[4 * k + 1], m[4 * k + 2], m[4 * k + 3]);
  }
  if (blockIdx.x == 0 && threadIdx.x < (a.n & 3u)) {      // the last n % 4 Gaussians, one thread each
    const size_t i = (size_t)4 * quads + threadIdx.x;
    float m[3] = {a.means[3 * i], a.means[3 * i + 1], a.means[3 * i + 2]};
    noise_one(a.quats + 4 * i, a.scales + 3 * i, a.logits[i], a.z + 3 * i, lambda, m);
    a.means[3 * i] = m[0], a.means[3 * i + 1] = m[1], a.means[3 * i + 2] = m[2];
  }
}

bool aligned16(const void* p) { return ((uintptr_t)p & 15) == 0; }

struct Layout {
  size_t recs, cdf, live, draws, tsrc, total;
};
Layout layout(uint64_t n, uint64_t max_targets) {
  Bump b(1);
  Layout L;
  L.recs = b.take(sizeof(Rec) * ((n + kItems - 1) / kItems));
  L.cdf = b.take(sizeof(double) * n);
  L.live = b.take(sizeof(uint32_t) * n);
  L.draws = b.take(sizeof(uint32_t) * n);
  L.tsrc = b.take(sizeof(uint32_t) * max_targets);
  L.total = b.total;
  return L;
}

int check_weights_args(const char* what, int64_t n, const float* opacities, float min_opacity, int mode, const float* w,
                       const int32_t* dead, const mgs_mcmc_stats* stats) {
  MGS_REQUIRE(n >= 0 && n < (1ll << 31), "%s: n %lld not in 0..2^31-1", what, (long long)n);
  MGS_REQUIRE(mode == MGS_MCMC_RELOCATE || mode == MGS_MCMC_ADD, "%s: mode %d is neither MGS_MCMC_RELOCATE nor MGS_MCMC_ADD",
              what, mode);
  MGS_REQUIRE(min_opacity > 0.f && min_opacity < 1.f, "%s: min_opacity %g not in (0, 1)", what, (double)min_opacity);
  MGS_REQUIRE(opacities && w && dead && stats, "%s: opacities, w, dead or stats is null", what);
  MGS_REQUIRE(aligned16(opacities), "%s: opacities is not 16-byte aligned", what);
  MGS_REQUIRE(aligned16(w), "%s: w is not 16-byte aligned", what);
  MGS_REQUIRE(((uintptr_t)stats & 7) == 0, "%s: stats is not 8-byte aligned", what);
  return MGS_OK;
}

// the three launches of (a); ws is the workspace of layout(n, .)
void enqueue_weights(uint32_t n, const float* opacities, float min_opacity, int mode, float* w, int32_t* dead,
                     mgs_mcmc_stats* stats, char* ws, const Layout& L, hipStream_t s) {
  const unsigned blocks = div_up(n, kItems);
  Rec* recs = reinterpret_cast<Rec*>(ws + L.recs);
  if (blocks)
    hipLaunchKernelGGL(weights_kernel, dim3(blocks), dim3(kBlock), 0, s, n, opacities, min_opacity, mode, w,
                       reinterpret_cast<uint32_t*>(ws + L.draws), recs);
  hipLaunchKernelGGL(scan_blocks_kernel, dim3(1), dim3(kBlock), 0, s, blocks, recs, stats);
  if (blocks)
    hipLaunchKernelGGL(scan_apply_kernel, dim3(blocks), dim3(kBlock), 0, s, n, (const float*)w, min_opacity,
                       (const Rec*)recs, dead, reinterpret_cast<double*>(ws + L.cdf),
                       reinterpret_cast<uint32_t*>(ws + L.live));
}

}  // namespace
}  // namespace mgs

using namespace mgs;

extern "C" int mgs_mcmc_weights(int64_t n, const float* opacities, float min_opacity, int mode, float* w, int32_t* dead,
                                mgs_mcmc_stats* stats, void* workspace, size_t* workspace_bytes, mgs_stream_t stream) {
  MGS_REQUIRE(workspace_bytes, "mcmc_weights: workspace_bytes is null");
  MGS_REQUIRE(n >= 0 && n < (1ll << 31), "mcmc_weights: n %lld not in 0..2^31-1", (long long)n);
  const Layout L = layout((uint64_t)n, 0);
  if (!workspace) {
    *workspace_bytes = L.total;
    return MGS_OK;
  }
  if (int rc = check_weights_args("mcmc_weights", n, opacities, min_opacity, mode, w, dead, stats)) return rc;
  MGS_REQUIRE(*workspace_bytes >= L.total, "mcmc_weights: workspace of %zu bytes, %zu needed", *workspace_bytes, L.total);
  MGS_REQUIRE(((uintptr_t)workspace & 255) == 0, "mcmc_weights: workspace is not 256-byte aligned");
  enqueue_weights((uint32_t)n, opacities, min_opacity, mode, w, dead, stats, static_cast<char*>(workspace), L,
                  (hipStream_t)stream);
  return check_launch("mcmc_weights");
}

extern "C" int mgs_mcmc_relocate(int mode, int64_t n, int64_t n_new, int64_t capacity, float* opacities, float* scales,
                                 int n_groups, const mgs_refine_group* groups, float min_opacity, const float* u, float* w,
                                 int32_t* dead, mgs_mcmc_stats* stats, int32_t* sources, void* workspace,
                                 size_t* workspace_bytes, mgs_stream_t stream) {
  MGS_REQUIRE(workspace_bytes, "mcmc_relocate: workspace_bytes is null");
  MGS_REQUIRE(n >= 0 && n < (1ll << 31), "mcmc_relocate: n %lld not in 0..2^31-1", (long long)n);
  MGS_REQUIRE(mode == MGS_MCMC_RELOCATE || mode == MGS_MCMC_ADD,
              "mcmc_relocate: mode %d is neither MGS_MCMC_RELOCATE nor MGS_MCMC_ADD", mode);
  MGS_REQUIRE(capacity >= n && capacity < (1ll << 31), "mcmc_relocate: capacity %lld not in n = %lld..2^31-1",
              (long long)capacity, (long long)n);
  if (mode == MGS_MCMC_RELOCATE) n_new = 0;
  MGS_REQUIRE(n_new >= 0 && n_new <= capacity - n, "mcmc_relocate: the append range [%lld, %lld) does not fit capacity %lld",
              (long long)n, (long long)(n + n_new), (long long)capacity);
  const uint64_t max_targets = mode == MGS_MCMC_RELOCATE ? (uint64_t)n : (uint64_t)n_new;
  const Layout L = layout((uint64_t)n, max_targets);
  if (!workspace) {
    *workspace_bytes = L.total;
    return MGS_OK;
  }
  if (int rc = check_weights_args("mcmc_relocate", n, opacities, min_opacity, mode, w, dead, stats)) return rc;
  MGS_REQUIRE(scales && u && sources, "mcmc_relocate: scales, u or sources is null");
  MGS_REQUIRE(n_groups >= 1 && n_groups <= kMaxGroups, "mcmc_relocate: n_groups %d not in 1..%d", n_groups, kMaxGroups);
  MGS_REQUIRE(groups, "mcmc_relocate: groups is null");
  CopyArgs a{};
  uint64_t row_sum = 0;
  for (int k = 0; k < n_groups; ++k) {
    const mgs_refine_group& h = groups[k];
    MGS_REQUIRE(h.row_floats >= 1, "mcmc_relocate: groups[%d].row_floats %d < 1", k, (int)h.row_floats);
    MGS_REQUIRE((uint64_t)capacity * (uint64_t)h.row_floats < (1ull << 32),
                "mcmc_relocate: groups[%d]: capacity * row_floats must be below 2^32", k);
    MGS_REQUIRE(h.param, "mcmc_relocate: groups[%d].param is null", k);
    MGS_REQUIRE(!h.exp_avg == !h.exp_avg_sq, "mcmc_relocate: groups[%d] has one moment and not the other", k);
    MGS_REQUIRE(aligned16(h.param), "mcmc_relocate: groups[%d].param is not 16-byte aligned", k);
    MGS_REQUIRE(aligned16(h.exp_avg), "mcmc_relocate: groups[%d].exp_avg is not 16-byte aligned", k);
    MGS_REQUIRE(aligned16(h.exp_avg_sq), "mcmc_relocate: groups[%d].exp_avg_sq is not 16-byte aligned", k);
    a.grp[k] = CopyGroup{h.param, h.exp_avg, h.exp_avg_sq, (uint32_t)h.row_floats, (uint32_t)row_sum};
    row_sum += (uint64_t)h.row_floats;
  }
  MGS_REQUIRE(row_sum < (1ull << 31), "mcmc_relocate: %llu floats per Gaussian", (unsigned long long)row_sum);
  a.n_groups = n_groups, a.row_sum = (uint32_t)row_sum;
  MGS_REQUIRE(*workspace_bytes >= L.total, "mcmc_relocate: workspace of %zu bytes, %zu needed", *workspace_bytes, L.total);
  MGS_REQUIRE(((uintptr_t)workspace & 255) == 0, "mcmc_relocate: workspace is not 256-byte aligned");
  char* ws = static_cast<char*>(workspace);
  hipStream_t s = (hipStream_t)stream;
  enqueue_weights((uint32_t)n, opacities, min_opacity, mode, w, dead, stats, ws, L, s);
  if (n > 0 && max_targets > 0) {
    uint32_t* draws = reinterpret_cast<uint32_t*>(ws + L.draws);
    uint32_t* tsrc = reinterpret_cast<uint32_t*>(ws + L.tsrc);
    hipLaunchKernelGGL(sample_kernel, dim3(div_up((unsigned)max_targets, kBlock)), dim3(kBlock), 0, s, mode,
                       (uint32_t)max_targets, (const mgs_mcmc_stats*)stats, u, reinterpret_cast<const double*>(ws + L.cdf),
                       reinterpret_cast<const uint32_t*>(ws + L.live), draws, tsrc, sources);
    hipLaunchKernelGGL(update_sources_kernel, dim3(div_up((unsigned)n, kBlock)), dim3(kBlock), 0, s, (uint32_t)n,
                       (const uint32_t*)draws, min_opacity, opacities, scales);
    const uint64_t work = max_targets * row_sum;
    const unsigned grid = (unsigned)std::min<uint64_t>((work + kBlock - 1) / kBlock, kMaxBlocks);
    hipLaunchKernelGGL(copy_rows_kernel, dim3(grid), dim3(kBlock), 0, s, a, mode, (uint32_t)n, (uint32_t)max_targets,
                       (const mgs_mcmc_stats*)stats, (const int32_t*)dead, (const uint32_t*)tsrc);
  }
  return check_launch("mcmc_relocate");
}

extern "C" int mgs_mcmc_noise(int64_t n, float* means, const float* quats, const float* scales, const float* opacities,
                              const float* z, double noise_lr, double lr, double lr_final, int32_t decay_steps,
                              const int32_t* step_state, mgs_stream_t stream) {
  MGS_REQUIRE(n >= 0 && n < (1ll << 30), "mcmc_noise: n %lld not in 0..2^30-1", (long long)n);
  MGS_REQUIRE(means && quats && scales && opacities && z, "mcmc_noise: means, quats, scales, opacities or z is null");
  MGS_REQUIRE(aligned16(means), "mcmc_noise: means is not 16-byte aligned");
  MGS_REQUIRE(aligned16(quats), "mcmc_noise: quats is not 16-byte aligned");
  MGS_REQUIRE(aligned16(scales), "mcmc_noise: scales is not 16-byte aligned");
  MGS_REQUIRE(aligned16(opacities), "mcmc_noise: opacities is not 16-byte aligned");
  MGS_REQUIRE(aligned16(z), "mcmc_noise: z is not 16-byte aligned");
  MGS_REQUIRE(noise_lr >= 0.0 && std::isfinite(noise_lr), "mcmc_noise: noise_lr %g", noise_lr);
  MGS_REQUIRE(lr >= 0.0 && std::isfinite(lr), "mcmc_noise: lr %g", lr);
  MGS_REQUIRE(decay_steps >= 0, "mcmc_noise: decay_steps %d is negative", (int)decay_steps);
  MGS_REQUIRE(decay_steps == 0 || (lr > 0.0 && lr_final > 0.0 && std::isfinite(lr_final)),
              "mcmc_noise: a schedule needs lr and lr_final > 0 (lr %g, lr_final %g)", lr, lr_final);
  if (n == 0) return MGS_OK;
  NoiseArgs a{};
  a.means = means, a.quats = quats, a.scales = scales, a.logits = opacities, a.z = z;
  a.n = (uint32_t)n;
  a.noise_lr = noise_lr, a.lr = lr;
  a.log_ratio = decay_steps ? std::log(lr_final / lr) : 0.0;
  a.decay_steps = decay_steps;
  a.state = step_state;
  const unsigned grid = std::max(1u, std::min(div_up((unsigned)(n / 4), kBlock), kMaxBlocks));
  hipLaunchKernelGGL(noise_kernel, dim3(grid), dim3(kBlock), 0, (hipStream_t)stream, a);
  return check_launch("mcmc_noise");
}
