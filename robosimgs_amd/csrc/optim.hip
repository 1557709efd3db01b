// optim.hip -- the optimiser half of the training step: torch.optim.Adam's update of every parameter group of a
// Gaussian scene in ONE streaming launch (include/mgs_optim.h), with what a captured splatfacto step needs and
// torch's optimiser does not have: the step counter and the learning-rate schedule live on the device (a replayed graph
// takes update t + 1), a row of a group can train at two rates (features_dc / features_rest inside one [N, K, 3]
// tensor), and the Gaussians no camera saw are skipped (gsplat's SelectiveAdam) -- they cost the read of their radii.
// HBM-bound: 16 B read and 12 B written per element, 16-byte accesses over the flat arrays, no LDS, no float atomics.
// Every element is updated by one thread in one evaluation order (explicit fmaf, the same inlined body under every
// visibility form), so the result is bit-reproducible and a masked call equals the unmasked one on the rows it touches.
#include <algorithm>
#include <cmath>

#include "mgs_common.h"
#include "../../include/mgs_optim.h"

namespace mgs {
namespace {

constexpr int kBlock = 256;
constexpr unsigned kMaxBlocks = 2048;      // grid cap; the rest is a grid-stride loop per group
constexpr int kMaxGroups = MGS_ADAM_MAX_GROUPS;

enum { kVisAll = 0, kVisRadii = 1, kVisMask = 2 };

struct Group {
  float* p;
  const float* g;
  float* m;
  float* v;
  uint32_t total;        // n * row_floats
  uint32_t row, head;    // head == row where the row is not split
  int decay_steps;
  double lr, log_ratio /* ln(lr_final / lr) */, rest_scale;
};

struct AdamArgs {
  Group grp[kMaxGroups];
  uint32_t first_block[kMaxGroups + 1];   // prefix sum of the groups' workgroup counts
  int n_groups;
  double ln_b1, ln_b2;
  float b1, omb1, b2, omb2, eps;
  int32_t* state;                         // { steps taken, ticket }
  const int32_t* radii;
  const int32_t* radii_y;
  int n_cams;
  size_t cam_stride;
  const uint8_t* mask;
};

// the per-step scalars of one group, the same in every thread of the launch
struct Coef {
  float b1, omb1, b2, omb2, eps;
  float sqrt_bc2;       // sqrt(1 - beta2^t)
  float step[2];         // lr_t / (1 - beta1^t) for the head and for the rest of a row
};

// One element.  Roundings (u = 2^-24): m' 3u and v' 3u of their magnitude sums (beta and 1 - beta as floats, one product,
// the fma); the step sqrtf, the division by sqrt(1 - beta2^t) (itself rounded once), + eps, m' / denominator, the step
// size rounded once, the final fma.
__device__ __forceinline__ void adam_element(const Coef& c, float step, float g, float& p, float& m, float& v) {
  m = fmaf(c.omb1, g, c.b1 * m);
  v = fmaf(c.omb2 * g, g, c.b2 * v);
  const float den = sqrtf(v) / c.sqrt_bc2 + c.eps;
  p = fmaf(-step, m / den, p);
}

// 16-byte accesses marked non-temporal: every byte of the update is touched once per step and the 1.65 GB of a 1 M
// Gaussian scene pass through the caches for nothing.  Measured at that size: 330 -> 317 us unmasked, 321 -> 262 us with
// half of the Gaussians visible (profiles/optim/README.md).
typedef float f4 __attribute__((ext_vector_type(4)));
__device__ __forceinline__ float4 load_once(const float4* q) {
  const f4 x = __builtin_nontemporal_load(reinterpret_cast<const f4*>(q));
  return make_float4(x.x, x.y, x.z, x.w);
}
__device__ __forceinline__ void store_once(float4* q, float4 x) {
  const f4 y = {x.x, x.y, x.z, x.w};
  __builtin_nontemporal_store(y, reinterpret_cast<f4*>(q));
}

template <int kVis> __device__ __forceinline__ bool visible(const AdamArgs& a, uint32_t gauss) {
  if constexpr (kVis == kVisAll) return true;
  if constexpr (kVis == kVisMask) return a.mask[gauss] != 0;
  bool vis = false;
  for (int c = 0; c < a.n_cams; ++c) {
    const size_t at = (size_t)c * a.cam_stride + gauss;
    vis |= a.radii[at] > 0;
    if (a.radii_y) vis |= a.radii_y[at] > 0;
  }
  return vis;
}

template <int kVis> __global__ __launch_bounds__(kBlock) void adam_step_kernel(const AdamArgs a) {
  // Every thread reads the counter before anything else; it is stored again only after every workgroup of the launch
  // has passed the barrier below, so no late-starting workgroup sees the advanced value.
  const int t = a.state[0] + 1;
  int gi = 0;
  while (gi < a.n_groups && blockIdx.x >= a.first_block[gi + 1]) ++gi;
  if (gi < a.n_groups) {
    const Group& G = a.grp[gi];
    Coef c;
    c.b1 = a.b1, c.omb1 = a.omb1, c.b2 = a.b2, c.omb2 = a.omb2, c.eps = a.eps;
    {  // fp64: 1 - beta^t has no digits left in fp32 at small t
      const double bc1 = -expm1((double)t * a.ln_b1), bc2 = -expm1((double)t * a.ln_b2);
      double lr = G.lr;
      if (G.decay_steps > 0)
        lr *= exp(G.log_ratio * ((double)min(t - 1, G.decay_steps) / (double)G.decay_steps));
      c.sqrt_bc2 = (float)sqrt(bc2);
      c.step[0] = (float)(lr / bc1);
      c.step[1] = (float)(lr * G.rest_scale / bc1);
    }
    const uint32_t row = G.row, head = G.head;
    const uint32_t n4 = G.total / 4;
    const uint32_t stride = (a.first_block[gi + 1] - a.first_block[gi]) * kBlock;
    const uint32_t first = (blockIdx.x - a.first_block[gi]) * kBlock + threadIdx.x;
    float4* p4 = reinterpret_cast<float4*>(G.p);
    const float4* g4 = reinterpret_cast<const float4*>(G.g);
    float4* m4 = reinterpret_cast<float4*>(G.m);
    float4* v4 = reinterpret_cast<float4*>(G.v);
    for (uint32_t i = first; i < n4; i += stride) {
      // the Gaussian and the row offset of each of the four elements: a float4 may straddle rows
      uint32_t q = (4 * i) / row, r = 4 * i - q * row;
      float step[4];
      bool vis[4];
      uint32_t q_prev = 0;
#pragma unroll
      for (int k = 0; k < 4; ++k) {
        step[k] = r < head ? c.step[0] : c.step[1];
        vis[k] = (k > 0 && q == q_prev) ? vis[k - 1] : visible<kVis>(a, q);
        q_prev = q;
        if (++r == row) r = 0, ++q;
      }
      if ((vis[0] && vis[1]) && (vis[2] && vis[3])) {
        float4 p = load_once(p4 + i), m = load_once(m4 + i), v = load_once(v4 + i);
        const float4 g = load_once(g4 + i);
        adam_element(c, step[0], g.x, p.x, m.x, v.x);
        adam_element(c, step[1], g.y, p.y, m.y, v.y);
        adam_element(c, step[2], g.z, p.z, m.z, v.z);
        adam_element(c, step[3], g.w, p.w, m.w, v.w);
        store_once(p4 + i, p), store_once(m4 + i, m), store_once(v4 + i, v);
      } else if constexpr (kVis != kVisAll) {
        // a float4 across a visible and an invisible Gaussian: the visible elements one by one, the others untouched
#pragma unroll
        for (int k = 0; k < 4; ++k)
          if (vis[k]) {
            const size_t e = (size_t)4 * i + k;
            float p = G.p[e], m = G.m[e], v = G.v[e];
            adam_element(c, step[k], G.g[e], p, m, v);
            G.p[e] = p, G.m[e] = m, G.v[e] = v;
          }
      }
    }
    if (blockIdx.x == a.first_block[gi] && threadIdx.x < (G.total & 3)) {   // scalar tail
      const uint32_t e = 4 * n4 + threadIdx.x;
      const uint32_t q = e / row, r = e - q * row;
      if (visible<kVis>(a, q)) {
        float p = G.p[e], m = G.m[e], v = G.v[e];
        adam_element(c, r < head ? c.step[0] : c.step[1], G.g[e], p, m, v);
        G.p[e] = p, G.m[e] = m, G.v[e] = v;
      }
    }
  }
  // The last workgroup to retire advances the counter and clears the ticket for the next launch.  Relaxed: the ticket
  // orders nothing but the counter, which every thread of a ticketed workgroup has long read (an agent-scope release
  // here would write back the XCD's dirty L2 lines -- the whole update; see loss.hip).
  __syncthreads();
  if (threadIdx.x == 0) {
    const int taken = __hip_atomic_fetch_add(a.state + 1, 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    if (taken == (int)gridDim.x - 1) {
      __hip_atomic_store(a.state, t, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
      __hip_atomic_store(a.state + 1, 0, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
  }
}

bool aligned16(const void* p) { return ((uintptr_t)p & 15) == 0; }

}  // namespace
}  // namespace mgs

using namespace mgs;

extern "C" int mgs_adam_step(int n_groups, const mgs_adam_group* groups, double beta1, double beta2, double eps,
                             int32_t* step_state, const int32_t* radii, const int32_t* radii_y, int n_cams,
                             size_t cam_stride, const uint8_t* mask, mgs_stream_t stream) {
  MGS_REQUIRE(n_groups >= 1 && n_groups <= kMaxGroups, "adam_step: n_groups %d not in 1..%d", n_groups, kMaxGroups);
  MGS_REQUIRE(groups, "adam_step: groups is null");
  MGS_REQUIRE(beta1 >= 0.0 && beta1 < 1.0, "adam_step: beta1 %g not in [0, 1)", beta1);
  MGS_REQUIRE(beta2 >= 0.0 && beta2 < 1.0, "adam_step: beta2 %g not in [0, 1)", beta2);
  MGS_REQUIRE(eps >= 0.0, "adam_step: eps %g is negative", eps);
  MGS_REQUIRE(!(radii && mask), "adam_step: both radii and mask are given (visibility takes one form)");
  MGS_REQUIRE(radii || !radii_y, "adam_step: radii_y without radii");
  MGS_REQUIRE(!radii || n_cams >= 1, "adam_step: n_cams %d with radii given", n_cams);
  const bool masked = radii || mask;
  AdamArgs a{};
  uint64_t work = 0;
  for (int k = 0; k < n_groups; ++k) {
    const mgs_adam_group& h = groups[k];
    MGS_REQUIRE(h.row_floats >= 1, "adam_step: groups[%d].row_floats %d < 1", k, (int)h.row_floats);
    MGS_REQUIRE(h.head_floats >= 0 && h.head_floats <= h.row_floats, "adam_step: groups[%d].head_floats %d not in 0..row_floats = %d",
                k, (int)h.head_floats, (int)h.row_floats);
    MGS_REQUIRE(h.n >= 0 && (uint64_t)h.n * (uint64_t)h.row_floats < (1ull << 32),
                "adam_step: groups[%d].n %lld: n * row_floats must be in 0..2^32-1", k, (long long)h.n);
    MGS_REQUIRE(!masked || h.n == groups[0].n, "adam_step: groups[%d].n %lld != groups[0].n %lld under a visibility mask",
                k, (long long)h.n, (long long)groups[0].n);
    MGS_REQUIRE(h.param && h.grad && h.exp_avg && h.exp_avg_sq, "adam_step: groups[%d] has a null pointer", k);
    MGS_REQUIRE(aligned16(h.param), "adam_step: groups[%d].param is not 16-byte aligned", k);
    MGS_REQUIRE(aligned16(h.grad), "adam_step: groups[%d].grad is not 16-byte aligned", k);
    MGS_REQUIRE(aligned16(h.exp_avg), "adam_step: groups[%d].exp_avg is not 16-byte aligned", k);
    MGS_REQUIRE(aligned16(h.exp_avg_sq), "adam_step: groups[%d].exp_avg_sq is not 16-byte aligned", k);
    MGS_REQUIRE(h.lr >= 0.0 && std::isfinite(h.lr), "adam_step: groups[%d].lr %g", k, h.lr);
    MGS_REQUIRE(h.decay_steps >= 0, "adam_step: groups[%d].decay_steps %d is negative", k, (int)h.decay_steps);
    MGS_REQUIRE(h.decay_steps == 0 || (h.lr > 0.0 && h.lr_final > 0.0 && std::isfinite(h.lr_final)),
                "adam_step: groups[%d]: a schedule needs lr and lr_final > 0 (lr %g, lr_final %g)", k, h.lr, h.lr_final);
    MGS_REQUIRE(h.head_floats == 0 || std::isfinite(h.rest_lr_scale), "adam_step: groups[%d].rest_lr_scale %g", k, h.rest_lr_scale);
    Group& G = a.grp[k];
    G.p = h.param, G.g = h.grad, G.m = h.exp_avg, G.v = h.exp_avg_sq;
    G.total = (uint32_t)((uint64_t)h.n * (uint64_t)h.row_floats);
    G.row = (uint32_t)h.row_floats;
    G.head = h.head_floats ? (uint32_t)h.head_floats : G.row;
    G.decay_steps = h.decay_steps;
    G.lr = h.lr;
    G.log_ratio = h.decay_steps ? std::log(h.lr_final / h.lr) : 0.0;
    G.rest_scale = h.head_floats ? h.rest_lr_scale : 1.0;
    work += G.total / 4;
  }
  MGS_REQUIRE(!radii || n_cams == 1 || cam_stride >= (size_t)groups[0].n, "adam_step: cam_stride %zu < n %lld", cam_stride,
              (long long)groups[0].n);
  MGS_REQUIRE(step_state, "adam_step: step_state is null");
  // workgroups per group: one per kBlock float4s, or the group's share of kMaxBlocks by size
  const uint64_t want = (work + kBlock - 1) / kBlock + n_groups;
  for (int k = 0; k < n_groups; ++k) {
    const uint64_t n4 = a.grp[k].total / 4;
    uint64_t blocks = (n4 + kBlock - 1) / kBlock;
    if (want > kMaxBlocks) blocks = std::min<uint64_t>(blocks, n4 * kMaxBlocks / work);
    if (blocks < 1 && a.grp[k].total > 0) blocks = 1;
    a.first_block[k + 1] = a.first_block[k] + (uint32_t)blocks;
  }
  a.n_groups = n_groups;
  a.ln_b1 = std::log(beta1), a.ln_b2 = std::log(beta2);      // ln 0 = -inf: 1 - beta^t = 1
  a.b1 = (float)beta1, a.omb1 = (float)(1.0 - beta1), a.b2 = (float)beta2, a.omb2 = (float)(1.0 - beta2);
  a.eps = (float)eps;
  a.state = step_state;
  a.radii = radii, a.radii_y = radii_y, a.n_cams = n_cams, a.cam_stride = cam_stride, a.mask = mask;
  const unsigned grid = a.first_block[n_groups] ? a.first_block[n_groups] : 1;
  hipStream_t s = (hipStream_t)stream;
  if (radii)
    hipLaunchKernelGGL(adam_step_kernel<kVisRadii>, dim3(grid), dim3(kBlock), 0, s, a);
  else if (mask)
    hipLaunchKernelGGL(adam_step_kernel<kVisMask>, dim3(grid), dim3(kBlock), 0, s, a);
  else
    hipLaunchKernelGGL(adam_step_kernel<kVisAll>, dim3(grid), dim3(kBlock), 0, s, a);
  return check_launch("adam_step");
}
