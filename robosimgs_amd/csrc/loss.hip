// loss.hip -- the photometric L1 term of the training step (BASELINE configs[2]: "L1 loss to
// random target"), forward and backward as two streaming HIP kernels instead of the six
// elementwise / reduction launches the same expression costs in eager PyTorch (72 -> ~20 us at
// 1920x1080x3).  HBM-bound: 8 B read per element forward, 8 B read + 4 B written backward.
// The sum is taken in a fixed order (per-thread strided partials, wave butterfly, per-block slots,
// one final block), so the loss is bit-reproducible.
//
// Under an image descriptor (mgs_image_loss) the same entry points compute splatfacto's L1 + D-SSIM loss
// (1 - lambda) mean|a - b| + lambda (1 - SSIM) and its gradient in ONE pass over a and b: ssim_kernel below, then the
// one-block l1 / ssim final kernel.  Gather form, no atomics: bit-reproducible as well.
//
// mgs_rgbd_loss_* (include/mgs_loss_rgbd.h) are that loss on the RGB+ED frame: ssim_kernel<., true>, the masked form that
// reads a 3- or 4-channel render in place, carries an L1 depth term and writes the complete cotangent.
#include <algorithm>
#include <climits>
#include <cmath>
#include <type_traits>

#include "mgs_common.h"
#include "../../include/mgs_loss_rgbd.h"

namespace mgs {
namespace {

constexpr int kBlock = 256;
constexpr int kMaxBlocks = 1024;

__device__ __forceinline__ float block_sum(float v, float* lds) {
#pragma unroll
  for (int d = 32; d >= 1; d >>= 1) v += __shfl_xor(v, d);
  if ((threadIdx.x & 63) == 0) lds[threadIdx.x >> 6] = v;
  __syncthreads();
  return lds[0] + lds[1] + lds[2] + lds[3];
}

__global__ __launch_bounds__(kBlock) void l1_partial_kernel(size_t n, const float* __restrict__ a,
                                                            const float* __restrict__ b,
                                                            float* __restrict__ partial) {
  __shared__ float lds[kBlock / 64];
  float acc = 0.f;
  const size_t n4 = n / 4, stride = (size_t)gridDim.x * kBlock;
  const float4* a4 = reinterpret_cast<const float4*>(a);
  const float4* b4 = reinterpret_cast<const float4*>(b);
  for (size_t i = (size_t)blockIdx.x * kBlock + threadIdx.x; i < n4; i += stride) {
    const float4 x = a4[i], y = b4[i];
    acc += (fabsf(x.x - y.x) + fabsf(x.y - y.y)) + (fabsf(x.z - y.z) + fabsf(x.w - y.w));
  }
  if (blockIdx.x == 0 && threadIdx.x < (n & 3)) acc += fabsf(a[4 * n4 + threadIdx.x] - b[4 * n4 + threadIdx.x]);
  const float s = block_sum(acc, lds);
  if (threadIdx.x == 0) partial[blockIdx.x] = s;
}

__global__ __launch_bounds__(kBlock) void l1_final_kernel(int n_partial, const float* __restrict__ partial,
                                                          float inv_n, float* __restrict__ loss) {
  __shared__ float lds[kBlock / 64];
  float acc = 0.f;
  for (int i = threadIdx.x; i < n_partial; i += kBlock) acc += partial[i];
  const float s = block_sum(acc, lds);
  if (threadIdx.x == 0) *loss = s * inv_n;
}

__global__ __launch_bounds__(kBlock) void l1_bwd_kernel(size_t n, const float* __restrict__ a,
                                                        const float* __restrict__ b,
                                                        const float* __restrict__ v_loss, float inv_n,
                                                        float* __restrict__ v_a) {
  const float g = (v_loss ? *v_loss : 1.f) * inv_n;
  const size_t n4 = n / 4, stride = (size_t)gridDim.x * kBlock;
  const float4* a4 = reinterpret_cast<const float4*>(a);
  const float4* b4 = reinterpret_cast<const float4*>(b);
  float4* o4 = reinterpret_cast<float4*>(v_a);
  auto sg = [g](float d) { return d > 0.f ? g : (d < 0.f ? -g : 0.f); };   // torch.sign: 0 at 0
  for (size_t i = (size_t)blockIdx.x * kBlock + threadIdx.x; i < n4; i += stride) {
    const float4 x = a4[i], y = b4[i];
    o4[i] = make_float4(sg(x.x - y.x), sg(x.y - y.y), sg(x.z - y.z), sg(x.w - y.w));
  }
  if (blockIdx.x == 0 && threadIdx.x < (n & 3)) {
    const size_t i = 4 * n4 + threadIdx.x;
    v_a[i] = sg(a[i] - b[i]);
  }
}

// Forward AND the gradient for v_loss = 1 in one pass over a and b: v_a = sign(a - b) / n beside the partial sums (12
// instead of 8 + 12 bytes per element for the pair of kernels above); l1_final_kernel adds the partials up as before.
// (Letting the block that finishes last do that -- __threadfence + a counter -- was measured: 51 us instead of ~18.  An
// agent-scope release on gfx950 writes the XCD's dirty L2 lines back, and here those are the 33 MB of v_a just stored.)
__global__ __launch_bounds__(kBlock) void l1_fwd_grad_kernel(size_t n, const float* __restrict__ a,
                                                             const float* __restrict__ b, float inv_n,
                                                             float* __restrict__ partial, float* __restrict__ v_a) {
  __shared__ float lds[kBlock / 64];
  float acc = 0.f;
  const size_t n4 = n / 4, stride = (size_t)gridDim.x * kBlock;
  const float4* a4 = reinterpret_cast<const float4*>(a);
  const float4* b4 = reinterpret_cast<const float4*>(b);
  float4* o4 = reinterpret_cast<float4*>(v_a);
  const float g = inv_n;
  auto sg = [g](float d) { return d > 0.f ? g : (d < 0.f ? -g : 0.f); };
  for (size_t i = (size_t)blockIdx.x * kBlock + threadIdx.x; i < n4; i += stride) {
    const float4 x = a4[i], y = b4[i];
    const float d0 = x.x - y.x, d1 = x.y - y.y, d2 = x.z - y.z, d3 = x.w - y.w;
    acc += (fabsf(d0) + fabsf(d1)) + (fabsf(d2) + fabsf(d3));
    o4[i] = make_float4(sg(d0), sg(d1), sg(d2), sg(d3));
  }
  if (blockIdx.x == 0 && threadIdx.x < (n & 3)) {
    const size_t i = 4 * n4 + threadIdx.x;
    const float d = a[i] - b[i];
    acc += fabsf(d);
    v_a[i] = sg(d);
  }
  const float s = block_sum(acc, lds);
  if (threadIdx.x == 0) partial[blockIdx.x] = s;
}

// v_a <- sign(v_a) * v_loss / n, in place (v_a as l1_fwd_grad_kernel left it, or this kernel).  v_loss == 1 -- the
// usual loss.backward() -- leaves at once: nothing to do, which is why the launch is kScaleBlocks workgroups only.
__global__ __launch_bounds__(kBlock) void l1_scale_kernel(size_t n, const float* __restrict__ v_loss, float inv_n,
                                                          float* __restrict__ v_a) {
  const float vl = *v_loss;
  if (vl == 1.f) return;
  const float g = vl * inv_n;
  const size_t n4 = n / 4, stride = (size_t)gridDim.x * kBlock;
  float4* o4 = reinterpret_cast<float4*>(v_a);
  auto sg = [g](float d) { return d > 0.f ? g : (d < 0.f ? -g : 0.f); };
  for (size_t i = (size_t)blockIdx.x * kBlock + threadIdx.x; i < n4; i += stride) {
    const float4 x = o4[i];
    o4[i] = make_float4(sg(x.x), sg(x.y), sg(x.z), sg(x.w));
  }
  if (blockIdx.x == 0 && threadIdx.x < (n & 3)) {
    const size_t i = 4 * n4 + threadIdx.x;
    v_a[i] = sg(v_a[i]);
  }
}

constexpr unsigned kScaleBlocks = 128;

// ---- L1 + D-SSIM (mgs_image_loss) ----------------------------------------------------------------------------------
// One workgroup per 32 x 32 output tile of one image, all channels in turn.  Per channel:
//   stage    x' = x - x(c), y' = y - y(c) on the tile + 10-pixel halo (52 x 52; zeros outside the image, shifted too),
//            where c is a pixel near the tile's centre: the variances below are differences of two moments, and taking
//            them about a local value keeps near-constant images from cancelling to nothing in fp32 (SSIM itself is
//            unchanged: mu = x(c) + g * x', sigma^2 = g * x'^2 - (g * x')^2);
//   pass 1   the window along rows: the five moments x', y', x'^2, y'^2, x'y' on 52 rows x 42 columns;
//   pass 2   along columns: the moments at the 42 x 42 window centres q (tile + 5-pixel halo), S(q), and the chained
//            partials A = dS/dmu_x - 2 mu_x' B - mu_y' C, B = dS/dsigma_x^2, C = dS/dsigma_xy (zero where q is not a
//            position of the loss: outside the valid region, or outside the image under "same");
//   pass 3/4 the window's transpose (the window is symmetric: the window itself) over A, B, C along rows, then columns:
//            dSSIM/dx(p) = (1/M) sum_q g(q - p) [A(q) + 2 x'(p) B(q) + y'(p) C(q)] on the tile.
// Each thread filters a strip of kP* outputs from kP* + 10 values in registers (2.2-2.6 LDS reads per output instead of
// 11).  LDS: x', y' (21.1 KiB, reused for A, B, C) + the row-filtered maps (42.7 KiB): 64 KiB, two workgroups per CU.
constexpr int kSsimTW = 32, kSsimTH = 32;                        // output tile
constexpr int kR = 5;                                            // window radius: 11 taps
constexpr int kXW = kSsimTW + 4 * kR, kXH = kSsimTH + 4 * kR;    // staged x', y'
constexpr int kMW = kSsimTW + 2 * kR, kMH = kSsimTH + 2 * kR;    // window centres whose partials reach the tile
constexpr int kP1 = 7, kP2 = 7, kP3 = 8, kP4 = 4;                // outputs per thread in passes 1..4
constexpr int kStage = (kXH * kXW + kBlock - 1) / kBlock;        // staged pixels per thread
static_assert(kMW % kP1 == 0 && kMH % kP2 == 0 && kSsimTW % kP3 == 0 && kSsimTH % kP4 == 0, "strips tile the passes");
constexpr int kLdsA = 2 * kXH * kXW;                             // x', y'; then A, B, C [3][kMH][kMW]
constexpr int kLdsB = 5 * kXH * kMW;                             // row-filtered moments; then row-filtered A, B, C
static_assert(3 * kMH * kMW <= kLdsA && 3 * kMH * kSsimTW <= kLdsB, "overlays fit");
constexpr float kC1 = 0.01f * 0.01f, kC2 = 0.03f * 0.03f;

struct SsimArgs {
  const float* a;
  const float* b;
  int height, width, channels, tiles_x, tiles_per_image, valid;
  float l1_scale;          // (1 - lambda) / n
  float s_scale;           // lambda / M
  const float* v_loss;     // nullable: 1
  float* partial;          // [2 * blocks]: per block sum |a - b|, then sum S; nullable (the backward)
  float* v_a;              // the gradient (kGrad)
  float g[2 * kR + 1];     // the normalised window
};

// The masked RGB-D form (include/mgs_loss_rgbd.h; kRgbd below): a is the render with a pixel stride of render_channels
// floats (3 or 4: colour, then depth), b the RGB target (stride 3), v_a strided as a.
struct RgbdArgs : SsimArgs {
  const float* mask;        // [images, H, W], nullable: 1
  const float* depth_t;     // [images, H, W] target depth; null: no depth term (depth_weight == 0)
  const float* sw_partial;  // [n_sw] the partial sums of w that sum_w_kernel left (depth_t only)
  int n_sw;                 // <= kBlock
  int render_channels;
  float depth_weight;
};

template <int K>
__device__ __forceinline__ void filter_strip(const float* v, const float* g, float* out) {
#pragma unroll
  for (int m = 0; m < K; ++m) {
    float s = 0.f;
#pragma unroll
    for (int k = 0; k <= 2 * kR; ++k) s += g[k] * v[m + k];
    out[m] = s;
  }
}

// the masked value of the select semantics: m c where m > 0, else exactly 0 whatever c holds (NaN and inf included)
__device__ __forceinline__ float masked(float m, float c) { return m > 0.f ? m * c : 0.f; }

// kRgbd: the masked, strided form with the depth term riding along (RgbdArgs).  The mask is applied at staging, so
// everything between staging and pass 4 is the unmasked kernel's; pass 4 multiplies by m(p) (x = m c) and writes into
// the render's stride.  A thread keeps the mask of its staged pixels and of its pass-4 pixels in registers across the
// three channels (measured against a reload per channel: profiles/rgbd_loss/README.md).
// A tile that stages a mask value other than 1 (tile_masked) departs from the unmasked arithmetic in three places, each
// marked below and argued in profiles/rgbd_loss/README.md section 4: removed pixels are staged at the shift and put back in
// closed form, the fifth moment is that of (x' - y')^2, and the tile adds up S - 1 and a count.  Every other tile, and so
// every tile without a mask or under a mask of ones, runs the unmasked instantiation's operations: the same bytes.
template <bool kGrad, bool kRgbd = false>
__global__ __launch_bounds__(kBlock) void ssim_kernel(const std::conditional_t<kRgbd, RgbdArgs, SsimArgs> p) {
  __shared__ float lds_a[kLdsA];
  __shared__ float lds_b[kLdsB];
  __shared__ float red[(kRgbd ? 5 : 2) * (kBlock / 64)];
  const int tid = threadIdx.x;
  const int img = blockIdx.x / p.tiles_per_image, t = blockIdx.x - img * p.tiles_per_image;
  const int ty0 = (t / p.tiles_x) * kSsimTH, tx0 = (t - (t / p.tiles_x) * p.tiles_x) * kSsimTW;
  const int H = p.height, W = p.width, C = p.channels;
  const size_t base = (size_t)img * H * W * C;
  int CA = C;                                          // a's (and v_a's) pixel stride
  size_t base_a = base;
  const float* __restrict__ M = nullptr;
  if constexpr (kRgbd) {
    CA = p.render_channels;
    base_a = (size_t)img * H * W * CA;
    if (p.mask) M = p.mask + (size_t)img * H * W;
  }
  const float* __restrict__ A = p.a + base_a;
  const float* __restrict__ B = p.b + base;
  const int qy_lo = p.valid ? kR : 0, qy_hi = p.valid ? H - kR : H;     // window centres that are loss positions
  const int qx_lo = p.valid ? kR : 0, qx_hi = p.valid ? W - kR : W;
  float g[2 * kR + 1];
#pragma unroll
  for (int k = 0; k <= 2 * kR; ++k) g[k] = p.g[k];
  const float vl = p.v_loss ? *p.v_loss : 1.f;
  const size_t centre_px = (size_t)min(ty0 + kSsimTH / 2, H - 1) * W + min(tx0 + kSsimTW / 2, W - 1);
  const size_t centre = centre_px * C;
  float* X = lds_a;
  float* Y = lds_a + kXH * kXW;
  float* Hm = lds_b;                 // [5][kXH][kMW]
  float* Abc = lds_a;                // [3][kMH][kMW]
  float* Habc = lds_b;               // [3][kMH][kSsimTW]
  float acc_l1 = 0.f, acc_s = 0.f;
  [[maybe_unused]] float m_centre = 1.f, ml[kStage], mp[kP4];     // kRgbd: the mask at the shift pixel, staged and pass-4 pixels
  [[maybe_unused]] size_t shift_px = centre_px;                   // kRgbd: the pixel whose masked value is the tile's shift
  // kRgbd, uniform: the tile stages a mask value other than 1 / a zero; Z and Z Zc of this thread's pass-2 strip
  [[maybe_unused]] bool tile_masked = false, tile_zero = false;
  // kRgbd, a masked tile: sum (S - 1) and the count of its loss positions instead of sum S (S - 1 from 1 - l and 1 - cs,
  // each a small quantity over a large one: adding up values next to 1 in fp32 would cost what the gate allows)
  [[maybe_unused]] float acc_dev = 0.f, acc_n = 0.f;
  [[maybe_unused]] float zr[kP2], zz[kP2];
  if constexpr (kRgbd) {
#pragma unroll
    for (int m = 0; m < kP2; ++m) zr[m] = zz[m] = 0.f;
#pragma unroll
    for (int s = 0; s < kStage; ++s) ml[s] = 1.f;
#pragma unroll
    for (int m = 0; m < kP4; ++m) mp[m] = 1.f;
    if (M) {
      m_centre = M[centre_px];
#pragma unroll
      for (int s = 0; s < kStage; ++s) {
        const int i = min(tid + s * kBlock, kXH * kXW - 1);
        const int r = i / kXW, col = i - r * kXW;
        const int gy = min(max(ty0 - 2 * kR + r, 0), H - 1), gx = min(max(tx0 - 2 * kR + col, 0), W - 1);
        ml[s] = M[(size_t)gy * W + gx];
      }
#pragma unroll
      for (int m = 0; m < kP4; ++m) {
        const int py = min(ty0 + (tid / kSsimTW) * kP4 + m, H - 1), px = min(tx0 + tid % kSsimTW, W - 1);
        mp[m] = M[(size_t)py * W + px];
      }
      int any_ne = 0, any_zero = 0;
#pragma unroll
      for (int s = 0; s < kStage; ++s) {
        const int i = tid + s * kBlock;
        const int r = i / kXW, col = i - r * kXW;
        const int gy = ty0 - 2 * kR + r, gx = tx0 - 2 * kR + col;
        if (i < kXH * kXW && gy >= 0 && gy < H && gx >= 0 && gx < W) {
          any_ne |= ml[s] != 1.f;
          any_zero |= !(ml[s] > 0.f);
        }
      }
      int flags = (any_ne ? 1 : 0) | (any_zero ? 2 : 0);
#pragma unroll
      for (int d = 32; d >= 1; d >>= 1) flags |= __shfl_xor(flags, d);
      if ((tid & 63) == 0) red[tid >> 6] = __int_as_float(flags);          // (red's first use; bits, not numbers)
      __syncthreads();
      flags = __float_as_int(red[0]) | __float_as_int(red[1]) | __float_as_int(red[2]) | __float_as_int(red[3]);
      tile_masked = flags & 1;
      tile_zero = flags & 2;
      __syncthreads();
      // A masked centre would shift by 0 and leave the pixels the mask lets through, the ones that carry the loss, far
      // from the shift: take the first staged pixel it lets through instead (none: the tile is all zeros, shift 0).
      if (!(m_centre > 0.f)) {                         // uniform: one value per workgroup
        int first = INT_MAX;
#pragma unroll
        for (int s = kStage - 1; s >= 0; --s) {
          const int i = tid + s * kBlock;
          const int r = i / kXW, col = i - r * kXW;
          const int gy = ty0 - 2 * kR + r, gx = tx0 - 2 * kR + col;
          if (i < kXH * kXW && gy >= 0 && gy < H && gx >= 0 && gx < W && ml[s] > 0.f) first = i;
        }
#pragma unroll
        for (int d = 32; d >= 1; d >>= 1) first = min(first, __shfl_xor(first, d));
        if ((tid & 63) == 0) red[tid >> 6] = __int_as_float(first);
        __syncthreads();
        first = min(min(__float_as_int(red[0]), __float_as_int(red[1])), min(__float_as_int(red[2]), __float_as_int(red[3])));
        if (first != INT_MAX) {
          const int r = first / kXW, col = first - r * kXW;
          shift_px = (size_t)(ty0 - 2 * kR + r) * W + (tx0 - 2 * kR + col);
          m_centre = M[shift_px];
        }
      }
      // The pixels the mask removes are exact zeros, a population of their own that no one shift serves together with the
      // image's values.  They are staged AT the shift (x' = y' = 0) and put back analytically in pass 2: with z = [m == 0],
      // Z = g * z and Zc = g * (1 - z) at the window centres (channel-independent, filtered once here, kept in registers),
      //   mu' = mu'' - s Z,   sigma^2 = sigma''^2 + 2 s Z mu'' + s^2 Z Zc      (Z Zc for Z (1 - Z): exactly 0 in a window of
      // zeros and in one without any), so a window of zeros has variance 0, not s^2 2^-23 against C2.
      if (tile_zero) {
#pragma unroll
        for (int s = 0; s < kStage; ++s) {
          const int i = tid + s * kBlock;
          if (i < kXH * kXW) {
            const int r = i / kXW, col = i - r * kXW;
            const int gy = ty0 - 2 * kR + r, gx = tx0 - 2 * kR + col;
            const bool z = gy >= 0 && gy < H && gx >= 0 && gx < W && !(ml[s] > 0.f);
            X[i] = z ? 1.f : 0.f;
            Y[i] = z ? 0.f : 1.f;
          }
        }
        __syncthreads();
        for (int it = tid; it < kXH * (kMW / kP1); it += kBlock) {
          const int r = it / (kMW / kP1), j0 = (it - r * (kMW / kP1)) * kP1;
          float xs[kP1 + 2 * kR], ys[kP1 + 2 * kR], out[kP1];
#pragma unroll
          for (int k = 0; k < kP1 + 2 * kR; ++k) {
            xs[k] = X[r * kXW + j0 + k];
            ys[k] = Y[r * kXW + j0 + k];
          }
          filter_strip<kP1>(xs, g, out);
#pragma unroll
          for (int m = 0; m < kP1; ++m) Hm[r * kMW + j0 + m] = out[m];
          filter_strip<kP1>(ys, g, out);
#pragma unroll
          for (int m = 0; m < kP1; ++m) Hm[(kXH + r) * kMW + j0 + m] = out[m];
        }
        __syncthreads();
        if (tid < kMW * (kMH / kP2)) {                 // pass 2's strip of this thread
          const int col = tid % kMW, i0 = (tid / kMW) * kP2;
          float v[kP2 + 2 * kR], zc[kP2];
#pragma unroll
          for (int k = 0; k < kP2 + 2 * kR; ++k) v[k] = Hm[(i0 + k) * kMW + col];
          filter_strip<kP2>(v, g, zr);
#pragma unroll
          for (int k = 0; k < kP2 + 2 * kR; ++k) v[k] = Hm[(kXH + i0 + k) * kMW + col];
          filter_strip<kP2>(v, g, zc);
#pragma unroll
          for (int m = 0; m < kP2; ++m) zz[m] = zr[m] * zc[m];
        }
        // (the channel's staging writes lds_a, last read before the barrier above; pass 1 writes lds_b behind the staging barrier)
      }
    }
  }

  for (int c = 0; c < C; ++c) {
    float sx, sy;
    if constexpr (kRgbd) {
      sx = masked(m_centre, A[shift_px * CA + c]);
      sy = masked(m_centre, B[shift_px * C + c]);
    } else {
      sx = A[centre + c];
      sy = B[centre + c];
    }
    // (no barrier needed here: lds_a was last read in pass 1 / pass 3 of the previous channel, behind a barrier since)
    // All of a thread's loads first, from clamped addresses, so that they are in flight together; zeros outside after.
    float xl[kStage], yl[kStage];
#pragma unroll
    for (int s = 0; s < kStage; ++s) {
      const int i = min(tid + s * kBlock, kXH * kXW - 1);
      const int r = i / kXW, col = i - r * kXW;
      const int gy = min(max(ty0 - 2 * kR + r, 0), H - 1), gx = min(max(tx0 - 2 * kR + col, 0), W - 1);
      const size_t o = ((size_t)gy * W + gx) * C + c;
      if constexpr (kRgbd) {
        xl[s] = A[((size_t)gy * W + gx) * CA + c];
      } else {
        xl[s] = A[o];
      }
      yl[s] = B[o];
    }
#pragma unroll
    for (int s = 0; s < kStage; ++s) {
      const int i = tid + s * kBlock;
      if (i < kXH * kXW) {
        const int r = i / kXW, col = i - r * kXW;
        const int gy = ty0 - 2 * kR + r, gx = tx0 - 2 * kR + col;
        const bool inside = gy >= 0 && gy < H && gx >= 0 && gx < W;
        float xv = inside ? xl[s] : 0.f, yv = inside ? yl[s] : 0.f;
        if constexpr (kRgbd) {
          xv = inside ? masked(ml[s], xl[s]) : 0.f;
          yv = inside ? masked(ml[s], yl[s]) : 0.f;
        }
        if (inside && r >= 2 * kR && r < 2 * kR + kSsimTH && col >= 2 * kR && col < 2 * kR + kSsimTW)
          acc_l1 += fabsf(xv - yv);
        X[i] = xv - sx;
        Y[i] = yv - sy;
        if constexpr (kRgbd) {
          if (inside && !(ml[s] > 0.f)) X[i] = Y[i] = 0.f;          // a removed pixel: at the shift (put back in pass 2)
        }
      }
    }
    __syncthreads();

    // pass 1: rows
    for (int it = tid; it < kXH * (kMW / kP1); it += kBlock) {
      const int r = it / (kMW / kP1), j0 = (it - r * (kMW / kP1)) * kP1;
      float xs[kP1 + 2 * kR], ys[kP1 + 2 * kR], prod[kP1 + 2 * kR], out[kP1];
#pragma unroll
      for (int k = 0; k < kP1 + 2 * kR; ++k) {
        xs[k] = X[r * kXW + j0 + k];
        ys[k] = Y[r * kXW + j0 + k];
      }
      float* h = Hm + r * kMW + j0;
      filter_strip<kP1>(xs, g, out);
#pragma unroll
      for (int m = 0; m < kP1; ++m) h[m] = out[m];
      filter_strip<kP1>(ys, g, out);
#pragma unroll
      for (int m = 0; m < kP1; ++m) h[kXH * kMW + m] = out[m];
#pragma unroll
      for (int k = 0; k < kP1 + 2 * kR; ++k) prod[k] = xs[k] * xs[k];
      filter_strip<kP1>(prod, g, out);
#pragma unroll
      for (int m = 0; m < kP1; ++m) h[2 * kXH * kMW + m] = out[m];
#pragma unroll
      for (int k = 0; k < kP1 + 2 * kR; ++k) prod[k] = ys[k] * ys[k];
      filter_strip<kP1>(prod, g, out);
#pragma unroll
      for (int m = 0; m < kP1; ++m) h[3 * kXH * kMW + m] = out[m];
#pragma unroll
      for (int k = 0; k < kP1 + 2 * kR; ++k) {
        prod[k] = xs[k] * ys[k];
        // under a mask x and y move together and 1 - S hangs on sigma_x^2 + sigma_y^2 - 2 sigma_xy = var(x - y): taken
        // from the moment of (x' - y')^2 itself, not as the difference of three large moments
        if constexpr (kRgbd) {
          if (tile_masked) {
#pragma clang fp contract(off)
            const float e = xs[k] - ys[k];
            prod[k] = e * e;
          }
        }
      }
      filter_strip<kP1>(prod, g, out);
#pragma unroll
      for (int m = 0; m < kP1; ++m) h[4 * kXH * kMW + m] = out[m];
    }
    __syncthreads();

    // pass 2: columns -> S and the partials at the window centres
    for (int it = tid; it < kMW * (kMH / kP2); it += kBlock) {
      const int col = it % kMW, i0 = (it / kMW) * kP2;
      float mo[5][kP2];
#pragma unroll
      for (int q = 0; q < 5; ++q) {
        float v[kP2 + 2 * kR];
#pragma unroll
        for (int k = 0; k < kP2 + 2 * kR; ++k) v[k] = Hm[(q * kXH + i0 + k) * kMW + col];
        filter_strip<kP2>(v, g, mo[q]);
      }
      const int qx = tx0 - kR + col;
      const bool own_x = col >= kR && col < kR + kSsimTW;
#pragma unroll
      for (int m = 0; m < kP2; ++m) {
        const int qy = ty0 - kR + i0 + m;
        const bool in = qy >= qy_lo && qy < qy_hi && qx >= qx_lo && qx < qx_hi;
        float mx = mo[0][m], my = mo[1][m];
        float vxx = mo[2][m] - mx * mx, vyy = mo[3][m] - my * my, vxy = mo[4][m] - mx * my;
        [[maybe_unused]] float ve = 0.f;
        if constexpr (kRgbd) {
          if (tile_masked) {
            // (no contraction: both instantiations must round alike -- the forward alone gives the training form's loss bits)
#pragma clang fp contract(off)
            const float Z = zr[m], ZZ = zz[m], me = mx - my, se = sx - sy;
            ve = (mo[4][m] - me * me) + (2.f * se * Z * me + se * se * ZZ);
            vxx = vxx + (2.f * sx * Z * mx + sx * sx * ZZ);        // (vxx, vyy as taken above: the unmasked form's very
            vyy = vyy + (2.f * sy * Z * my + sy * sy * ZZ);        //  instructions, not a second copy for CSE to merge)
            vxy = 0.5f * (vxx + vyy - ve);
            mx = mx - sx * Z;
            my = my - sy * Z;
          }
        }
        const float mux = sx + mx, muy = sy + my;
        const float n1 = 2.f * mux * muy + kC1, n2 = 2.f * vxy + kC2;
        const float d1 = mux * mux + muy * muy + kC1, d2 = vxx + vyy + kC2;
        const float inv = 1.f / (d1 * d2);
        const float S = n1 * n2 * inv;
        if (in && own_x && i0 + m >= kR && i0 + m < kR + kSsimTH) {
          bool dev_form = false;
          if constexpr (kRgbd) dev_form = tile_masked;
          if (dev_form) {
#pragma clang fp contract(off)
            const float dm = mux - muy, a = dm * dm / d1, b = ve / d2;      // 1 - l, 1 - cs
            acc_dev -= (a + b) - a * b;
            acc_n += 1.f;
          } else {
            acc_s += S;
          }
        }
        if (kGrad) {
          float pa = 0.f, pb = 0.f, pc = 0.f;
          if (in) {
            pb = -S / d2;
            pc = 2.f * n1 * inv;
            pa = 2.f * muy * n2 * inv - 2.f * mux * S / d1 - 2.f * mx * pb - my * pc;
          }
          Abc[(i0 + m) * kMW + col] = pa;
          Abc[(kMH + i0 + m) * kMW + col] = pb;
          Abc[(2 * kMH + i0 + m) * kMW + col] = pc;
        }
      }
    }
    if (!kGrad) continue;        // the next channel's staging writes lds_a, which pass 2 did not touch
    __syncthreads();

    // pass 3: the transposed window along rows
    for (int it = tid; it < kMH * (kSsimTW / kP3); it += kBlock) {
      const int r = it / (kSsimTW / kP3), j0 = (it - r * (kSsimTW / kP3)) * kP3;
#pragma unroll
      for (int q = 0; q < 3; ++q) {
        float v[kP3 + 2 * kR], out[kP3];
#pragma unroll
        for (int k = 0; k < kP3 + 2 * kR; ++k) v[k] = Abc[(q * kMH + r) * kMW + j0 + k];
        filter_strip<kP3>(v, g, out);
#pragma unroll
        for (int m = 0; m < kP3; ++m) Habc[(q * kMH + r) * kSsimTW + j0 + m] = out[m];
      }
    }
    __syncthreads();

    // pass 4: along columns, and the gradient on the tile
    for (int it = tid; it < kSsimTW * (kSsimTH / kP4); it += kBlock) {
      const int col = it % kSsimTW, i0 = (it / kSsimTW) * kP4;
      float f[3][kP4];
#pragma unroll
      for (int q = 0; q < 3; ++q) {
        float v[kP4 + 2 * kR];
#pragma unroll
        for (int k = 0; k < kP4 + 2 * kR; ++k) v[k] = Habc[(q * kMH + i0 + k) * kSsimTW + col];
        filter_strip<kP4>(v, g, f[q]);
      }
      const int px = tx0 + col;
#pragma unroll
      for (int m = 0; m < kP4; ++m) {
        const int py = ty0 + i0 + m;
        if (py < H && px < W) {
          const size_t o = ((size_t)py * W + px) * C + c;
          if constexpr (kRgbd) {
            const size_t oa = ((size_t)py * W + px) * CA + c;
            const float xv = masked(mp[m], A[oa]), yv = masked(mp[m], B[o]), d = xv - yv;
            const float sg = d > 0.f ? 1.f : (d < 0.f ? -1.f : 0.f);
            const float ds = f[0][m] + 2.f * (xv - sx) * f[1][m] + (yv - sy) * f[2][m];
            const float gx = p.l1_scale * sg - p.s_scale * ds;                // dL/dx; dL/dc = m dL/dx
            p.v_a[base_a + oa] = mp[m] > 0.f ? (mp[m] * gx) * vl : 0.f;
          } else {
            const float xv = A[o], yv = B[o], d = xv - yv;
            const float sg = d > 0.f ? 1.f : (d < 0.f ? -1.f : 0.f);
            const float ds = f[0][m] + 2.f * (xv - sx) * f[1][m] + (yv - sy) * f[2][m];
            p.v_a[base + o] = (p.l1_scale * sg - p.s_scale * ds) * vl;
          }
        }
      }
    }
    // (the next channel's staging writes lds_a, last read in pass 3; pass 1 writes lds_b after the staging barrier)
  }

  // The depth term on the tile's own pixels: w = m [d* finite and > 0] (a select: a NaN in d* or d under w = 0 never
  // enters), the partial of sum w |d - d*|, and channel 3 of the gradient, depth_weight w sign(d - d*) / sum w -- zeros
  // where there is no depth term, so that a four-channel cotangent is complete.
  [[maybe_unused]] float acc_d = 0.f;
  if constexpr (kRgbd) {
    const float* __restrict__ DT = p.depth_t && CA == 4 ? p.depth_t + (size_t)img * H * W : nullptr;
    float k = 0.f;                                     // depth_weight / sum w, 0 where sum w == 0
    if (kGrad && DT) {
      // every workgroup adds sum_w_kernel's partials up itself, in one order: the same bits in each, and no launch
      float sw = tid < p.n_sw ? p.sw_partial[tid] : 0.f;
#pragma unroll
      for (int d = 32; d >= 1; d >>= 1) sw += __shfl_xor(sw, d);
      if ((tid & 63) == 0) red[tid >> 6] = sw;        // (red's first use)
      __syncthreads();
      sw = red[0] + red[1] + red[2] + red[3];        // block_sum's order: rgbd_final_kernel's sum w, bit for bit
      k = sw > 0.f ? p.depth_weight * (1.f / sw) : 0.f;
      __syncthreads();
    }
    if (DT || (kGrad && CA == 4)) {
      for (int i = tid; i < kSsimTW * kSsimTH; i += kBlock) {
        const int py = ty0 + i / kSsimTW, px = tx0 + i % kSsimTW;
        if (py < H && px < W) {
          const size_t px_i = (size_t)py * W + px;
          float g3 = 0.f;
          if (DT) {
            const float dt = DT[px_i], m = M ? M[px_i] : 1.f;
            const float w = (dt > 0.f && dt < INFINITY) ? m : 0.f;
            if (w > 0.f) {
              const float d = A[px_i * CA + 3] - dt;
              acc_d += w * fabsf(d);
              g3 = ((w * k) * (d > 0.f ? 1.f : (d < 0.f ? -1.f : 0.f))) * vl;
            }
          }
          if (kGrad && CA == 4) p.v_a[base_a + px_i * CA + 3] = g3;
        }
      }
    }
  }
  if (p.partial) {
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) {
      acc_l1 += __shfl_xor(acc_l1, d);
      acc_s += __shfl_xor(acc_s, d);
      if constexpr (kRgbd) {
        acc_d += __shfl_xor(acc_d, d);
        acc_dev += __shfl_xor(acc_dev, d);
        acc_n += __shfl_xor(acc_n, d);
      }
    }
    if ((tid & 63) == 0) {
      red[tid >> 6] = acc_l1;
      red[kBlock / 64 + (tid >> 6)] = acc_s;
      if constexpr (kRgbd) {
        red[2 * (kBlock / 64) + (tid >> 6)] = acc_d;
        red[3 * (kBlock / 64) + (tid >> 6)] = acc_dev;
        red[4 * (kBlock / 64) + (tid >> 6)] = acc_n;
      }
    }
    __syncthreads();
    if (tid == 0) {
      p.partial[blockIdx.x] = (red[0] + red[1]) + (red[2] + red[3]);
      p.partial[gridDim.x + blockIdx.x] = (red[4] + red[5]) + (red[6] + red[7]);
      if constexpr (kRgbd) {
        p.partial[2 * gridDim.x + blockIdx.x] = (red[8] + red[9]) + (red[10] + red[11]);
        p.partial[3 * gridDim.x + blockIdx.x] = (red[12] + red[13]) + (red[14] + red[15]);
        p.partial[4 * gridDim.x + blockIdx.x] = (red[16] + red[17]) + (red[18] + red[19]);
      }
    }
  }
}
static_assert(kBlock == 256, "ssim_kernel's reduction assumes four waves");
static_assert(kSsimTW * (kSsimTH / kP4) == kBlock, "kRgbd: pass 4 is one strip per thread (mp)");

// loss = (1 - lambda) * sum|a - b| / n + lambda * (1 - sum S / M), the per-block sums added in a fixed order
__global__ __launch_bounds__(kBlock) void ssim_final_kernel(int n_partial, const float* __restrict__ partial,
                                                            float inv_n, float inv_m, float lambda,
                                                            float* __restrict__ loss) {
  __shared__ float lds[kBlock / 64];
  float acc = 0.f;
  for (int i = threadIdx.x; i < n_partial; i += kBlock) acc += partial[i];
  const float l1 = block_sum(acc, lds);
  __syncthreads();
  acc = 0.f;
  for (int i = threadIdx.x; i < n_partial; i += kBlock) acc += partial[n_partial + i];
  const float s = block_sum(acc, lds);
  if (threadIdx.x == 0) *loss = (1.f - lambda) * (l1 * inv_n) + lambda * (1.f - s * inv_m);
}

// ---- the masked RGB-D loss (mgs_rgbd_loss) -------------------------------------------------------------------------
// sum w, w = m [d* finite and > 0], over all images: depends on mask and target_depth only, and channel 3 of the gradient
// needs it, so it is taken first.  At most kBlock blocks, each a strided partial in a fixed order; ssim_kernel<., true>
// and rgbd_final_kernel add the partials up themselves (no second launch, nothing read back).
constexpr unsigned kSwBlocks = kBlock;

__global__ __launch_bounds__(kBlock) void sum_w_kernel(size_t n_px, const float* __restrict__ mask,
                                                       const float* __restrict__ depth_t, float* __restrict__ partial) {
  __shared__ float lds[kBlock / 64];
  float acc = 0.f;
  const size_t stride = (size_t)gridDim.x * kBlock;
  // four strides per trip, the loads first: at most kSwBlocks workgroups stream the two maps, so each keeps several in flight
  for (size_t i0 = (size_t)blockIdx.x * kBlock + threadIdx.x; i0 < n_px; i0 += 4 * stride) {
    float dt[4], m[4];
#pragma unroll
    for (int u = 0; u < 4; ++u) {
      const size_t i = min(i0 + u * stride, n_px - 1);
      dt[u] = depth_t[i];
      m[u] = mask ? mask[i] : 1.f;
    }
#pragma unroll
    for (int u = 0; u < 4; ++u)
      if (i0 + u * stride < n_px && dt[u] > 0.f && dt[u] < INFINITY && m[u] > 0.f) acc += m[u];
  }
  const float s = block_sum(acc, lds);
  if (threadIdx.x == 0) partial[blockIdx.x] = s;
}

// ssim_final_kernel's colour loss, in its very operations (the same bits where the two losses coincide), + depth_weight D,
// D = sum w |d - d*| / sum w (0 where sum w == 0); terms (nullable) <- {mean|x - y|, SSIM, D, sum w}.
__global__ __launch_bounds__(kBlock) void rgbd_final_kernel(int n_partial, const float* __restrict__ partial, float inv_n,
                                                            float inv_m, float m_f, float lambda, float depth_weight,
                                                            const float* __restrict__ sw_partial, int n_sw,
                                                            float* __restrict__ loss, float* __restrict__ terms) {
  __shared__ float lds[kBlock / 64];
  float acc = 0.f;
  for (int i = threadIdx.x; i < n_partial; i += kBlock) acc += partial[i];
  const float l1 = block_sum(acc, lds);
  __syncthreads();
  acc = 0.f;
  for (int i = threadIdx.x; i < n_partial; i += kBlock) acc += partial[n_partial + i];
  const float s = block_sum(acc, lds);
  // the masked tiles' share: their count of positions n_m (an exact integer) and sum (S - 1); both 0 without a mask, and
  // the expression below is then ssim_final_kernel's, bit for bit
  __syncthreads();
  acc = 0.f;
  for (int i = threadIdx.x; i < n_partial; i += kBlock) acc += partial[3 * n_partial + i];
  const float dev = block_sum(acc, lds);
  __syncthreads();
  acc = 0.f;
  for (int i = threadIdx.x; i < n_partial; i += kBlock) acc += partial[4 * n_partial + i];
  const float n_m = block_sum(acc, lds);
  const float dssim = ((1.f - s * inv_m) - n_m / m_f) - dev * inv_m;      // 1 - SSIM
  const float colour = (1.f - lambda) * (l1 * inv_n) + lambda * dssim;
  float D = 0.f, sw = 0.f;
  if (sw_partial) {                                   // uniform: the depth term is on
    __syncthreads();
    acc = 0.f;
    for (int i = threadIdx.x; i < n_partial; i += kBlock) acc += partial[2 * n_partial + i];
    const float sd = block_sum(acc, lds);
    __syncthreads();
    sw = block_sum((int)threadIdx.x < n_sw ? sw_partial[threadIdx.x] : 0.f, lds);   // ssim_kernel's order
    D = sw > 0.f ? sd * (1.f / sw) : 0.f;
  }
  if (threadIdx.x == 0) {
    *loss = sw_partial ? colour + depth_weight * D : colour;
    if (terms) {
      terms[0] = l1 * inv_n;
      terms[1] = 1.f - dssim;
      terms[2] = D;
      terms[3] = sw;
    }
  }
}

// The descriptor checked against n, the grid and the scales.  Host only: runs before any size query answers.
struct SsimPlan {
  SsimArgs args;
  unsigned blocks;
  float inv_n, inv_m, lambda;
};

int ssim_plan(size_t n, const mgs_image_loss* d, const char* what, SsimPlan* plan) {
  MGS_REQUIRE(d->images >= 1 && d->height >= 1 && d->width >= 1, "%s: images %d, height %d, width %d must be positive",
              what, d->images, d->height, d->width);
  MGS_REQUIRE(d->channels >= 1 && d->channels <= 4, "%s: channels %d not in 1..4", what, d->channels);
  MGS_REQUIRE(d->padding == MGS_SSIM_VALID || d->padding == MGS_SSIM_SAME,
              "%s: padding %d is neither MGS_SSIM_VALID nor MGS_SSIM_SAME", what, d->padding);
  MGS_REQUIRE(d->padding == MGS_SSIM_SAME || (d->height >= 2 * kR + 1 && d->width >= 2 * kR + 1),
              "%s: padding MGS_SSIM_VALID needs height and width >= 11 (got %d x %d)", what, d->height, d->width);
  MGS_REQUIRE(d->ssim_weight >= 0.f && d->ssim_weight <= 1.f, "%s: ssim_weight %g not in [0, 1]", what,
              (double)d->ssim_weight);
  const size_t elems = (size_t)d->images * d->height * d->width * d->channels;
  MGS_REQUIRE(n == elems, "%s: n %zu != images x height x width x channels = %zu", what, n, elems);
  const size_t tiles_x = div_up(d->width, kSsimTW), tiles_y = div_up(d->height, kSsimTH);
  const size_t blocks = tiles_x * tiles_y * d->images;
  MGS_REQUIRE(blocks <= (size_t)INT_MAX / 2, "%s: %zu tiles exceed the grid", what, blocks);
  const bool valid = d->padding == MGS_SSIM_VALID;
  const double positions = valid ? (double)(d->height - 2 * kR) * (d->width - 2 * kR) : (double)d->height * d->width;
  const double m = positions * d->channels * d->images;
  SsimArgs& a = plan->args;
  a = SsimArgs{};
  a.height = d->height;
  a.width = d->width;
  a.channels = d->channels;
  a.tiles_x = (int)tiles_x;
  a.tiles_per_image = (int)(tiles_x * tiles_y);
  a.valid = valid ? 1 : 0;
  a.l1_scale = (float)((1.0 - d->ssim_weight) / (double)n);
  a.s_scale = (float)(d->ssim_weight / m);
  double w[2 * kR + 1], sum = 0.0;
  for (int i = 0; i <= 2 * kR; ++i) sum += (w[i] = std::exp(-(double)((i - kR) * (i - kR)) / (2.0 * 1.5 * 1.5)));
  for (int i = 0; i <= 2 * kR; ++i) a.g[i] = (float)(w[i] / sum);
  plan->blocks = (unsigned)blocks;
  plan->inv_n = (float)(1.0 / (double)n);
  plan->inv_m = (float)(1.0 / m);
  plan->lambda = d->ssim_weight;
  return MGS_OK;
}

size_t ssim_workspace_bytes(const SsimPlan& plan) { return 2 * (size_t)plan.blocks * sizeof(float); }


unsigned grid_for(size_t n) {
  size_t blocks = (n / 4 + kBlock - 1) / kBlock;
  return (unsigned)(blocks < 1 ? 1 : (blocks > kMaxBlocks ? kMaxBlocks : blocks));
}

}  // namespace
}  // namespace mgs

using namespace mgs;

namespace {

// the L1 + D-SSIM forms of the three entry points below (image != NULL); the descriptor is already planned
int ssim_fwd(const SsimPlan& plan, const float* a, const float* b, float* loss, float* v_a, void* workspace,
             size_t* workspace_bytes, hipStream_t s, const char* what) {
  const size_t need = ssim_workspace_bytes(plan);
  if (!workspace) {
    *workspace_bytes = need;
    return MGS_OK;
  }
  if (*workspace_bytes < need)
    return set_error(MGS_ERR_WORKSPACE_TOO_SMALL, "%s: workspace %zu < %zu bytes", what, *workspace_bytes, need);
  MGS_REQUIRE(a && b && loss, "%s: null pointer", what);
  SsimArgs args = plan.args;
  args.a = a;
  args.b = b;
  args.partial = static_cast<float*>(workspace);
  args.v_a = v_a;
  if (v_a)
    hipLaunchKernelGGL(ssim_kernel<true>, dim3(plan.blocks), dim3(kBlock), 0, s, args);
  else
    hipLaunchKernelGGL(ssim_kernel<false>, dim3(plan.blocks), dim3(kBlock), 0, s, args);
  hipLaunchKernelGGL(ssim_final_kernel, dim3(1), dim3(kBlock), 0, s, (int)plan.blocks, args.partial, plan.inv_n,
                     plan.inv_m, plan.lambda, loss);
  return check_launch(what);
}

}  // namespace

extern "C" int mgs_l1_loss_fwd(size_t n, const float* a, const float* b, float* loss,
                               void* workspace, size_t* workspace_bytes, mgs_stream_t stream,
                               const mgs_image_loss* image) {
  MGS_REQUIRE(workspace_bytes, "l1_loss_fwd: workspace_bytes is null");
  if (image) {
    SsimPlan plan;
    if (int rc = ssim_plan(n, image, "l1_loss_fwd", &plan)) return rc;
    return ssim_fwd(plan, a, b, loss, nullptr, workspace, workspace_bytes, (hipStream_t)stream, "l1_loss_fwd");
  }
  const size_t need = kMaxBlocks * sizeof(float);
  if (!workspace) {
    *workspace_bytes = need;
    return MGS_OK;
  }
  if (*workspace_bytes < need)
    return set_error(MGS_ERR_WORKSPACE_TOO_SMALL, "l1_loss_fwd: workspace %zu < %zu bytes",
                     *workspace_bytes, need);
  MGS_REQUIRE(n > 0 && a && b && loss, "l1_loss_fwd: empty input or null pointer");
  MGS_REQUIRE(((uintptr_t)a & 15) == 0 && ((uintptr_t)b & 15) == 0, "l1_loss_fwd: inputs must be 16-byte aligned");
  hipStream_t s = (hipStream_t)stream;
  float* partial = static_cast<float*>(workspace);
  const unsigned grid = grid_for(n);
  hipLaunchKernelGGL(l1_partial_kernel, dim3(grid), dim3(kBlock), 0, s, n, a, b, partial);
  hipLaunchKernelGGL(l1_final_kernel, dim3(1), dim3(kBlock), 0, s, (int)grid, partial,
                     (float)(1.0 / (double)n), loss);
  return check_launch("l1_loss_fwd");
}

extern "C" int mgs_l1_loss_bwd(size_t n, const float* a, const float* b, const float* v_loss,
                               float* v_a, mgs_stream_t stream, const mgs_image_loss* image) {
  if (image) {
    SsimPlan plan;
    if (int rc = ssim_plan(n, image, "l1_loss_bwd", &plan)) return rc;
    MGS_REQUIRE(a && b && v_a, "l1_loss_bwd: null pointer");
    SsimArgs args = plan.args;
    args.a = a;
    args.b = b;
    args.v_loss = v_loss;
    args.v_a = v_a;
    hipLaunchKernelGGL(ssim_kernel<true>, dim3(plan.blocks), dim3(kBlock), 0, (hipStream_t)stream, args);
    return check_launch("l1_loss_bwd");
  }
  MGS_REQUIRE(n > 0 && a && b && v_a, "l1_loss_bwd: empty input or null pointer");
  MGS_REQUIRE(((uintptr_t)a & 15) == 0 && ((uintptr_t)b & 15) == 0 && ((uintptr_t)v_a & 15) == 0,
              "l1_loss_bwd: buffers must be 16-byte aligned");
  hipLaunchKernelGGL(l1_bwd_kernel, dim3(grid_for(n)), dim3(kBlock), 0, (hipStream_t)stream, n, a, b,
                     v_loss, (float)(1.0 / (double)n), v_a);
  return check_launch("l1_loss_bwd");
}

extern "C" int mgs_l1_loss_fwd_grad(size_t n, const float* a, const float* b, float* loss, float* v_a,
                                    void* workspace, size_t* workspace_bytes, mgs_stream_t stream,
                                    const mgs_image_loss* image) {
  MGS_REQUIRE(workspace_bytes, "l1_loss_fwd_grad: workspace_bytes is null");
  if (image) {
    SsimPlan plan;
    if (int rc = ssim_plan(n, image, "l1_loss_fwd_grad", &plan)) return rc;
    MGS_REQUIRE(v_a || !workspace, "l1_loss_fwd_grad: v_a is null");
    return ssim_fwd(plan, a, b, loss, v_a, workspace, workspace_bytes, (hipStream_t)stream, "l1_loss_fwd_grad");
  }
  const size_t need = kMaxBlocks * sizeof(float);
  if (!workspace) {
    *workspace_bytes = need;
    return MGS_OK;
  }
  if (*workspace_bytes < need)
    return set_error(MGS_ERR_WORKSPACE_TOO_SMALL, "l1_loss_fwd_grad: workspace %zu < %zu bytes",
                     *workspace_bytes, need);
  MGS_REQUIRE(n > 0 && a && b && loss && v_a, "l1_loss_fwd_grad: empty input or null pointer");
  MGS_REQUIRE(((uintptr_t)a & 15) == 0 && ((uintptr_t)b & 15) == 0 && ((uintptr_t)v_a & 15) == 0,
              "l1_loss_fwd_grad: buffers must be 16-byte aligned");
  hipStream_t s = (hipStream_t)stream;
  float* partial = static_cast<float*>(workspace);
  const unsigned grid = grid_for(n);
  hipLaunchKernelGGL(l1_fwd_grad_kernel, dim3(grid), dim3(kBlock), 0, s, n, a, b, (float)(1.0 / (double)n), partial, v_a);
  hipLaunchKernelGGL(l1_final_kernel, dim3(1), dim3(kBlock), 0, s, (int)grid, partial, (float)(1.0 / (double)n), loss);
  return check_launch("l1_loss_fwd_grad");
}

extern "C" int mgs_l1_loss_bwd_scale(size_t n, const float* v_loss, float* v_a, mgs_stream_t stream) {
  MGS_REQUIRE(n > 0 && v_loss && v_a, "l1_loss_bwd_scale: empty input or null pointer");
  MGS_REQUIRE(((uintptr_t)v_a & 15) == 0, "l1_loss_bwd_scale: v_a must be 16-byte aligned");
  hipLaunchKernelGGL(l1_scale_kernel, dim3(std::min(grid_for(n), kScaleBlocks)), dim3(kBlock), 0, (hipStream_t)stream, n, v_loss,
                     (float)(1.0 / (double)n), v_a);
  return check_launch("l1_loss_bwd_scale");
}

// ---- mgs_loss_rgbd.h ----------------------------------------------------------------------------------------------
namespace {

struct RgbdPlan {
  SsimPlan ssim;          // of the colour images: {images, height, width, 3, ssim_weight, padding}
  size_t n_px;
  float m_f;              // the number of SSIM positions (x channels x images)
  unsigned sw_blocks;
  bool depth;             // depth_weight > 0
};

// workspace: [5 * blocks] the tile kernel's partials (sum |x - y|, sum S, the depth sum, sum (S - 1) and the position count of
// masked tiles), then [kSwBlocks] sum_w_kernel's
size_t rgbd_workspace_bytes(const RgbdPlan& plan) { return (5 * (size_t)plan.ssim.blocks + kSwBlocks) * sizeof(float); }

int rgbd_plan(const mgs_rgbd_loss* d, const char* what, RgbdPlan* plan) {
  MGS_REQUIRE(d, "%s: desc is null", what);
  MGS_REQUIRE(d->render_channels == 3 || d->render_channels == 4, "%s: render_channels %d is neither 3 nor 4", what,
              d->render_channels);
  MGS_REQUIRE(d->depth_weight >= 0.f && std::isfinite(d->depth_weight), "%s: depth_weight %g must be finite and >= 0",
              what, (double)d->depth_weight);
  MGS_REQUIRE(d->depth_weight == 0.f || d->render_channels == 4,
              "%s: depth_weight %g > 0 needs render_channels == 4 (the depth channel)", what, (double)d->depth_weight);
  const mgs_image_loss image{d->images, d->height, d->width, 3, d->ssim_weight, d->padding};
  const size_t n = (size_t)std::max(d->images, 0) * std::max(d->height, 0) * std::max(d->width, 0) * 3;
  if (int rc = ssim_plan(n, &image, what, &plan->ssim)) return rc;
  plan->n_px = n / 3;
  plan->m_f = (float)(3.0 * d->images * (d->padding == MGS_SSIM_VALID ? (double)(d->height - 2 * kR) * (d->width - 2 * kR)
                                                                        : (double)d->height * d->width));
  plan->sw_blocks = (unsigned)std::min<size_t>(kSwBlocks, (plan->n_px + kBlock - 1) / kBlock);
  plan->depth = d->depth_weight > 0.f;
  return MGS_OK;
}

// the three entry points: the forward alone (want_loss), the backward alone (want_grad), or both
int rgbd_run(const mgs_rgbd_loss* d, const float* render, const float* target_rgb, const float* target_depth,
             const float* mask, const float* v_loss, float* loss, float* terms, float* v_render, bool want_loss,
             bool want_grad, void* workspace, size_t* workspace_bytes, hipStream_t s, const char* what) {
  MGS_REQUIRE(workspace_bytes, "%s: workspace_bytes is null", what);
  RgbdPlan plan;
  if (int rc = rgbd_plan(d, what, &plan)) return rc;
  const size_t need = rgbd_workspace_bytes(plan);
  if (!workspace) {
    *workspace_bytes = need;
    return MGS_OK;
  }
  if (*workspace_bytes < need)
    return set_error(MGS_ERR_WORKSPACE_TOO_SMALL, "%s: workspace %zu < %zu bytes", what, *workspace_bytes, need);
  MGS_REQUIRE(render && target_rgb && (loss || !want_loss) && (v_render || !want_grad), "%s: null pointer", what);
  MGS_REQUIRE(!plan.depth || target_depth, "%s: depth_weight %g > 0 needs target_depth", what, (double)d->depth_weight);
  float* partial = static_cast<float*>(workspace);
  float* sw_partial = partial + 5 * (size_t)plan.ssim.blocks;
  RgbdArgs args{};
  static_cast<SsimArgs&>(args) = plan.ssim.args;
  args.a = render;
  args.b = target_rgb;
  args.v_loss = v_loss;
  args.partial = want_loss ? partial : nullptr;
  args.v_a = v_render;
  args.mask = mask;
  args.depth_t = plan.depth ? target_depth : nullptr;
  args.sw_partial = sw_partial;
  args.n_sw = (int)plan.sw_blocks;
  args.render_channels = d->render_channels;
  args.depth_weight = d->depth_weight;
  if (plan.depth)
    hipLaunchKernelGGL(sum_w_kernel, dim3(plan.sw_blocks), dim3(kBlock), 0, s, plan.n_px, mask, target_depth, sw_partial);
  if (want_grad)
    hipLaunchKernelGGL((ssim_kernel<true, true>), dim3(plan.ssim.blocks), dim3(kBlock), 0, s, args);
  else
    hipLaunchKernelGGL((ssim_kernel<false, true>), dim3(plan.ssim.blocks), dim3(kBlock), 0, s, args);
  if (want_loss)
    hipLaunchKernelGGL(rgbd_final_kernel, dim3(1), dim3(kBlock), 0, s, (int)plan.ssim.blocks, partial, plan.ssim.inv_n,
                       plan.ssim.inv_m, plan.m_f, plan.ssim.lambda, d->depth_weight, plan.depth ? sw_partial : nullptr,
                       (int)plan.sw_blocks, loss, terms);
  return check_launch(what);
}

}  // namespace

extern "C" int mgs_rgbd_loss_fwd(const mgs_rgbd_loss* desc, const float* render, const float* target_rgb,
                                 const float* target_depth, const float* mask, float* loss, float* terms,
                                 void* workspace, size_t* workspace_bytes, mgs_stream_t stream) {
  return rgbd_run(desc, render, target_rgb, target_depth, mask, nullptr, loss, terms, nullptr, true, false, workspace,
                  workspace_bytes, (hipStream_t)stream, "rgbd_loss_fwd");
}

extern "C" int mgs_rgbd_loss_fwd_grad(const mgs_rgbd_loss* desc, const float* render, const float* target_rgb,
                                      const float* target_depth, const float* mask, float* loss, float* terms,
                                      float* v_render, void* workspace, size_t* workspace_bytes, mgs_stream_t stream) {
  return rgbd_run(desc, render, target_rgb, target_depth, mask, nullptr, loss, terms, v_render, true, true, workspace,
                  workspace_bytes, (hipStream_t)stream, "rgbd_loss_fwd_grad");
}

extern "C" int mgs_rgbd_loss_bwd(const mgs_rgbd_loss* desc, const float* render, const float* target_rgb,
                                 const float* target_depth, const float* mask, const float* v_loss, float* v_render,
                                 void* workspace, size_t* workspace_bytes, mgs_stream_t stream) {
  return rgbd_run(desc, render, target_rgb, target_depth, mask, v_loss, nullptr, nullptr, v_render, false, true, workspace,
                  workspace_bytes, (hipStream_t)stream, "rgbd_loss_bwd");
}
