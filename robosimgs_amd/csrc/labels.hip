// labels.hip -- per-pixel part labels of a frame (include/mgs_labels.h), gfx950.
//
// raster_labels_kernel walks one camera's tile lists the way raster_fwd_kernel does (raster_common.h: one wave per 16x16
// tile, four pixels per lane, batches of kQueue entries culled with quadrant_reach and queued in LDS, started in
// tile_group_order) and re-evaluates every pair with the forward's own chain -- pair_power_poly on poly_coefs, v_exp,
// the clamp and the sigma test on batches that are not entry_is_safe, next_T = fma(-alpha, T, T), w = alpha T -- so the
// T and w of every pixel are the forward's bit for bit, as the backward's are.  The queue entry carries the Gaussian's
// class where the forward's carries features, and w goes into the accumulator of that class.
//
// Accumulators.  K classes x 256 pixels of floats per tile in dynamic LDS (K KB): the word of (class, quadrant k, lane)
// sits at class * 1 KB + k * 256 B + lane * 4 B, so the 64 lanes of an evaluation touch 64 consecutive words -- no bank
// conflict -- and the class, which is the same for all lanes, only moves the base.  Indexing a register array with the
// class would send it to scratch.  The update is one ds_add_f32 without return: LDS operations of a wave complete in
// order, nothing waits for it, and round(W + w) is what the forward's fma(w, 1, W) gives for a one-hot feature.
// A class outside 0..K-1 skips the update (scalar branch): the Gaussian occludes and is reported for no class.
// The epilogue scans the K words of a pixel in ascending class with a strict >.
#include "raster_common.h"
#include "pair_weight.h"
#include "tile_order.h"
#include "../../include/mgs_labels.h"

namespace mgs {
namespace {

struct LabelEntry {
  float4 geo0;                       // q0, q1, q2, A   (raster_common.h: poly_coefs; A, B, C: conic pre-scaled)
  float4 geo1;                       // B, C, class (bits), unused
  float4 geo3;                       // mean - tile centre (x, y): read only by batches that test sigma >= 0
};

__global__ __launch_bounds__(64) void raster_labels_kernel(
    const float* __restrict__ means2d, const float* __restrict__ conics, const float* __restrict__ opacities,
    const float4* __restrict__ splats, const int32_t* __restrict__ class_ids, int n_classes, int width, int height,
    int tile_w, int n_tiles, const int32_t* __restrict__ tile_offsets, const int32_t* __restrict__ flatten_ids,
    const int32_t* __restrict__ group_order, uint8_t* __restrict__ labels, float* __restrict__ label_weights) {
  __shared__ LabelEntry queue[kQueue + 1];
  extern __shared__ __attribute__((aligned(16))) float class_w[];      // [n_classes][256]: pixel k * 64 + lane of the tile
  const int tile = tile_of_unit((int)blockIdx.x, n_tiles, group_order);      // tile_order.h
  if (tile < 0) return;
  const unsigned lane = threadIdx.x & 63u;
  const int tx = tile % tile_w, ty = tile / tile_w;
  const float tile_x = (float)(tx * 16), tile_y = (float)(ty * 16);
  const int start = tile_offsets[tile], end = tile_offsets[tile + 1];
  const int ix = tx * 16 + (int)(lane & 7), iy = ty * 16 + (int)(lane >> 3);
  if (start >= end) {                             // no list: no label anywhere in the tile
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      const int x = ix + 8 * (k & 1), y = iy + 8 * (k >> 1);
      if (x < width && y < height) {
        const size_t p = (size_t)y * width + x;
        labels[p] = MGS_LABEL_NONE;
        if (label_weights) label_weights[p] = 0.f;
      }
    }
    return;
  }
  const float xo = (float)(lane & 7) - 7.5f, yo = (float)(lane >> 3) - 7.5f;
  PixelPoly pq[4];
#pragma unroll
  for (int k = 0; k < 4; ++k) pq[k] = pixel_poly(xo + 8.f * (k & 1), yo + 8.f * (k >> 1));
  const float ctr_x = tile_x + 8.f, ctr_y = tile_y + 8.f;

  for (int i = 0; i < n_classes; ++i)
    reinterpret_cast<float4*>(class_w)[i * 64 + lane] = make_float4(0.f, 0.f, 0.f, 0.f);

  float T[4];
  unsigned long long alive[4];                    // the quadrant's open pixels
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    T[k] = 1.f;
    alive[k] = ballot(ix + 8 * (k & 1) < width && iy + 8 * (k >> 1) < height);      // pixels outside the image start finished
  }

  // the batch registers: one list entry per lane
  int r_idx = start + (int)lane;
  bool r_ok = r_idx < end;
  float2 r_xy = make_float2(0.f, 0.f);
  float r_ca = 1.f, r_cb = 0.f, r_cc = 1.f, r_op = 0.f;
  int r_cls = -1;
  auto fetch = [&](int idx, bool ok) {
    if (!ok) return;
    const int g = flatten_ids[idx];
    r_cls = class_ids[g];
    if (splats) {                                 // the packed 48-byte record: its first two quarters
      const float4 p0 = splats[3 * (size_t)g], p1 = splats[3 * (size_t)g + 1];
      r_xy = make_float2(p0.x, p0.y);
      r_ca = p0.z; r_cb = p0.w; r_cc = p1.x; r_op = p1.y;
    } else {
      r_xy = reinterpret_cast<const float2*>(means2d)[g];
      r_ca = conics[3 * (size_t)g + 0];
      r_cb = conics[3 * (size_t)g + 1];
      r_cc = conics[3 * (size_t)g + 2];
      r_op = opacities[g];
    }
  };
  fetch(r_idx, r_ok);
  __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");      // the zeroed accumulators, before the first update
  __builtin_amdgcn_wave_barrier();
  __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");

  for (int b = start; b < end; b += kQueue) {
    unsigned live = 0;
#pragma unroll
    for (int k = 0; k < 4; ++k)
      if (alive[k] != 0ull) live |= 1u << k;
    if (live == 0) break;

    // this batch's entries (the first batch was fetched above, beside the zeroing of the accumulators)
    if (b != start) { r_idx = b + (int)lane; r_ok = r_idx < end; fetch(r_idx, r_ok); }
    const bool c_ok = r_ok;
    const float2 c_xy = r_xy;
    const float c_ca = r_ca, c_cb = r_cb, c_cc = r_cc, c_op = r_op;
    const int c_cls = r_cls;

    unsigned long long reach[4];
    quadrant_reach(c_xy.x, c_xy.y, c_ca, c_cb, c_cc, c_op, c_ok, tile_x, tile_y, live, reach);
    const unsigned long long keep = reach[0] | reach[1] | reach[2] | reach[3];
    const bool queued = __builtin_amdgcn_inverse_ballot_w64(keep);
    const bool all_safe = ballot(queued && !entry_is_safe(c_ca, c_cb, c_cc, c_op)) == 0ull;
    if (queued) {
      LabelEntry& e = queue[mask_rank(keep)];
      const float sA = -0.5f * kLog2e * c_ca, sB = -kLog2e * c_cb, sC = -0.5f * kLog2e * c_cc;
      const float m_x = c_xy.x - ctr_x, m_y = c_xy.y - ctr_y;
      const PolyCoef q = poly_coefs(m_x, m_y, sA, sB, sC, __log2f(c_op));
      e.geo0 = make_float4(q.q0, q.q1, q.q2, sA);
      e.geo1 = make_float4(sB, sC, __int_as_float(c_cls), 0.f);
      e.geo3 = make_float4(m_x, m_y, 0.f, 0.f);
    }
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");

    auto walk = [&](auto safe_tag) {
      constexpr bool SAFE = decltype(safe_tag)::value;
      // entry j was queued by the lane of the j-th set bit of `keep`
      unsigned long long rest = keep;
      const LabelEntry* e = queue;
      while (rest != 0ull) {
        const int at = __builtin_ctzll(rest);
        rest &= rest - 1ull;
        const float4 g0 = e->geo0, g1 = e->geo1;
        float4 g3 = make_float4(0.f, 0.f, 0.f, 0.f);
        if constexpr (!SAFE) g3 = e->geo3;
        ++e;
        // the class is the same for all 64 lanes of the evaluation: a scalar, and with it the accumulator's base
        const int cls = __builtin_amdgcn_readfirstlane(__float_as_int(g1.z));
        const bool counted = (unsigned)cls < (unsigned)n_classes;
        float* slot = class_w + (counted ? cls : 0) * 256 + lane;
#pragma unroll
        for (int k = 0; k < 4; ++k) {
          if ((reach[k] >> at) & 1ull) {
            const float w = pair_weight<SAFE>(T[k], alive[k], pq[k], g0.x, g0.y, g0.z, g0.w, g1.x, g1.y, g3.x, g3.y);
            if (counted) atomicAdd(slot + 64 * k, w);      // ds_add_f32, no return
            if (alive[k] == 0ull) reach[k] = 0ull;         // the quadrant's last pixel closed: the batch skips it
          }
        }
      }
    };
    if (all_safe) walk(std::true_type{}); else walk(std::false_type{});
    __builtin_amdgcn_wave_barrier();   // queue is rewritten by the next batch
  }

  __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
  __builtin_amdgcn_wave_barrier();
  __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
  float best[4] = {0.f, 0.f, 0.f, 0.f};
  int label[4] = {MGS_LABEL_NONE, MGS_LABEL_NONE, MGS_LABEL_NONE, MGS_LABEL_NONE};
  for (int c = 0; c < n_classes; ++c) {           // ascending class, strict >: ties go to the lowest class
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      const float v = class_w[c * 256 + 64 * k + lane];
      if (v > best[k]) { best[k] = v; label[k] = c; }
    }
  }
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    const int x = ix + 8 * (k & 1), y = iy + 8 * (k >> 1);
    if (x < width && y < height) {
      const size_t p = (size_t)y * width + x;
      labels[p] = (uint8_t)label[k];
      if (label_weights) label_weights[p] = best[k];
    }
  }
}

}  // namespace

int check_label_args(const char* fn, const int32_t* class_ids, int n_classes, const uint8_t* labels) {
  MGS_REQUIRE(n_classes >= 1 && n_classes <= MGS_LABELS_MAX_CLASSES, "%s: n_classes %d outside 1..%d", fn, n_classes,
              MGS_LABELS_MAX_CLASSES);
  MGS_REQUIRE(class_ids, "%s: class_ids is null", fn);
  MGS_REQUIRE(labels, "%s: labels is null", fn);
  return MGS_OK;
}

}  // namespace mgs

using namespace mgs;

extern "C" int mgs_raster_labels(int n, const float* means2d, const float* conics, const float* opacities,
                                 const float* splats, const int32_t* class_ids, int n_classes, int width, int height,
                                 int tile_w, int tile_h, const int32_t* tile_offsets, const int32_t* flatten_ids,
                                 const int32_t* tile_group_order, uint8_t* labels, float* label_weights,
                                 mgs_stream_t stream) {
  const int rc = check_label_args("raster_labels", class_ids, n_classes, labels);
  if (rc) return rc;
  MGS_REQUIRE(splats || (means2d && conics && opacities),
              "raster_labels: neither packed records (splats) nor means2d, conics and opacities given");
  MGS_REQUIRE(n >= 0 && width > 0 && height > 0, "raster_labels: bad sizes");
  MGS_REQUIRE(tile_w == (width + 15) / 16 && tile_h == (height + 15) / 16,
              "raster_labels: tile grid %dx%d does not match %dx%d at tile size 16", tile_w, tile_h, width, height);
  MGS_REQUIRE(tile_offsets && flatten_ids, "raster_labels: null tile lists");
  const int n_tiles = tile_w * tile_h;
  const int n_units = tile_group_order ? (n_tiles + 3) / 4 * 4 : n_tiles;       // tile slots of the launch
  hipLaunchKernelGGL(raster_labels_kernel, dim3(n_units), dim3(64), (size_t)n_classes * 1024, (hipStream_t)stream, means2d,
                     conics, opacities, reinterpret_cast<const float4*>(splats), class_ids, n_classes, width, height, tile_w,
                     n_tiles, tile_offsets, flatten_ids, tile_group_order, labels, label_weights);
  return check_launch("raster_labels");
}
