// labels.hip -- per-pixel part labels of a frame (include/mgs_labels.h), gfx950.
//
// raster_labels_kernel walks one camera's tile lists the way raster_fwd_kernel does and re-evaluates every pair with the
// forward's own chain (weight_walk.h: weight_walk, shared with raster_votes_kernel, started in tile_group_order), so the
// T and w of every pixel are the forward's bit for bit, as the backward's are.  The queue entry carries the Gaussian's
// class where the forward's carries features, and w goes into the accumulator of that class.  What is this kernel's own:
// the accumulators, the LDS add per reached quadrant and the epilogue.
//
// Accumulators.  K classes x 256 pixels of floats per tile in dynamic LDS (K KB): the word of (class, quadrant k, lane)
// sits at class * 1 KB + k * 256 B + lane * 4 B, so the 64 lanes of an evaluation touch 64 consecutive words -- no bank
// conflict -- and the class, which is the same for all lanes, only moves the base.  Indexing a register array with the
// class would send it to scratch.  The update is one ds_add_f32 without return: LDS operations of a wave complete in
// order, nothing waits for it, and round(W + w) is what the forward's fma(w, 1, W) gives for a one-hot feature.
// A class outside 0..K-1 skips the update (scalar branch): the Gaussian occludes and is reported for no class.
// The epilogue scans the K words of a pixel in ascending class with a strict >.
#include "weight_walk.h"
#include "tile_order.h"
#include "../../include/mgs_labels.h"

namespace mgs {
namespace {

__global__ __launch_bounds__(64) void raster_labels_kernel(
    const float* __restrict__ means2d, const float* __restrict__ conics, const float* __restrict__ opacities,
    const float4* __restrict__ splats, const int32_t* __restrict__ class_ids, int n_classes, int width, int height,
    int tile_w, int n_tiles, const int32_t* __restrict__ tile_offsets, const int32_t* __restrict__ flatten_ids,
    const int32_t* __restrict__ group_order, uint8_t* __restrict__ labels, float* __restrict__ label_weights) {
  __shared__ WeightEntry queue[kQueue + 1];
  extern __shared__ __attribute__((aligned(16))) float class_w[];      // [n_classes][256]: pixel k * 64 + lane of the tile
  const int tile = tile_of_unit((int)blockIdx.x, n_tiles, group_order);      // tile_order.h
  if (tile < 0) return;
  const unsigned lane = threadIdx.x & 63u;
  const TileFrame fr = tile_frame(tile, tile_w, lane);
  const int start = tile_offsets[tile], end = tile_offsets[tile + 1];
  const int ix = fr.ix, iy = fr.iy;
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

  for (int i = 0; i < n_classes; ++i)
    reinterpret_cast<float4*>(class_w)[i * 64 + lane] = make_float4(0.f, 0.f, 0.f, 0.f);

  unsigned long long alive[4];                    // the quadrant's open pixels
#pragma unroll
  for (int k = 0; k < 4; ++k)
    alive[k] = ballot(ix + 8 * (k & 1) < width && iy + 8 * (k >> 1) < height);      // pixels outside the image start finished
  __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");      // the zeroed accumulators, before the first update
  __builtin_amdgcn_wave_barrier();
  __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");

  weight_walk(queue, fr, lane, start, end, splats, means2d, conics, opacities, flatten_ids, alive,
              [&](int g) { return class_ids[g]; },
              [&](int cls, auto quad) {
                // the class moves only the accumulator's base
                const bool counted = (unsigned)cls < (unsigned)n_classes;
                float* slot = class_w + (counted ? cls : 0) * 256 + lane;
#pragma unroll
                for (int k = 0; k < 4; ++k) {
                  float w;
                  if (quad(k, w) && counted) atomicAdd(slot + 64 * k, w);      // ds_add_f32, no return
                }
              });

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
  const int n_tiles = tile_w * tile_h, n_units = tile_launch_units(n_tiles, tile_group_order);
  hipLaunchKernelGGL(raster_labels_kernel, dim3(n_units), dim3(64), (size_t)n_classes * 1024, (hipStream_t)stream, means2d,
                     conics, opacities, reinterpret_cast<const float4*>(splats), class_ids, n_classes, width, height, tile_w,
                     n_tiles, tile_offsets, flatten_ids, tile_group_order, labels, label_weights);
  return check_launch("raster_labels");
}
