// mgs_common.h -- host-side plumbing shared by the libmgs.so translation units.
#ifndef MGS_COMMON_H_
#define MGS_COMMON_H_

#include <hip/hip_runtime.h>
#include <stdarg.h>
#include <stdint.h>
#include <stdio.h>

#include <type_traits>

#include "../../include/mgs.h"
#include "../../include/mgs_lens.h"
#include "../../include/mgs_lens_pinhole.h"

namespace mgs {

// thread-local last-error text behind mgs_last_error_string()
char* error_buffer();
int set_error(int code, const char* fmt, ...);

inline int check_launch(const char* what) {
  hipError_t e = hipGetLastError();
  if (e != hipSuccess)
    return set_error((int)e, "%s: launch failed: %s", what, hipGetErrorString(e));
  return MGS_OK;
}

inline unsigned div_up(unsigned a, unsigned b) { return (a + b - 1) / b; }
inline size_t align_up(size_t v, size_t a) { return (v + a - 1) / a * a; }

#define MGS_REQUIRE(cond, ...) \
  do {                         \
    if (!(cond)) return ::mgs::set_error(MGS_ERR_INVALID_ARGUMENT, __VA_ARGS__); \
  } while (0)

// Bump allocator of a workspace or state layout: fields in the order taken, each on a 256-byte boundary.
// min_field: the smallest size a field is given -- 1 keeps a 256-byte slot (and a distinct address) for an empty one.
struct Bump {
  size_t total = 0, min_field;
  explicit Bump(size_t min_field) : min_field(min_field) {}
  size_t take(size_t bytes) {
    const size_t at = total;
    total += align_up(bytes > min_field ? bytes : min_field, 256);
    return at;
  }
};

// ---- typed launch dispatch ----------------------------------------------------------------
// Each helper maps a (validated) runtime value to a std::integral_constant and calls f with it, so that a generic lambda
// names its instantiation as kernel<decltype(x)::value>.  Only the values listed are instantiated; a launch that exists
// for some combinations only says so with `if constexpr`.
template <int V> using int_c = std::integral_constant<int, V>;
template <bool V> using bool_c = std::integral_constant<bool, V>;

template <class F> void with_bool(bool b, F&& f) {
  if (b) f(bool_c<true>{});
  else f(bool_c<false>{});
}
// v in Lo..Hi-1 -> int_c<v>; any other value -> int_c<Hi>
template <int Lo, int Hi, class F> void with_int(int v, F&& f) {
  if constexpr (Lo == Hi) f(int_c<Hi>{});
  else if (v == Lo) f(int_c<Lo>{});
  else with_int<Lo + 1, Hi>(v, f);
}
// MGS_CAMERA_*: anything past MGS_CAMERA_FISHEYE_KB is MGS_CAMERA_PINHOLE_BC
template <class F> void with_camera(int model, F&& f) { with_int<MGS_CAMERA_PINHOLE, MGS_CAMERA_PINHOLE_BC>(model, f); }
inline bool is_camera_model(int model) { return model >= MGS_CAMERA_PINHOLE && model <= MGS_CAMERA_PINHOLE_BC; }
// floats per camera behind a `K` / `Ks` pointer (include/mgs.h at MGS_CAMERA_*, include/mgs_lens_pinhole.h)
inline size_t camera_row_floats(int model) {
  return (model == MGS_CAMERA_FISHEYE_KB || model == MGS_CAMERA_PINHOLE_BC) ? MGS_LENS_ROW_FLOATS : 9;
}
// Where a call names the model in its camera_model argument (mgs_projection_fwd / _bwd, mgs_project_color_bwd),
// MGS_CAMERA_PINHOLE_BC is taken only together with its camera row: K == NULL is refused before anything else, for n == 0
// too (include/mgs_lens_pinhole.h).  The value 4 was "no camera model" before this model existed, and a caller that
// probes for that with an empty call keeps getting MGS_ERR_INVALID_ARGUMENT.
constexpr const char* kPinholeLensNeedsRow =
    "camera_model MGS_CAMERA_PINHOLE_BC needs K, the camera's 16-float row (include/mgs_lens_pinhole.h), for n = 0 too";
// SH degree 0..3: anything past 2 is 3
template <class F> void with_sh_degree(int degree, F&& f) { with_int<0, 3>(degree, f); }
// MGS_RADIUS_OPACITY_AWARE when per_axis, MGS_RADIUS_CLASSIC otherwise
template <class F> void with_radius_rule(bool per_axis, F&& f) {
  if (per_axis) f(int_c<MGS_RADIUS_OPACITY_AWARE>{});
  else f(int_c<MGS_RADIUS_CLASSIC>{});
}
// channels 1..MGS_MAX_CHANNELS -> the kernels' channel width: 1, 2, 3, 4, 8, 16 or 32
template <class F> void with_channels(int channels, F&& f) {
  if (channels == 1) f(int_c<1>{});
  else if (channels == 2) f(int_c<2>{});
  else if (channels == 3) f(int_c<3>{});
  else if (channels == 4) f(int_c<4>{});
  else if (channels <= 8) f(int_c<8>{});
  else if (channels <= 16) f(int_c<16>{});
  else f(int_c<32>{});
}

// the camera model the MGS_BIN_CAMERA_* bits of a bin_flags word select (at most one is set: the caller checks)
inline int bin_camera_model(int bin_flags) {
  return (bin_flags & MGS_BIN_CAMERA_ORTHO) ? MGS_CAMERA_ORTHO
         : (bin_flags & MGS_BIN_CAMERA_FISHEYE) ? MGS_CAMERA_FISHEYE
         : (bin_flags & MGS_BIN_CAMERA_FISHEYE_KB) ? MGS_CAMERA_FISHEYE_KB
         : (bin_flags & MGS_BIN_CAMERA_PINHOLE_BC) ? MGS_CAMERA_PINHOLE_BC : MGS_CAMERA_PINHOLE;
}
// more than one of the camera bits `bits` set in `flags`
inline bool several_camera_bits(int flags, int bits) { const int c = flags & bits; return (c & (c - 1)) != 0; }

// ---- wave64 helpers -----------------------------------------------------------------
#if defined(__HIPCC__)
__device__ __forceinline__ unsigned lane_id() {
  return __builtin_amdgcn_mbcnt_hi(~0u, __builtin_amdgcn_mbcnt_lo(~0u, 0u));
}
// wave64 ballot of a predicate: the lane mask the compare already produced.  (HIP's __ballot(int) turns the predicate
// into 0 / 1 and compares that with zero again: a v_cndmask and a v_cmp per call that the compiler does not always fold
// away -- two of the per-tile sort's group filter's instructions per list entry were exactly these.)
__device__ __forceinline__ unsigned long long ballot(bool p) { return __builtin_amdgcn_ballot_w64(p); }
// number of set bits of `mask` strictly below this lane
__device__ __forceinline__ unsigned mask_rank(unsigned long long mask) {
  return __builtin_amdgcn_mbcnt_hi((unsigned)(mask >> 32),
                                   __builtin_amdgcn_mbcnt_lo((unsigned)mask, 0u));
}
// wave-wide OR / AND / sum of one 32-bit value per lane, returned wave-uniform.  Six DPP steps (quad_perm x2,
// row_half_mirror, row_mirror, row_bcast15, row_bcast31: the total lands in lane 63) and a readlane, instead of six
// ds_bpermute round trips with their lane-index arithmetic (__shfl_xor).
#define MGS_DPP_STEP(OP, IDENT, CTRL, RMASK) \
  v = v OP (uint32_t)__builtin_amdgcn_update_dpp((int)(IDENT), (int)v, CTRL, RMASK, 0xf, false);
#define MGS_WAVE_REDUCE(NAME, OP, IDENT)                                         \
  __device__ __forceinline__ uint32_t NAME(uint32_t v) {                         \
    MGS_DPP_STEP(OP, IDENT, 0xB1, 0xf)                                           \
    MGS_DPP_STEP(OP, IDENT, 0x4E, 0xf)                                           \
    MGS_DPP_STEP(OP, IDENT, 0x141, 0xf)                                          \
    MGS_DPP_STEP(OP, IDENT, 0x140, 0xf)                                          \
    MGS_DPP_STEP(OP, IDENT, 0x142, 0xa)                                          \
    MGS_DPP_STEP(OP, IDENT, 0x143, 0xc)                                          \
    return (uint32_t)__builtin_amdgcn_readlane((int)v, 63);                      \
  }
MGS_WAVE_REDUCE(wave_or, |, 0u)
MGS_WAVE_REDUCE(wave_and, &, ~0u)
MGS_WAVE_REDUCE(wave_sum_u32, +, 0u)
#undef MGS_WAVE_REDUCE
#undef MGS_DPP_STEP
#endif

// ---- internal launchers shared between translation units ---------------------------------
// Workspace sizes (what the size queries of mgs_isect_tiles and mgs_rasterize_bwd_det report): binning n Gaussians
// into at most `capacity` pairs on n_tiles tiles; the deterministic raster backward (checkpoint_interval 0: no
// checkpoints; otherwise a power of two >= 64).  Hidden: they add nothing to the library's exported symbols.
__attribute__((visibility("hidden"))) size_t isect_tiles_workspace_bytes(int n, uint32_t capacity, int n_tiles);
__attribute__((visibility("hidden"))) size_t rasterize_bwd_det_workspace_bytes(int channels, bool absgrad, uint32_t capacity,
                                                                               int tile_w, int tile_h, int checkpoint_interval);

// The label arguments mgs_raster_labels and mgs_render_frames_labeled share (labels.hip; include/mgs_labels.h): checked
// under the caller's name `fn` before anything is enqueued.
__attribute__((visibility("hidden"))) int check_label_args(const char* fn, const int32_t* class_ids, int n_classes,
                                                           const uint8_t* labels);

// Radix sort of (key, value) uint32 pairs on bits [0, key_bits) with the element count read
// from device memory.  Buffers a/b alternate; the sorted result ends in (keys_out, vals_out).
// temp: radix_sort_temp_bytes(capacity).
size_t radix_sort_temp_bytes(uint32_t capacity);
int radix_sort_pairs(const uint32_t* n_dev, uint32_t capacity, int key_bits, uint32_t* keys_in,
                     uint32_t* vals_in, uint32_t* keys_out, uint32_t* vals_out, void* temp,
                     hipStream_t stream);

// Orders flatten_ids[offsets[t] .. offsets[t+1]) of every tile by (depth bits, Gaussian id)
// (tile_sort.hip).  temp: tile_depth_sort_temp_bytes(capacity).
size_t tile_depth_sort_temp_bytes(uint32_t capacity, int n_tiles);
// first word of the list of long tiles inside `temp` (a header of eight counters, 16-byte aligned: they must be zero when
// tile_depth_sort starts)
uint32_t* tile_depth_sort_long_list(void* temp, uint32_t capacity);
// tile_ids_fill (may be null): also stores every entry's tile id (the direct binning path has not written them).
// staging / group_offsets / group_shift (staging may be null): the lists arrive grouped, 2^group_shift tiles per
// segment of `staging`, and the kernel also WRITES tile_offsets (see tile_sort.hip).
// long_list_zeroed: an earlier kernel of the caller has stored the zeros (otherwise a 32-byte memset is enqueued).
// scratch_k / scratch_i: two more arrays of `capacity` words that nobody reads once the per-tile sort's first launch is
// done (scratch_i may be `staging`): scratch of the kernel that sorts the units of long lists; null: no list is deferred.
int tile_depth_sort(int n_tiles, const int32_t* tile_offsets, const float* depths, uint32_t capacity,
                    uint32_t* flatten_ids, uint32_t* tile_ids_fill, void* temp, hipStream_t stream,
                    uint32_t* scratch_k, uint32_t* scratch_i,
                    const uint32_t* staging = nullptr, const int32_t* group_offsets = nullptr, int group_shift = 0,
                    bool long_list_zeroed = false);

// mgs_debug_set_sort_opts() bits (sort.hip): 1 one-sweep radix passes, 2 ... also for small inputs,
// 4 binning partitions by tile with the radix passes even where the direct path applies
int sort_opts();

}  // namespace mgs
#endif
