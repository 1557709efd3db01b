// mesh_texture.hip -- textured triangle meshes (include/mgs_mesh_texture.h), gfx950: the mip chain of a texture set and the
// textured resolve stage.  The vertex and raster stages are mesh.hip's, and so is the untextured resolve kernel: a mesh
// without textures never comes here.  Every expression that decides an index or a value is mesh_texture.h's, shared with
// the host harness (tests/host_harness/mesh_texture_harness.cpp); what is here is the launch shape.  The argument checks
// are mesh_checks.h's, shared with mesh.hip and mesh_lens.hip.
//
// mesh_mips_kernel              one thread per texel of the destination level, one launch per (texture, level): four 32-bit
//                               loads, the per-byte sums in registers, one 32-bit store.
// mesh_resolve_textured_kernel  one thread per (camera, pixel), like mesh_resolve_kernel.  The wave compares the texture ids
//                               of its covered, textured pixels: where they agree (the usual case: a wave is 64 neighbours
//                               of a row) the descriptor is read through that one wave-uniform index, one address for
//                               the whole wave, which leaves the compiler free to use scalar loads; otherwise each lane
//                               reads its own.  Texel fetches are 4-byte vector loads, four per level.  No atomics, no
//                               LDS, nothing written but the outputs.
#include "mgs_common.h"
#include "../../include/mgs_mesh_texture.h"

#define MGS_MESH_HD __host__ __device__ __forceinline__
#include "mesh_texture.h"
#include "mesh_checks.h"

namespace mgs {
namespace {

using namespace mesh;
static_assert(sizeof(TexDesc) == 4 * kTexDescWords && kTexDescWords == MGS_MESH_TEXTURE_DESC_WORDS, "descriptor layout");
static_assert(kTexMaxSide == MGS_MESH_TEXTURE_MAX_SIDE && kTexMaxTextures == MGS_MESH_MAX_TEXTURES, "limits disagree");
static_assert(kFilterBilinear == MGS_MESH_FILTER_BILINEAR && kFilterTrilinear == MGS_MESH_FILTER_TRILINEAR, "filters disagree");
static_assert(kWrapRepeat == MGS_MESH_WRAP_REPEAT && kWrapClamp == MGS_MESH_WRAP_CLAMP && kWrapMirror == MGS_MESH_WRAP_MIRROR,
              "wrap modes disagree");

__global__ __launch_bounds__(kGroup) void mesh_mips_kernel(const uint32_t* __restrict__ src, int sw, int sh,
                                                          uint32_t* __restrict__ dst, int dw, int dh) {
  const long long i = (long long)blockIdx.x * kGroup + threadIdx.x;
  if (i >= (long long)dw * dh) return;
  const int x = (int)(i % dw), y = (int)(i / dw);
  dst[i] = mip_texel(src, sw, sh, x, y);
}

template <int kFilter>
__global__ __launch_bounds__(kGroup) void mesh_resolve_textured_kernel(
    int V, const float* __restrict__ verts_cam, int F, const int32_t* __restrict__ faces, const float* __restrict__ vertex_colors,
    const float* __restrict__ face_colors, const float* __restrict__ Ks, int width, int height, int headlight, float ambient,
    const unsigned long long* __restrict__ vis, const float* __restrict__ face_uvs, const int32_t* __restrict__ face_textures,
    int T, const TexDesc* __restrict__ descs, const uint32_t* __restrict__ texels, uint64_t texel_count, float* __restrict__ rgb,
    float* __restrict__ depth, int32_t* __restrict__ face_ids, float* __restrict__ normals) {
  const int c = (int)blockIdx.y;
  const long long p = (long long)blockIdx.x * kGroup + threadIdx.x;
  const bool inside = p < (long long)width * height;     // nobody leaves before the wave has compared its texture ids
  const int px = inside ? (int)(p % width) : 0, py = inside ? (int)(p / width) : 0;
  const size_t at = pixel_index(c, width, height, px, py);
  const uint64_t key = inside ? vis[at] : kEmptyKey;
  const int32_t tid = key_texture(key, face_textures, F, T);                // -1, or inside 0 .. T-1
  const unsigned long long textured = ballot(tid >= 0);
  const float* vc = verts_cam + vertex_index(c, V, 0);
  const Cam cam = load_cam(Ks + 9 * (size_t)c);
  const int32_t first = textured ? __builtin_amdgcn_readlane(tid, __builtin_ctzll(textured)) : 0;       // inside 0 .. T-1
  Shaded s;
  if (ballot(tid >= 0 && tid != first) == 0ull)                             // the wave agrees: one descriptor, one address
    s = resolve_pixel_textured(key, vc, V, faces, F, vertex_colors, face_colors, cam, px, py, headlight != 0, ambient, face_uvs,
                               tid >= 0, descs + first, texels, texel_count, kFilter);
  else
    s = resolve_pixel_textured(key, vc, V, faces, F, vertex_colors, face_colors, cam, px, py, headlight != 0, ambient, face_uvs,
                               tid >= 0, descs + (tid >= 0 ? tid : 0), texels, texel_count, kFilter);
  if (inside) store_shaded(s, at, rgb, depth, face_ids, normals);
}

int check_texture_count(const char* fn, int T) {
  MGS_REQUIRE(T >= 1 && T <= kTexMaxTextures, "%s: n_textures %d is outside 1 .. %d", fn, T, kTexMaxTextures);
  return MGS_OK;
}

}  // namespace
}  // namespace mgs

using namespace mgs;

extern "C" int mgs_mesh_texture_layout(int n_textures, const int32_t* sizes, const int32_t* wraps, int32_t* descriptors,
                                       size_t* texel_count) {
  MGS_TRY(check_texture_count("mesh_texture_layout", n_textures));
  MGS_REQUIRE(sizes && texel_count, "mesh_texture_layout: sizes or texel_count is null");
  for (int t = 0; t < n_textures; ++t) {
    const int w = sizes[2 * t], h = sizes[2 * t + 1];
    MGS_REQUIRE(w >= 1 && w <= kTexMaxSide && h >= 1 && h <= kTexMaxSide,
                "mesh_texture_layout: texture %d is %d x %d, each side must be in 1 .. %d", t, w, h, kTexMaxSide);
    MGS_REQUIRE(!wraps || (wrap_ok(wraps[2 * t]) && wrap_ok(wraps[2 * t + 1])),
                "mesh_texture_layout: texture %d has wrap modes %d, %d, each must be 0 (repeat), 1 (clamp) or 2 (mirror)", t,
                wraps ? wraps[2 * t] : 0, wraps ? wraps[2 * t + 1] : 0);
  }
  const uint64_t n = texture_layout(n_textures, sizes, wraps, reinterpret_cast<TexDesc*>(descriptors));
  MGS_REQUIRE(n != 0, "mesh_texture_layout: the texels of all levels of %d textures reach 2^31", n_textures);
  *texel_count = (size_t)n;
  return MGS_OK;
}

extern "C" int mgs_mesh_build_mips(int n_textures, const int32_t* descriptors, void* texels, size_t texel_count,
                                   mgs_stream_t stream) {
  MGS_TRY(check_texture_count("mesh_build_mips", n_textures));
  MGS_REQUIRE(descriptors && texels, "mesh_build_mips: descriptors or texels is null");
  MGS_REQUIRE(((uintptr_t)texels & 3u) == 0, "mesh_build_mips: texels is not 4-byte aligned");
  // the descriptors drive the launches: they must be exactly what mgs_mesh_texture_layout gives for their own sizes
  const TexDesc* d = reinterpret_cast<const TexDesc*>(descriptors);
  uint64_t at = 0;
  for (int t = 0; t < n_textures; ++t) {
    MGS_REQUIRE(d[t].w >= 1 && d[t].w <= kTexMaxSide && d[t].h >= 1 && d[t].h <= kTexMaxSide,
                "mesh_build_mips: descriptor %d is %d x %d, each side must be in 1 .. %d", t, d[t].w, d[t].h, kTexMaxSide);
    MGS_REQUIRE(d[t].levels == level_count(d[t].w, d[t].h), "mesh_build_mips: descriptor %d has %d levels, %d x %d has %d", t,
                d[t].levels, d[t].w, d[t].h, level_count(d[t].w, d[t].h));
    for (int l = 0; l < d[t].levels; ++l) {
      MGS_REQUIRE((uint64_t)d[t].offset[l] == at, "mesh_build_mips: descriptor %d, level %d starts at texel %u, the layout has %llu",
                  t, l, d[t].offset[l], (unsigned long long)at);
      at += (uint64_t)level_side(d[t].w, l) * (uint64_t)level_side(d[t].h, l);
      MGS_REQUIRE(at < (1ull << 31), "mesh_build_mips: the texels of all levels reach 2^31");
    }
  }
  MGS_REQUIRE((uint64_t)texel_count == at, "mesh_build_mips: texel_count %zu, the descriptors describe %llu", texel_count,
              (unsigned long long)at);
  uint32_t* base = static_cast<uint32_t*>(texels);
  for (int t = 0; t < n_textures; ++t)
    for (int l = 1; l < d[t].levels; ++l) {
      const int sw = level_side(d[t].w, l - 1), sh = level_side(d[t].h, l - 1), dw = level_side(d[t].w, l), dh = level_side(d[t].h, l);
      const size_t n = (size_t)dw * (size_t)dh;                              // <= 2^26
      hipLaunchKernelGGL(mesh_mips_kernel, dim3((unsigned)((n + kGroup - 1) / kGroup)), dim3(kGroup), 0, (hipStream_t)stream,
                         (const uint32_t*)(base + (size_t)d[t].offset[l - 1]), sw, sh, base + (size_t)d[t].offset[l], dw, dh);
      MGS_TRY(check_launch("mesh_build_mips"));
    }
  return MGS_OK;
}

namespace {
int check_texture_args(const char* fn, const float* face_uvs, const int32_t* face_textures, int T, const int32_t* descriptors,
                       const void* texels, size_t texel_count, int filter) {
  MGS_TRY(check_texture_count(fn, T));
  MGS_REQUIRE(face_uvs && face_textures && descriptors && texels, "%s: face_uvs, face_textures, descriptors or texels is null", fn);
  MGS_REQUIRE(((uintptr_t)texels & 3u) == 0 && ((uintptr_t)descriptors & 3u) == 0, "%s: texels or descriptors is not 4-byte aligned", fn);
  MGS_REQUIRE(texel_count >= 1 && (uint64_t)texel_count < (1ull << 31), "%s: texel_count %zu is outside 1 .. 2^31 - 1", fn, texel_count);
  MGS_REQUIRE(filter == kFilterBilinear || filter == kFilterTrilinear, "%s: filter %d is neither 0 (bilinear) nor 1 (trilinear)", fn,
              filter);
  return MGS_OK;
}
}  // namespace

extern "C" int mgs_mesh_resolve_textured(int n_cams, int V, const float* verts_cam, int F, const int32_t* faces,
                                         const float* vertex_colors, const float* face_colors, const float* Ks, int width,
                                         int height, int headlight, float ambient, const void* workspace, size_t workspace_bytes,
                                         float* rgb, float* depth, int32_t* face_ids, float* normals, const float* face_uvs,
                                         const int32_t* face_textures, int n_textures, const int32_t* descriptors,
                                         const void* texels, size_t texel_count, int filter, mgs_stream_t stream) {
  const char* fn = "mesh_resolve_textured";
  // the sizes in this entry point's own order (n_cams above 65535 is reported before V, F and the image)
  MGS_REQUIRE(n_cams >= 1 && n_cams <= 65535, "%s: n_cams %d is outside 1 .. 65535", fn, n_cams);
  MGS_REQUIRE(V >= 1, "%s: V %d vertices, at least 1 needed", fn, V);
  MGS_REQUIRE(F >= 1, "%s: F %d faces, at least 1 needed", fn, F);
  MGS_REQUIRE(width >= 1 && width <= kMaxSide && height >= 1 && height <= kMaxSide, "%s: image %d x %d, each side must be in 1 .. %d",
              fn, width, height, kMaxSide);
  MGS_TRY(check_ambient(fn, ambient));
  MGS_REQUIRE(verts_cam && faces && Ks, "%s: verts_cam, faces or Ks is null", fn);
  MGS_REQUIRE(rgb && depth && face_ids, "%s: an output (rgb, depth, face_ids) is null", fn);
  MGS_TRY(check_texture_args(fn, face_uvs, face_textures, n_textures, descriptors, texels, texel_count, filter));
  const Layout l = workspace_layout(n_cams, F, width, height);
  MGS_TRY(check_workspace(fn, "workspace", workspace, workspace_bytes, l.total));
  const unsigned long long* vis = reinterpret_cast<const unsigned long long*>(static_cast<const char*>(workspace) + l.vis);
  const size_t n_px = (size_t)width * (size_t)height;                        // <= 16368^2 < 2^28
  const dim3 grid((unsigned)((n_px + kGroup - 1) / kGroup), (unsigned)n_cams), block(kGroup);
  const TexDesc* d = reinterpret_cast<const TexDesc*>(descriptors);
  const uint32_t* tx = static_cast<const uint32_t*>(texels);
  with_bool(filter == kFilterTrilinear, [&](auto tri) {
    constexpr int kF = decltype(tri)::value ? kFilterTrilinear : kFilterBilinear;
    hipLaunchKernelGGL(mesh_resolve_textured_kernel<kF>, grid, block, 0, (hipStream_t)stream, V, verts_cam, F, faces, vertex_colors,
                       face_colors, Ks, width, height, headlight, ambient, vis, face_uvs, face_textures, n_textures, d, tx,
                       (uint64_t)texel_count, rgb, depth, face_ids, normals);
  });
  return check_launch(fn);
}

extern "C" int mgs_rasterize_mesh_textured(int n_cams, int V, const float* vertices, const int32_t* link_ids, int L,
                                           const float* rotations, const float* translations, const float* scales,
                                           const float* viewmats, const float* Ks, int F, const int32_t* faces,
                                           const float* vertex_colors, const float* face_colors, int width, int height,
                                           float near_plane, float far_plane, int cull_backfaces, int headlight, float ambient,
                                           void* workspace, size_t workspace_bytes, float* verts_cam, float* rgb, float* depth,
                                           int32_t* face_ids, float* normals, const float* face_uvs, const int32_t* face_textures,
                                           int n_textures, const int32_t* descriptors, const void* texels, size_t texel_count,
                                           int filter, mgs_stream_t stream) {
  // every argument is checked before the first launch: the texture arguments here, the others by a refused call of the
  // untextured operator's own checks below (mgs_mesh_vertices and mgs_mesh_raster check theirs before they launch)
  const char* fn = "rasterize_mesh_textured";
  MGS_TRY(check_texture_args(fn, face_uvs, face_textures, n_textures, descriptors, texels, texel_count, filter));
  MGS_TRY(check_ambient(fn, ambient));
  MGS_TRY(check_planes(fn, near_plane, far_plane));
  MGS_TRY(check_links(fn, L, rotations, translations));
  MGS_REQUIRE(vertices && viewmats && Ks && faces, "%s: vertices, viewmats, Ks or faces is null", fn);
  MGS_REQUIRE(verts_cam && rgb && depth && face_ids, "%s: an output (verts_cam, rgb, depth, face_ids) is null", fn);
  size_t need = 0;
  MGS_TRY(mgs_mesh_workspace_bytes(n_cams, V, F, width, height, &need));     // the sizes
  MGS_TRY(check_workspace(fn, "workspace", workspace, workspace_bytes, need));
  MGS_TRY(mgs_mesh_vertices(n_cams, V, vertices, link_ids, L, rotations, translations, scales, viewmats, verts_cam, stream));
  MGS_TRY(mgs_mesh_raster(n_cams, V, verts_cam, F, faces, Ks, width, height, near_plane, far_plane, cull_backfaces, workspace,
                          workspace_bytes, stream));
  return mgs_mesh_resolve_textured(n_cams, V, verts_cam, F, faces, vertex_colors, face_colors, Ks, width, height, headlight,
                                   ambient, workspace, workspace_bytes, rgb, depth, face_ids, normals, face_uvs, face_textures,
                                   n_textures, descriptors, texels, texel_count, filter, stream);
}
