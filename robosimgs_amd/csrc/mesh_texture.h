// mesh_texture.h -- the arithmetic of textured meshes (include/mgs_mesh_texture.h, csrc/mesh_texture.hip): the texture
// layout, the mip box filter, wrap, bilinear / trilinear sampling, the analytic level of detail and the textured shading of
// a pixel, as __host__ __device__-clean inline functions beside mesh_raster.h's.  mesh_texture.hip's kernels and the g++
// harness (tests/host_harness/mesh_texture_harness.cpp) share this one text.  The semantics and the fp32 evaluation order
// are the statement's (tests/texture_ref.py); contraction is off, as in mesh_raster.h: every fma is written out.
#ifndef MGS_MESH_TEXTURE_H_
#define MGS_MESH_TEXTURE_H_

#include "mesh_raster.h"

#if defined(__clang__)
#pragma clang fp contract(off)
#endif

namespace mgs {
namespace mesh {

constexpr int kTexMaxSide = 16384;            // a level-0 side: 1 .. 2^14, so at most 15 levels
constexpr int kTexMaxLevels = 15;
constexpr int kTexMaxTextures = 4096;
constexpr int kTexDescWords = 20;
constexpr int kWrapRepeat = 0, kWrapClamp = 1, kWrapMirror = 2;
constexpr int kFilterBilinear = 0, kFilterTrilinear = 1;

// One texture of a set: 20 int32 words.  offset[l] is the index, in texels from the start of the set's texel array, of
// level l's first texel (row-major, row 0 at the top); levels follow each other without gaps, textures likewise.
struct TexDesc {
  int32_t w, h, levels;
  int32_t wrap;                               // wrap_s | wrap_t << 8
  uint32_t offset[16];                        // entries past `levels` are 0
};

MGS_MESH_HD int level_side(int side, int l) { const int s = side >> l; return s < 1 ? 1 : s; }
inline int level_count(int w, int h) {
  int m = w > h ? w : h, n = 1;
  while (m > 1) { m >>= 1; ++n; }
  return n;
}
inline bool wrap_ok(int m) { return m == kWrapRepeat || m == kWrapClamp || m == kWrapMirror; }

// Fill descs[0 .. T-1] from sizes [T,2] = (w, h) and wraps [T,2] = (wrap_s, wrap_t) (null: repeat) and return the texels of
// all levels of all textures; 0 where a size or a wrap mode is out of range or the total reaches 2^31.
inline uint64_t texture_layout(int T, const int32_t* sizes, const int32_t* wraps, TexDesc* descs) {
  uint64_t at = 0;
  for (int t = 0; t < T; ++t) {
    const int w = sizes[2 * t], h = sizes[2 * t + 1];
    const int ws = wraps ? wraps[2 * t] : kWrapRepeat, wt = wraps ? wraps[2 * t + 1] : kWrapRepeat;
    if (w < 1 || w > kTexMaxSide || h < 1 || h > kTexMaxSide || !wrap_ok(ws) || !wrap_ok(wt)) return 0;
    TexDesc d;
    d.w = w; d.h = h; d.levels = level_count(w, h); d.wrap = ws | (wt << 8);
    for (int l = 0; l < 16; ++l) d.offset[l] = 0u;
    for (int l = 0; l < d.levels; ++l) {
      d.offset[l] = (uint32_t)at;
      at += (uint64_t)level_side(w, l) * (uint64_t)level_side(h, l);
      if (at >= (1ull << 31)) return 0;
    }
    if (descs) descs[t] = d;
  }
  return at;
}

// ---- mip chain: texel (x, y) of a level from the level below (sw x sh), per byte (s00 + s01 + s10 + s11 + 2) >> 2 -------
MGS_MESH_HD uint32_t mip_texel(const uint32_t* src, int sw, int sh, int x, int y) {
  const int x0 = 2 * x < sw - 1 ? 2 * x : sw - 1, x1 = 2 * x + 1 < sw - 1 ? 2 * x + 1 : sw - 1;
  const int y0 = 2 * y < sh - 1 ? 2 * y : sh - 1, y1 = 2 * y + 1 < sh - 1 ? 2 * y + 1 : sh - 1;
  const uint32_t a = src[(size_t)y0 * (size_t)sw + (size_t)x0], b = src[(size_t)y0 * (size_t)sw + (size_t)x1];
  const uint32_t c = src[(size_t)y1 * (size_t)sw + (size_t)x0], d = src[(size_t)y1 * (size_t)sw + (size_t)x1];
  // bytes 0 and 2 in one word, 1 and 3 in the other: a sum of four bytes plus 2 stays below 2^16
  const uint32_t even = (a & 0x00FF00FFu) + (b & 0x00FF00FFu) + (c & 0x00FF00FFu) + (d & 0x00FF00FFu) + 0x00020002u;
  const uint32_t odd = ((a >> 8) & 0x00FF00FFu) + ((b >> 8) & 0x00FF00FFu) + ((c >> 8) & 0x00FF00FFu) +
                       ((d >> 8) & 0x00FF00FFu) + 0x00020002u;
  return ((even >> 2) & 0x00FF00FFu) | (((odd >> 2) & 0x00FF00FFu) << 8);
}

// ---- sampling ------------------------------------------------------------------------------------------------------------
// A finite coordinate into 0 .. 1 by the wrap mode; no integer conversion here, so any finite value may come in.
MGS_MESH_HD float wrap_coord(float u, int mode) {
  if (mode == kWrapClamp) return fminf(fmaxf(u, 0.0f), 1.0f);
  if (mode == kWrapMirror) {
    const float t = fmaf(-2.0f, floorf(u * 0.5f), u);
    return 1.0f - fabsf(t - 1.0f);
  }
  return u - floorf(u);
}
// The two texel columns (or rows) around wrapped coordinate u01 of a level `side` wide and the weight of the second.
// u01 is in 0 .. 1 (a value outside, which no wrap mode produces, is clamped first), so x is in -0.5 .. side - 0.5.
MGS_MESH_HD void texel_pair(float u01, int side, int mode, int& i0, int& i1, float& f) {
  const float x = fmaf(fminf(fmaxf(u01, 0.0f), 1.0f), (float)side, -0.5f);
  const float fl = floorf(x);
  f = x - fl;
  i0 = (int)fl;
  i1 = i0 + 1;
  if (mode == kWrapRepeat) {
    if (i0 < 0) i0 += side;
    if (i1 >= side) i1 -= side;
  }
  i0 = i0 < 0 ? 0 : (i0 > side - 1 ? side - 1 : i0);
  i1 = i1 < 0 ? 0 : (i1 > side - 1 ? side - 1 : i1);
}
MGS_MESH_HD float texel_byte(uint32_t t, int j) { return (float)((t >> (8 * j)) & 0xFFu); }

// Bilinear sample of level l of texture d at wrapped (u01, v01), in byte units 0 .. 255.  Four 4-byte loads; every index is
// inside the level by texel_pair, the level inside 0 .. 15, and the sum is held below texel_count.
MGS_MESH_HD void sample_level(const TexDesc* d, const uint32_t* texels, uint64_t texel_count, int l, float u01, float v01,
                              float out[3]) {
  l = l < 0 ? 0 : (l > kTexMaxLevels - 1 ? kTexMaxLevels - 1 : l);
  const int w = level_side(d->w, l), h = level_side(d->h, l);
  const int ws = d->wrap & 0xFF, wt = (d->wrap >> 8) & 0xFF;
  int x0, x1, y0, y1;
  float fx, fy;
  texel_pair(u01, w, ws, x0, x1, fx);
  texel_pair(v01, h, wt, y0, y1, fy);
  const uint64_t base = (uint64_t)d->offset[l], last = texel_count - 1;
  uint64_t i00 = base + (uint64_t)y0 * (uint64_t)w + (uint64_t)x0, i01 = base + (uint64_t)y0 * (uint64_t)w + (uint64_t)x1;
  uint64_t i10 = base + (uint64_t)y1 * (uint64_t)w + (uint64_t)x0, i11 = base + (uint64_t)y1 * (uint64_t)w + (uint64_t)x1;
  i00 = i00 > last ? last : i00; i01 = i01 > last ? last : i01; i10 = i10 > last ? last : i10; i11 = i11 > last ? last : i11;
  const uint32_t t00 = texels[i00], t01 = texels[i01], t10 = texels[i10], t11 = texels[i11];
  for (int j = 0; j < 3; ++j) {
    const float a = texel_byte(t00, j), b = texel_byte(t01, j), c = texel_byte(t10, j), e = texel_byte(t11, j);
    const float top = fmaf(fx, b - a, a), bot = fmaf(fx, e - c, c);
    out[j] = fmaf(fy, bot - top, top);
  }
}

// The level of detail from the analytic derivatives of (u, v) by the pixel: 0 where rho <= 1 or rho is a NaN.
MGS_MESH_HD float level_of_detail(float dudx, float dvdx, float dudy, float dvdy, int w, int h, int levels) {
  const float ax = (float)w * dudx, bx = (float)h * dvdx, ay = (float)w * dudy, by = (float)h * dvdy;
  const float rho2 = fmaxf(fmaf(bx, bx, ax * ax), fmaf(by, by, ay * ay));
  if (!(rho2 > 1.0f)) return 0.0f;
  return fminf(0.5f * log2f(rho2), (float)(levels - 1));
}

// The texture id of face f, or -1 where it has none (checked before any descriptor is read).
MGS_MESH_HD int32_t face_texture(const int32_t* face_textures, int32_t f, int T) {
  const int32_t t = face_textures[f];
  return t >= 0 && t < T ? t : -1;
}
// The texture id of the face that won pixel `key`, -1 where the pixel is uncovered, the key names no face or the face
// has no texture: what a wave compares before it chooses how to read the descriptors.
MGS_MESH_HD int32_t key_texture(uint64_t key, const int32_t* face_textures, int F, int T) {
  if (key == kEmptyKey) return -1;
  const int32_t f = key_face(key);
  if (f < 0 || f >= F) return -1;
  return face_texture(face_textures, f, T);
}

// resolve_pixel under the pinhole with a texture between the tint and the shade: the statements of mesh_raster.h's
// resolve_pixel_at in the same order, so that a pixel whose face has no texture (textured false), or whose uv or
// (trilinear) uv derivatives are not finite, gets resolve_pixel's bits.  Stages 1 and 2 are written out here and only
// stage 3 (normal_and_shade) is shared: as resolve_pixel_at with the texture block as its callable the same arithmetic
// compiled to another control flow, and the trilinear kernel measured 1.1 us slower at 1080p
// (profiles/mesh_refactor/README.md); this text compiles to the kernel it was.  textured, tex: whether key_texture gave
// the pixel a texture, and that texture's descriptor (read only if textured: a separate flag, so that a wave whose
// pixels agree can pass one wave-uniform pointer).
MGS_MESH_HD Shaded resolve_pixel_textured(uint64_t key, const float* verts_cam_c, int V, const int32_t* faces, int F,
                                          const float* vertex_colors, const float* face_colors, Cam k, int px, int py,
                                          bool headlight, float ambient, const float* face_uvs, bool textured,
                                          const TexDesc* tex, const uint32_t* texels, uint64_t texel_count, int filter) {
  Shaded o;
  o.rgb[0] = o.rgb[1] = o.rgb[2] = 0.0f; o.depth = 0.0f; o.normal[0] = o.normal[1] = o.normal[2] = 0.0f; o.face = -1;
  if (key == kEmptyKey) return o;
  const int32_t f = key_face(key);
  if (f < 0 || f >= F) return o;
  const int32_t i0 = faces[3 * (size_t)f + 0], i1 = faces[3 * (size_t)f + 1], i2 = faces[3 * (size_t)f + 2];
  if (!index_ok(i0, V) || !index_ok(i1, V) || !index_ok(i2, V)) return o;
  const float* pa = verts_cam_c + 3 * (size_t)i0;
  const float* pb = verts_cam_c + 3 * (size_t)i1;
  const float* pc = verts_cam_c + 3 * (size_t)i2;
  const float a[3] = {pa[0], pa[1], pa[2]}, b[3] = {pb[0], pb[1], pb[2]}, c[3] = {pc[0], pc[1], pc[2]};
  FaceRec r;
  r.face = f;
  if (!face_planes(a, b, c, k, false, r)) return o;
  float e[3], S;
  const float dx = ((float)px + 0.5f) - k.cx, dy = ((float)py + 0.5f) - k.cy;
  pixel_edges_at(r, dx, dy, e, S);
  o.face = f;
  o.depth = key_depth(key);
  const float l0 = e[0] / S, l1 = e[1] / S, l2 = e[2] / S;
  if (vertex_colors) {
    const float* c0 = vertex_colors + 3 * (size_t)i0;
    const float* c1 = vertex_colors + 3 * (size_t)i1;
    const float* c2 = vertex_colors + 3 * (size_t)i2;
    for (int j = 0; j < 3; ++j) o.rgb[j] = fmaf(l2, c2[j], fmaf(l1, c1[j], l0 * c0[j]));
  } else if (face_colors) {
    for (int j = 0; j < 3; ++j) o.rgb[j] = face_colors[3 * (size_t)f + j];
  } else if (!textured) {
    o.rgb[0] = o.rgb[1] = o.rgb[2] = 0.7f;
  } else {
    o.rgb[0] = o.rgb[1] = o.rgb[2] = 1.0f;               // the tint of a textured face without colours
  }
  if (textured) {
    const float* uv = face_uvs + 6 * (size_t)f;          // read only now: the pixel is covered and its face textured
    const float u0 = uv[0], v0 = uv[1], u1 = uv[2], v1 = uv[3], u2 = uv[4], v2 = uv[5];
    const float u = fmaf(l2, u2, fmaf(l1, u1, l0 * u0)), v = fmaf(l2, v2, fmaf(l1, v1, l0 * v0));
    bool ok = is_finite(u) && is_finite(v);
    float lod = 0.0f;
    const int levels = tex->levels < 1 ? 1 : (tex->levels > kTexMaxLevels ? kTexMaxLevels : tex->levels);
    if (ok && filter == kFilterTrilinear) {
      const float sA = (r.A[0] + r.A[1]) + r.A[2], sB = (r.B[0] + r.B[1]) + r.B[2];
      const float uA = fmaf(u2, r.A[2], fmaf(u1, r.A[1], u0 * r.A[0])), uB = fmaf(u2, r.B[2], fmaf(u1, r.B[1], u0 * r.B[0]));
      const float vA = fmaf(v2, r.A[2], fmaf(v1, r.A[1], v0 * r.A[0])), vB = fmaf(v2, r.B[2], fmaf(v1, r.B[1], v0 * r.B[0]));
      const float dudx = fmaf(-u, sA, uA) / S, dudy = fmaf(-u, sB, uB) / S;
      const float dvdx = fmaf(-v, sA, vA) / S, dvdy = fmaf(-v, sB, vB) / S;
      ok = is_finite(dudx) && is_finite(dudy) && is_finite(dvdx) && is_finite(dvdy);
      if (ok) lod = level_of_detail(dudx, dvdx, dudy, dvdy, tex->w, tex->h, levels);
    }
    if (ok) {
      const float uw = wrap_coord(u, tex->wrap & 0xFF), vw = wrap_coord(v, (tex->wrap >> 8) & 0xFF);
      const float lf = floorf(lod);                      // lod is in 0 .. levels - 1 <= 14
      const int la = (int)lf, lb = la + 1 < levels - 1 ? la + 1 : levels - 1;
      const float wgt = lod - lf;
      float ca[3];
      sample_level(tex, texels, texel_count, la, uw, vw, ca);
      if (wgt > 0.0f) {                                  // weight 0 returns ca's bits: the second level is not fetched
        float cb[3];
        sample_level(tex, texels, texel_count, lb, uw, vw, cb);
        for (int j = 0; j < 3; ++j) ca[j] = fmaf(wgt, cb[j] - ca[j], ca[j]);
      }
      for (int j = 0; j < 3; ++j) o.rgb[j] = (ca[j] * (1.0f / 255.0f)) * o.rgb[j];
    } else if (!vertex_colors && !face_colors) {
      o.rgb[0] = o.rgb[1] = o.rgb[2] = 0.7f;             // shaded untextured: resolve_pixel's grey
    }
  }
  normal_and_shade(a, b, c, k, dx, dy, headlight, ambient, o);
  return o;
}

}  // namespace mesh
}  // namespace mgs
#endif  // MGS_MESH_TEXTURE_H_
