// mesh_raster.h -- the arithmetic of the triangle-mesh rasteriser (include/mgs_mesh.h, csrc/mesh.hip): everything that
// decides an index or a value, as __host__ __device__-clean inline functions.  The kernels (mesh_kernels.h, instantiated
// by mesh.hip and mesh_lens.hip) and the g++ harnesses (tests/host_harness/mesh_walk.h, which walks the same launches
// serially on heap buffers of the ABI's sizes) share this one text.  The semantics and the fp32 evaluation order are the
// statement's (tests/mesh_ref.py): adjugate rows in the edge-difference form, cx / cy not folded in, the fmas exactly
// where the statement counts them -- so contraction is switched off for this header and for what includes it: no product
// and sum is fused that is not written as fmaf here.
#ifndef MGS_MESH_RASTER_H_
#define MGS_MESH_RASTER_H_

#include <math.h>
#include <stddef.h>
#include <stdint.h>

#if defined(__clang__)
#pragma clang fp contract(off)
#endif

#ifndef MGS_MESH_HD
#define MGS_MESH_HD __host__ __device__ __forceinline__
#endif

namespace mgs {
namespace mesh {

constexpr int kBlockSide = 8;                 // a wave walks 8 x 8 pixel blocks, one pixel per lane
constexpr int kWave = 64;
constexpr int kGroup = 256;                   // threads of a workgroup of every kernel here
constexpr int kLargeBlocks = 15;              // a face whose box touches more blocks than this goes to the fixed grid
constexpr int kLargeWaves = 2048;             // waves of the fixed grid, per camera
constexpr int kMaxSide = 16368;               // 1023 tiles of 16 pixels: the image sizes the rest of the project allows
constexpr uint64_t kEmptyKey = ~0ull;         // what the clear kernel stores: above every key

struct Cam { float fx, fy, cx, cy; };

// What the walk of one face needs: the oriented planes e_i = A_i dx + B_i dy + C_i, |det| and the box in blocks.
// 16 dwords: also the record of the large-face list.
struct FaceRec {
  float A[3], B[3], C[3];
  float absdet;
  int32_t face;
  int32_t bx0, by0, nbx, nby;                 // blocks bx0 .. bx0 + nbx - 1 by by0 .. by0 + nby - 1, all inside the image's grid
  int32_t pad;
};

// ---- workspace layout: fields in this order, each on a 256-byte boundary (include/mgs_mesh.h) ---------------------------
struct Layout { size_t vis, counters, large, total; };
inline size_t align256(size_t v) { return (v + 255) / 256 * 256; }
inline size_t vis_bytes(int n_cams, int width, int height) { return 8 * (size_t)n_cams * (size_t)height * (size_t)width; }
inline size_t counter_bytes(int n_cams) { return 4 * (size_t)n_cams; }
inline size_t large_bytes(int n_cams, int F) { return sizeof(FaceRec) * (size_t)n_cams * (size_t)F; }
inline Layout workspace_layout(int n_cams, int F, int width, int height) {
  Layout l;
  l.vis = 0;
  l.counters = l.vis + align256(vis_bytes(n_cams, width, height));
  l.large = l.counters + align256(counter_bytes(n_cams));
  l.total = l.large + align256(large_bytes(n_cams, F));
  return l;
}

// ---- small helpers -------------------------------------------------------------------------------------------------------
MGS_MESH_HD bool is_finite(float x) { return fabsf(x) <= 3.4028234663852886e38f; }      // false for NaN and the infinities
MGS_MESH_HD uint32_t float_bits(float x) { uint32_t u; __builtin_memcpy(&u, &x, 4); return u; }
MGS_MESH_HD float bits_float(uint32_t u) { float x; __builtin_memcpy(&x, &u, 4); return x; }
MGS_MESH_HD bool index_ok(int32_t i, int V) { return i >= 0 && i < V; }
MGS_MESH_HD Cam load_cam(const float* K) { Cam k; k.fx = K[0]; k.fy = K[4]; k.cx = K[2]; k.cy = K[5]; return k; }

// z > 0, so the bit pattern orders as the value does; face < 2^31
MGS_MESH_HD uint64_t pack_key(float z, int32_t face) { return ((uint64_t)float_bits(z) << 32) | (uint32_t)face; }
MGS_MESH_HD float key_depth(uint64_t key) { return bits_float((uint32_t)(key >> 32)); }
MGS_MESH_HD int32_t key_face(uint64_t key) { return (int32_t)(uint32_t)key; }

// ---- indices ---------------------------------------------------------------------------------------------------------------
MGS_MESH_HD size_t vertex_index(int c, int V, int v) { return ((size_t)c * (size_t)V + (size_t)v) * 3; }
MGS_MESH_HD size_t pixel_index(int c, int width, int height, int px, int py) {
  return ((size_t)c * (size_t)height + (size_t)py) * (size_t)width + (size_t)px;
}
MGS_MESH_HD size_t large_index(int c, int F, uint32_t slot) { return (size_t)c * (size_t)F + (size_t)slot; }
MGS_MESH_HD bool large_slot_ok(uint32_t slot, int F) { return slot < (uint32_t)F; }      // the list has room for F: always true
MGS_MESH_HD int n_blocks(const FaceRec& r) { return r.nbx * r.nby; }                     // <= 2046^2 < 2^24
// Faces a wave of the face stage sets up (one per lane, lanes past it idle): as many as leave the launch at least 4096
// waves, at least 8.  A wave walks its faces one after the other, so a mesh of few faces is spread over more waves.
inline int faces_per_wave(int F) {
  for (int n = kWave; n > 8; n /= 2)
    if (((long long)F + n - 1) / n >= 4096) return n;
  return 8;
}
// the face lane `lane` of wave `wave` sets up, -1 where it has none
MGS_MESH_HD long long face_of_lane(long long wave, int per_wave, int lane, int F) {
  const long long f = wave * per_wave + lane;
  return lane < per_wave && f < F ? f : -1;
}
// q = k / n and r = k % n for 0 <= k < 2^24 and n >= 1: a float estimate (off by one at most), corrected
MGS_MESH_HD void div_mod(int k, int n, int& q, int& r) {
  q = (int)((float)k * (1.0f / (float)n));
  r = k - q * n;
  if (r < 0) { --q; r += n; }
  if (r >= n) { ++q; r -= n; }
}
// lane `lane` of the wave that walks block (bxi, byi) of the face's box: its pixel, and whether the pixel is in the image
MGS_MESH_HD bool block_pixel(const FaceRec& r, int bxi, int byi, int lane, int width, int height, int& px, int& py) {
  px = (r.bx0 + bxi) * kBlockSide + (lane & (kBlockSide - 1));
  py = (r.by0 + byi) * kBlockSide + (lane >> 3);
  return bxi >= 0 && bxi < r.nbx && byi >= 0 && byi < r.nby && px >= 0 && py >= 0 && px < width && py < height;
}
// Fixed grid: the blocks of all large faces are numbered through (offset = the blocks of the faces before, modulo the
// number of waves) and block g belongs to wave g mod n_waves: the first block of a face that wave w takes.
MGS_MESH_HD int first_block_of_wave(int offset, int w, int n_waves) { return (w + n_waves - offset) % n_waves; }
MGS_MESH_HD int next_offset(int offset, long long blocks, int n_waves) { return (int)(((long long)offset + blocks) % n_waves); }

// ---- vertex stage ------------------------------------------------------------------------------------------------------------
// x' = s R x + t for a vertex with a link in 0..L-1 (a copy otherwise), cam = V x' + t_view, in the statement's fma order.
MGS_MESH_HD void vertex_to_camera(const float x[3], int link, int L, const float* rotations, const float* translations,
                                  const float* scales, const float* viewmat, float cam[3]) {
  float xp[3] = {x[0], x[1], x[2]};
  if (link >= 0 && link < L) {
    const float* R = rotations + 9 * (size_t)link;
    const float* t = translations + 3 * (size_t)link;
    const float s = scales ? scales[link] : 1.0f;
    for (int k = 0; k < 3; ++k) {
      const float y = fmaf(R[3 * k + 2], x[2], fmaf(R[3 * k + 1], x[1], R[3 * k + 0] * x[0]));
      xp[k] = fmaf(s, y, t[k]);
    }
  }
  for (int k = 0; k < 3; ++k)
    cam[k] = fmaf(viewmat[4 * k + 2], xp[2], fmaf(viewmat[4 * k + 1], xp[1], fmaf(viewmat[4 * k + 0], xp[0], viewmat[4 * k + 3])));
}

// ---- face setup --------------------------------------------------------------------------------------------------------------
MGS_MESH_HD void cross3(const float p[3], const float d[3], float n[3]) {
  n[0] = p[1] * d[2] - p[2] * d[1];
  n[1] = p[2] * d[0] - p[0] * d[2];
  n[2] = p[0] * d[1] - p[1] * d[0];
}

// The oriented planes of a face: false where the face is dropped (non-finite, det = 0, culled).
MGS_MESH_HD bool face_planes(const float a[3], const float b[3], const float c[3], Cam k, bool cull, FaceRec& r) {
  bool finite = true;
  for (int j = 0; j < 3; ++j) finite = finite && is_finite(a[j]) && is_finite(b[j]) && is_finite(c[j]);
  const float d0[3] = {c[0] - b[0], c[1] - b[1], c[2] - b[2]};
  const float d1[3] = {a[0] - c[0], a[1] - c[1], a[2] - c[2]};
  const float d2[3] = {b[0] - a[0], b[1] - a[1], b[2] - a[2]};
  float n0[3], n1[3], n2[3];
  cross3(b, d0, n0);                                   // n_0 = b x (c - b)
  cross3(c, d1, n1);                                   // n_1 = c x (a - c)
  cross3(a, d2, n2);                                   // n_2 = a x (b - a)
  for (int j = 0; j < 3; ++j) finite = finite && is_finite(n0[j]) && is_finite(n1[j]) && is_finite(n2[j]);
  const float det = fmaf(a[2], n0[2], fmaf(a[1], n0[1], a[0] * n0[0]));
  if (!finite || !is_finite(det) || det == 0.0f) return false;
  if (cull && !(det < 0.0f)) return false;             // the normal (b - a) x (c - a) faces the camera iff det < 0
  const float s = det < 0.0f ? -1.0f : 1.0f;
  const float sfx = s / k.fx, sfy = s / k.fy;
  r.A[0] = n0[0] * sfx; r.A[1] = n1[0] * sfx; r.A[2] = n2[0] * sfx;
  r.B[0] = n0[1] * sfy; r.B[1] = n1[1] * sfy; r.B[2] = n2[1] * sfy;
  r.C[0] = s * n0[2]; r.C[1] = s * n1[2]; r.C[2] = s * n2[2];
  r.absdet = fabsf(det);
  return true;
}

struct BoxAcc { float lox, loy, hix, hiy; };
MGS_MESH_HD void box_add(BoxAcc& bx, float u, float v) {
  bx.lox = fminf(bx.lox, u); bx.hix = fmaxf(bx.hix, u);
  bx.loy = fminf(bx.loy, v); bx.hiy = fmaxf(bx.hiy, v);
}
// floor of a coordinate clamped to -10 .. limit + 10 (an infinity lands on the clamp; a NaN on -10)
MGS_MESH_HD int clamped_floor(float v, int limit) { return (int)floorf(fminf(fmaxf(v, -10.0f), (float)(limit + 10))); }

// The pixel box of a face from its projections clipped to z = near, widened by one pixel (three where the face crosses the
// near plane: the clipped points carry the error of a division by `near`) and clipped to the image; then the 8 x 8 blocks it
// touches.  False where the box misses the image.  width, height in 1 .. kMaxSide.
MGS_MESH_HD bool face_box(const float a[3], const float b[3], const float c[3], Cam k, float near_plane, int width, int height,
                          FaceRec& r) {
  const float* v[3] = {a, b, c};
  const float inf = __builtin_inff();
  BoxAcc bx = {inf, inf, -inf, -inf};
  bool crosses = false;
  for (int i = 0; i < 3; ++i) {
    const float* p = v[i];
    const float* q = v[(i + 1) % 3];
    const bool pin = p[2] >= near_plane, qin = q[2] >= near_plane;
    if (pin) box_add(bx, k.fx * p[0] / p[2] + k.cx, k.fy * p[1] / p[2] + k.cy);
    if (pin != qin) {
      crosses = true;
      const float t = (near_plane - p[2]) / (q[2] - p[2]);
      const float x = p[0] + t * (q[0] - p[0]), y = p[1] + t * (q[1] - p[1]);
      box_add(bx, k.fx * x / near_plane + k.cx, k.fy * y / near_plane + k.cy);
    }
  }
  const int widen = crosses ? 3 : 1;
  int x0 = clamped_floor(bx.lox, width - 1) - widen, x1 = clamped_floor(bx.hix, width - 1) + widen;
  int y0 = clamped_floor(bx.loy, height - 1) - widen, y1 = clamped_floor(bx.hiy, height - 1) + widen;
  x0 = x0 < 0 ? 0 : x0; y0 = y0 < 0 ? 0 : y0;
  x1 = x1 > width - 1 ? width - 1 : x1; y1 = y1 > height - 1 ? height - 1 : y1;
  if (x0 > x1 || y0 > y1) return false;
  r.bx0 = x0 / kBlockSide; r.by0 = y0 / kBlockSide;                 // 0 <= x0 <= x1 <= width - 1: inside the block grid
  r.nbx = x1 / kBlockSide - r.bx0 + 1; r.nby = y1 / kBlockSide - r.by0 + 1;
  return true;
}

// The vertex indices of face `face` and its vertices in one camera's frame.  False where an index is outside 0 .. V-1: the
// three indices are checked BEFORE any vertex is loaded.
struct FaceVerts { int32_t i0, i1, i2; float a[3], b[3], c[3]; };
MGS_MESH_HD bool load_face(const float* verts_cam_c, int V, const int32_t* faces, int face, FaceVerts& t) {
  t.i0 = faces[3 * (size_t)face + 0]; t.i1 = faces[3 * (size_t)face + 1]; t.i2 = faces[3 * (size_t)face + 2];
  if (!index_ok(t.i0, V) || !index_ok(t.i1, V) || !index_ok(t.i2, V)) return false;
  const float* pa = verts_cam_c + 3 * (size_t)t.i0;
  const float* pb = verts_cam_c + 3 * (size_t)t.i1;
  const float* pc = verts_cam_c + 3 * (size_t)t.i2;
  t.a[0] = pa[0]; t.a[1] = pa[1]; t.a[2] = pa[2];
  t.b[0] = pb[0]; t.b[1] = pb[1]; t.b[2] = pb[2];
  t.c[0] = pc[0]; t.c[1] = pc[1]; t.c[2] = pc[2];
  return true;
}

// ---- the view of one camera ----------------------------------------------------------------------------------------------
// What the raster asks of a camera (the pinhole here, a lens in mesh_lens_raster.h):
//   plane_cam()                                     the camera the planes of a face are set up under;
//   box(a, b, c, near, cam_index, width, height, r) the blocks of a face's box into r, false where it has none;
//   ray(at, px, py, dx, dy)                         (dx, dy), the first two components of the ray of pixel (px, py) (index
//                                                   `at`) in the units of the planes, false where the pixel has no ray.
// The pinhole's ray is (px + 0.5 - cx, py + 0.5 - cy) with planes set up under K.  The views of all cameras of a call
// (PinholeViews: the K matrices) give camera(c).  They travel to a kernel as their three pointers p0(), p1(), p2() (types
// P0, P1, P2; void and null where a view has fewer), which the kernel declares __restrict__ and puts together again with
// from(): inside a by-value struct the pointers lose the qualifier, and the kernels are then not the ones they were
// (profiles/mesh_refactor/README.md).
struct PinholeView {
  Cam k;
  MGS_MESH_HD Cam plane_cam() const { return k; }
  MGS_MESH_HD bool box(const float a[3], const float b[3], const float c[3], float near_plane, int, int width, int height,
                       FaceRec& r) const {
    return face_box(a, b, c, k, near_plane, width, height, r);
  }
  MGS_MESH_HD bool ray(size_t, int px, int py, float& dx, float& dy) const {
    dx = ((float)px + 0.5f) - k.cx;
    dy = ((float)py + 0.5f) - k.cy;
    return true;
  }
};
struct PinholeViews {
  const float* Ks;                            // [C,3,3]
  MGS_MESH_HD PinholeView camera(int c) const { PinholeView v; v.k = load_cam(Ks + 9 * (size_t)c); return v; }
  using P0 = float;
  using P1 = void;
  using P2 = void;
  const P0* p0() const { return Ks; }
  const P1* p1() const { return nullptr; }
  const P2* p2() const { return nullptr; }
  MGS_MESH_HD static PinholeViews from(const P0* Ks, const P1*, const P2*) { PinholeViews v; v.Ks = Ks; return v; }
};

// The whole setup of face `face` of camera `cam_index`, whose vertices are verts_cam_c.
template <class View>
MGS_MESH_HD bool face_setup(const View& view, const float* verts_cam_c, int V, const int32_t* faces, int face, float near_plane,
                            int cam_index, int width, int height, bool cull, FaceRec& r) {
  FaceVerts t;
  if (!load_face(verts_cam_c, V, faces, face, t)) return false;
  r.face = face;
  r.pad = 0;
  return face_planes(t.a, t.b, t.c, view.plane_cam(), cull, r) && view.box(t.a, t.b, t.c, near_plane, cam_index, width, height, r);
}

// ---- per pixel ---------------------------------------------------------------------------------------------------------------
// The pixel enters only through (dx, dy), its view's ray.  e_i and S there; true where the pixel is inside (e_i >= 0,
// inclusive, and S > 0).
MGS_MESH_HD bool pixel_edges_at(const FaceRec& r, float dx, float dy, float e[3], float& S) {
  for (int i = 0; i < 3; ++i) e[i] = fmaf(r.A[i], dx, fmaf(r.B[i], dy, r.C[i]));
  S = (e[0] + e[1]) + e[2];
  return e[0] >= 0.0f && e[1] >= 0.0f && e[2] >= 0.0f && S > 0.0f;
}
// the key of the face at (dx, dy); false where it does not count there
MGS_MESH_HD bool pixel_key_at(const FaceRec& r, float dx, float dy, float near_plane, float far_plane, uint64_t& key) {
  float e[3], S;
  if (!pixel_edges_at(r, dx, dy, e, S)) return false;
  const float z = r.absdet / S;
  if (!(z >= near_plane && z <= far_plane)) return false;
  key = pack_key(z, r.face);
  return true;
}
// the key of the face at pixel (px, py) (index `at`) of a view; a pixel without a ray is never inside
template <class View>
MGS_MESH_HD bool pixel_key(const View& view, const FaceRec& r, size_t at, int px, int py, float near_plane, float far_plane,
                           uint64_t& key) {
  float dx, dy;
  return view.ray(at, px, py, dx, dy) && pixel_key_at(r, dx, dy, near_plane, far_plane, key);
}

// ---- resolve -----------------------------------------------------------------------------------------------------------------
// From the winning key of a pixel: depth, face id, colour from the barycentrics recomputed in the raster's order (vertex
// colours, face colours or 0.7 grey, optionally times the headlight shade) and the unit normal turned toward the camera.
// Everything 0 and the id -1 where the pixel is uncovered (or the key names no valid face: never after the raster).  In
// three stages; the textured resolve (mesh_texture.h) writes out the first two and shares the third.
struct Shaded { float rgb[3], depth, normal[3]; int32_t face; };
MGS_MESH_HD void store_shaded(const Shaded& s, size_t at, float* rgb, float* depth, int32_t* face_ids, float* normals) {
  rgb[3 * at + 0] = s.rgb[0]; rgb[3 * at + 1] = s.rgb[1]; rgb[3 * at + 2] = s.rgb[2];
  depth[at] = s.depth;
  face_ids[at] = s.face;
  if (normals) { normals[3 * at + 0] = s.normal[0]; normals[3 * at + 1] = s.normal[1]; normals[3 * at + 2] = s.normal[2]; }
}

// the face that covers a pixel: its vertices, its planes under k, S and the barycentrics at the pixel's ray
struct Covered { FaceVerts t; FaceRec r; float S, l0, l1, l2; };

// Stage 2: vertex colours, face colours, or 0.7 grey
MGS_MESH_HD void base_colour(const Covered& cv, const float* vertex_colors, const float* face_colors, float rgb[3]) {
  if (vertex_colors) {
    const float* c0 = vertex_colors + 3 * (size_t)cv.t.i0;
    const float* c1 = vertex_colors + 3 * (size_t)cv.t.i1;
    const float* c2 = vertex_colors + 3 * (size_t)cv.t.i2;
    for (int j = 0; j < 3; ++j) rgb[j] = fmaf(cv.l2, c2[j], fmaf(cv.l1, c1[j], cv.l0 * c0[j]));
  } else if (face_colors) {
    for (int j = 0; j < 3; ++j) rgb[j] = face_colors[3 * (size_t)cv.r.face + j];
  } else {
    rgb[0] = rgb[1] = rgb[2] = 0.7f;
  }
}

// Stage 3: n = (b - a) x (c - a), normalised; the ray through the pixel, normalised; cos between them
MGS_MESH_HD void normal_and_shade(const float a[3], const float b[3], const float c[3], Cam k, float dx, float dy, bool headlight,
                                  float ambient, Shaded& o) {
  const float u[3] = {b[0] - a[0], b[1] - a[1], b[2] - a[2]}, w[3] = {c[0] - a[0], c[1] - a[1], c[2] - a[2]};
  float n[3];
  n[0] = u[1] * w[2] - u[2] * w[1]; n[1] = u[2] * w[0] - u[0] * w[2]; n[2] = u[0] * w[1] - u[1] * w[0];
  const float n2 = fmaf(n[2], n[2], fmaf(n[1], n[1], n[0] * n[0]));
  const float ninv = n2 > 0.0f ? 1.0f / sqrtf(n2) : 0.0f;
  const float nh[3] = {n[0] * ninv, n[1] * ninv, n[2] * ninv};
  const float rx = dx / k.fx, ry = dy / k.fy;
  const float rinv = 1.0f / sqrtf(fmaf(ry, ry, fmaf(rx, rx, 1.0f)));
  const float cosv = fmaf(nh[2], rinv, fmaf(nh[1], ry * rinv, nh[0] * (rx * rinv)));
  const float flip = cosv > 0.0f ? -1.0f : 1.0f;
  for (int j = 0; j < 3; ++j) o.normal[j] = flip * nh[j];
  if (headlight) {
    const float shade = fmaf(1.0f - ambient, fabsf(cosv), ambient);
    for (int j = 0; j < 3; ++j) o.rgb[j] *= shade;
  }
}

// The resolve of the pixel at (dx, dy) (k: the camera the planes are set up under).  Stage 1, the covered face: key decode,
// index check, vertex loads, planes, e, S, barycentrics, with the uncovered pixel returned from where it is found.  Stage 2,
// base_colour.  Stage 3, normal_and_shade.  Stage 1 is written here and not as a function that returns a flag: behind a
// flag the early returns meet in one block and the compiler repeats three subtractions (profiles/mesh_refactor/README.md).
MGS_MESH_HD Shaded resolve_pixel_at(uint64_t key, const float* verts_cam_c, int V, const int32_t* faces, int F,
                                    const float* vertex_colors, const float* face_colors, Cam k, float dx, float dy,
                                    bool headlight, float ambient) {
  Shaded o;
  o.rgb[0] = o.rgb[1] = o.rgb[2] = 0.0f; o.depth = 0.0f; o.normal[0] = o.normal[1] = o.normal[2] = 0.0f; o.face = -1;
  if (key == kEmptyKey) return o;
  const int32_t f = key_face(key);
  if (f < 0 || f >= F) return o;
  Covered cv;
  if (!load_face(verts_cam_c, V, faces, f, cv.t)) return o;
  cv.r.face = f;
  if (!face_planes(cv.t.a, cv.t.b, cv.t.c, k, false, cv.r)) return o;
  float e[3];
  pixel_edges_at(cv.r, dx, dy, e, cv.S);
  o.face = f;
  o.depth = key_depth(key);
  cv.l0 = e[0] / cv.S; cv.l1 = e[1] / cv.S; cv.l2 = e[2] / cv.S;
  base_colour(cv, vertex_colors, face_colors, o.rgb);
  normal_and_shade(cv.t.a, cv.t.b, cv.t.c, k, dx, dy, headlight, ambient, o);
  return o;
}

// the pixel (px, py) (index `at`) of a view; a pixel without a ray is uncovered
template <class View>
MGS_MESH_HD Shaded resolve_pixel(const View& view, uint64_t key, const float* verts_cam_c, int V, const int32_t* faces, int F,
                                 const float* vertex_colors, const float* face_colors, size_t at, int px, int py, bool headlight,
                                 float ambient) {
  float dx, dy;
  const bool has = view.ray(at, px, py, dx, dy);
  return resolve_pixel_at(has ? key : kEmptyKey, verts_cam_c, V, faces, F, vertex_colors, face_colors, view.plane_cam(), dx, dy,
                          headlight, ambient);
}

// The pinhole's setup, key and resolve by their earlier names, for callers that hold a Cam and no view
MGS_MESH_HD bool face_setup(const float* verts_cam_c, int V, const int32_t* faces, int face, Cam k, float near_plane, int width,
                            int height, bool cull, FaceRec& r) {
  const PinholeView view = {k};
  return face_setup(view, verts_cam_c, V, faces, face, near_plane, 0, width, height, cull, r);
}
MGS_MESH_HD bool pixel_key(const FaceRec& r, Cam k, int px, int py, float near_plane, float far_plane, uint64_t& key) {
  const PinholeView view = {k};
  return pixel_key(view, r, 0, px, py, near_plane, far_plane, key);
}
MGS_MESH_HD Shaded resolve_pixel(uint64_t key, const float* verts_cam_c, int V, const int32_t* faces, int F,
                                 const float* vertex_colors, const float* face_colors, Cam k, int px, int py, bool headlight,
                                 float ambient) {
  const PinholeView view = {k};
  return resolve_pixel(view, key, verts_cam_c, V, faces, F, vertex_colors, face_colors, 0, px, py, headlight, ambient);
}

}  // namespace mesh
}  // namespace mgs
#endif  // MGS_MESH_RASTER_H_
