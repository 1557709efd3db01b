// mesh_lens_raster.h -- the arithmetic of the mesh rasteriser under a lens (include/mgs_mesh_lens.h, csrc/mesh_lens.hip):
// the per-pixel ray map (the inverse of the lens), its block tables and the face's box in ray space, as __host__
// __device__-clean inline functions over mesh_raster.h, and LensView, the view through which mesh_raster.h's face setup,
// key and resolve and mesh_kernels.h's kernels see a camera under a lens.  mesh_lens.hip and the g++ harness
// (tests/host_harness/mesh_lens_harness.cpp) share this one text; the statement is tests/mesh_lens_ref.py.
//
// The raster is homogeneous: the pixel enters the edge test only through its ray.  Under a lens the triangle is unchanged
// and a pixel's ray is (x_u, y_u, 1) with (x_u, y_u) the preimage of the pixel's distorted normalised point d under the
// distortion map.  So the planes are mesh_raster.h's, set up under Cam{1, 1, 0, 0} (s / 1 is exact), and the walk is
// pixel_edges_at at (x_u, y_u): LensView below.
//
// Roundings (U = 2^-24) of one evaluation of the forward map, on its absolute value |D|(q) (every coefficient and
// coordinate replaced by its modulus), in the order written below:
//   pinhole lens  u = fma(a, a, b b): 2; the cubic term k3 u^3 carries 3 x 2 from u and 3 Horner fmas; the product with a
//                 inside the outer fma: 1 -- 10 in all; every other term carries fewer.
//   fisheye       u = theta theta: 1; k4 u^4 carries 4 from u and 4 Horner fmas; the product with theta: 1 -- 9.
// kEvalRoundings = 10 covers both.  A ray is accepted where the fp32 residual max|D(q) - d| is within kResidualFactor x
// that bound: the last Newton step cannot do better than one evaluation's error and the factor covers the update's rounding.
#ifndef MGS_MESH_LENS_RASTER_H_
#define MGS_MESH_LENS_RASTER_H_

#include "mesh_raster.h"

#if defined(__clang__)
#pragma clang fp contract(off)
#endif

namespace mgs {
namespace mesh {

constexpr int kModelFisheyeKb = 3;            // MGS_CAMERA_FISHEYE_KB
constexpr int kModelPinholeBc = 4;            // MGS_CAMERA_PINHOLE_BC
constexpr int kLensRowFloats = 16;            // MGS_LENS_ROW_FLOATS
constexpr int kNewtonSteps = 12;
constexpr int kSuperSide = 8;                 // a superblock is 8 x 8 blocks: 64 x 64 pixels
constexpr float kUnit = 5.9604644775390625e-8f;   // 2^-24
constexpr float kEvalRoundings = 10.0f;
constexpr float kResidualFactor = 2.0f;

struct Ray { float x, y; };                   // (x_u, y_u); both NaN where the pixel has no ray
struct Rect { float x0, y0, x1, y1; };        // min x_u, min y_u, max x_u, max y_u; empty: (+inf, +inf, -inf, -inf)

MGS_MESH_HD Ray no_ray() { Ray r; r.x = r.y = __builtin_nanf(""); return r; }
MGS_MESH_HD bool has_ray(Ray r) { return r.x == r.x && r.y == r.y; }
MGS_MESH_HD Rect empty_rect() { const float inf = __builtin_inff(); Rect r = {inf, inf, -inf, -inf}; return r; }
MGS_MESH_HD bool rect_empty(Rect r) { return !(r.x0 <= r.x1 && r.y0 <= r.y1); }
MGS_MESH_HD void rect_add(Rect& r, Ray q) {
  r.x0 = fminf(r.x0, q.x); r.x1 = fmaxf(r.x1, q.x);
  r.y0 = fminf(r.y0, q.y); r.y1 = fmaxf(r.y1, q.y);
}
MGS_MESH_HD void rect_join(Rect& r, Rect o) {
  r.x0 = fminf(r.x0, o.x0); r.x1 = fmaxf(r.x1, o.x1);
  r.y0 = fminf(r.y0, o.y0); r.y1 = fmaxf(r.y1, o.y1);
}
// closed rectangles; false where either is empty
MGS_MESH_HD bool rect_overlap(Rect a, Rect b) { return a.x0 <= b.x1 && b.x0 <= a.x1 && a.y0 <= b.y1 && b.y0 <= a.y1; }

// ---- lens workspace layout: fields in this order, each on a 256-byte boundary (include/mgs_mesh_lens.h) -----------------
MGS_MESH_HD int blocks_of(int side) { return (side + kBlockSide - 1) / kBlockSide; }
MGS_MESH_HD int supers_of(int side) { return (blocks_of(side) + kSuperSide - 1) / kSuperSide; }
struct LensLayout { size_t rays, blocks, supers, total; };
inline size_t ray_bytes(int n_cams, int width, int height) { return sizeof(Ray) * (size_t)n_cams * (size_t)height * (size_t)width; }
inline size_t block_rect_bytes(int n_cams, int width, int height) {
  return sizeof(Rect) * (size_t)n_cams * (size_t)blocks_of(height) * (size_t)blocks_of(width);
}
inline size_t super_rect_bytes(int n_cams, int width, int height) {
  return sizeof(Rect) * (size_t)n_cams * (size_t)supers_of(height) * (size_t)supers_of(width);
}
inline LensLayout lens_layout(int n_cams, int width, int height) {
  LensLayout l;
  l.rays = 0;
  l.blocks = l.rays + align256(ray_bytes(n_cams, width, height));
  l.supers = l.blocks + align256(block_rect_bytes(n_cams, width, height));
  l.total = l.supers + align256(super_rect_bytes(n_cams, width, height));
  return l;
}
MGS_MESH_HD size_t rect_index(int c, int nx, int ny, int x, int y) { return ((size_t)c * (size_t)ny + (size_t)y) * (size_t)nx + (size_t)x; }

// ---- the forward maps, as the lens headers state them -----------------------------------------------------------------------
// include/mgs_lens_pinhole.h: (xd, yd) = D(a, b) with Jd = [[j00, j01], [j01, j11]], u = a^2 + b^2, and the bound of one
// fp32 evaluation of (xd, yd) in this order
struct Distorted { float xd, yd, j00, j01, j11, u, bound; };
MGS_MESH_HD Distorted distort_bc(const float* k, float a, float b) {
  const float k1 = k[0], k2 = k[1], p1 = k[2], p2 = k[3], k3 = k[4];
  Distorted o;
  const float aa = a * a, bb = b * b, ab = a * b;
  o.u = fmaf(a, a, bb);
  const float rad = fmaf(o.u, fmaf(o.u, fmaf(o.u, k3, k2), k1), 1.0f);
  const float rad1 = fmaf(o.u, fmaf(o.u, 3.0f * k3, 2.0f * k2), k1);
  o.xd = fmaf(a, rad, fmaf(2.0f * p1, ab, p2 * fmaf(2.0f, aa, o.u)));
  o.yd = fmaf(b, rad, fmaf(p1, fmaf(2.0f, bb, o.u), (2.0f * p2) * ab));
  o.j00 = fmaf(2.0f * aa, rad1, rad) + fmaf(2.0f * p1, b, (6.0f * p2) * a);
  o.j01 = fmaf(2.0f * ab, rad1, fmaf(2.0f * p1, a, (2.0f * p2) * b));
  o.j11 = fmaf(2.0f * bb, rad1, rad) + fmaf(6.0f * p1, b, (2.0f * p2) * a);
  const float rad_abs = fmaf(o.u, fmaf(o.u, fmaf(o.u, fabsf(k3), fabsf(k2)), fabsf(k1)), 1.0f);
  const float xa = fmaf(fabsf(a), rad_abs, fmaf(2.0f * fabsf(p1), fabsf(ab), fabsf(p2) * fmaf(2.0f, aa, o.u)));
  const float ya = fmaf(fabsf(b), rad_abs, fmaf(fabsf(p1), fmaf(2.0f, bb, o.u), (2.0f * fabsf(p2)) * fabsf(ab)));
  o.bound = (kEvalRoundings * kUnit) * fmaxf(xa, ya);
  return o;
}

// include/mgs.h MGS_CAMERA_FISHEYE_KB: theta_d = theta P(theta^2), its derivative P + 2 u P', and the bound of one fp32
// evaluation of theta_d in this order
struct Radial { float td, deriv, bound; };
MGS_MESH_HD Radial distort_kb(const float* k, float theta) {
  const float k1 = k[0], k2 = k[1], k3 = k[2], k4 = k[3];
  Radial o;
  const float u = theta * theta;
  const float P = fmaf(u, fmaf(u, fmaf(u, fmaf(u, k4, k3), k2), k1), 1.0f);
  o.td = theta * P;
  o.deriv = fmaf(u, fmaf(u, fmaf(u, fmaf(u, 9.0f * k4, 7.0f * k3), 5.0f * k2), 3.0f * k1), 1.0f);
  const float Pa = fmaf(u, fmaf(u, fmaf(u, fmaf(u, fabsf(k4), fabsf(k3)), fabsf(k2)), fabsf(k1)), 1.0f);
  o.bound = (kEvalRoundings * kUnit) * (fabsf(theta) * Pa);
  return o;
}

// ---- the ray of a pixel ----------------------------------------------------------------------------------------------------
// d = ((px + 0.5 - cx) / fx, (py + 0.5 - cy) / fy), the pixel's distorted normalised point
MGS_MESH_HD void pixel_distorted(const float* row, int px, int py, float& dx, float& dy) {
  dx = (((float)px + 0.5f) - row[2]) / row[0];
  dy = (((float)py + 0.5f) - row[5]) / row[4];
}

// MGS_CAMERA_PINHOLE_BC: Newton on D(q) = d from q = d, kNewtonSteps steps.  Valid iff at the final q: u < u_max, det Jd > 0
// and the residual is inside the threshold (every comparison is false for a NaN: a diverged solve has no ray).
MGS_MESH_HD Ray ray_bc(const float* row, float dx, float dy) {
  const float* k = row + 9;
  const float u_max = row[14];
  float a = dx, b = dy;
  for (int it = 0; it < kNewtonSteps; ++it) {
    const Distorted D = distort_bc(k, a, b);
    const float rx = D.xd - dx, ry = D.yd - dy;
    const float det = D.j00 * D.j11 - D.j01 * D.j01;
    const float inv = 1.0f / det;
    a = a - (D.j11 * rx - D.j01 * ry) * inv;
    b = b - (D.j00 * ry - D.j01 * rx) * inv;
  }
  const Distorted D = distort_bc(k, a, b);
  const float det = D.j00 * D.j11 - D.j01 * D.j01;
  const float res = fmaxf(fabsf(D.xd - dx), fabsf(D.yd - dy));
  const bool ok = is_finite(a) && is_finite(b) && D.u < u_max && det > 0.0f && res <= kResidualFactor * D.bound;
  Ray q;
  q.x = a; q.y = b;
  return ok ? q : no_ray();
}

// MGS_CAMERA_FISHEYE_KB (all k zero: the ideal fisheye): Newton on theta P(theta^2) = |d| from theta = |d|.  Valid iff
// theta^2 < u_max, the residual is inside its threshold and cos(theta) > 0 AS EVALUATED (fl(pi/2) > pi/2: a theta that
// passes theta < fl(pi/2) can still have a negative tangent); then q = d sin(theta) / (cos(theta) |d|), and q = d at d = 0.
MGS_MESH_HD Ray ray_kb(const float* row, float dx, float dy) {
  const float* k = row + 9;
  const float u_max = row[13];
  const float rd = sqrtf(fmaf(dx, dx, dy * dy));
  float theta = rd;
  for (int it = 0; it < kNewtonSteps; ++it) {
    const Radial R = distort_kb(k, theta);
    theta = theta - (R.td - rd) / R.deriv;
  }
  const Radial R = distort_kb(k, theta);
  const float c = cosf(theta), s = sinf(theta);
  const bool ok = is_finite(theta) && theta >= 0.0f && theta * theta < u_max && fabsf(R.td - rd) <= kResidualFactor * R.bound &&
                  c > 0.0f;
  Ray q;
  if (rd == 0.0f) {
    q.x = dx; q.y = dy;
    return ok ? q : no_ray();
  }
  const float g = s / (c * rd);
  q.x = dx * g; q.y = dy * g;
  return ok && is_finite(q.x) && is_finite(q.y) ? q : no_ray();
}

MGS_MESH_HD Ray pixel_ray(int camera_model, const float* row, int px, int py) {
  float dx, dy;
  pixel_distorted(row, px, py, dx, dy);
  if (!is_finite(dx) || !is_finite(dy)) return no_ray();
  return camera_model == kModelPinholeBc ? ray_bc(row, dx, dy) : ray_kb(row, dx, dy);
}

// ---- block tables ----------------------------------------------------------------------------------------------------------
// The rectangle of block (bx, by) of camera c: over the valid rays of its 8 x 8 pixels and of the one-pixel ring around
// them, clipped to the image (this path's counterpart of the pinhole box's "widened by one pixel": it absorbs the fp32 edge
// margin the same way); empty where the block has no valid pixel of its own.
MGS_MESH_HD Rect block_rect(const Ray* rays, int c, int width, int height, int bx, int by) {
  Rect r = empty_rect();
  bool own = false;
  const int x0 = bx * kBlockSide, y0 = by * kBlockSide;
  for (int y = y0 - 1; y <= y0 + kBlockSide; ++y)
    for (int x = x0 - 1; x <= x0 + kBlockSide; ++x) {
      if (x < 0 || y < 0 || x >= width || y >= height) continue;
      const Ray q = rays[pixel_index(c, width, height, x, y)];
      if (!has_ray(q)) continue;
      rect_add(r, q);
      own = own || (x >= x0 && x < x0 + kBlockSide && y >= y0 && y < y0 + kBlockSide);
    }
  return own ? r : empty_rect();
}
// the rectangle of superblock (sx, sy): the join of its blocks' rectangles
MGS_MESH_HD Rect super_rect(const Rect* blocks, int c, int nbx, int nby, int sx, int sy) {
  Rect r = empty_rect();
  for (int j = 0; j < kSuperSide; ++j)
    for (int i = 0; i < kSuperSide; ++i) {
      const int bx = sx * kSuperSide + i, by = sy * kSuperSide + j;
      if (bx < nbx && by < nby) rect_join(r, blocks[rect_index(c, nbx, nby, bx, by)]);
    }
  return r;
}

// ---- the face's box ----------------------------------------------------------------------------------------------------------
// In ray space, where the triangle is straight: the box of x/z, y/z over the points face_box takes (the vertices with
// z >= near and the near-plane crossings), each widened by the counted fp32 bound of its quotient: 2 U |x/z| for a vertex
// (one division), 8 U (|p| + |q - p|) / near for a crossing (t: 3 roundings; p + t (q - p): 3; the division: 1; |t| <= 1 up
// to its own rounding).  False where no point is in front of the near plane.  A box that is not ordered (a NaN) is
// returned as the whole plane: it drops nothing.
MGS_MESH_HD bool face_ray_box(const float a[3], const float b[3], const float c[3], float near_plane, Rect& box) {
  const float* v[3] = {a, b, c};
  box = empty_rect();
  bool any = false;
  for (int i = 0; i < 3; ++i) {
    const float* p = v[i];
    const float* q = v[(i + 1) % 3];
    const bool pin = p[2] >= near_plane, qin = q[2] >= near_plane;
    if (pin) {
      const float x = p[0] / p[2], y = p[1] / p[2];
      const float wx = (2.0f * kUnit) * fabsf(x), wy = (2.0f * kUnit) * fabsf(y);
      box.x0 = fminf(box.x0, x - wx); box.x1 = fmaxf(box.x1, x + wx);
      box.y0 = fminf(box.y0, y - wy); box.y1 = fmaxf(box.y1, y + wy);
      any = true;
    }
    if (pin != qin) {
      const float t = (near_plane - p[2]) / (q[2] - p[2]);
      const float ex = q[0] - p[0], ey = q[1] - p[1];
      const float x = (p[0] + t * ex) / near_plane, y = (p[1] + t * ey) / near_plane;
      const float wx = (8.0f * kUnit) * (fabsf(p[0]) + fabsf(ex)) / near_plane;
      const float wy = (8.0f * kUnit) * (fabsf(p[1]) + fabsf(ey)) / near_plane;
      box.x0 = fminf(box.x0, x - wx); box.x1 = fmaxf(box.x1, x + wx);
      box.y0 = fminf(box.y0, y - wy); box.y1 = fmaxf(box.y1, y + wy);
      any = true;
    }
  }
  if (!any) return false;
  if (rect_empty(box)) { const float inf = __builtin_inff(); box.x0 = box.y0 = -inf; box.x1 = box.y1 = inf; }
  return true;
}

// The blocks of camera c whose rectangle the box overlaps, as their bounding box in block indices: the superblock
// rectangles first, then the blocks of each overlapping superblock.  False where there is none.
MGS_MESH_HD bool box_blocks(Rect box, const Rect* blocks, const Rect* supers, int c, int width, int height, FaceRec& r) {
  const int nbx = blocks_of(width), nby = blocks_of(height), nsx = supers_of(width), nsy = supers_of(height);
  int bx0 = nbx, by0 = nby, bx1 = -1, by1 = -1;
  for (int sy = 0; sy < nsy; ++sy)
    for (int sx = 0; sx < nsx; ++sx) {
      if (!rect_overlap(box, supers[rect_index(c, nsx, nsy, sx, sy)])) continue;
      for (int j = 0; j < kSuperSide; ++j)
        for (int i = 0; i < kSuperSide; ++i) {
          const int bx = sx * kSuperSide + i, by = sy * kSuperSide + j;
          if (bx >= nbx || by >= nby || !rect_overlap(box, blocks[rect_index(c, nbx, nby, bx, by)])) continue;
          bx0 = bx < bx0 ? bx : bx0; bx1 = bx > bx1 ? bx : bx1;
          by0 = by < by0 ? by : by0; by1 = by > by1 ? by : by1;
        }
    }
  if (bx1 < 0) return false;
  r.bx0 = bx0; r.by0 = by0; r.nbx = bx1 - bx0 + 1; r.nby = by1 - by0 + 1;
  return true;
}

// ---- the view of one camera under a lens (see PinholeView) ------------------------------------------------------------------
// The planes are set up under Cam{1, 1, 0, 0}, the box comes from the block tables, and a pixel's ray is one 8-byte load from
// the ray map: the headlight's ray is then (q, 1) normalised.  The tables hold all cameras, so the view of camera c is the
// struct itself.
struct LensView {
  const Ray* rays;                            // [C,H,W]
  const Rect* blocks;                         // [C,BY,BX]
  const Rect* supers;                         // [C,SY,SX]
  MGS_MESH_HD LensView camera(int) const { return *this; }
  using P0 = Ray;
  using P1 = Rect;
  using P2 = Rect;
  const P0* p0() const { return rays; }
  const P1* p1() const { return blocks; }
  const P2* p2() const { return supers; }
  MGS_MESH_HD static LensView from(const P0* rays, const P1* blocks, const P2* supers) {
    LensView v; v.rays = rays; v.blocks = blocks; v.supers = supers; return v;
  }
  MGS_MESH_HD Cam plane_cam() const { const Cam unit = {1.0f, 1.0f, 0.0f, 0.0f}; return unit; }
  MGS_MESH_HD bool box(const float a[3], const float b[3], const float c[3], float near_plane, int cam_index, int width,
                       int height, FaceRec& r) const {
    Rect bx;
    return face_ray_box(a, b, c, near_plane, bx) && box_blocks(bx, blocks, supers, cam_index, width, height, r);
  }
  MGS_MESH_HD bool ray(size_t at, int, int, float& dx, float& dy) const {
    const Ray q = rays[at];
    dx = q.x; dy = q.y;
    return has_ray(q);
  }
};

// The lens path's setup, key and resolve by their earlier names, for callers that hold the tables or one ray and no view
MGS_MESH_HD bool face_setup_lens(const float* verts_cam_c, int V, const int32_t* faces, int face, float near_plane,
                                 const Rect* blocks, const Rect* supers, int c, int width, int height, bool cull, FaceRec& r) {
  const LensView view = {nullptr, blocks, supers};
  return face_setup(view, verts_cam_c, V, faces, face, near_plane, c, width, height, cull, r);
}
MGS_MESH_HD bool pixel_key_lens(const FaceRec& r, Ray q, float near_plane, float far_plane, uint64_t& key) {
  return has_ray(q) && pixel_key_at(r, q.x, q.y, near_plane, far_plane, key);
}
MGS_MESH_HD Shaded resolve_pixel_lens(uint64_t key, const float* verts_cam_c, int V, const int32_t* faces, int F,
                                      const float* vertex_colors, const float* face_colors, Ray q, bool headlight, float ambient) {
  const Cam unit = {1.0f, 1.0f, 0.0f, 0.0f};
  return resolve_pixel_at(has_ray(q) ? key : kEmptyKey, verts_cam_c, V, faces, F, vertex_colors, face_colors, unit, q.x, q.y,
                          headlight, ambient);
}

}  // namespace mesh
}  // namespace mgs
#endif  // MGS_MESH_LENS_RASTER_H_
