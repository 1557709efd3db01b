// mesh_checks.h -- the argument checks of the mesh entry points (mesh.hip, mesh_lens.hip, mesh_texture.hip), host side.
// Each returns MGS_OK or has set the error; `fn` is the entry point's name as the message carries it.
#ifndef MGS_MESH_CHECKS_H_
#define MGS_MESH_CHECKS_H_

#include "mgs_common.h"
#include "mesh_raster.h"

#define MGS_TRY(expr)        \
  do {                       \
    const int rc_ = (expr);  \
    if (rc_) return rc_;     \
  } while (0)

namespace mgs {
namespace mesh {

inline int check_sizes(const char* fn, int n_cams, int V, int F, int width, int height) {
  MGS_REQUIRE(n_cams >= 1, "%s: n_cams %d, at least 1 needed", fn, n_cams);
  MGS_REQUIRE(V >= 1, "%s: V %d vertices, at least 1 needed", fn, V);
  MGS_REQUIRE(F >= 1, "%s: F %d faces, at least 1 needed", fn, F);
  MGS_REQUIRE(width >= 1 && width <= kMaxSide && height >= 1 && height <= kMaxSide,
              "%s: image %d x %d, each side must be in 1 .. %d", fn, width, height, kMaxSide);
  MGS_REQUIRE(n_cams <= 65535, "%s: n_cams %d is above 65535", fn, n_cams);
  return MGS_OK;
}

inline int check_planes(const char* fn, float near_plane, float far_plane) {
  MGS_REQUIRE(near_plane > 0.f, "%s: near_plane %g is not a positive number", fn, (double)near_plane);
  MGS_REQUIRE(far_plane >= near_plane, "%s: far_plane %g is not a number at or above near_plane %g", fn, (double)far_plane,
              (double)near_plane);
  return MGS_OK;
}

inline int check_ambient(const char* fn, float ambient) {
  MGS_REQUIRE(ambient >= 0.f && ambient <= 1.f, "%s: ambient %g is outside 0 .. 1", fn, (double)ambient);
  return MGS_OK;
}

inline int check_links(const char* fn, int L, const float* rotations, const float* translations) {
  MGS_REQUIRE(L >= 0, "%s: L %d links is negative", fn, L);
  MGS_REQUIRE(L == 0 || (rotations && translations), "%s: %d links but rotations or translations is null", fn, L);
  return MGS_OK;
}

// `what` names the argument: "workspace" or "lens_workspace"
inline int check_workspace(const char* fn, const char* what, const void* workspace, size_t workspace_bytes, size_t need) {
  MGS_REQUIRE(workspace, "%s: %s is null", fn, what);
  MGS_REQUIRE(((uintptr_t)workspace & 255u) == 0, "%s: %s is not 256-byte aligned", fn, what);
  MGS_REQUIRE(workspace_bytes >= need, "%s: %s of %zu bytes, %zu needed", fn, what, workspace_bytes, need);
  return MGS_OK;
}

}  // namespace mesh
}  // namespace mgs
#endif  // MGS_MESH_CHECKS_H_
