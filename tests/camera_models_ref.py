"""fp64 restatement of the projection under the three camera models (include/mgs.h MGS_CAMERA_*), in NumPy and in torch.

A helper module of the camera-model tests (not a conftest).  `project` / `project_torch` return the dicts of
oracle.gs_oracle_np.project / oracle.gs_oracle_torch.project ("lam", "extent_xy", ... included), so the oracle's stage
functions (sh_colors, isect_tiles, isect_offsets, rasterize, gaussian_edge_mask, gs_oracle_torch.rasterize) take them;
`render_model` / `render_model_torch` compose those stages the way O.render / OT.render do.  Pinhole is the oracle's own
projection; ortho and fisheye change the mean and the Jacobian J only:
  ortho    mean (fx x + cx, fy y + cy), J = [[fx, 0, 0], [0, fy, 0]]
  fisheye  rho = |(x, y)|, theta = atan2(rho, z), s = theta / rho, mean (fx s x + cx, fy s y + cy),
           J = [[fx (s + x^2 a), fx x y a, -fx x / r2], [fy x y a, fy (s + y^2 a), -fy y / r2]],
           r2 = rho^2 + z^2, a = (z / r2 - s) / rho^2
with no frustum clamp; depth is z and near / far cull on it as for pinhole.
"""
from __future__ import annotations

import numpy as np
import torch

from oracle import gs_oracle_np as O
from oracle import gs_oracle_torch as OT

MODELS = ("pinhole", "ortho", "fisheye")
# below t = rho^2 / z^2 = 1e-3 the fisheye terms come from their series (fp64: 8 terms are exact to rounding)
_SERIES_T = 1e-3


def _fisheye_s_a(q, z, xp):
    """s = theta / rho and a = (z / r2 - s) / q as functions of q = rho^2 and z, fp64, with the series near the axis
    (xp = numpy or torch; the torch form keeps both branches finite so that autograd through `where` stays finite)."""
    where = np.where if xp is np else torch.where
    z2 = z * z
    small = q < _SERIES_T * z2
    t = where(small, q / z2, xp.zeros_like(q))
    s_ser = sum(((-t) ** n) / (2 * n + 1) for n in range(8)) / z
    a_ser = sum(((-1) ** (n + 1)) * 2.0 * (n + 1) / (2 * n + 3) * t ** n for n in range(8)) / (z2 * z)
    qs = where(small, xp.ones_like(q), q)           # the closed form, away from the axis
    rho = xp.sqrt(qs)
    atan2 = np.arctan2 if xp is np else torch.atan2
    s_dir = atan2(rho, z) / rho
    a_dir = (z / (qs + z2) - s_dir) / qs
    return where(small, s_ser, s_dir), where(small, a_ser, a_dir)


def _mean_and_J(x, y, z, fx, fy, cx, cy, camera_model, xp):
    zero = xp.zeros_like(x)
    if camera_model == "ortho":
        mu = (fx * x + cx, fy * y + cy)
        J = (fx + zero, zero, zero, zero, fy + zero, zero)
    elif camera_model == "fisheye":
        q = x * x + y * y
        s, a = _fisheye_s_a(q, z, xp)
        ir2 = 1.0 / (q + z * z)
        mu = (fx * s * x + cx, fy * s * y + cy)
        J = (fx * (s + x * x * a), fx * x * y * a, -fx * x * ir2, fy * x * y * a, fy * (s + y * y * a), -fy * y * ir2)
    else:
        raise ValueError(camera_model)
    return mu, J


def project(means, quats, scales, viewmat, K, width, height, eps2d=0.3, near_plane=0.01, far_plane=1e10,
            radius_clip=0.0, radius_rule="classic", opacities=None, antialiased=False, camera_model="pinhole"):
    """oracle.gs_oracle_np.project under a camera model (fp64)."""
    if camera_model == "pinhole":
        return O.project(means, quats, scales, viewmat, K, width, height, eps2d, near_plane, far_plane, radius_clip,
                         radius_rule=radius_rule, opacities=opacities, antialiased=antialiased)
    dt = np.float64
    means = np.asarray(means, dtype=dt)
    viewmat, K = np.asarray(viewmat, dtype=dt), np.asarray(K, dtype=dt)
    N = means.shape[0]
    Rcw, tcw = viewmat[:3, :3], viewmat[:3, 3]
    fx, fy, cx, cy = K[0, 0], K[1, 1], K[0, 2], K[1, 2]
    W, H = dt(width), dt(height)
    pc = means @ Rcw.T + tcw
    x, y, z = pc[:, 0], pc[:, 1], pc[:, 2]
    valid = (z >= near_plane) & (z <= far_plane)
    zs = np.where(valid, z, 1.0)
    cov_c = Rcw[None] @ O.covar_world(quats, scales, dt) @ Rcw.T[None]
    (mx, my), Jt = _mean_and_J(x, y, zs, fx, fy, cx, cy, camera_model, np)
    J = np.stack(Jt, axis=-1).reshape(N, 2, 3)
    cov2 = J @ cov_c @ np.swapaxes(J, 1, 2)
    mu = np.stack([mx, my], axis=-1)
    a, b, c = cov2[:, 0, 0], cov2[:, 0, 1], cov2[:, 1, 1]
    det0 = a * c - b * b
    a, c = a + eps2d, c + eps2d
    det = a * c - b * b
    valid &= det > 0
    dets = np.where(det > 0, det, 1.0)
    comp = np.sqrt(np.maximum(0.0, det0 / dets))
    conic = np.stack([c / dets, -b / dets, a / dets], axis=-1)
    m = 0.5 * (a + c)
    lam = m + np.sqrt(np.maximum(0.01, m * m - dets))
    extra = {}
    if radius_rule == "classic":
        radius = np.ceil(3.0 * np.sqrt(lam))
        radius_y = radius
        valid &= radius > radius_clip
        extra["extent_xy"] = np.stack([3.0 * np.sqrt(lam)] * 2, axis=-1)
    elif radius_rule == "opacity_aware":
        ext = np.full(N, O.EXTENT_MAX)
        op_ok = np.ones(N, dtype=bool)
        if opacities is not None:
            op = np.asarray(opacities, dtype=dt)
            if antialiased:
                op = op * comp
            op_ok = op >= 1.0 / 255.0
            with np.errstate(invalid="ignore", divide="ignore"):
                ext = np.minimum(ext, np.sqrt(2.0 * np.log(np.where(op_ok, op, 1.0) * 255.0)))
            extra["op_rule"] = op
        valid &= op_ok
        ex, ey = ext * np.sqrt(np.maximum(a, 0)), ext * np.sqrt(np.maximum(c, 0))
        radius, radius_y = np.ceil(ex), np.ceil(ey)
        valid &= ((radius > radius_clip) | (radius_y > radius_clip)) & (radius > 0) & (radius_y > 0)
        extra["extent_xy"] = np.stack([ex, ey], axis=-1)
        extra["extent"] = ext
    else:
        raise ValueError(radius_rule)
    valid &= ~((mu[:, 0] + radius <= 0) | (mu[:, 0] - radius >= W) | (mu[:, 1] + radius_y <= 0) | (mu[:, 1] - radius_y >= H))
    if radius_rule == "classic":
        radii = np.where(valid, radius, 0).astype(np.int32)
    else:
        radii = np.where(valid[:, None], np.stack([radius, radius_y], axis=-1), 0).astype(np.int32)
    zok = (z >= near_plane) & (z <= far_plane)
    return {"lam": lam, "mu": mu, "z": z, "det_ok": det > 0, "conics_all": conic, "z_ok": zok, **extra,
            "radii": radii, "means2d": np.where(valid[:, None], mu, 0), "depths": np.where(valid, z, 0),
            "conics": np.where(valid[:, None], conic, 0), "compensations": np.where(valid, comp, 0)}


def project_torch(means, quats, scales, viewmat, K, width, height, eps2d=0.3, near_plane=0.01, far_plane=1e10,
                  radius_clip=0.0, radius_rule="classic", opacities=None, antialiased=False, camera_model="pinhole"):
    """oracle.gs_oracle_torch.project under a camera model: differentiable in means / quats / scales / viewmat."""
    if camera_model == "pinhole":
        return OT.project(means, quats, scales, viewmat, K, width, height, eps2d, near_plane, far_plane, radius_clip,
                          radius_rule=radius_rule, opacities=opacities, antialiased=antialiased)
    Rcw, tcw = viewmat[:3, :3], viewmat[:3, 3]
    fx, fy, cx, cy = K[0, 0], K[1, 1], K[0, 2], K[1, 2]
    pc = means @ Rcw.T + tcw
    x, y, z = pc.unbind(-1)
    valid = (z >= near_plane) & (z <= far_plane)
    zs = torch.where(valid, z, torch.ones_like(z))
    M = OT.quat_to_rotmat(quats) * scales[:, None, :]
    cov_c = Rcw @ (M @ M.transpose(1, 2)) @ Rcw.T
    (mx, my), Jt = _mean_and_J(x, y, zs, fx, fy, cx, cy, camera_model, torch)
    J = torch.stack(Jt, dim=-1).reshape(-1, 2, 3)
    cov2 = J @ cov_c @ J.transpose(1, 2)
    mu = torch.stack([mx, my], dim=-1)
    a, b, c = cov2[:, 0, 0], cov2[:, 0, 1], cov2[:, 1, 1]
    det0 = a * c - b * b
    a, c = a + eps2d, c + eps2d
    det = a * c - b * b
    valid = valid & (det > 0)
    dets = torch.where(det > 0, det, torch.ones_like(det))
    comp = torch.sqrt(torch.clamp(det0 / dets, min=0.0))
    conic = torch.stack([c / dets, -b / dets, a / dets], dim=-1)
    m = 0.5 * (a + c)
    lam = m + torch.sqrt(torch.clamp(m * m - dets, min=0.01))
    if radius_rule == "classic":
        radius = torch.ceil(3.0 * torch.sqrt(lam)).detach()
        radius_y = radius
        valid = valid & (radius > radius_clip)
    else:
        ext = torch.full_like(lam, O.EXTENT_MAX)
        if opacities is not None:
            op = (opacities * comp if antialiased else opacities).detach()
            ok = op >= 1.0 / 255.0
            ext = torch.minimum(ext, torch.sqrt(2.0 * torch.log(torch.where(ok, op, torch.ones_like(op)) * 255.0)))
            valid = valid & ok
        radius = torch.ceil(ext * torch.sqrt(a)).detach()
        radius_y = torch.ceil(ext * torch.sqrt(c)).detach()
        valid = valid & ((radius > radius_clip) | (radius_y > radius_clip)) & (radius > 0) & (radius_y > 0)
    valid = valid & ~((mu[:, 0] + radius <= 0) | (mu[:, 0] - radius >= width)
                      | (mu[:, 1] + radius_y <= 0) | (mu[:, 1] - radius_y >= height))
    vf = valid.to(means.dtype)
    rr = radius if radius_rule == "classic" else torch.stack([radius, radius_y], dim=-1)
    vr = valid if radius_rule == "classic" else valid[:, None]
    return {"radii": torch.where(vr, rr, torch.zeros_like(rr)).to(torch.int32),
            "means2d": mu * vf[:, None], "depths": z * vf, "conics": conic * vf[:, None], "compensations": comp * vf}


def render_model(means, quats, scales, opacities, sh_or_colors, viewmat, K, width, height, sh_degree=None,
                 tile_size=16, render_mode="RGB", eps2d=0.3, near_plane=0.01, far_plane=1e10, radius_clip=0.0,
                 background=None, rasterize_mode="classic", margins=False, flip_eps=None, radius_rule="classic",
                 camera_model="pinhole"):
    """oracle.gs_oracle_np.render under a camera model (same stages, same meta keys)."""
    dt = np.float64
    tile_w, tile_h = -(-width // tile_size), -(-height // tile_size)
    p = project(means, quats, scales, viewmat, K, width, height, eps2d, near_plane, far_plane, radius_clip,
                radius_rule=radius_rule, opacities=opacities, antialiased=rasterize_mode == "antialiased",
                camera_model=camera_model)
    opac = np.asarray(opacities, dtype=dt)
    if rasterize_mode == "antialiased":
        opac = opac * p["compensations"]
    if sh_degree is None:
        rgb = np.asarray(sh_or_colors, dtype=dt)
    else:
        rgb = O.sh_colors(sh_degree, means, O.campos_from_viewmat(viewmat), sh_or_colors, dt)
        rgb = np.where(O.visible(p["radii"])[:, None], rgb, 0)
    depth = p["depths"][:, None]
    feats = {"RGB": rgb, "D": depth, "ED": depth}.get(render_mode)
    if feats is None:
        feats = np.concatenate([rgb, depth], axis=-1)
    tpg, isect_ids, flatten_ids = O.isect_tiles(p["means2d"], p["radii"], p["depths"], tile_size, tile_w, tile_h, dtype=dt)
    offs = O.isect_offsets(isect_ids, 1, tile_w, tile_h)[0]
    bg = None if background is None else np.asarray(background, dtype=dt)
    img, alpha, last, stats = O.rasterize(p["means2d"], p["conics"], feats, opac, flatten_ids, offs, width, height,
                                          tile_size, bg, dt, margins=margins, depths=p["depths"] if margins else None,
                                          flip_eps=flip_eps if margins else None)
    if render_mode in ("ED", "RGB+ED"):
        img = img.copy()
        img[..., -1] = img[..., -1] / np.maximum(alpha, 1e-10)
    meta = dict(p)
    if margins:
        em, n_edge, ew = O.gaussian_edge_mask(p, opac, width, height, tile_size, near_plane=near_plane,
                                              far_plane=far_plane, return_weight=True)
        meta.update(edge_mask=em, n_edge_gaussians=n_edge)
        if flip_eps is not None:
            fw = stats.pop("flip_weight") + ew
            fw = fw + np.where(em & (stats["margins"][1] < flip_eps["T"] + ew), stats.pop("t_at_min"), 0.0)
            vis = O.visible(p["radii"])
            meta.update(flip_weight=fw, feat_max=(np.abs(feats[vis]).max(axis=0) if vis.any()
                                                  else np.zeros(feats.shape[1])))
    meta.update(tiles_per_gauss=tpg, isect_ids=isect_ids, flatten_ids=flatten_ids, isect_offsets=offs, last_ids=last,
                colors=rgb, opacities=opac, tile_width=tile_w, tile_height=tile_h, n_isect=len(flatten_ids),
                n_vis=int(O.visible(p["radii"]).sum()), **stats)
    return img, alpha[..., None], meta


def render_model_torch(means, quats, scales, opacities, sh_or_colors, viewmat, K, width, height, sh_degree=None,
                       tile_size=16, render_mode="RGB", eps2d=0.3, near_plane=0.01, far_plane=1e10, radius_clip=0.0,
                       background=None, rasterize_mode="classic", radius_rule="classic", camera_model="pinhole"):
    """oracle.gs_oracle_torch.render under a camera model: differentiable w.r.t. means / quats / scales / opacities /
    colours / viewmat; the (integer) tile lists come from the NumPy oracle at the current values."""
    p = project_torch(means, quats, scales, viewmat, K, width, height, eps2d, near_plane, far_plane, radius_clip,
                      radius_rule=radius_rule, opacities=opacities, antialiased=rasterize_mode == "antialiased",
                      camera_model=camera_model)
    opac = opacities * p["compensations"] if rasterize_mode == "antialiased" else opacities
    vis = p["radii"] > 0 if p["radii"].dim() == 1 else p["radii"][:, 0] > 0
    if sh_degree is None:
        rgb = sh_or_colors
    else:
        campos = -viewmat[:3, :3].T @ viewmat[:3, 3]
        rgb = torch.clamp(OT.spherical_harmonics(sh_degree, means - campos, sh_or_colors) + 0.5, min=0.0)
        rgb = rgb * vis.to(rgb.dtype)[:, None]
    depth = p["depths"][:, None]
    feats = {"RGB": rgb, "D": depth, "ED": depth}.get(render_mode)
    if feats is None:
        feats = torch.cat([rgb, depth], dim=-1)
    tile_w, tile_h = -(-width // tile_size), -(-height // tile_size)
    _, isect_ids, flatten_ids = O.isect_tiles(p["means2d"].detach().numpy(), p["radii"].numpy(),
                                              p["depths"].detach().numpy(), tile_size, tile_w, tile_h)
    offs = O.isect_offsets(isect_ids, 1, tile_w, tile_h)[0]
    img, alpha = OT.rasterize(p["means2d"], p["conics"], feats, opac, flatten_ids, offs, width, height, tile_size,
                              background)
    if render_mode in ("ED", "RGB+ED"):
        img = torch.cat([img[..., :-1], img[..., -1:] / alpha.clamp(min=1e-10)[..., None]], -1)
    return img, alpha[..., None], p
