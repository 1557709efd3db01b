"""How a triangle mesh is rasterised under a lens, in fp64 (NumPy), with the bounds an fp32 evaluation in the stated order can
be held to (a helper module, not a test file).  The statement include/mgs_mesh_lens.h, csrc/mesh_lens_raster.h and
csrc/mesh_lens.hip are built and tested against; it stands on tests/mesh_ref.py (the raster), tests/pinhole_lens_ref.py and
tests/lens_ref.py (the lenses: D, u_max, theta_max).

Semantics.  mesh_ref's raster is homogeneous: e = adj(M) r with r the pixel's ray, and the pixel enters through r alone.  Under
a lens the triangle is unchanged and the ray of pixel (px, py) is (x_u, y_u, 1) with q = (x_u, y_u) the preimage, under the
lens's distortion map, of d = ((px + 0.5 - cx) / fx, (py + 0.5 - cy) / fy).  A pixel has a ray iff that preimage exists inside
the lens's valid range (pinhole lens: u < u_max and det Jd > 0; fisheye: theta < theta_max <= pi/2).  A pixel without a ray
is uncovered.  Everything else -- the planes (set up under K = I: s / 1 is exact), inside, z, the drop rules, the winner,
the resolve -- is mesh_ref's, with the headlight's ray (q, 1) normalised.

Ray stage.  The reference inverts robustly: for the pinhole lens Newton to 1e-14 from 25 starts along the pixel's own
direction, for the fisheye a bisection of theta P(theta^2) = |d| on [0, theta_max] (1-D, monotone there).  The kernel runs 12
Newton steps in fp32 and accepts q where its fp32 residual is within 2 B(q), B(q) = 10 U |D|(q) the counted bound of one fp32
evaluation of D at q (|D|: every coefficient and coordinate replaced by its modulus; the count is in mesh_lens_raster.h).  The
fp32 residual is itself off by at most B(q), d = ((px + 0.5) - cx) / fx carries two roundings, so the true residual is
    |D(q_gpu) - d| <= res := 3 B(q) + gamma_2 |d|                      (fisheye: gamma_5 |d|, for |d| = sqrt(fma(dx, dx, dy dy)))
and by the mean value theorem |q_gpu - q_64| <= sup |Jd^-1| res, the supremum over the segment between them: evaluated at q_64
and at the four corners of twice the first-order box; a pixel where that supremum exceeds twice the value at q_64 is
ill-conditioned (none may be, outside the fold's neighbourhood).  The fisheye's q = d sin(theta) / (cos(theta) |d|) adds
gamma_12 |q| (sin, cos at 2 ulp each, the product, the quotient, |d|'s and d's roundings) to |d| / (|d| cos^2) dtheta.

Validity.  The fp32 solve and the fp64 one may disagree only next to a fold: `near_fold` marks the pixels whose |d| is within
1e-3 (relative) of the fold's image along the pixel's direction.

Raster stage.  The pixel's ray is an fp32 INPUT here (the stages are held separately: on the harness's or the GPU's own ray
map).  gamma_8 remains a valid count for e_i: the 1 / f and dx roundings it includes do not occur.  Pairs come by brute force
over all pixels; the acceptance rule is mesh_ref.RasterRef.check_raster, inherited.
"""
import math

import numpy as np

import lens_ref as LR
import mesh_ref as MR
import pinhole_lens_ref as PR

U, gamma = MR.U, MR.gamma
BC, KB = 4, 3                                  # MGS_CAMERA_PINHOLE_BC, MGS_CAMERA_FISHEYE_KB
EVAL_ROUNDINGS = 10
NEAR_FOLD = 1e-3
NEAR_FOLD_CAP = 0.02

# the four lenses of the tests: (camera model, coefficients, the lens of pinhole_lens_ref.intrinsics that gives K)
LENSES = {"bc_mild": (BC, PR.MILD, "mild"), "bc_folding": (BC, PR.FOLDING, "folding"),
          "kb_mild": (KB, LR.MILD, "mild"), "kb_folding": (KB, LR.FOLDING, "folding")}


def intrinsics(lens, width, height):
    """K float32 [3,3] of a test lens at width x height."""
    return PR.intrinsics(LENSES[lens][2], width, height).astype(np.float32)


def lens_row(lens, K):
    """(camera model, the 16-float camera row float32) of a test lens under K."""
    model, k, _ = LENSES[lens]
    row = PR.lens_row(K, k) if model == BC else LR.lens_row(K, k)
    return model, row.astype(np.float32)


def pixel_d(K, width, height):
    """d fp64 [H,W,2] of the fp32 K."""
    K = np.asarray(K, np.float32).astype(np.float64)
    x, y = np.meshgrid(np.arange(width) + 0.5, np.arange(height) + 0.5)
    return np.stack([(x - K[0, 2]) / K[0, 0], (y - K[1, 2]) / K[1, 1]], -1)


# ---- the pinhole lens ------------------------------------------------------------------------------------------------------
def _bc_abs(a, b, k):
    """|D|(q): the forward map with every coefficient and coordinate replaced by its modulus, max over the two components."""
    xd, yd, _, _ = PR.distort(np.abs(a), np.abs(b), [abs(v) for v in PR.full(k)])
    return np.maximum(xd, yd)


def _bc_jinv_abs(a, b, k):
    """|Jd^-1| [.., 2, 2] at q."""
    _, _, (d00, d01, d11), _ = PR.distort(a, b, k)
    det = d00 * d11 - d01 * d01
    with np.errstate(divide="ignore", invalid="ignore"):
        return np.abs(np.stack([np.stack([d11, -d01], -1), np.stack([-d01, d00], -1)], -2) / det[..., None, None])


def _bc_solve(d, k, umax):
    """(q [n,2], valid [n]) by Newton to 1e-14 from 25 starts s d, s = 0.1 .. 2.5: the first start that converges inside the
    valid range (u < u_max, det Jd > 0: the map is injective there)."""
    n = len(d)
    q_out, valid = np.full((n, 2), np.nan), np.zeros(n, bool)
    for s in np.linspace(0.1, 2.5, 25):
        todo = np.flatnonzero(~valid)
        if not len(todo):
            break
        t = d[todo]
        q = s * t
        with np.errstate(all="ignore"):
            for _ in range(60):
                xd, yd, (d00, d01, d11), _ = PR.distort(q[:, 0], q[:, 1], k)
                rx, ry, det = xd - t[:, 0], yd - t[:, 1], d00 * d11 - d01 * d01
                q = q - np.stack([d11 * rx - d01 * ry, d00 * ry - d01 * rx], 1) / det[:, None]
            xd, yd, (d00, d01, d11), u = PR.distort(q[:, 0], q[:, 1], k)
            ok = (np.maximum(np.abs(xd - t[:, 0]), np.abs(yd - t[:, 1])) <= 1e-14 * np.maximum(1.0, np.abs(t).max(1))) \
                & (u < umax) & (d00 * d11 - d01 * d01 > 0) & np.isfinite(q).all(1)
        q_out[todo[ok]], valid[todo[ok]] = q[ok], True
    return q_out, valid


def _bc_fold_radius(phi, k, umax, n_az=1 << 12):
    """|d| of the fold's image along the d-space directions phi (inf where the lens has no fold that way): the border of the
    valid range along n_az rays of q space (a scan and a bisection), mapped through D and interpolated over its azimuth."""
    az = np.linspace(-math.pi, math.pi, n_az, endpoint=False)
    c, s = np.cos(az), np.sin(az)
    r_end = math.sqrt(min(umax, 64.0))

    def inside(r):
        _, _, (d00, d01, d11), u = PR.distort(r * c, r * s, k)
        return (u < umax) & (d00 * d11 - d01 * d01 > 0)
    lo, hi, found = np.zeros(n_az), np.full(n_az, r_end), np.zeros(n_az, bool)
    for r in np.linspace(0.0, r_end, 4001)[1:]:
        out = ~inside(np.full(n_az, r)) & ~found
        hi[out], found[out] = r, True
        lo[~found] = r
    if not found.any():
        return np.full(np.shape(phi), np.inf)
    for _ in range(60):
        mid = 0.5 * (lo + hi)
        ins = inside(mid)
        lo, hi = np.where(ins, mid, lo), np.where(ins, hi, mid)
    xd, yd, _, _ = PR.distort(lo * c, lo * s, k)
    rb = np.where(found, np.hypot(xd, yd), np.inf)
    ab = np.arctan2(yd, xd)
    o = np.argsort(ab)
    return np.interp(phi, ab[o], rb[o], period=2 * math.pi)


# ---- the fisheye -------------------------------------------------------------------------------------------------------------
def _kb_P(k, u, absolute=False):
    k1, k2, k3, k4 = (abs(float(v)) if absolute else float(v) for v in k)
    return 1.0 + u * (k1 + u * (k2 + u * (k3 + u * k4)))


def _kb_solve(rd, k, tmax):
    """(theta [n], valid [n]): bisection of theta P(theta^2) = rd on [0, theta_max], where the left side grows."""
    g = lambda t: t * _kb_P(k, t * t)
    valid = rd < g(tmax)
    lo, hi = np.zeros_like(rd), np.full_like(rd, tmax)
    for _ in range(100):
        mid = 0.5 * (lo + hi)
        below = g(mid) < rd
        lo, hi = np.where(below, mid, lo), np.where(below, hi, mid)
    return 0.5 * (lo + hi), valid


class RayRef:
    """The ray map of one camera in fp64: q [H,W,2] (NaN where the pixel has no ray), valid [H,W], near_fold [H,W], bound
    [H,W,2] (on |q_fp32 - q|, inf where ill-conditioned), conditioned [H,W]."""

    def __init__(self, model, K, k, width, height):
        self.width, self.height = int(width), int(height)
        d = pixel_d(K, width, height).reshape(-1, 2)
        n = len(d)
        rd = np.hypot(d[:, 0], d[:, 1])
        if model == BC:
            umax = PR.u_max(k)
            q, valid = _bc_solve(d, k, umax)
            rb = _bc_fold_radius(np.arctan2(d[:, 1], d[:, 0]), k, umax)
            qs = np.where(valid[:, None], q, 0.0)
            res = 3 * gamma(EVAL_ROUNDINGS + 1) * _bc_abs(qs[:, 0], qs[:, 1], k) + gamma(2) * np.abs(d).max(1)
            b0 = _bc_jinv_abs(qs[:, 0], qs[:, 1], k).sum(-1) * res[:, None]
            bound = b0.copy()
            for sx in (-2, 2):
                for sy in (-2, 2):
                    ji = _bc_jinv_abs(qs[:, 0] + sx * b0[:, 0], qs[:, 1] + sy * b0[:, 1], k)
                    bound = np.maximum(bound, ji.sum(-1) * res[:, None])
        elif model == KB:
            tmax = LR.theta_max(k)
            theta, valid = _kb_solve(rd, k, tmax)
            rb = np.full(n, tmax * _kb_P(k, tmax * tmax))          # the fold, or the ray at 90 degrees: the range ends there alike
            th = np.where(valid, theta, 0.0)
            with np.errstate(divide="ignore", invalid="ignore"):
                g = np.where(rd > 0, np.tan(th) / rd, 1.0)
            q = d * g[:, None]
            res = 3 * gamma(EVAL_ROUNDINGS + 1) * th * _kb_P(k, th * th, absolute=True) + gamma(5) * rd
            dth0 = res / LR._D(k, th * th)
            dth = np.maximum(dth0, res / LR._D(k, (th + 2 * dth0) ** 2))
            dth = np.maximum(dth, res / LR._D(k, np.maximum(th - 2 * dth0, 0.0) ** 2))
            sec2 = 1.0 / np.cos(np.minimum(th + 2 * dth0, 0.5 * math.pi)) ** 2
            with np.errstate(divide="ignore", invalid="ignore"):
                unit = np.where(rd[:, None] > 0, np.abs(d) / rd[:, None], 0.0)
            b0 = unit * (dth0 / np.cos(th) ** 2)[:, None] + gamma(12) * np.abs(q)
            bound = unit * (sec2 * dth)[:, None] + gamma(12) * np.abs(q)
        else:
            raise ValueError(f"camera model {model} has no ray map")
        with np.errstate(invalid="ignore", divide="ignore"):
            near = np.abs(rd / rb - 1.0) < NEAR_FOLD
            cond = (bound <= 2 * b0 + 1e-300).all(1)
        shape = (self.height, self.width)
        self.valid, self.near_fold = valid.reshape(shape), near.reshape(shape)
        self.q = np.where(valid[:, None], q, np.nan).reshape(shape + (2,))
        self.conditioned = (cond | ~valid).reshape(shape)
        self.bound = np.where((valid & cond)[:, None], bound, np.inf).reshape(shape + (2,))

    def check_rays(self, rays):
        """Hold a kernel's ray map float32 [H,W,2] to the statement: validity equal outside the fold's neighbourhood (which
        may hold at most NEAR_FOLD_CAP of the frame), both components NaN where there is no ray, and every ray within its
        bound.  Returns dict(worst = error over bound, valid, near_fold = counts)."""
        r = np.asarray(rays, np.float64).reshape(self.height, self.width, 2)
        has = ~np.isnan(r).any(-1)
        assert (np.isnan(r).all(-1) | has).all(), "a ray with one NaN component"
        assert np.isfinite(r[has]).all(), "an infinite ray"
        assert self.near_fold.mean() <= NEAR_FOLD_CAP, f"{self.near_fold.mean():.3%} of the frame is next to a fold"
        differs = (has != self.valid) & ~self.near_fold
        assert not differs.any(), f"validity differs at {int(differs.sum())} pixels away from a fold, first (y, x): " \
                                  f"{np.argwhere(differs)[:5].tolist()}"
        both = has & self.valid & ~self.near_fold
        assert self.conditioned[both].all(), f"{int((~self.conditioned[both]).sum())} ill-conditioned pixels away from a fold"
        ratio = np.abs(r[both] - self.q[both]) / (self.bound[both] + 1e-300)
        worst = float(ratio.max()) if ratio.size else 0.0
        assert worst <= 1, f"a ray is off its bound: worst ratio {worst:.3g}"
        return {"worst": worst, "valid": int(self.valid.sum()), "near_fold": int(self.near_fold.sum())}


# ---- the raster under a ray map ------------------------------------------------------------------------------------------------
_FAR_CENTRE = float(2 ** 29)                   # the setup's box is not this path's: a camera that keeps every face's box non-empty
_UNIT_K = np.array([[1.0, 0.0, _FAR_CENTRE], [0.0, 1.0, _FAR_CENTRE], [0.0, 0.0, 1.0]])


class LensRasterRef(MR.RasterRef):
    """mesh_ref.RasterRef with the pixel's ray given: rays float32 [H,W,2] (NaN: no ray) taken as exact.  The same attributes,
    so check_raster, mask, tolerance_share and pair_of are inherited; shade_ref takes the headlight's ray from the map."""

    def __init__(self, verts_cam, faces, rays, width, height, near_plane=0.01, far_plane=1e10, cull_backfaces=False):
        # planes under K = I (cx, cy are not folded into the planes, so the far centre only keeps the setup's pixel box open)
        self.setup = st = MR.FaceSetup(verts_cam, faces, _UNIT_K, 2 ** 30, 2 ** 30, near_plane, cull_backfaces)
        self.width, self.height, self.near, self.far = int(width), int(height), float(near_plane), float(far_plane)
        W, H = self.width, self.height
        n_px = W * H
        r = np.asarray(rays, np.float32).astype(np.float64).reshape(n_px, 2)
        self.rays = r
        has = np.flatnonzero(~np.isnan(r).any(1))
        live = np.flatnonzero(st.live)
        out = {k: [] for k in ("pix", "face", "e", "err", "S")}
        step = max(1, (1 << 21) // max(1, len(has)))
        qx, qy = r[has, 0][None, :], r[has, 1][None, :]
        for k0 in range(0, len(live), step):
            ff = live[k0:k0 + step]
            e = [st.A[ff, i][:, None] * qx + st.B[ff, i][:, None] * qy + st.C[ff, i][:, None] for i in range(3)]
            err = [gamma(8) * (st.NA[ff, i][:, None] * np.abs(qx) + st.NB[ff, i][:, None] * np.abs(qy) + st.NC[ff, i][:, None])
                   for i in range(3)]
            S = e[0] + e[1] + e[2]
            ok = (S > 0) & (e[0] >= -err[0]) & (e[1] >= -err[1]) & (e[2] >= -err[2])
            fi, pi = np.nonzero(ok)
            out["pix"].append(has[pi])
            out["face"].append(ff[fi])
            out["e"].append(np.stack([ei[fi, pi] for ei in e], 1))
            out["err"].append(np.stack([ei[fi, pi] for ei in err], 1))
            out["S"].append(S[fi, pi])
        cat = lambda k, shape: np.concatenate(out[k]) if out[k] else np.zeros(shape)
        pix, face = cat("pix", (0,)).astype(np.int64), cat("face", (0,)).astype(np.int64)
        e, err, S = cat("e", (0, 3)), cat("err", (0, 3)), cat("S", (0,))
        order = np.lexsort((face, pix))
        self.pix, self.face, self.e, self.err, self.S = pix[order], face[order], e[order], err[order], S[order]
        self._verdicts(cull_backfaces)

    def _verdicts(self, cull_backfaces):
        """mesh_ref.RasterRef.__init__ from the pairs on: tolerances, the three sets, the winner, the rivals."""
        st, n_px = self.setup, self.width * self.height
        self.errS = self.err.sum(1) + 2 * U * np.abs(self.e).sum(1)
        self.z = st.absdet[self.face] / self.S
        with np.errstate(divide="ignore", invalid="ignore"):
            rel = st.errdet[self.face] / st.absdet[self.face] + self.errS / self.S + U
            self.tolz = np.where(rel < 1, self.z * rel / (1 - rel), np.inf)
        z, tz = self.z, self.tolz
        self.possible = (z >= self.near - tz) & (z <= self.far + tz)
        self.certain = ((self.e >= self.err).all(1) & st.live_certain[self.face] & (z >= self.near + tz) & (z <= self.far - tz))
        self.exact = (self.e >= 0).all(1) & (z >= self.near) & (z <= self.far) & (st.front[self.face] if cull_backfaces else True)
        self.key = self.pix * max(st.F, 1) + self.face
        self.winner = np.full(n_px, -1, np.int64)
        self.zwin = np.zeros(n_px)
        ex = np.flatnonzero(self.exact)
        o = ex[np.lexsort((self.face[ex], self.z[ex], self.pix[ex]))]
        first = np.r_[True, self.pix[o][1:] != self.pix[o][:-1]] if len(o) else np.zeros(0, bool)
        self.win_pair = np.full(n_px, -1, np.int64)
        self.win_pair[self.pix[o][first]] = o[first]
        self.winner[self.pix[o][first]] = self.face[o][first]
        self.zwin[self.pix[o][first]] = self.z[o][first]
        self.zfront = np.full(n_px, np.inf)
        c = np.flatnonzero(self.certain)
        np.minimum.at(self.zfront, self.pix[c], (z + tz)[c])
        self.has_certain = np.isfinite(self.zfront)
        rival = self.possible & (z - tz <= self.zfront[self.pix])
        n_rival = np.bincount(self.pix[rival], minlength=n_px)
        n_rival_certain = np.bincount(self.pix[rival & self.certain], minlength=n_px)
        self.rival = rival
        self.by_tolerance = ~(((n_rival == 1) & (n_rival_certain == 1)) | (n_rival == 0))
        self.covered = self.winner >= 0

    def shade_ref(self, pairs, pixels, faces, vertex_colors=None, face_colors=None, headlight=False, ambient=0.3):
        """mesh_ref.RasterRef.shade_ref with the headlight's ray (q, 1) normalised."""
        st = self.setup
        f = self.face[pairs]
        faces = np.asarray(faces, np.int64)
        lam = self.e[pairs] / self.S[pairs, None]
        S, eS = self.S[pairs], self.errS[pairs]
        tl = (self.err[pairs] + np.abs(lam) * eS[:, None]) / (S - eS)[:, None] + U * np.abs(lam)
        n_p = len(pairs)
        if vertex_colors is not None:
            col = np.asarray(vertex_colors, np.float64)[faces[f]]
            rgb = (lam[:, :, None] * col).sum(1)
            tol = (tl[:, :, None] * np.abs(col)).sum(1) + gamma(3) * (np.abs(lam)[:, :, None] * np.abs(col)).sum(1)
        elif face_colors is not None:
            rgb, tol = np.asarray(face_colors, np.float64)[f], np.zeros((n_p, 3))
        else:
            rgb, tol = np.full((n_p, 3), float(np.float32(0.7))), np.zeros((n_p, 3))
        a, b, c = (v[f] for v in st.verts)
        n, Nn = MR._cross(b - a, c - a), MR._abs_cross(b - a, c - a)
        ln = np.linalg.norm(n, axis=1)
        nh = n / ln[:, None]
        tn = 2 * gamma(3) * np.linalg.norm(Nn, axis=1) / ln + 8 * U
        ray = np.concatenate([self.rays[pixels], np.ones((n_p, 1))], 1)
        rh = ray / np.linalg.norm(ray, axis=1)[:, None]
        cos = (nh * rh).sum(1)
        tc = 2 * tn + 16 * U
        normal = np.where(cos[:, None] > 0, -nh, nh)
        if headlight:
            shade = ambient + (1 - ambient) * np.abs(cos)
            tshade = (1 - ambient) * tc + 2 * U
            tol = tol * shade[:, None] + np.abs(rgb) * tshade[:, None] + U * np.abs(rgb) * shade[:, None]
            rgb = rgb * shade[:, None]
        return {"rgb": rgb, "tol_rgb": tol + 1e-300, "normal": normal, "tol_normal": tn, "flip_open": np.abs(cos) <= tc}


# ---- scenes ----------------------------------------------------------------------------------------------------------------------
def undistort64(model, k, d):
    """q fp64 [n,2] of distorted normalised points d [n,2] inside the lens's valid range (NaN outside)."""
    d = np.asarray(d, np.float64).reshape(-1, 2)
    if model == BC:
        q, valid = _bc_solve(d, k, PR.u_max(k))
    else:
        rd = np.hypot(d[:, 0], d[:, 1])
        theta, valid = _kb_solve(rd, k, LR.theta_max(k))
        with np.errstate(divide="ignore", invalid="ignore"):
            q = d * np.where(rd > 0, np.tan(theta) / rd, 1.0)[:, None]
    return np.where(valid[:, None], q, np.nan)


def markers(model, k, K, pixels, z, size_px=6.0):
    """Fronto-parallel marker triangles at depth z whose centroids project, under the lens, to the pixel positions `pixels`
    [n,2] (continuous coordinates), about size_px pixels across: (vertices float32 [3 n,3], faces int32 [n,3])."""
    K = np.asarray(K, np.float64)
    p = np.asarray(pixels, np.float64).reshape(-1, 2)
    q = undistort64(model, k, np.stack([(p[:, 0] - K[0, 2]) / K[0, 0], (p[:, 1] - K[1, 2]) / K[1, 1]], 1))
    assert np.isfinite(q).all(), "a marker pixel has no ray"
    h = 0.5 * size_px / K[0, 0]
    corners = np.array([[-1.0, -0.6], [1.0, -0.6], [0.0, 1.2]]) * h          # centroid at the origin
    xy = q[:, None, :] + corners[None]
    v = np.concatenate([xy * z, np.full(xy.shape[:2] + (1,), float(z))], -1).reshape(-1, 3)
    return v.astype(np.float32), np.arange(len(v), dtype=np.int32).reshape(-1, 3)
