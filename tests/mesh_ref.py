"""How a triangle mesh is rasterised as the opaque foreground of a frame, in fp64 (NumPy), with the bounds that an fp32
evaluation in the order stated below can be held to.  Every bound is a count of roundings, none is tuned to an output.  This
module is the statement a rasteriser is built and tested against; the project has none yet.

Semantics.  vertices [V,3] fp32, faces [F,3] int32, optional link_ids [V] (-1 static) with per-link rotations [L,3,3],
translations [L,3], scales [L] in the convention of transform_gaussians (x' = s R x + t), viewmats [C,4,4] and Ks [C,3,3] of an
OpenCV pinhole camera.  Vertex stage: x_cam = R_view x' + t_view.  Raster stage, homogeneous, no clipping: for face f with
camera-space vertices a, b, c and M = [a b c], the edge values at the pixel centre p = (x + 0.5, y + 0.5) with ray
r = K^-1 (p, 1) are e = adj(M) r, oriented by the sign of det M; inside is e_i >= 0 (inclusive), sum e_i > 0 is required,
z = |det M| / sum e_i, and the face counts iff near <= z <= far; barycentrics are e_i / sum e_i.  Dropped: det M = 0, a
vertex index outside 0..V-1, non-finite vertices, and with cull_backfaces det M >= 0.  Per pixel the winner is the smallest
(z, face index).  (In exact arithmetic two faces that share an edge leave no crack.  In fp32 that holds bit for bit only if
both faces compute the shared edge's plane from the same operands in the same order, e.g. always from the vertex with the
lower index; otherwise a pixel centre within tau of the edge may be refused by both, which the acceptance rule below
permits because neither face is certain there.)

Evaluation order the bounds are counted for: adj(M)'s rows as n_0 = b x (c - b), n_1 = c x (a - c), n_2 = a x (b - a) (the
edge-difference form: its rounding error is U |a| |edge|, not the raw cross product's U |a|^2), det = a . n_0,
A_i = n_i.x * (s / fx), B_i = n_i.y * (s / fy), C_i = s n_i.z with s the sign of det, per pixel dx = (x + 0.5) - cx,
dy = (y + 0.5) - cy (cx, cy not folded into C_i), e_i = fma(A_i, dx, fma(B_i, dy, C_i)), S = (e_0 + e_1) + e_2, z = |det| / S.

U = 2^-24 is the unit roundoff of fp32; gamma_k = k U / (1 - k U).  The inputs (verts_cam, K, colours) are fp32 values taken
as exact; the reference evaluates the same formulas in fp64, whose own error (1e-16 relative, times a cancellation of at most
a few thousand) is far below every bound.

Vertex stage.  y_k = fma(R_k2, x_2, fma(R_k1, x_1, R_k0 x_0)) has 3 roundings on its first term, x'_k = fma(s, y_k, t_k) one
more: |dx'_k| <= gamma_4 X'_k with X'_k = |s| sum_j |R_kj| |x_j| + |t_k| (X' = |x| for a static vertex, which is copied).
cam_k = fma(V_k2, x'_2, fma(V_k1, x'_1, fma(V_k0, x'_0, tv_k))) carries the error of x' and adds 3 roundings:
    |dcam_k| <= gamma_8 (sum_j |V_kj| X'_j + |tv_k|).

Edge values.  Row i of adj(M) is n_i = p x d with d = q - p (one rounding); a component p_y d_z - p_z d_y is two rounded
products and a rounded difference: 3 roundings on |p_y d_z| + |p_z d_y| =: N_i.x (the *absolute* cross product).
A_i = n_i.x * (s / fx): 1 / fx rounded, the product rounded: 5 roundings; B_i alike; C_i = s n_i.z: 3.  Per pixel dx = (x + 0.5)
- cx is one rounding and e_i = fma(A_i, dx, fma(B_i, dy, C_i)) two: the A term sees 5 + 1 + 1 = 7 roundings, the B term 5 + 1 + 2
= 8, the C term 3 + 2 = 5.  With E_i = N_i.x |dx| / fx + N_i.y |dy| / fy + N_i.z:
    |de_i| <= err_i := gamma_8 E_i.
In pixels that is tau_i = err_i / |grad_p e_i|, grad_p e_i = (A_i, B_i): the margin by which fp32 can move edge i.  (On the
open box, z = 10, faces 0.02 across, f = 858: tau is about 1e-3 px.)
S = (e_0 + e_1) + e_2: |dS| <= errS := sum err_i + 2 U sum |e_i|.
det = fma(a_2, n_0.z, fma(a_1, n_0.y, a_0 n_0.x)): at most 3 + 1 + 2 = 6 roundings: |ddet| <= errdet := gamma_6 sum_k |a_k| N_0.k.
A face whose |det| <= errdet has no certain orientation ("uncertain"): it can be in S, never in C.
z = |det| / S, one more rounding: rel := errdet / |det| + errS / S + U and tol_z := z rel / (1 - rel) (infinite for rel >= 1).

Acceptance (check_raster).  Face f is *possible* at pixel p, f in S(p), iff e_i >= -err_i for all i, S > 0 and
near - tol_z <= z <= far + tol_z; it is *certain*, f in C(p), iff e_i >= +err_i for all i, its orientation is certain and
near + tol_z <= z <= far - tol_z.  The kernel's winner g must be in S(p) (nothing may win only where C(p) is empty);
z_g - tol_z(g) <= min over C of (z_f + tol_z(f)); its depth is within tol_z(g) of z_g.  A pixel is *decided by tolerance*
unless exactly one possible face f0 has z_f - tol_z(f) <= min over C of (z + tol_z) and that face is certain (or no face is
possible at all); everywhere else the face id must be the reference's own winner.  A face that repeats the index triple of
a face with a lower index is the same fp32 computation with a larger key, so it can never win and is in neither set.

Resolve.  lambda_i = e_i / S: |dlambda_i| <= tl_i := (err_i + |lambda_i| errS) / (S - errS) + U |lambda_i|.
rgb_k = fma(l_2, c_2k, fma(l_1, c_1k, l_0 c_0k)): |drgb_k| <= sum tl_i |c_ik| + gamma_3 sum |lambda_i| |c_ik|.
Normal n = (b - a) x (c - a): 3 roundings on the absolute cross product Nn: eps := gamma_3 |Nn| / |n| is its relative vector
error; the squared length (3 roundings), the root, the reciprocal and the scaling add at most 6 U: |dn^_k| <= tn := 2 eps + 8 U.
The ray's unit vector is good to 8 U per component, the three-term dot product adds 3 U: |dcos| <= tc := 2 tn + 16 U; where
|cos| <= tc the direction of the flip is open.  shade = fma(1 - ambient, |cos|, ambient): (1 - ambient) tc + 2 U, and the product
with rgb adds U.
"""
import numpy as np

U = 2.0 ** -24


def gamma(k):
    return k * U / (1 - k * U)


# ---- vertex stage ---------------------------------------------------------------------------------------------------
def vertex_ref(vertices, link_ids, rotations, translations, scales, viewmats):
    """(verts_cam fp64 [C,V,3], bound [C,V,3]) of the fp32 arrays given."""
    x = np.asarray(vertices, np.float64)
    V = x.shape[0]
    xp, Xp = x.copy(), np.abs(x)
    L = 0 if rotations is None else len(rotations)
    if link_ids is not None and L:
        l = np.asarray(link_ids)
        mv = (l >= 0) & (l < L)
        R = np.asarray(rotations, np.float64)[l[mv]]
        t = np.asarray(translations, np.float64)[l[mv]]
        s = np.ones(L) if scales is None else np.asarray(scales, np.float64)
        s = s[l[mv]][:, None]
        xp[mv] = s * np.einsum("nkj,nj->nk", R, x[mv]) + t
        Xp[mv] = np.abs(s) * np.einsum("nkj,nj->nk", np.abs(R), np.abs(x[mv])) + np.abs(t)
    Vm = np.asarray(viewmats, np.float64)
    cam = np.einsum("ckj,vj->cvk", Vm[:, :3, :3], xp) + Vm[:, None, :3, 3]
    bound = gamma(8) * (np.einsum("ckj,vj->cvk", np.abs(Vm[:, :3, :3]), Xp) + np.abs(Vm[:, None, :3, 3]))
    assert cam.shape == (len(Vm), V, 3)
    return cam, bound


# ---- raster stage ---------------------------------------------------------------------------------------------------
def _cross(p, q):
    return np.stack([p[:, 1] * q[:, 2] - p[:, 2] * q[:, 1], p[:, 2] * q[:, 0] - p[:, 0] * q[:, 2],
                     p[:, 0] * q[:, 1] - p[:, 1] * q[:, 0]], 1)


def _abs_cross(p, q):
    p, q = np.abs(p), np.abs(q)
    return np.stack([p[:, 1] * q[:, 2] + p[:, 2] * q[:, 1], p[:, 2] * q[:, 0] + p[:, 0] * q[:, 2],
                     p[:, 0] * q[:, 1] + p[:, 1] * q[:, 0]], 1)


class FaceSetup:
    """Per face of one camera, fp64: oriented planes A, B, C [F,3] (e_i = A_i dx + B_i dy + C_i), their absolute versions
    for the error terms, |det|, errdet, sign, live (not dropped), box (x0, y0, x1, y1: where the face can be possible)."""

    def __init__(self, verts_cam, faces, K, width, height, near_plane=0.01, cull_backfaces=False, widen=3):
        vc, faces = np.asarray(verts_cam, np.float64), np.asarray(faces, np.int64)
        K = np.asarray(K, np.float64)
        F, V = len(faces), len(vc)
        self.F, self.width, self.height, self.K, self.near = F, int(width), int(height), K, float(near_plane)
        fx, fy, cx, cy = K[0, 0], K[1, 1], K[0, 2], K[1, 2]
        self.bad_index = ((faces < 0) | (faces >= V)).any(1)
        idx = np.where(self.bad_index[:, None], 0, faces)
        v = [vc[idx[:, i]] for i in range(3)]
        n, N = [], []
        for i in range(3):
            p, q = v[(i + 1) % 3], v[(i + 2) % 3]
            n.append(_cross(p, q - p))
            N.append(_abs_cross(p, q - p))
        n, N = np.stack(n, 1), np.stack(N, 1)                                   # [F,3 rows,3 xyz]
        with np.errstate(invalid="ignore", over="ignore"):
            det = (v[0] * n[:, 0]).sum(1)
            self.errdet = gamma(6) * (np.abs(v[0]) * N[:, 0]).sum(1)
        finite = np.isfinite(vc[idx]).all((1, 2)) & np.isfinite(n.astype(np.float32)).all((1, 2))
        self.sign = np.where(det < 0, -1.0, 1.0)
        self.absdet = np.abs(det)
        self.certain = self.absdet > self.errdet
        # a face that repeats an earlier face's index triple is the same computation with a larger key: it never wins
        _, first = np.unique(faces, axis=0, return_index=True)
        self.repeat = np.ones(F, bool)
        self.repeat[first] = False
        self.live = finite & ~self.bad_index & (det != 0) & ~self.repeat
        self.front = det < 0                                                      # the normal (b - a) x (c - a) faces the camera
        if cull_backfaces:
            self.live_certain = self.live & self.front & self.certain
            self.live = self.live & (self.front | ~self.certain)
        else:
            self.live_certain = self.live & self.certain
        s = self.sign[:, None]
        self.A, self.B, self.C = s * n[:, :, 0] / fx, s * n[:, :, 1] / fy, s * n[:, :, 2]
        self.NA, self.NB, self.NC = N[:, :, 0] / fx, N[:, :, 1] / fy, N[:, :, 2]
        self.verts = v
        # the box: projections of the triangle clipped to z = near, widened
        lo, hi = np.full((F, 2), np.inf), np.full((F, 2), -np.inf)
        f = np.array([fx, fy]); c0 = np.array([cx, cy])
        with np.errstate(all="ignore"):
            for i in range(3):
                p, q = v[i], v[(i + 1) % 3]
                pin, qin = p[:, 2] >= near_plane, q[:, 2] >= near_plane
                uv = f * p[:, :2] / p[:, 2:3] + c0
                lo = np.where(pin[:, None], np.minimum(lo, uv), lo)
                hi = np.where(pin[:, None], np.maximum(hi, uv), hi)
                t = (near_plane - p[:, 2]) / (q[:, 2] - p[:, 2])
                x = p + t[:, None] * (q - p)
                uv = f * x[:, :2] / near_plane + c0
                cr = (pin != qin)[:, None]
                lo = np.where(cr, np.minimum(lo, uv), lo)
                hi = np.where(cr, np.maximum(hi, uv), hi)
        self.live &= np.isfinite(lo).all(1) & np.isfinite(hi).all(1)
        self.live_certain &= self.live
        lo = np.where(self.live[:, None], lo, 0.0); hi = np.where(self.live[:, None], hi, -1.0)
        wh = np.array([width - 1, height - 1])
        self.box_lo = np.clip(np.floor(np.clip(lo, -10, wh + 10)) - widen, 0, None).astype(np.int64)
        self.box_hi = np.minimum(np.floor(np.clip(hi, -10, wh + 10)) + widen, wh).astype(np.int64)
        self.live &= (self.box_lo <= self.box_hi).all(1)


class RasterRef:
    """All (pixel, face) pairs at which a face is possible, and the per-pixel verdicts.  Flat arrays over pairs, sorted by
    (pixel, face): pix, face, e [n,3], err [n,3], S, errS, z, tolz, possible, certain, exact (the fp64 rule itself)."""

    def __init__(self, verts_cam, faces, K, width, height, near_plane=0.01, far_plane=1e10, cull_backfaces=False):
        self.setup = st = FaceSetup(verts_cam, faces, K, width, height, near_plane, cull_backfaces)
        self.width, self.height, self.near, self.far = int(width), int(height), float(near_plane), float(far_plane)
        W, H = self.width, self.height
        cx, cy = st.K[0, 2], st.K[1, 2]
        live = np.flatnonzero(st.live)
        side = np.maximum(st.box_hi[live] - st.box_lo[live] + 1, 1).max(1) if len(live) else np.zeros(0, np.int64)
        cls = np.ceil(np.log2(np.maximum(side, 4))).astype(np.int64) if len(live) else side
        out = {k: [] for k in ("pix", "face", "e", "err", "S", "errS")}
        for c in np.unique(cls):
            fs, s = live[cls == c], 1 << int(c)
            step = max(1, (1 << 21) // (s * s))
            ar = np.arange(s)
            for k in range(0, len(fs), step):
                ff = fs[k:k + step]
                x = st.box_lo[ff, 0][:, None, None] + ar[None, None, :]
                y = st.box_lo[ff, 1][:, None, None] + ar[None, :, None]
                ok = (x <= st.box_hi[ff, 0][:, None, None]) & (y <= st.box_hi[ff, 1][:, None, None])
                dx, dy = (x + 0.5) - cx, (y + 0.5) - cy
                e = [st.A[ff, i][:, None, None] * dx + st.B[ff, i][:, None, None] * dy + st.C[ff, i][:, None, None] for i in range(3)]
                err = [gamma(8) * (st.NA[ff, i][:, None, None] * np.abs(dx) + st.NB[ff, i][:, None, None] * np.abs(dy)
                                   + st.NC[ff, i][:, None, None]) for i in range(3)]
                S = e[0] + e[1] + e[2]
                ok = ok & (S > 0) & (e[0] >= -err[0]) & (e[1] >= -err[1]) & (e[2] >= -err[2])
                fi, yi, xi = np.nonzero(ok)
                sel = (fi, yi, xi)
                out["pix"].append((y[fi, yi, 0] * W + x[fi, 0, xi]).astype(np.int64))
                out["face"].append(ff[fi])
                out["e"].append(np.stack([ei[sel] for ei in e], 1))
                out["err"].append(np.stack([ei[sel] for ei in err], 1))
                out["S"].append(S[sel])
        cat = lambda k, shape: np.concatenate(out[k]) if out[k] else np.zeros(shape)
        pix, face = cat("pix", (0,)).astype(np.int64), cat("face", (0,)).astype(np.int64)
        e, err, S = cat("e", (0, 3)), cat("err", (0, 3)), cat("S", (0,))
        order = np.lexsort((face, pix))
        self.pix, self.face, self.e, self.err, self.S = pix[order], face[order], e[order], err[order], S[order]
        self.errS = self.err.sum(1) + 2 * U * np.abs(self.e).sum(1)
        self.z = st.absdet[self.face] / self.S
        with np.errstate(divide="ignore", invalid="ignore"):
            rel = st.errdet[self.face] / st.absdet[self.face] + self.errS / self.S + U
            self.tolz = np.where(rel < 1, self.z * rel / (1 - rel), np.inf)
        z, tz = self.z, self.tolz
        self.possible = (z >= self.near - tz) & (z <= self.far + tz)
        self.certain = ((self.e >= self.err).all(1) & st.live_certain[self.face] & (z >= self.near + tz) & (z <= self.far - tz))
        # the fp64 rule itself takes the fp64 orientation: an uncertain one only matters through the cull and through C
        self.exact = (self.e >= 0).all(1) & (z >= self.near) & (z <= self.far) & (st.front[self.face] if cull_backfaces else True)
        self.key = self.pix * max(st.F, 1) + self.face
        n_px = W * H
        # the fp64 winner: smallest (z, face) among exact pairs
        self.winner = np.full(n_px, -1, np.int64)
        self.zwin = np.zeros(n_px)
        ex = np.flatnonzero(self.exact)
        o = ex[np.lexsort((self.face[ex], self.z[ex], self.pix[ex]))]
        first = np.r_[True, self.pix[o][1:] != self.pix[o][:-1]] if len(o) else np.zeros(0, bool)
        self.win_pair = np.full(n_px, -1, np.int64)
        self.win_pair[self.pix[o][first]] = o[first]
        self.winner[self.pix[o][first]] = self.face[o][first]
        self.zwin[self.pix[o][first]] = self.z[o][first]
        # zfront(p) = min over C of z + tol_z
        self.zfront = np.full(n_px, np.inf)
        c = np.flatnonzero(self.certain)
        np.minimum.at(self.zfront, self.pix[c], (z + tz)[c])
        self.has_certain = np.isfinite(self.zfront)
        rival = self.possible & (z - tz <= self.zfront[self.pix])               # K(p)
        n_rival = np.bincount(self.pix[rival], minlength=n_px)
        n_rival_certain = np.bincount(self.pix[rival & self.certain], minlength=n_px)
        self.rival = rival
        self.by_tolerance = ~(((n_rival == 1) & (n_rival_certain == 1)) | (n_rival == 0))
        self.covered = self.winner >= 0

    def mask(self):
        return self.covered.reshape(self.height, self.width)

    def tolerance_share(self):
        """Pixels decided by tolerance over covered pixels."""
        return float(self.by_tolerance.sum()) / max(1, int(self.covered.sum()))

    def pair_of(self, pix, face):
        """Index of the pair (pix, face), -1 where the face is not possible there."""
        key = np.asarray(pix, np.int64) * max(self.setup.F, 1) + np.asarray(face, np.int64)
        at = np.searchsorted(self.key, key)
        at = np.minimum(at, max(len(self.key) - 1, 0))
        hit = (self.key[at] == key) if len(self.key) else np.zeros(len(key), bool)
        return np.where(hit, at, -1)

    def check_raster(self, face_ids, depth):
        """The acceptance rule on a kernel's face ids and depth [H,W].  Returns dict(pairs = the winner's pair per covered
        pixel, ratios and counts); raises AssertionError with the first offending pixels."""
        g = np.asarray(face_ids).reshape(-1).astype(np.int64)
        d = np.asarray(depth, np.float64).reshape(-1)
        n_px = self.width * self.height
        assert g.shape == (n_px,) and d.shape == (n_px,)

        def fail(what, bad):
            p = np.flatnonzero(bad)[:5]
            raise AssertionError(f"{what}: {int(bad.sum())} pixels, first (x, y, face, ref): "
                                 f"{[(int(q % self.width), int(q // self.width), int(g[q]), int(self.winner[q])) for q in p]}")
        none = g < 0
        if (none & self.has_certain).any():
            fail("uncovered where a face is certain", none & self.has_certain)
        if (d[none] != 0).any():
            fail("depth not 0 where uncovered", none & (d != 0))
        cov = np.flatnonzero(~none)
        pr = self.pair_of(cov, g[cov])
        bad = np.zeros(n_px, bool)
        bad[cov] = (pr < 0) | ~self.possible[np.maximum(pr, 0)]
        if bad.any():
            fail("the winner is not a possible face", bad)
        zg, tg = self.z[pr], self.tolz[pr]
        bad[cov] = zg - tg > self.zfront[cov]
        if bad.any():
            fail("the winner is behind a certain face by more than tol_z", bad)
        with np.errstate(invalid="ignore"):
            ratio = np.where(np.isfinite(tg), np.abs(d[cov] - zg) / tg, 0.0)
        bad[cov] = ratio > 1
        if bad.any():
            fail(f"depth off by more than tol_z (worst ratio {ratio.max():.3g})", bad)
        strict = ~self.by_tolerance
        if (g[strict] != self.winner[strict]).any():
            fail("face id differs where the pixel is not decided by tolerance", strict & (g != self.winner))
        return {"pixels": cov, "pairs": pr, "depth_ratio": float(ratio.max()) if len(ratio) else 0.0,
                "by_tolerance": int(self.by_tolerance.sum()), "covered": int(self.covered.sum()),
                "differs": int((g != self.winner).sum())}

    # ---- resolve ------------------------------------------------------------------------------------------------------
    def shade_ref(self, pairs, pixels, faces, vertex_colors=None, face_colors=None, headlight=False, ambient=0.3):
        """For the winner pairs of check_raster: dict(rgb, tol_rgb, normal, tol_normal, flip_open) in fp64, per covered pixel."""
        st = self.setup
        f = self.face[pairs]
        faces = np.asarray(faces, np.int64)
        lam = self.e[pairs] / self.S[pairs, None]
        S, eS = self.S[pairs], self.errS[pairs]
        tl = (self.err[pairs] + np.abs(lam) * eS[:, None]) / (S - eS)[:, None] + U * np.abs(lam)
        n_p = len(pairs)
        if vertex_colors is not None:
            col = np.asarray(vertex_colors, np.float64)[faces[f]]                       # [n,3 verts,3 rgb]
            rgb = (lam[:, :, None] * col).sum(1)
            tol = (tl[:, :, None] * np.abs(col)).sum(1) + gamma(3) * (np.abs(lam)[:, :, None] * np.abs(col)).sum(1)
        elif face_colors is not None:
            rgb, tol = np.asarray(face_colors, np.float64)[f], np.zeros((n_p, 3))
        else:
            rgb, tol = np.full((n_p, 3), float(np.float32(0.7))), np.zeros((n_p, 3))
        a, b, c = (v[f] for v in st.verts)
        n, Nn = _cross(b - a, c - a), _abs_cross(b - a, c - a)
        ln = np.linalg.norm(n, axis=1)
        nh = n / ln[:, None]
        tn = 2 * gamma(3) * np.linalg.norm(Nn, axis=1) / ln + 8 * U
        x, y = pixels % self.width, pixels // self.width
        ray = np.stack([((x + 0.5) - st.K[0, 2]) / st.K[0, 0], ((y + 0.5) - st.K[1, 2]) / st.K[1, 1], np.ones(n_p)], 1)
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


# ---- scenes of the tests (seeded) ---------------------------------------------------------------------------------------
def pinhole(width, height, f=None):
    f = float(f if f is not None else 0.9 * max(width, height))
    return np.array([[f, 0, width / 2 + 0.25], [0, f * 1.0625, height / 2 - 0.125], [0, 0, 1]], np.float32)


def random_faces(n_faces, width, height, seed, z=(2.0, 6.0), size=0.12, K=None):
    """n_faces small triangles in camera space whose centres project into the image: (vertices [3 n,3] float32, faces)."""
    rng = np.random.default_rng(seed)
    K = pinhole(width, height) if K is None else K
    zc = rng.uniform(*z, n_faces)
    u, v = rng.uniform(0, width, n_faces), rng.uniform(0, height, n_faces)
    ctr = np.stack([(u - K[0, 2]) / K[0, 0] * zc, (v - K[1, 2]) / K[1, 1] * zc, zc], 1)
    verts = (ctr[:, None, :] + rng.normal(scale=size, size=(n_faces, 3, 3)) * zc[:, None, None] / 4).reshape(-1, 3)
    return verts.astype(np.float32), np.arange(3 * n_faces, dtype=np.int32).reshape(-1, 3)


def box_in_blocks(bx0, by0, nbx, nby, K, z=3.0):
    """A right triangle in camera space at depth z whose pixel box (widened by one pixel) touches exactly
    the 8x8 blocks bx0 .. bx0 + nbx - 1 by by0 .. by0 + nby - 1: its projected corners lie 2.2 .. 2.7 px inside those blocks, so
    that no edge runs through pixel centres."""
    u0, u1 = 8 * bx0 + 2.3, 8 * (bx0 + nbx) - 2.4
    v0, v1 = 8 * by0 + 2.2, 8 * (by0 + nby) - 2.7
    uv = np.array([[u0, v0], [u1, v0], [u0, v1]])
    return np.stack([(uv[:, 0] - K[0, 2]) / K[0, 0] * z, (uv[:, 1] - K[1, 2]) / K[1, 1] * z, np.full(3, z)], 1).astype(np.float32)


def raster_cases(width, height):
    """name -> dict(verts float32 [V,3] (camera space: the tests view them through the identity), faces int32 [F,3], K, and
    optionally near, far, cull).  The cases a raster stage is to be run through; tests/test_mesh_host.py holds the reference
    itself to the tolerance cap on them."""
    K = pinhole(width, height)
    cases = {}
    for n in (1, 63, 64, 65, 129):
        v, f = random_faces(n, width, height, seed=100 + n, K=K)
        cases[f"random{n}"] = dict(verts=v, faces=f)
    # one triangle over the whole image (large-face path) in front of and behind 64 small ones
    v, f = random_faces(64, width, height, seed=7, K=K, z=(2.0, 6.0))
    big = np.array([[-40, -30, 4.0], [40, -30, 4.0], [0, 50, 4.0]], np.float32)
    cases["full_image_plus_64"] = dict(verts=np.concatenate([big, v]), faces=np.concatenate([[[0, 1, 2]], f + 3]).astype(np.int32))
    # faces whose boxes touch 14, 15 and 16 blocks of 8 x 8 pixels (around a rasteriser's large-face threshold), overlapping,
    # at three depths
    shapes = [s for s in ((2, 7), (3, 5), (4, 4)) if 8 * s[0] <= width and 8 * s[1] <= height]
    if len(shapes) == 3:
        v = np.concatenate([box_in_blocks(1 + i, 0, nbx, nby, K, z=3.0 + i) for i, (nbx, nby) in enumerate(shapes)])
        cases["threshold_blocks"] = dict(verts=v, faces=np.arange(9, dtype=np.int32).reshape(3, 3), blocks=[14, 15, 16])
    cases["crosses_near"] = dict(verts=np.array([[-0.5, -0.3, 2.0], [0.6, -0.2, 2.5], [0.1, 0.4, -1.0]], np.float32),
                                 faces=np.array([[0, 1, 2]], np.int32), near=0.5)
    cases["behind_offscreen_degenerate"] = dict(
        verts=np.array([[-0.5, -0.3, -2.0], [0.6, -0.2, -2.5], [0.1, 0.4, -1.0],            # 0..2 wholly behind the camera
                        [100, 0, 2.0], [101, 0, 2.0], [100, 1, 2.0],                          # 3..5 wholly off-screen
                        [0, 0, 2.0], [0.25, 0.25, 2.0], [0.5, 0.5, 2.0],                      # 6..8 colinear
                        [0, 0, 1.0], [0, 0, 2.0], [1, 0, 3.0],                                # 9..11 in a plane through the eye
                        [-0.2, -0.2, 3.0], [0.3, -0.2, 3.0], [-0.2, 0.3, 3.0]], np.float32),  # 12..14 an honest face
        faces=np.array([[0, 1, 2], [3, 4, 5], [6, 7, 8], [6, 6, 8], [9, 10, 11], [12, 13, 14]], np.int32), only_face=5)
    v, f = random_faces(20, width, height, seed=11, K=K)
    cases["identical_pairs"] = dict(verts=v, faces=np.repeat(f, 2, axis=0), identical=True)
    v, f = random_faces(30, width, height, seed=12, K=K)
    f2 = f.copy()
    f2[::3, 2] = len(v)                                                                       # every third face names vertex V
    cases["index_equal_V"] = dict(verts=v, faces=f2, bad_index=True)
    v, f = random_faces(65, width, height, seed=13, K=K)
    cases["cull_off"] = dict(verts=v, faces=f, cull=False)
    cases["cull_on"] = dict(verts=v, faces=f, cull=True)
    for c in cases.values():
        c.setdefault("K", K), c.setdefault("near", 0.01), c.setdefault("far", 1e10), c.setdefault("cull", False)
    return cases
