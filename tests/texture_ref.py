"""How a textured triangle mesh is shaded, in fp64 (NumPy), with the bounds an fp32 evaluation in the order stated below can
be held to: the statement csrc/mesh_texture.h is built and tested against, beside tests/mesh_ref.py (which it imports and
leaves as it is: coverage, depth, face ids, barycentrics, tint, normal and headlight shade are mesh_ref's).  Every bound is
a count of roundings, none is tuned to an output.  U = 2^-24, gamma_k as in mesh_ref.

Data.  A texture is uint8 [h,w,4]; an RGB image gets alpha 255; alpha is carried and ignored (the layer is opaque).  It is
stored as one little-endian 32-bit word per texel (byte 0 red), row-major, row 0 at the top.  Texel values are used as they
are, byte / 255: splat colours here are display-referred, so nothing is linearised (no sRGB decode), and mip levels are
averaged in that same space.  Per texture wrap_s, wrap_t in {repeat, clamp, mirror} (glTF 10497 / 33071 / 33648).  Per face
face_uvs float32 [F,3,2], one uv per corner (an OBJ seam and a glTF vertex are the same data), origin top-left, v down (the
glTF convention; OBJ's vt is flipped at load), and face_textures int32 [F]: a value outside 0 .. T-1 means "not textured".

Mip chain.  Level l is max(1, w >> l) x max(1, h >> l); 1 + floor(log2(max(w, h))) levels; texel (x, y) of level l+1 is per
byte (s00 + s01 + s10 + s11 + 2) >> 2 of level l's texels at columns min(2x, w_l - 1), min(2x + 1, w_l - 1) and rows likewise.
Integer arithmetic: the same bytes everywhere (mip_chain below is compared bit for bit).

Evaluation order (fp32) at the winning face, with mesh_ref's e_i, S, lambda_i = e_i / S, A_i, B_i:
    u = fma(l2, u2, fma(l1, u1, l0 u0)), v alike.
    trilinear only: sA = (A0 + A1) + A2, uA = fma(u2, A2, fma(u1, A1, u0 A0)), du/dx = fma(-u, sA, uA) / S; with B for y; v alike.
      (d e_i / dx = A_i, so d(e_i / S)/dx = (A_i - lambda_i sA) / S and du/dx = (sum u_i A_i - u sum A_i) / S: analytic, not
      taken from neighbouring pixels.)  ax = w du/dx, bx = h dv/dx, ay, by alike (level-0 texels per pixel);
      rho^2 = max(fma(bx, bx, ax ax), fma(by, by, ay ay)); lod = min(0.5 log2(rho^2), L - 1) if rho^2 > 1, else 0 (which
      covers a NaN).
    wrap, in floating point before any scaling, so that no large value reaches an integer conversion:
      repeat u' = u - floor(u); mirror t = fma(-2, floor(0.5 u), u), u' = 1 - |t - 1|; clamp u' = min(max(u, 0), 1).
    per level: x = fma(u', w_l, -0.5), i0 = floor(x), f = x - i0 (exact), i1 = i0 + 1; i0, i1 modulo w_l for repeat, clamped
      to 0 .. w_l - 1 for clamp and mirror; rows alike.  In byte units: top = fma(fx, t01 - t00, t00), bot = fma(fx, t11 - t10,
      t10), c = fma(fy, bot - top, top).
    bilinear: level 0.  trilinear: l0 = floor(lod), l1 = min(l0 + 1, L - 1), g = lod - l0, c = fma(g, c_l1 - c_l0, c_l0) (g = 0
      returns c_l0's bits, so the second level need not be fetched).
    rgb = (c * (1 / 255)) * tint, tint = the interpolated vertex colour or the face colour where the mesh has one, else 1
      (glTF's COLOR_0 x texture); then mesh_ref's headlight shade.
A pixel whose face is not textured, or whose u or v (or, trilinear, one of the four derivatives) is not finite, is shaded
exactly as mesh_ref's resolve shades it (tint 0.7 grey where the mesh has no colours).

Bounds.  Bilinear and trilinear sampling are continuous in u, v and lod -- across floor flips and wrap seams too (at a repeat
seam x = -0.5 and x = w - 0.5 both give the mean of texels w - 1 and 0; at lod = k both sides give level k) -- so an error in
u, v, lod moves the colour by at most that error times a local slope, and no flip bookkeeping is needed.
  du  <= sum tl_i |u_i| + gamma_3 sum |lambda_i| |u_i|, tl_i mesh_ref's bound on lambda_i.
  wrap: repeat rounds once on a value <= 1: U.  mirror: 0.5 u and floor are exact, the fma rounds a value <= 2, t - 1 and 1 - |.|
        round values <= 1: 4 U.  clamp: 0.
  scale: x = fma(u', w_l, -0.5) rounds once, |x| <= w_l: in texels of level l, dx_l <= w_l (du + wrap) + U w_l.
  slope: inside a cell the bilinear surface's x-slope is a mean of two horizontal texel differences; an error below one texel
        can reach the neighbouring cell, so D_l = the largest difference between horizontally (vertically for y) adjacent
        texels in the footprint widened by one texel each way (4 x 4 texels: the 3 x 3 cells around the footprint), per
        channel.  e_l = dx_l Dx_l + dy_l Dy_l, and 1 (everything) where dx_l or dy_l exceeds one texel.
  derivatives: |dA_i| <= gamma_5 NA_i (mesh_ref), so uA carries gamma_8 sum |u_i| NA_i and sA gamma_7 sum NA_i; the numerator
        n = fma(-u, sA, uA), where the two terms cancel, carries e_n = gamma_8 sum |u_i| NA_i + du |sA| + |u| gamma_7 sum NA_i +
        U (|uA| + |u sA|) absolutely; d(du/dx) <= e_n / (S - errS) + |du/dx| (errS / (S - errS) + U).  ax = w du/dx adds U |ax|.
  rho:  |d|s_x|| <= hypot(e_ax, e_bx) + 2 U |s_x| (the squares, the fma and the half of the log's argument), drho the larger of
        the two; dlod = log2 max(rho + drho, 1) - log2 max(rho - drho, 1), both clamped to L - 1 (that is the relative error
        of rho over ln 2, and it is 0 while rho + drho <= 1) + 4 U (L - 1) for a log2f good to 2 ulp + U.
  lod slope: |c_{k+1} - c_k| at (u, v), the largest over the level pairs from l0 - 1 to l1 + 1 (an error in lod may step over
        an integer); uv slope: the largest e_l over those levels.
  lerps: each fma rounds a value <= 255; top, bot: 1 each; c: bot - top and the fma on inputs off by U 255: <= 6 U 255; the
        level lerp the same again on top: <= 8 U 255; times 1 / 255 (rounded) and its product: 10 U in 0 .. 1 units.
  tc = e_uv + dlod * slope + 10 U (at most 1).  rgb before the shade: tc |tint| + c ttint + tc ttint + U |c tint|; the shade as in
  mesh_ref.  A pixel mesh_ref calls "decided by tolerance" is skipped for colour, as the resolve checks do.
Cap (a condition on the test scenes, asserted without a GPU): at most 5 % of textured covered pixels may have a colour bound
above 4 / 255; above that the check says little.
"""
import numpy as np

import mesh_ref as MR

U, gamma = MR.U, MR.gamma
FLT_MAX = 3.4028234663852886e38
REPEAT, CLAMP, MIRROR = "repeat", "clamp", "mirror"
CAP_TOL, CAP_SHARE = 4.0 / 255.0, 0.05


def rgba(image):
    """uint8 [h,w,4] of a uint8 [h,w,3|4] image: alpha 255 where it has none."""
    image = np.asarray(image)
    assert image.dtype == np.uint8 and image.ndim == 3 and image.shape[2] in (3, 4)
    if image.shape[2] == 3:
        image = np.concatenate([image, np.full(image.shape[:2] + (1,), 255, np.uint8)], 2)
    return np.ascontiguousarray(image)


def n_levels(w, h):
    return 1 + int(np.floor(np.log2(max(w, h))))


def mip_chain(image):
    """[level 0, level 1, ..] uint8 [h_l,w_l,4] of a uint8 image."""
    levels = [rgba(image)]
    h, w = levels[0].shape[:2]
    for l in range(1, n_levels(w, h)):
        s = levels[-1].astype(np.uint32)
        sh, sw = s.shape[:2]
        dh, dw = max(1, h >> l), max(1, w >> l)
        x0, x1 = np.minimum(2 * np.arange(dw), sw - 1), np.minimum(2 * np.arange(dw) + 1, sw - 1)
        y0, y1 = np.minimum(2 * np.arange(dh), sh - 1), np.minimum(2 * np.arange(dh) + 1, sh - 1)
        acc = s[y0][:, x0] + s[y0][:, x1] + s[y1][:, x0] + s[y1][:, x1] + 2
        levels.append((acc >> 2).astype(np.uint8))
        assert levels[-1].shape == (dh, dw, 4)
    return levels


def pack_words(image):
    """The little-endian 32-bit words of a uint8 [h,w,4] image, [h,w] uint32."""
    return rgba(image).view("<u4")[..., 0]


def wrap(u, mode):
    if mode == CLAMP:
        return np.clip(u, 0.0, 1.0)
    if mode == MIRROR:
        t = u - 2.0 * np.floor(0.5 * u)
        return 1.0 - np.abs(t - 1.0)
    return u - np.floor(u)


WRAP_ROUNDINGS = {REPEAT: 1, CLAMP: 0, MIRROR: 4}


def _index(i, side, mode):
    return np.mod(i, side) if mode == REPEAT else np.clip(i, 0, side - 1)


def sample_level(level, u01, v01, wrap_s, wrap_t):
    """Bilinear sample of one level (uint8 [h,w,4]) at wrapped coordinates [n]: (c [n,3] in 0 .. 1, Dx, Dy [n,3]: the largest
    difference between horizontally / vertically adjacent texels in the footprint widened by one texel, in 0 .. 1)."""
    h, w = level.shape[:2]
    t = level[..., :3].astype(np.float64) / 255.0
    x, y = u01 * w - 0.5, v01 * h - 0.5
    i0, j0 = np.floor(x).astype(np.int64), np.floor(y).astype(np.int64)
    fx, fy = (x - i0)[:, None], (y - j0)[:, None]
    cols = np.stack([_index(i0 + d, w, wrap_s) for d in (-1, 0, 1, 2)], 1)           # [n,4]
    rows = np.stack([_index(j0 + d, h, wrap_t) for d in (-1, 0, 1, 2)], 1)
    patch = t[rows[:, :, None], cols[:, None, :]]                                      # [n,4 rows,4 cols,3]
    top = patch[:, 1, 1] + fx * (patch[:, 1, 2] - patch[:, 1, 1])
    bot = patch[:, 2, 1] + fx * (patch[:, 2, 2] - patch[:, 2, 1])
    c = top + fy * (bot - top)
    Dx = np.abs(np.diff(patch, axis=2)).max((1, 2))
    Dy = np.abs(np.diff(patch, axis=1)).max((1, 2))
    return c, Dx, Dy


def _finite32(x):
    with np.errstate(invalid="ignore"):
        return np.abs(x) <= FLT_MAX


def texel_ref(R, pairs, face_uvs, face_textures, textures, texture_filter):
    """For winner pairs of RasterRef R: dict(textured bool [n], c [n,3] the sampled colour in 0 .. 1, tc [n,3] its bound, u, v,
    lod [n]) -- c = 1, tc = 0 where not textured.  textures: list of (image uint8 [h,w,3|4], wrap_s, wrap_t)."""
    assert texture_filter in ("bilinear", "trilinear")
    st = R.setup
    f = R.face[pairs]
    n = len(pairs)
    T = len(textures)
    tid = np.asarray(face_textures, np.int64)[f]
    uv = np.asarray(face_uvs, np.float32).astype(np.float64)[f]                       # [n,3 corners,2]
    S, eS, e, err = R.S[pairs], R.errS[pairs], R.e[pairs], R.err[pairs]
    lam = e / S[:, None]
    tl = (err + np.abs(lam) * eS[:, None]) / (S - eS)[:, None] + U * np.abs(lam)
    out = dict(textured=np.zeros(n, bool), c=np.ones((n, 3)), tc=np.zeros((n, 3)), u=np.zeros(n), v=np.zeros(n), lod=np.zeros(n))
    with np.errstate(all="ignore"):
        coord = (lam[:, :, None] * uv).sum(1)                                         # [n,2]
        dcoord = (tl[:, :, None] * np.abs(uv)).sum(1) + gamma(3) * (np.abs(lam)[:, :, None] * np.abs(uv)).sum(1)
        ok = (tid >= 0) & (tid < T) & _finite32(coord).all(1) & np.isfinite(uv).all((1, 2))
        A, B, NA, NB = st.A[f], st.B[f], st.NA[f], st.NB[f]
        der, dder = np.zeros((n, 2, 2)), np.zeros((n, 2, 2))                          # [n, x|y, u|v]
        for k, (P, NP) in enumerate(((A, NA), (B, NB))):
            sP, sNP = P.sum(1), NP.sum(1)
            for j in range(2):
                uP = (uv[:, :, j] * P).sum(1)
                num = uP - coord[:, j] * sP
                e_num = (gamma(8) * (np.abs(uv[:, :, j]) * NP).sum(1) + dcoord[:, j] * np.abs(sP)
                         + np.abs(coord[:, j]) * gamma(7) * sNP + U * (np.abs(uP) + np.abs(coord[:, j] * sP)))
                der[:, k, j] = num / S
                dder[:, k, j] = e_num / (S - eS) + np.abs(num / S) * (eS / (S - eS) + U)
        if texture_filter == "trilinear":
            ok &= _finite32(der).all((1, 2))
    out["textured"], out["u"], out["v"] = ok, coord[:, 0], coord[:, 1]
    for t in np.unique(tid[ok]):
        sel = np.flatnonzero(ok & (tid == t))
        image, ws, wt = textures[t]
        chain = mip_chain(image)
        L = len(chain)
        h, w = chain[0].shape[:2]
        u, v, du, dv = coord[sel, 0], coord[sel, 1], dcoord[sel, 0], dcoord[sel, 1]
        with np.errstate(all="ignore"):
            uw, vw = wrap(u, ws), wrap(v, wt)
            du, dv = du + WRAP_ROUNDINGS[ws] * U, dv + WRAP_ROUNDINGS[wt] * U
        use = range(L) if texture_filter == "trilinear" else range(1)
        c_all, e_all = np.zeros((L, len(sel), 3)), np.zeros((L, len(sel), 3))
        for l in use:
            c_all[l], Dx, Dy = sample_level(chain[l], uw, vw, ws, wt)
            wl, hl = chain[l].shape[1], chain[l].shape[0]
            with np.errstate(all="ignore"):
                dx, dy = wl * du + U * wl, hl * dv + U * hl
                e_l = dx[:, None] * Dx + dy[:, None] * Dy
                e_all[l] = np.where(((dx <= 1) & (dy <= 1))[:, None], e_l, 1.0)
        if texture_filter == "bilinear":
            c, tc, lod = c_all[0], e_all[0], np.zeros(len(sel))
        else:
            wh = np.array([w, h], np.float64)
            with np.errstate(all="ignore"):
                s = der[sel] * wh                                                         # [m, x|y, (ax, bx)]
                es = dder[sel] * wh + U * np.abs(s)
                length = np.sqrt((s * s).sum(2))                                          # [m, x|y]
                dlen = np.sqrt((es * es).sum(2)) + 2 * U * length
                rho, drho = length.max(1), dlen.max(1)
                clampL = lambda r: np.clip(np.log2(np.maximum(r, 1.0)), 0.0, L - 1.0)
                lod = clampL(rho)
                dlod = clampL(rho + drho) - clampL(rho - drho) + 4 * U * (L - 1) + U
            la = np.floor(lod).astype(np.int64)
            lb = np.minimum(la + 1, L - 1)
            g = (lod - la)[:, None]
            m = np.arange(len(sel))
            c = c_all[la, m] + g * (c_all[lb, m] - c_all[la, m])
            lo, hi = np.maximum(la - 1, 0), np.minimum(lb + 1, L - 1)
            slope, e_uv = np.zeros((len(sel), 3)), np.zeros((len(sel), 3))
            for l in range(L):
                inside = ((l >= lo) & (l <= hi))[:, None]
                e_uv = np.maximum(e_uv, np.where(inside, e_all[l], 0.0))
                if l + 1 < L:
                    both = ((l >= lo) & (l + 1 <= hi))[:, None]
                    slope = np.maximum(slope, np.where(both, np.abs(c_all[l + 1] - c_all[l]), 0.0))
            tc = e_uv + dlod[:, None] * slope
        out["c"][sel], out["tc"][sel], out["lod"][sel] = c, np.minimum(tc + 10 * U, 1.0), lod
    return out


def shade_textured_ref(R, pairs, pixels, faces, face_uvs, face_textures, textures, texture_filter, vertex_colors=None,
                       face_colors=None, headlight=False, ambient=0.3):
    """RasterRef.shade_ref with textures: dict(rgb, tol_rgb, normal, tol_normal, flip_open, textured, lod) per covered pixel.
    Where not textured, rgb and tol_rgb are shade_ref's own."""
    plain = R.shade_ref(pairs, pixels, faces, vertex_colors=vertex_colors, face_colors=face_colors, headlight=headlight, ambient=ambient)
    tint = R.shade_ref(pairs, pixels, faces, vertex_colors=vertex_colors, face_colors=face_colors, headlight=False)
    tx = texel_ref(R, pairs, face_uvs, face_textures, textures, texture_filter)
    n = len(pairs)
    if vertex_colors is None and face_colors is None:
        t, tt = np.ones((n, 3)), np.zeros((n, 3))                                     # a textured face without colours: tint 1
    else:
        t, tt = tint["rgb"], tint["tol_rgb"]
    c, tc = tx["c"], tx["tc"]
    pre = c * t
    tpre = tc * np.abs(t) + np.abs(c) * tt + tc * tt + U * np.abs(pre)
    if headlight:
        # shade and its bound, read off shade_ref on a colour of exactly 1: rgb = shade, tol = tshade + U shade
        one = R.shade_ref(pairs, pixels, faces, face_colors=np.ones((len(faces), 3)), headlight=True, ambient=ambient)
        shade = one["rgb"]
        tshade = one["tol_rgb"] - U * shade
        tpre = tpre * shade + np.abs(pre) * tshade + U * np.abs(pre) * shade
        pre = pre * shade
    on = tx["textured"][:, None]
    out = dict(plain)
    out["rgb"], out["tol_rgb"] = np.where(on, pre, plain["rgb"]), np.where(on, tpre + 1e-300, plain["tol_rgb"])
    out["textured"], out["lod"] = tx["textured"], tx["lod"]
    return out


def check_textured_shading(R, r, faces, rgb, face_uvs, face_textures, textures, texture_filter, **shade):
    """Hold rgb [H,W,3] of one camera to shade_textured_ref at the winners check_raster returned, skipping the pixels decided
    by tolerance: error over bound <= 1, exact zeros where uncovered.  Returns dict(worst ratio, textured pixels, share over
    the cap's tolerance)."""
    ref = shade_textured_ref(R, r["pairs"], r["pixels"], faces, face_uvs, face_textures, textures, texture_filter, **shade)
    n_px = R.width * R.height
    rgb = np.asarray(rgb, np.float64).reshape(n_px, 3)
    un = np.ones(n_px, bool)
    un[r["pixels"]] = False
    assert (rgb[un] == 0).all(), "rgb is not exactly 0 where uncovered"
    strict = ~R.by_tolerance[r["pixels"]]
    ratio = np.abs(rgb[r["pixels"]] - ref["rgb"]) / ref["tol_rgb"]
    worst = float(ratio[strict].max()) if strict.any() else 0.0
    assert worst <= 1, f"{texture_filter}: rgb off its bound: worst ratio {worst:.3g}"
    return dict(worst=worst, textured=int((ref["textured"] & strict).sum()), over_cap=cap_share(ref, strict), ref=ref)


def cap_share(ref, strict=None):
    """Share of textured (strict) pixels whose colour bound is above CAP_TOL."""
    on = ref["textured"] if strict is None else ref["textured"] & strict
    return float((ref["tol_rgb"][on].max(1) > CAP_TOL).sum()) / max(1, int(on.sum()))


# ---- scenes of the tests (seeded) ---------------------------------------------------------------------------------------
def noise_checker(w, h, seed, cells=4):
    """uint8 [h,w,4]: band-limited noise (a few low-frequency cosines per channel) times a coarse checker."""
    rng = np.random.default_rng(seed)
    y, x = np.mgrid[0:h, 0:w]
    x, y = (x + 0.5) / w, (y + 0.5) / h
    img = np.zeros((h, w, 4))
    for ch in range(3):
        acc = np.zeros((h, w))
        for _ in range(4):
            kx, ky = rng.integers(0, 3, 2)
            acc += rng.uniform(0.3, 1.0) * np.cos(2 * np.pi * (kx * x + ky * y) + rng.uniform(0, 2 * np.pi))
        img[..., ch] = 0.5 + 0.1 * acc
    check = ((np.floor(x * cells) + np.floor(y * cells)) % 2).astype(np.float64)
    img[..., :3] *= (0.55 + 0.45 * check)[..., None]
    img[..., 3] = rng.uniform(0, 1, (h, w))                                           # alpha: carried, ignored
    return np.clip(np.round(img * 255), 0, 255).astype(np.uint8)


def scene_textures(wraps=(REPEAT, CLAMP, MIRROR)):
    """The three textures of the random scenes: 1 x 1, 5 x 3 and 64 x 32, one wrap mode each (both axes)."""
    sizes = ((1, 1), (5, 3), (64, 32))
    return [(noise_checker(w, h, 40 + k), wraps[k], wraps[(k + 1) % 3]) for k, (w, h) in enumerate(sizes)]


def random_textured_scene(width, height, n_faces=129, seed=229, untextured_every=0):
    """MR.random_faces with per-corner uvs uniform in [-2, 3] and a texture id per face in 0 .. 2 (every untextured_every-th
    face -1): dict(verts, faces, K, face_uvs, face_textures)."""
    K = MR.pinhole(width, height)
    verts, faces = MR.random_faces(n_faces, width, height, seed=seed, K=K)
    rng = np.random.default_rng(seed + 1)
    uvs = rng.uniform(-2.0, 3.0, (n_faces, 3, 2)).astype(np.float32)
    ids = rng.integers(0, 3, n_faces).astype(np.int32)
    if untextured_every:
        ids[::untextured_every] = -1
    return dict(verts=verts, faces=faces, K=K, face_uvs=uvs, face_textures=ids)


def quad(K, width, height, z=3.0, z_right=None, uv_scale=(1.0, 1.0)):
    """Two triangles whose projection covers the pixel rectangle 0 .. width x 0 .. height exactly, at depth z (z_right: the
    depth of the right edge, a quad tilted in depth), uv = (0, 0) at the top-left pixel corner and uv_scale at the bottom-right:
    dict(verts [4,3], faces [2,3], face_uvs [2,3,2], corner_uv [4,2])."""
    zr = z if z_right is None else z_right
    px = np.array([[0, 0], [width, 0], [width, height], [0, height]], np.float64)
    zs = np.array([z, zr, zr, z], np.float64)
    verts = np.stack([(px[:, 0] - K[0, 2]) / K[0, 0] * zs, (px[:, 1] - K[1, 2]) / K[1, 1] * zs, zs], 1).astype(np.float32)
    cuv = np.array([[0, 0], [uv_scale[0], 0], [uv_scale[0], uv_scale[1]], [0, uv_scale[1]]], np.float32)
    faces = np.array([[0, 1, 2], [0, 2, 3]], np.int32)
    return dict(verts=verts, faces=faces, face_uvs=cuv[faces], corner_uv=cuv)
