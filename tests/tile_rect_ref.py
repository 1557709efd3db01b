"""Cases and the fp64 reference for the tile rectangles of robosimgs_amd/csrc/tile_rect.h (tile_rect, tighten_rect,
pack_tile_rect).  A helper module, not a test file: tests/test_tile_rect_host.py holds a g++ build of the header to it on
the CPU, tests/test_gpu_tile_rect.py the kernels that run it (tile_count_kernel, the seed of project_color_fwd_kernel).
Pure numpy; reads nothing outside tests/.

A case is what the rule receives, in fp32: mean (mx, my), conic (a, b, c), opacity, an integer radius pair (rx, ry; equal
under the classic rule) and the tile grid.  Rectangles are int64 [n, 4] rows x0, y0, w, h in tiles.

The reference of the tightened rectangle is a SANDWICH, every quantity in fp64 from the fp32 inputs:
    Sigma = conic^-1,  thr = max(ln(255 o), 0),  slack and lim as the header writes them,  E_x = sqrt(lim Sigma_xx), E_y likewise,
    box(e) = the tiles of the classic rectangle that hold a pixel centre within mean +- e on both axes,
    box(E)  is inside  tight  is inside  box(1.001 E + 0.02).
The outer margin is the code's own 1.0001 / 0.01 px widened for the fp32 rounding of det, 1 / det, logf and sqrtf (together
below 1e-5 relative on lim >= 0.1).  Where the fp32 path falls back (det <= 0, a <= 0, c <= 0, a NaN in mean or conic) the
answer is the classic rectangle exactly; below the gate 0.95 / 255 (or NaN opacity) it is empty.  A case whose fp64 determinant lies
within 1e-6 relative of zero may give either answer (`borderline`).
"""
import numpy as np

TILE = 16
T255 = np.float32(1.0 / 255.0)
GATE = np.float32(0.95) * T255           # the rule's opacity gate: the raster's own (raster_common.h cull_opacity_ok)
EMPTY_WORD = 1 << 20                     # kEmptyTileRect: width 1, count 0
PINNED_DEG = (0.0, 0.5, 1.0, 44.0, 45.0, 46.0, 89.0, 90.0)
FIELDS = ("mx", "my", "a", "b", "c", "op")
WHOLE_GRID_RADIUS = 20000


def _ulp_shift(v, steps):
    """fp32 v moved by steps in {-1, 0, 1} units in the last place."""
    v = v.astype(np.float32)
    up, dn = np.nextafter(v, np.float32(np.inf)), np.nextafter(v, np.float32(-np.inf))
    return np.where(steps > 0, up, np.where(steps < 0, dn, v)).astype(np.float32)


def cases(n, tile_w, tile_h, seed, per_axis=False, giant_every=48):
    """n cases on a tile_w x tile_h grid.
    Conics: eigenvalues up to 1 / 0.3 (the 2D covariance carries eps2d = 0.3) and down to 0.03 with ratios down to 1e-4,
    every fifth case at 1e-4; angles uniform, a quarter pinned to PINNED_DEG; every giant_every-th case has Sigma's long
    axis at 5 .. 2,000 px (thinned: such a case's classic rectangle is the whole grid); one case in 64 is degenerate
    (a or c <= 0, det < 0, all zero) and one in 2,048 has b = +-sqrt(a c) rounded to fp32 (det within rounding of zero).
    Radii: ceil(3 sqrt(lambda_1)) of the generating covariance, or (per_axis) gsplat >= 1.5's extents ceil(e sqrt(Sigma_xx)),
    ceil(e sqrt(Sigma_yy)) with e = min(3.33, sqrt(2 ln(255 o))) and nothing under 1/255; one case in 512 covers the
    whole grid whatever its conic, and every other one of those has an ellipse that does so too.
    Means: inside the image; on tile lines and on pixel centres, +- one ulp; up to 40 px outside a border; so far outside
    that the classic rectangle clamps to width 0; near the last column / row.
    Opacities: uniform; 1/255 and one ulp to either side; 0.999; 1.0; log-uniform in [1/255, 0.02]; uniform in
    [0.9 / 255, 1/255), across the gate; the gate and one ulp to either side.
    One case in 512 has a NaN in one field."""
    rng = np.random.default_rng(seed)
    W, H = float(TILE * tile_w), float(TILE * tile_h)
    idx = np.arange(n)
    # ---- conics
    l1 = 10.0 ** rng.uniform(-1.5, np.log10(1.0 / 0.3), n)
    ratio = 10.0 ** rng.uniform(-4.0, 0.0, n)
    ratio[::5] = 1e-4
    huge = idx % 1024 == 11                                     # an ellipse far larger than any grid: tight == classic
    l1 = np.where(huge, l1 * 1e-8, l1)
    l2 = l1 * ratio
    giant = (idx % giant_every == 7) & ~huge
    long_px = 10.0 ** rng.uniform(np.log10(5.0), np.log10(2000.0), n)
    g_l2 = 1.0 / long_px ** 2
    g_ratio = np.maximum(ratio, g_l2 * 0.3)                     # keeps the other eigenvalue at or under 1 / 0.3
    l2 = np.where(giant, g_l2, l2)
    l1 = np.where(giant, g_l2 / g_ratio, l1)
    th = rng.uniform(0.0, np.pi, n)
    pinned = rng.integers(0, 4, n) == 0
    th[pinned] = np.radians(np.array(PINNED_DEG)[rng.integers(0, len(PINNED_DEG), pinned.sum())])
    cs, sn = np.cos(th), np.sin(th)
    a, c, b = l1 * cs * cs + l2 * sn * sn, l1 * sn * sn + l2 * cs * cs, (l1 - l2) * cs * sn
    sxx, syy = c / (l1 * l2), a / (l1 * l2)                     # the generating covariance
    # ---- opacities
    op = rng.uniform(0.0, 1.0, n).astype(np.float32)
    ok = rng.integers(0, 14, n)
    op[ok == 0] = T255
    op[ok == 1] = np.nextafter(T255, np.float32(0.0))
    op[ok == 2] = np.nextafter(T255, np.float32(1.0))
    op[ok == 3] = np.float32(0.999)
    op[ok == 4] = np.float32(1.0)
    near = (ok == 5) | (ok == 6)
    op[near] = (10.0 ** rng.uniform(np.log10(1.0 / 255.0), np.log10(0.02), near.sum())).astype(np.float32)
    op[near] = np.maximum(op[near], T255)
    sub = ok == 7
    op[sub] = np.minimum((rng.uniform(0.9, 1.0, sub.sum()) / 255.0).astype(np.float32), np.nextafter(T255, np.float32(0.0)))
    at_gate = ok == 8
    op[at_gate] = _ulp_shift(np.full(at_gate.sum(), GATE, np.float32), rng.integers(-1, 2, at_gate.sum()))
    nan_at = idx % 512 == 5
    nan_field = (idx // 512) % 6
    op[nan_at & (nan_field == 5)] = np.nan
    # ---- radii
    if per_axis:
        with np.errstate(all="ignore"):
            e = np.minimum(3.33, np.sqrt(np.maximum(2.0 * np.log(255.0 * op.astype(np.float64)), 0.0)))
        rx, ry = np.ceil(e * np.sqrt(sxx)), np.ceil(e * np.sqrt(syy))
        gone = ~(op >= T255) | ~(rx > 0) | ~(ry > 0)
        rx, ry = np.where(gone, 0, rx), np.where(gone, 0, ry)
    else:
        rx = ry = np.ceil(3.0 * np.sqrt(1.0 / l2))
    whole = (idx % 512 == 11) & (rx > 0)
    rx, ry = np.where(whole, WHOLE_GRID_RADIUS, rx), np.where(whole, WHOLE_GRID_RADIUS, ry)
    # ---- means
    kind = rng.integers(0, 10, n)
    mx, my = rng.uniform(0.0, W, n), rng.uniform(0.0, H, n)
    k3, k4, k5, k6, k7, k8 = (kind == k for k in (3, 4, 5, 6, 7, 8))
    mx[k3] = TILE * rng.integers(0, tile_w + 1, k3.sum())
    my[k4] = TILE * rng.integers(0, tile_h + 1, k4.sum())
    mx[k5] = rng.integers(0, TILE * tile_w, k5.sum()) + 0.5
    my[k5] = rng.integers(0, TILE * tile_h, k5.sum()) + 0.5
    side = rng.integers(0, 4, n)
    out = rng.uniform(0.0, 40.0, n)
    far_x, far_y = rx + rng.uniform(1.0, 100.0, n), ry + rng.uniform(1.0, 100.0, n)
    for s, (lo_x, lo_y) in enumerate(((True, None), (False, None), (None, True), (None, False))):
        m6, m7 = k6 & (side == s), k7 & (side == s)
        if lo_x is not None:
            mx[m6] = (-out if lo_x else W + out)[m6]
            my[m6] = rng.uniform(-40.0, H + 40.0, m6.sum())
            mx[m7] = (-far_x if lo_x else W + far_x)[m7]
        else:
            my[m6] = (-out if lo_y else H + out)[m6]
            mx[m6] = rng.uniform(-40.0, W + 40.0, m6.sum())
            my[m7] = (-far_y if lo_y else H + far_y)[m7]
    last_x, last_y = k8 & (side < 2), k8 & (side >= 2)
    mx[last_x] = rng.uniform(W - 48.0, W + 40.0, last_x.sum())
    my[last_y] = rng.uniform(H - 48.0, H + 40.0, last_y.sum())
    f = lambda v: np.ascontiguousarray(v, dtype=np.float32)
    mx, my = f(mx), f(my)
    mx = np.where(k3 | k5, _ulp_shift(mx, rng.integers(-1, 2, n)), mx)
    my = np.where(k4 | k5, _ulp_shift(my, rng.integers(-1, 2, n)), my)
    # ---- degenerate conics (the fallback) and the determinant's branch point
    a, b, c = f(a), f(b), f(c)
    deg = idx % 64 == 9
    dk = rng.integers(0, 6, n)
    sgn = np.where(rng.integers(0, 2, n) == 0, -1.0, 1.0)
    root = np.sqrt(a.astype(np.float64) * c.astype(np.float64))
    a = np.where(deg & (dk == 0), -a, a)
    c = np.where(deg & (dk == 1), -c, c)
    a = np.where(deg & (dk == 2), 0.0, a)
    b = np.where(deg & (dk == 3), sgn * root * 1.01, b)
    b = np.where(deg & (dk == 4), sgn * root * 1.001, b)
    zero = deg & (dk == 5)
    a, b, c = np.where(zero, 0.0, a), np.where(zero, 0.0, b), np.where(zero, 0.0, c)
    b = np.where(idx % 2048 == 9, sgn * root, b)
    z = dict(mx=f(mx), my=f(my), a=f(a), b=f(b), c=f(c), op=f(op))
    for i, k in enumerate(FIELDS[:5]):
        z[k][nan_at & (nan_field == i)] = np.nan
    z["rx"] = np.ascontiguousarray(rx, dtype=np.int32)
    z["ry"] = np.ascontiguousarray(ry, dtype=np.int32)
    z["tile_w"] = np.full(n, tile_w, np.int32)
    z["tile_h"] = np.full(n, tile_h, np.int32)
    return z


def concat(parts):
    return {k: np.ascontiguousarray(np.concatenate([p[k] for p in parts])) for k in parts[0]}


def take(z, sel):
    return {k: np.ascontiguousarray(v[sel]) for k, v in z.items()}


# ----------------------------------------------------------------------------------------------------------------------
# the reference
# ----------------------------------------------------------------------------------------------------------------------
def classic_rects(z, per_axis=True):
    """A.2 step 7 in fp32, as oracle.gs_oracle_np.tile_rects(dtype=np.float32) states it (the host test compares the two):
    mean +- radius in tiles, floor / ceil, clamped to the grid; per_axis=False takes rx on both axes.  A NaN bound counts
    as 0, which is what the float-to-int conversion of the GPU (and of x86) makes of it before the clamp."""
    f, ts = np.float32, np.float32(TILE)
    rx = z["rx"].astype(f) / ts
    ry = (z["ry"] if per_axis else z["rx"]).astype(f) / ts
    tx, ty = z["mx"] / ts, z["my"] / ts
    tw, th = z["tile_w"].astype(np.float64), z["tile_h"].astype(np.float64)
    with np.errstate(invalid="ignore"):
        cl = lambda v, hi: np.clip(np.nan_to_num(v.astype(np.float64), nan=0.0), 0.0, hi).astype(np.int64)
        x0, x1 = cl(np.floor(tx - rx), tw), cl(np.ceil(tx + rx), tw)
        y0, y1 = cl(np.floor(ty - ry), th), cl(np.ceil(ty + ry), th)
    r = np.stack([x0, y0, x1 - x0, y1 - y0], axis=1)
    r[~(z["rx"] > 0)] = 0
    return r


def extents_f64(z):
    """(det, E_x, E_y, lim): the header's formulas in fp64 on the fp32 inputs."""
    a, b, c, o = (z[k].astype(np.float64) for k in ("a", "b", "c", "op"))
    with np.errstate(all="ignore"):
        det = a * c - b * b
        sxx, syy = c / det, a / det
        thr = np.maximum(np.log(255.0 * o), 0.0)
        e2 = 2.0 * (thr + 0.05) * (sxx + syy)
        slack = 0.05 + 8e-6 * (np.abs(a) + np.abs(c) + 2.0 * np.abs(b)) * (e2 + 512.0)
        lim = 2.0 * (thr + slack)
        return det, np.sqrt(lim * sxx), np.sqrt(lim * syy), lim


def branches(z):
    """Which answer the rule owes a case: dict of boolean masks culled (radius 0), low (opacity under the gate or NaN: empty),
    fallback (classic exactly), borderline (either), regular (the sandwich).  a > 0, c > 0 and opacity >= GATE are exact
    fp32 compares; the determinant's sign is taken in fp64 and is borderline within 1e-6 of |a c| + b^2 of zero."""
    a, b, c = (z[k].astype(np.float64) for k in ("a", "b", "c"))
    culled = ~(z["rx"] > 0)
    low = ~(z["op"] >= GATE) & ~culled
    nan_geo = np.isnan(z["mx"]) | np.isnan(z["my"]) | np.isnan(a) | np.isnan(b) | np.isnan(c)
    with np.errstate(invalid="ignore"):
        det = a * c - b * b
        rel = det / (np.abs(a * c) + b * b)
        sure_bad = nan_geo | ~(z["a"] > 0) | ~(z["c"] > 0)
        near = ~sure_bad & (np.abs(rel) <= 1e-6)
        fallback = (sure_bad | (~near & ~(det > 0))) & ~low & ~culled
    borderline = near & ~low & ~culled
    regular = ~(culled | low | fallback | borderline)
    return dict(culled=culled, low=low, fallback=fallback, borderline=borderline, regular=regular, nan_geo=nan_geo)


def box(z, classic, ex, ey):
    """The tiles of the classic rectangle that hold a pixel centre (i + 0.5) within mean +- (ex, ey): int64 [n, 4] as
    x0, y0, x1, y1 (exclusive) and a mask of the non-empty ones."""
    mx, my = z["mx"].astype(np.float64), z["my"].astype(np.float64)
    with np.errstate(invalid="ignore"):
        plx, phx = np.ceil(mx - ex - 0.5), np.floor(mx + ex - 0.5)
        ply, phy = np.ceil(my - ey - 0.5), np.floor(my + ey - 0.5)
        ok = (phx >= plx) & (phy >= ply)
        cx0, cy0 = classic[:, 0].astype(np.float64), classic[:, 1].astype(np.float64)
        cx1, cy1 = cx0 + classic[:, 2], cy0 + classic[:, 3]
        x0, x1 = np.maximum(cx0, np.floor(plx / TILE)), np.minimum(cx1, np.floor(phx / TILE) + 1.0)
        y0, y1 = np.maximum(cy0, np.floor(ply / TILE)), np.minimum(cy1, np.floor(phy / TILE) + 1.0)
        ok &= (x1 > x0) & (y1 > y0)
    r = np.stack([np.where(ok, v, 0.0) for v in (x0, y0, x1, y1)], axis=1).astype(np.int64)
    return r, ok


def _inside(inner, inner_ok, outer, outer_ok):
    """inner (x0, y0, x1, y1 + mask) lies inside outer."""
    fits = ((outer[:, 0] <= inner[:, 0]) & (outer[:, 1] <= inner[:, 1]) & (outer[:, 2] >= inner[:, 2])
            & (outer[:, 3] >= inner[:, 3]))
    return ~inner_ok | (outer_ok & fits)


def corners(rect):
    """x0, y0, w, h -> (x0, y0, x1, y1, non-empty mask)."""
    ok = (rect[:, 2] > 0) & (rect[:, 3] > 0)
    return np.stack([rect[:, 0], rect[:, 1], rect[:, 0] + rect[:, 2], rect[:, 1] + rect[:, 3]], axis=1), ok


def sandwich(z, tight, classic=None, outer_scale=1.001, outer_add=0.02):
    """Hold tightened rectangles `tight` [n, 4] to the reference.  Returns the masks of the cases that break a bound --
    bad_inner (box(E) not inside tight), bad_outer (tight not inside box(1.001 E + 0.02)), bad_fallback (not the classic
    rectangle exactly), bad_low (not empty), bad_culled (not 0 0 0 0), bad_either -- plus the branch masks and the boxes.  A borderline case must meet the fallback's
    answer or the sandwich."""
    classic = classic_rects(z) if classic is None else classic
    br = branches(z)
    _, ex, ey, _ = extents_f64(z)
    t, t_ok = corners(tight)
    inner, inner_ok = box(z, classic, ex, ey)
    outer, outer_ok = box(z, classic, outer_scale * ex + outer_add, outer_scale * ey + outer_add)
    bad_inner = ~_inside(inner, inner_ok, t, t_ok)
    bad_outer = ~_inside(t, t_ok, outer, outer_ok)
    is_classic = (tight == classic).all(axis=1)
    # A NaN mean coordinate gives the classic rectangle extent 0 on that axis already (count 0); the rule may then still
    # find the OTHER axis empty and zero both extents: the same corner, the same count of 0 -- the same record.
    nan_mean = np.isnan(z["mx"]) | np.isnan(z["my"])
    is_classic |= (nan_mean & (tight[:, :2] == classic[:, :2]).all(axis=1) & (classic[:, 2] * classic[:, 3] == 0)
                   & (tight[:, 2:] == 0).all(axis=1))
    either = br["borderline"] & ~is_classic & (bad_inner | bad_outer)
    return dict(br, bad_inner=bad_inner & br["regular"], bad_outer=bad_outer & br["regular"],
                bad_fallback=br["fallback"] & ~is_classic, bad_low=br["low"] & ((tight[:, 2] != 0) | (tight[:, 3] != 0)),
                bad_culled=br["culled"] & (tight != 0).any(axis=1), bad_either=either, outer_box=outer, outer_ok=outer_ok, inner_box=inner, inner_ok=inner_ok, classic=classic)


def unpack(words):
    """The packed record [n, 2] (x0 | y0 << 10 | max(w, 1) << 20, count) -> (x0, y0, stored width, count) as int64."""
    w = np.asarray(words).astype(np.int64) & 0xffffffff
    return w[:, 0] & 1023, (w[:, 0] >> 10) & 1023, w[:, 0] >> 20, w[:, 1]


def pack(rect):
    """pack_tile_rect in numpy: [n, 2] int64."""
    r = np.asarray(rect).astype(np.int64)
    return np.stack([r[:, 0] | (r[:, 1] << 10) | (np.maximum(r[:, 2], 1) << 20), r[:, 2] * r[:, 3]], axis=1)


def tile_min_sigma_f64(z, case, tx, ty):
    """fp64 minimum of sigma = 0.5 (a dx^2 + c dy^2) + b dx dy over the 16 x 16 pixel centres' rectangle of tile (tx, ty)
    for the (case, tile) pairs given as index arrays: zero when the mean lies inside, otherwise on an edge -- the clamped
    minimiser of the quadratic along that edge (the construction of test_cull_host._rect_min_fp64).  Needs a, c > 0."""
    a, b, c, mx, my = (z[k].astype(np.float64)[case] for k in ("a", "b", "c", "mx", "my"))

    def edge(e, wu, wv, lo, hi):
        v = np.clip(-b * e / wv, lo, hi)
        return 0.5 * (wu * e * e + wv * v * v) + b * e * v

    x0, y0 = TILE * tx + 0.5 - mx, TILE * ty + 0.5 - my
    x1, y1 = x0 + (TILE - 1.0), y0 + (TILE - 1.0)
    s = np.minimum(np.minimum(edge(x0, a, c, y0, y1), edge(x1, a, c, y0, y1)),
                   np.minimum(edge(y0, c, a, x0, x1), edge(y1, c, a, x0, x1)))
    return np.where((x0 <= 0) & (x1 >= 0) & (y0 <= 0) & (y1 >= 0), 0.0, s)


def tile_centres_min_sigma_f64(z, case, tx, ty):
    """The same minimum over the 256 pixel centres themselves, one by one: what the alpha test sees.  The rectangle's
    minimum above is a lower bound of it that a Gaussian smaller than a pixel, sitting between centres, does not meet."""
    a, b, c, mx, my = (z[k].astype(np.float64)[case][:, None] for k in ("a", "b", "c", "mx", "my"))
    k = np.arange(TILE * TILE)
    dx = (TILE * tx)[:, None] + (k % TILE)[None, :] + 0.5 - mx
    dy = (TILE * ty)[:, None] + (k // TILE)[None, :] + 0.5 - my
    return (0.5 * (a * dx * dx + c * dy * dy) + b * dx * dy).min(axis=1)


def dropped_pairs(classic, tight):
    """(case, tx, ty) of every tile in classic \\ tight, as three int64 arrays."""
    t, t_ok = corners(tight)
    cs, ts_x, ts_y = [], [], []
    for i in np.flatnonzero((classic[:, 2] > 0) & (classic[:, 3] > 0)):
        x0, y0, w, h = classic[i]
        gx, gy = np.meshgrid(np.arange(x0, x0 + w), np.arange(y0, y0 + h))
        keep = np.ones(gx.shape, bool)
        if t_ok[i]:
            keep = ~((gx >= t[i, 0]) & (gx < t[i, 2]) & (gy >= t[i, 1]) & (gy < t[i, 3]))
        cs.append(np.full(int(keep.sum()), i, np.int64)), ts_x.append(gx[keep]), ts_y.append(gy[keep])
    cat = lambda v: np.concatenate(v) if v else np.zeros(0, np.int64)
    return cat(cs), cat(ts_x).astype(np.int64), cat(ts_y).astype(np.int64)
