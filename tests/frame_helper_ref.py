"""fp64 statements of the kernels at the two ends of a data-generation frame -- composite_kernel, frame_to_u8_kernel
(csrc/composite.hip), points_sample_mask_kernel and points_project_kernel (csrc/points.hip), transform_kernel
(csrc/transform.hip) -- with the error bound each GPU test holds its kernel to, and the builders of the randomised
inputs those tests feed.  A helper module, not a test file: tests/test_frame_helpers_host.py checks the references on
closed-form cases and the inputs' caps without a GPU; the four GPU modules import the same builders, so the caps are
checked on the very arrays the kernels see.

U = 2^-24 is one fp32 rounding (unit roundoff), EPS32 = 2^-23 the spacing of fp32 at 1.  A bound "k U sum|terms|" is
the forward error of k chained roundings (gamma_k = k U / (1 - k U), whose second-order part the 1 % in GAMMA pays)."""
import functools

import numpy as np

U = 2.0 ** -24
EPS32 = 2.0 ** -23
GAMMA = 1.01 * U


# ---- composite_over ------------------------------------------------------------------------------------
def composite_rule(bg, a, zb, fg, zf, mask, backdrop):
    """include/mgs.h's rule, comparison by comparison (`a > 0` is false for NaN, and so on), in fp64:
      has_fg = mask != 0 if a mask is given (any numeric type), else 0 < zf < inf
      front  = has_fg and (not (a > 0) or zf <= zb)
      rgb    = front ? fg : bg + (1 - a) * (has_fg ? fg : backdrop)          depth = front ? zf : (a > 0 ? zb : +inf)
    bg, fg [...,3]; a, zb, zf [...]; backdrop three floats.  Returns (rgb, depth, front)."""
    bg, a, zb, fg, zf = (np.asarray(x, dtype=np.float64) for x in (bg, a, zb, fg, zf))
    with np.errstate(invalid="ignore"):
        has = (np.asarray(mask) != 0) if mask is not None else ((zf > 0) & (zf < np.inf))
        splats = a > 0
        front = has & (~splats | (zf <= zb))
        src = np.where(has[..., None], fg, np.asarray(backdrop, dtype=np.float64).reshape((1,) * a.ndim + (3,)))
        rgb = np.where(front[..., None], fg, bg + (1 - a)[..., None] * src)
    depth = np.where(front, zf, np.where(splats, zb, np.inf))
    return rgb, depth, front


def composite_blend_bound(bg, a, fg_or_backdrop):
    """A blended channel is b + (1 - a) f in fp32: three roundings, each of a quantity no larger than |b| + |f| for a in
    [0, 1]: 3 U (|b| + |f|) <= 2 EPS32 (|b| + |f|), the bound the tests use."""
    return 2 * EPS32 * (np.abs(np.asarray(bg, dtype=np.float64)) + np.abs(np.asarray(fg_or_backdrop, dtype=np.float64)))


COMPOSITE_ROWS = ("front: no splats", "front: nearer", "behind", "no fg, splats", "no fg, no splats")


def composite_rows(a, zb, zf, mask):
    """Which row of the truth table each pixel is (index into COMPOSITE_ROWS)."""
    z3 = np.zeros(np.shape(a) + (3,))
    _, _, front = composite_rule(z3, a, zb, z3, zf, mask, (0, 0, 0))
    a, zf = np.asarray(a, dtype=np.float64), np.asarray(zf, dtype=np.float64)
    with np.errstate(invalid="ignore"):
        has = (np.asarray(mask) != 0) if mask is not None else ((zf > 0) & (zf < np.inf))
        splats = a > 0
    return np.select([front & ~splats, front, has, splats], [0, 1, 2, 3], 4)


ALPHAS = np.array([0.0, -0.0, 2.0 ** -149, 0.5, 1.0, np.nan], dtype=np.float32)
ZBS = np.array([0.0, 1.0, np.inf, np.nan], dtype=np.float32)
MASK_KINDS = ("none", "uint8", "bool", "float")
MASK_VALUES = {"uint8": np.array([0, 1, 2, 255], np.uint8), "bool": np.array([False, True]),
               "float": np.array([0.0, 0.5, 256.0, -0.0], np.float32)}


def composite_truth_table(kind):
    """Every alpha in ALPHAS x every zb in ZBS x zf in {-1, 0, 1, zb, nextafter(zb, -inf), nextafter(zb, +inf), inf,
    NaN} x every mask value of `kind`; every third pixel's splat colour non-finite (inf, -inf, NaN by channel).
    Returns dict(bg, a, zb, fg, zf, mask) of fp32 arrays [P,...] (mask None for "none")."""
    rows = []
    for zb in ZBS:
        zfs = [-1.0, 0.0, 1.0, zb, np.nextafter(zb, np.float32(-np.inf)), np.nextafter(zb, np.float32(np.inf)), np.inf, np.nan]
        rows += [(a, zb, np.float32(zf)) for a in ALPHAS for zf in zfs]
    a, zb, zf = (np.array([r[i] for r in rows], dtype=np.float32) for i in range(3))
    mask = None
    if kind != "none":
        vals = MASK_VALUES[kind]
        mask = np.repeat(vals, len(rows))
        a, zb, zf = (np.tile(x, len(vals)) for x in (a, zb, zf))
    n = a.shape[0]
    rng = np.random.default_rng(17)
    bg = rng.uniform(0, 1, (n, 3)).astype(np.float32)
    fg = rng.uniform(0, 1, (n, 3)).astype(np.float32)
    bg[::3] = np.array([np.inf, -np.inf, np.nan], np.float32)
    return dict(bg=bg, a=a, zb=zb, fg=fg, zf=zf, mask=mask)


@functools.lru_cache(maxsize=None)
def composite_random_frame(h, w, masked, seed=0):
    """A frame for the grid-stride loop: alpha 0 on a fifth of the pixels, foreground on 60 %, depths of both layers
    from one range (both occlusion orders), a tenth of the depth pairs exactly equal."""
    rng = np.random.default_rng(seed)
    a = rng.uniform(0, 1, (h, w)).astype(np.float32)
    a[rng.random((h, w)) < 0.2] = 0
    zb = rng.uniform(2, 12, (h, w)).astype(np.float32)
    zf = rng.uniform(2, 12, (h, w)).astype(np.float32)
    eq = rng.random((h, w)) < 0.1
    zf[eq] = zb[eq]
    present = rng.random((h, w)) < 0.6
    mask = present.astype(np.uint8) if masked else None
    if not masked:
        zf[~present] = np.inf
    bg = (rng.uniform(0, 1, (h, w, 3)) * a[..., None]).astype(np.float32)
    fg = rng.uniform(0, 1, (h, w, 3)).astype(np.float32)
    return dict(bg=bg, a=a, zb=zb, fg=fg, zf=zf, mask=mask)


# ---- frame_to_u8 ---------------------------------------------------------------------------------------
U8_DELTA = 2e-4
U8_BACKGROUND = (0.2, 0.4, 0.9)


def u8_rule(colors, alpha, bg=None):
    """The exact byte rint(255 fmin(fmax(v, 0), 1)) of v = rgb + (1 - alpha) bg in fp64, half to even, NaN -> 0 (fmax
    drops a NaN), and the near-tie mask |frac(255 v) - 0.5| <= U8_DELTA at which an fp32 evaluation may give the
    neighbouring byte.  U8_DELTA: the kernel rounds 1 - alpha, the product, the sum and 255 * v, four roundings of
    quantities of magnitude <= 2.1 (|rgb| <= 1.1, (1 - alpha) bg <= 1), in units of the byte 4 * 2^-24 * 2.1 * 255 =
    1.3e-4, rounded up to 2e-4.  colors [P,>=3], alpha [P] -> (uint8 [P,3], bool [P,3])."""
    c = np.asarray(colors, dtype=np.float64)[..., :3]
    a = np.asarray(alpha, dtype=np.float64).reshape(c.shape[:-1])
    b = np.zeros(3) if bg is None else np.asarray(bg, dtype=np.float32).astype(np.float64)   # the kernel gets fp32
    with np.errstate(invalid="ignore"):
        x = 255.0 * np.fmin(np.fmax(c + (1 - a)[..., None] * b, 0.0), 1.0)
    near = np.abs(x - np.floor(x) - 0.5) <= U8_DELTA
    return np.rint(x).astype(np.uint8), near


def u8_check(got, colors, alpha, bg=None):
    """(differing bytes, unexplained bytes, largest |difference|) of a uint8 [P,3] result against u8_rule."""
    ref, near = u8_rule(colors, alpha, bg)
    d = np.abs(np.asarray(got).reshape(ref.shape).astype(np.int16) - ref.astype(np.int16))
    return int((d > 0).sum()), int(((d > 0) & ~near).sum()), int(d.max(initial=0))


@functools.lru_cache(maxsize=None)
def u8_random_inputs(n_px, stride, seed=0):
    """colours [n_px, stride] in [-0.1, 1.1], alpha [n_px] in [0, 1] with 0 and 1 themselves on a tenth each."""
    rng = np.random.default_rng(seed + 1000 * stride + n_px)
    c = (rng.random((n_px, stride), dtype=np.float32) * np.float32(1.2) - np.float32(0.1))
    a = rng.random(n_px, dtype=np.float32)
    sel = rng.random(n_px, dtype=np.float32)
    a[sel < 0.1] = 0
    a[sel > 0.9] = 1
    return c, a


U8_CASES = ((1027, 3), (1027, 4), (1027, 7), (4_195_507, 3), (1_049_093, 4))     # (pixels, stride)


def u8_tie_colors():
    """For k = 0..254 the fp32 c with fl32(255 c) == k + 0.5 exactly (searched among fl32((k + 0.5) / 255) and its two
    neighbours; None where there is none), and the byte half-to-even makes of it: k if k is even, else k + 1."""
    out, want = [], []
    for k in range(255):
        c0 = np.float32((k + 0.5) / 255.0)
        cands = [np.nextafter(c0, np.float32(0)), c0, np.nextafter(c0, np.float32(1))]
        hit = [c for c in cands if np.float32(255.0) * c == np.float32(k + 0.5)]
        out.append(hit[0] if hit else None)
        want.append(k if k % 2 == 0 else k + 1)
    return out, np.array(want, dtype=np.uint8)


def u8_tie_frame(stride):
    """255 pixels whose three channels walk the tie values (channel j of pixel i is tie (i + 85 j) mod 255), alpha 1:
    packed, that is 63 quads and a tail of 3.  Returns (colors [255,stride], alpha [255], expected uint8 [255,3])."""
    ties, want = u8_tie_colors()
    t = np.array(ties, dtype=np.float32)
    idx = (np.arange(255)[:, None] + 85 * np.arange(3)[None]) % 255
    c = np.full((255, stride), 0.25, dtype=np.float32)
    c[:, :3] = t[idx]
    return c, np.ones(255, np.float32), want[idx]


def u8_clamp_inputs():
    """Every colour in {-1, -0.0, 0.31, 1.5, inf, -inf, NaN} under every alpha in {0, 0.5, 1, -1, 2, inf, -inf, NaN}."""
    cs = np.array([-1.0, -0.0, 0.31, 1.5, np.inf, -np.inf, np.nan], np.float32)
    als = np.array([0.0, 0.5, 1.0, -1.0, 2.0, np.inf, -np.inf, np.nan], np.float32)
    c = np.repeat(cs, len(als))
    colors = np.stack([c, np.roll(c, 8), np.roll(c, 24)], axis=1)
    return np.ascontiguousarray(colors), np.tile(als, len(cs))


# ---- mask_pcd_2d ---------------------------------------------------------------------------------------
def bilinear_fp64(img, uv):
    """F.grid_sample(img, (uv - [w/2, h/2]) / [w/2, h/2], bilinear, border padding, align_corners=True) in fp64 from
    the fp32 uv the kernel reads, and a bound on |kernel's fp32 sample - this|.  Returns (sample [N], bound [N]).

    The bound.  The kernel's x = fl(fl(fl(fl(u - w/2) / (w/2)) + 1) * 0.5 * (w - 1)) takes four roundings (the halving
    is exact): of u - w/2 and of the quotient g, each worth U |g| (w - 1) / 2 in x, of g + 1, worth U |g + 1| (w - 1) / 2,
    and of x itself, U |x|: ex = U ((w - 1) / 2 (2 |g| + |g + 1|) + |x|), a few ulp of w inside the image; likewise
    ey.  The clamp to [0, w - 1] only shrinks an error, and a coordinate that is farther outside than ex is clamped to
    the same border by both sides: ex = 0 there.  x - floor(x) and y - floor(y) are exact.  The sample is continuous
    and piecewise bilinear in (x, y) with slopes of at most R = max(img) - min(img), so a coordinate error moves it by
    at most R (ex + ey) -- across a cell boundary too.  The interpolation itself rounds 1 - fx, 1 - fy, two products
    per term and three additions, at most 7 roundings over terms whose magnitudes sum to at most M = max|img|: 7 U M.
    bound = 1.01 (R (ex + ey) + 7 U M).  A NaN coordinate gives NaN for both."""
    img = np.asarray(img, dtype=np.float64)
    h, w = img.shape
    uv = np.asarray(uv, dtype=np.float32).astype(np.float64)

    def axis(u, n):
        g = (u - n / 2) / (n / 2)
        xu = (g + 1) * 0.5 * (n - 1)
        e = U * ((n - 1) / 2 * (2 * np.abs(g) + np.abs(g + 1)) + np.abs(xu))
        with np.errstate(invalid="ignore"):
            e = np.where((xu < -e) | (xu > n - 1 + e), 0.0, e)
            x = np.clip(xu, 0, n - 1)
        return x, e
    x, ex = axis(uv[:, 0], w)
    y, ey = axis(uv[:, 1], h)
    bad = np.isnan(x) | np.isnan(y)
    x, y = np.where(bad, 0, x), np.where(bad, 0, y)
    x0, y0 = np.floor(x), np.floor(y)
    fx, fy = x - x0, y - y0
    x0, y0 = x0.astype(np.int64), y0.astype(np.int64)
    x1, y1 = np.minimum(x0 + 1, w - 1), np.minimum(y0 + 1, h - 1)
    s = (img[y0, x0] * (1 - fx) * (1 - fy) + img[y0, x1] * fx * (1 - fy)
         + img[y1, x0] * (1 - fx) * fy + img[y1, x1] * fx * fy)
    bound = 1.01 * ((img.max() - img.min()) * (ex + ey) + 7 * U * np.abs(img).max())
    return np.where(bad, np.nan, s), np.where(bad, np.nan, bound)


def mask_rule(uv, mask, thresh, depth=None, pnt_depth=None, depth_thresh=0.1):
    """mask_pcd_2d in fp64 (the thresholds are the fp32 numbers the kernel gets): keep [N] bool, and `near` [N] bool --
    a decision of the kernel may differ from `keep` only where one of the comparisons that decide it is within its
    bound: |sample - thresh| <= bilinear bound, or ||depth sample - pnt_depth| - depth_thresh| <= bilinear bound +
    U |depth sample - pnt_depth| (the subtraction's rounding).  A NaN coordinate keeps nothing and is never near."""
    thresh, depth_thresh = float(np.float32(thresh)), float(np.float32(depth_thresh))
    s, b = bilinear_fp64(mask, uv)
    with np.errstate(invalid="ignore"):
        keep = s > thresh
        near = np.abs(s - thresh) <= b
        if depth is not None:
            sd, bd = bilinear_fp64(depth, uv)
            diff = np.abs(sd - np.asarray(pnt_depth, dtype=np.float32).astype(np.float64).reshape(len(sd), -1)[:, 0])
            keep = keep & (diff < depth_thresh)
            near = near | (np.abs(diff - depth_thresh) <= bd + U * diff)
    return keep, near


@functools.lru_cache(maxsize=None)
def mask_inputs(h, w, n, uv_stride, seed=5):
    """A binary mask, a depth map in [1, 3], uv over the image and 5 pixels around it (fp32, [n,uv_stride]) and point
    depths in [1, 3].  The first rows are the corners, edge midpoints and centre {0, w/2, w} x {0, h/2, h}, four points
    far outside and one NaN row."""
    rng = np.random.default_rng(seed + h * w)
    mask = (rng.uniform(size=(h, w)) > 0.5).astype(np.float32)
    depth = rng.uniform(1, 3, size=(h, w)).astype(np.float32)
    uv = np.ones((n, uv_stride), np.float32)
    uv[:, 0], uv[:, 1] = rng.uniform(-5, w + 5, n), rng.uniform(-5, h + 5, n)
    fixed = [(u, v) for u in (0, w / 2, w) for v in (0, h / 2, h)]
    fixed += [(-1e6, h / 3), (1e6, h / 3), (w / 3, -1e30), (3e9, 3e9), (np.nan, 1.0), (1.0, np.nan)]
    uv[:len(fixed), :2] = np.array(fixed, np.float32)
    pd = rng.uniform(1, 3, size=(n, 1)).astype(np.float32)
    return mask, depth, uv, pd


MASK_CASES = ((60, 80, 30000, 2), (1, 81, 2000, 3), (61, 1, 2000, 2), (37, 53, 2000, 3))      # (h, w, n, uv_stride)


# ---- get_depth_map --------------------------------------------------------------------------------------
def cells_off_ties(rng, n, cw, ch, scale, uv_stride=2):
    """uv [n,uv_stride] fp32 whose quotient uv / scale sits within 0.45 of an integer in [-3, cells + 3): no decision
    of round-half-even is within 0.05 of flipping, so an fp32 and an fp64 division choose the same cell."""
    q = np.stack([rng.integers(-3, cw + 3, n), rng.integers(-3, ch + 3, n)], 1) + rng.uniform(-0.45, 0.45, (n, 2))
    uv = np.ones((n, uv_stride), np.float32)
    uv[:, :2] = (q * scale).astype(np.float32)
    return uv


def depth_map_far_inputs():
    """uv [15,2]: each of inf, -inf, NaN, 3e9, -3e9, 2^31, -2^31 as u (v = 2), then as v (u = 2), then the largest fp32
    below 2^31 as u; depths 1, 2, 3, ... so that the first point of a cell wins it."""
    big = [np.inf, -np.inf, np.nan, 3e9, -3e9, 2.0 ** 31, -2.0 ** 31]
    uv = np.array([[b, 2.0] for b in big] + [[2.0, b] for b in big] + [[2.0 ** 31 - 128, 2.0]], np.float32)
    return uv, np.arange(1, len(uv) + 1, dtype=np.float32)


# ---- project_pcd ---------------------------------------------------------------------------------------
def project_bound(pnt_w, K, c2w):
    """Forward-error bounds (cam [N,3], uv [N,3]) of points_project_kernel's fp32 arithmetic, from fp64 magnitudes; K
    and c2w are the fp32 matrices the kernel reads.
      d_j = fl(p_j - t_j): U |d_j|.   cam_k = sum_j d_j R_jk, three products and two additions on rounded d: 4 U
      sum_j |d_j| |R_jk|.   x = cam_0 / z, y = cam_1 / z: |dx| <= (|d cam_0| + |x| |d cam_2|) / |z| + U |x|; z / z = 1
      exactly.   uv_k = x K_k0 + y K_k1 + K_k2: sum_j |K_kj| |dx_j| + 3 U sum_j |K_kj| |x_j|."""
    p, K, c = (np.asarray(a, dtype=np.float64) for a in (pnt_w, K, c2w))
    d = np.abs(p - c[:3, 3])
    ecam = 4 * GAMMA * (d @ np.abs(c[:3, :3]))
    cam = (p - c[:3, 3]) @ c[:3, :3]
    with np.errstate(divide="ignore", invalid="ignore"):
        xy = np.abs(cam / cam[:, 2:])
        exy = (ecam + xy * ecam[:, 2:]) / np.abs(cam[:, 2:]) + GAMMA * xy
        exy[:, 2] = 0
        euv = exy @ np.abs(K).T + 3 * GAMMA * (xy @ np.abs(K).T)
    return ecam, euv


# ---- transform_gaussians --------------------------------------------------------------------------------
def quat_to_rotmat(q):
    """Rotation matrices [N,3,3] of quaternions [N,4] (wxyz, any non-zero norm)."""
    q = np.asarray(q, dtype=np.float64)
    w, x, y, z = (q / np.linalg.norm(q, axis=-1, keepdims=True)).T
    return np.stack([1 - 2 * (y * y + z * z), 2 * (x * y - w * z), 2 * (x * z + w * y),
                     2 * (x * y + w * z), 1 - 2 * (x * x + z * z), 2 * (y * z - w * x),
                     2 * (x * z - w * y), 2 * (y * z + w * x), 1 - 2 * (x * x + y * y)], -1).reshape(-1, 3, 3)


def transform_ref(means, quats, scales, colors, sh_degree, gids, n_groups, rotations, translations, group_scales):
    """mgs_transform_gaussians in fp64 for the rows with 0 <= gid < n_groups (every other row passes through and is
    compared bit for bit by the caller).  Inputs are the fp32 arrays the kernel reads, rotations / translations /
    group_scales the fp64 values handed to pack_transforms.  Returns dict of (value, bound) pairs over ALL rows (rows
    that do not move hold the input and a zero bound):

      means   s R p + t.  The kernel reads M = fl(s R) and fl(t): 3 products and 3 additions on a rounded matrix,
              5 U (sum_j |s R_ij| |p_j| + |t_i|).
      scales  s scales: the rounding of s and of the product, 2 U |s scales|.
      norm    |q'| = |q|, rot  R(q') = R_g R(q).  q'_c is a sum of four products a_i b_j with a = fl(q_R): four
              roundings of the arithmetic and one of a_i, e_c = 5 U sum_i |a_i| |b_sigma_c(i)|.  So |dq'|_2 <= |e|_2,
              ||q'| - |q|| <= |e|_2, the unit quaternion moves by at most |e|_2 / |q|, and an entry of the rotation
              matrix by that times the 2-norm of its gradient in the unit quaternion: 2 for an off-diagonal entry
              2 (x y -+ w z), 4 sqrt(y^2 + z^2) for a diagonal entry 1 - 2 (y^2 + z^2).
      colors  each degree-l block times the fp64 matrix M_l of sh_rotation_matrices: 2l + 1 products and additions on
              a matrix rounded to fp32, (2l + 2) U sum_j |M_ij| |c_j|.  DC and coefficients above the degree: input.
    """
    from robosimgs_amd.gaussians import _quat_mul, _rotmat_to_quat, sh_rotation_matrices
    p, q, s3, c = (np.asarray(a, dtype=np.float32).astype(np.float64) for a in (means, quats, scales, colors))
    gids = np.asarray(gids)
    out = {k: [v.copy(), np.zeros_like(v)] for k, v in (("means", p), ("scales", s3), ("colors", c))}
    out["norm"] = [np.linalg.norm(q, axis=1), np.zeros(len(q))]
    out["rot"] = [quat_to_rotmat(q), np.zeros((len(q), 3, 3))]
    for g in range(n_groups):
        sel = gids == g
        if not sel.any():
            continue
        R, t, s = np.asarray(rotations[g], np.float64), np.asarray(translations[g], np.float64), float(group_scales[g])
        out["means"][0][sel] = p[sel] @ (s * R).T + t
        out["means"][1][sel] = 5 * GAMMA * (np.abs(p[sel]) @ np.abs(s * R).T + np.abs(t))
        out["scales"][0][sel] = s * s3[sel]
        out["scales"][1][sel] = 2 * GAMMA * np.abs(s * s3[sel])
        qr = _rotmat_to_quat(R)
        aa, ab = np.abs(qr), np.abs(q[sel])                                 # |a_i| |b_j| over the product's index pairs
        e = 5 * GAMMA * np.stack([ab[:, [0, 1, 2, 3]] @ aa, ab[:, [1, 0, 3, 2]] @ aa, ab[:, [2, 3, 0, 1]] @ aa,
                                  ab[:, [3, 2, 1, 0]] @ aa], axis=1)
        e2 = np.linalg.norm(e, axis=1)
        out["norm"][1][sel] = e2
        Rn = R @ quat_to_rotmat(q[sel])
        qn = _quat_mul(qr[None], q[sel])
        w, x, y, z = (qn / np.linalg.norm(qn, axis=1, keepdims=True)).T
        grad = np.full((len(qn), 3, 3), 2.0)
        grad[:, 0, 0], grad[:, 1, 1], grad[:, 2, 2] = 4 * np.hypot(y, z), 4 * np.hypot(x, z), 4 * np.hypot(x, y)
        out["rot"][0][sel] = Rn
        out["rot"][1][sel] = grad * (e2 / np.linalg.norm(q[sel], axis=1))[:, None, None]
        Ms = sh_rotation_matrices(R, sh_degree)
        for l in range(1, sh_degree + 1):
            blk = slice(l * l, (l + 1) * (l + 1))
            out["colors"][0][sel, blk] = np.einsum("ij,njc->nic", Ms[l], c[sel, blk])
            out["colors"][1][sel, blk] = (2 * l + 2) * GAMMA * np.einsum("ij,njc->nic", np.abs(Ms[l]), np.abs(c[sel, blk]))
    return {k: tuple(v) for k, v in out.items()}


TRANSFORM_GIDS = (-1, 0, 1, 2, 3, 7)        # with n_groups = 3: -1, 3 and 7 do not move
TRANSFORM_CASES = ((16, 1), (16, 2), (16, 3), (4, 1), (9, 2), (12, 1), (9, 1))       # (K, degree)
SENTINEL = 0x7FA5A5A5                       # a signalling-NaN pattern: any arithmetic on it changes its bits


@functools.lru_cache(maxsize=None)
def transform_inputs(n, K, seed=0, gids=None):
    """n Gaussians with [n,K,3] SH rows, group ids drawn from TRANSFORM_GIDS (or the tuple `gids` repeated), and
    three similarity transforms.  Returns dict of fp32 arrays plus rotations, translations, group_scales."""
    rng = np.random.default_rng(seed + 100 * n + K)
    q = rng.normal(size=(n, 4))
    q *= rng.uniform(0.5, 2.0, (n, 1)) / np.linalg.norm(q, axis=1, keepdims=True)       # unnormalised, as stored
    gid = (rng.choice(TRANSFORM_GIDS, n) if gids is None else np.resize(np.array(gids), n)).astype(np.int32)
    Rs = []
    for _ in range(3):
        r, _r = np.linalg.qr(rng.normal(size=(3, 3)))
        if np.linalg.det(r) < 0:
            r[:, 0] = -r[:, 0]
        Rs.append(r)
    return dict(means=rng.normal(size=(n, 3)).astype(np.float32) * 3, quats=q.astype(np.float32),
                scales=np.exp(rng.normal(-3, 1, (n, 3))).astype(np.float32),
                opacities=rng.uniform(0.1, 1, n).astype(np.float32),
                colors=rng.normal(0, 0.3, (n, K, 3)).astype(np.float32), gids=gid,
                rotations=Rs, translations=[rng.normal(size=3) for _ in range(3)], group_scales=[1.0, 1.3, 0.8])


def worst_ratio(got, value, bound):
    """max |got - value| / bound over the entries with a positive bound; entries with a zero bound must be equal."""
    got, value, bound = (np.asarray(a, dtype=np.float64) for a in (got, value, bound))
    err = np.abs(got - value)
    zero = bound == 0
    assert np.array_equal(got[zero], value[zero]), "an entry that no arithmetic touches differs"
    return float((err[~zero] / bound[~zero]).max(initial=0.0))
