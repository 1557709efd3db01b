"""The exact mesh-over-splat composite (include/mgs_hybrid.h) stated once in fp64, its gate, the foregrounds and the list
of cases shared by tests/test_hybrid_host.py and tests/test_gpu_hybrid.py (a helper module, not a test file).

Statement.  `HybridReference` walks one camera's tile lists on the given fp32 arrays the way oracle.gs_oracle_np.rasterize
does -- alpha = min(0.999, opacity exp(-sigma)), counted iff sigma >= 0 and alpha >= 1/255, w = alpha T, the Gaussian at
which T (1 - alpha) <= 1e-4 closes the pixel and is not counted -- and at a pixel with foreground (0 < fg_depth < inf,
d = fg_depth) keeps of the counted Gaussians those with depths[i] < d, an fp32 comparison of the two given arrays in every
precision:
    rgb = sum_F w c + T_F fg_rgb,   depth = sum_F w z + T_F d,   fg_visibility = T_F = prod_F (1 - alpha).
The lists are ordered by (depth bits, index): the constructor asserts that every tile's depths ascend, so F is a prefix and
a pixel is finished at the first entry with depths >= d.  The margins and the flip weight are O.rasterize's, for the same
three decisions (alpha >= 1/255, T (1 - alpha) <= 1e-4, sigma >= 0) under O.EPS_STAGE, taken over the pairs evaluated
while the pixel is still in front of d: a decision behind the foreground cannot move the output.
A pixel without foreground is `pass_through`: composite_over's third rule on the given frame, in fp32 with every product
and sum rounded on its own, so it is compared byte for byte.

dtype=np.float32 is the emulation: the same walk in fp32 NumPy, with fg_visibility kept as T_F -= w the way the kernel
keeps it (`tf_sub`).  tests/test_hybrid_host.py puts it through the gate on every case of CASES.

Gate (`check_hybrid`).  O.check_frame's rule as feature_channel_gates.check_forward applies it, on the four channels
(r, g, b, depth) with 1 - fg_visibility in alpha's place: tolerance 1e-4, every pixel over it on a near-threshold decision
of the reference's own walk within F, such a pixel off by no more than FLIP_SLACK x flip weight x 2 x the largest feature
-- per colour channel the larger of the Gaussians' and the foreground's, for the depth channel the largest depth among the
listed Gaussians and the foreground -- zero unexplained pixels, could-flip share under check_frame's 5 %.
"""
import numpy as np

from feature_channel_gates import MULTI, TILE, tiles_of
from oracle import gs_oracle_np as O

QUEUE = 64                               # entries per batch of the walk's queue (csrc/raster_common.h: kQueue)
# (scene, setup, camera, foreground): every case tests/test_gpu_hybrid.py runs against the reference.  "tiles" is
# FRAMES["tiles"] (one camera); the others are MULTI's setups.  empty_tail differs from ring in camera 2 only.
FOREGROUNDS = ("none", "near", "far", "main", "strict")
CASES = tuple(("tiles", None, 0, fg) for fg in FOREGROUNDS) + tuple(("multi", "ring", c, "main") for c in range(MULTI["n_cams"])) \
    + (("multi", "empty_tail", 2, "main"), ("multi", "empty_tail", 2, "far"))
BACKDROP = (0.05, 0.3, 0.08)
N_STRICT = 32


def has_foreground(fg_depth):
    d = np.asarray(fg_depth, np.float32)
    with np.errstate(invalid="ignore"):
        return (d > 0) & (d < np.inf)


def pass_through(render, alphas, backdrop=None):
    """(rgb [h,w,3], depth [h,w], visibility [h,w]) float32 of a frame with no foreground anywhere."""
    render, a = np.asarray(render, np.float32), np.asarray(alphas, np.float32).reshape(np.asarray(render).shape[:2])
    rgb = render[..., :3].copy()
    if backdrop is not None:
        t = (np.float32(1) - a).astype(np.float32)
        rgb = (rgb + (t[..., None] * np.asarray(backdrop, np.float32)).astype(np.float32)).astype(np.float32)
    with np.errstate(invalid="ignore"):
        depth = np.where(a > 0, render[..., 3], np.float32(np.inf)).astype(np.float32)
    return rgb, depth, np.zeros_like(a)


def listed_depth_range(depths, flatten_ids):
    z = np.asarray(depths, np.float32)[np.unique(np.asarray(flatten_ids))]
    return float(z.min()), float(np.median(z)), float(z.max())


def foreground(kind, w, h, means2d, depths, flatten_ids, seed=7):
    """(fg_rgb float32 [h,w,3], fg_depth float32 [h,w]) of foreground `kind`, from one camera's projected arrays and lists.
      none    no foreground: zeros, with a NaN, an inf and a negative depth among them
      near    a plane nearer than every listed Gaussian
      far     a plane beyond every listed Gaussian
      main    a slanted plane through the median listed depth over the left two thirds of the image, its right edge cut by
              a checkerboard of 3-pixel cells, and one isolated foreground pixel in a tile that has no other
      strict  main, and at the centre pixels of N_STRICT listed Gaussians (the nearest ones with distinct centre pixels)
              fg_depth is that Gaussian's depths value exactly: it is behind."""
    rng = np.random.default_rng(seed)
    fg_rgb = rng.random((h, w, 3)).astype(np.float32)
    fg_depth = np.zeros((h, w), np.float32)
    if len(flatten_ids) == 0:
        z_lo, z_med, z_hi = 1.0, 2.0, 4.0
    else:
        z_lo, z_med, z_hi = listed_depth_range(depths, flatten_ids)
    if kind == "none":
        fg_depth[1, 2], fg_depth[h // 2, w // 2], fg_depth[h - 1, w - 1] = np.nan, np.inf, -1.0
    elif kind == "near":
        fg_depth[:] = np.float32(0.5 * z_lo)
    elif kind == "far":
        fg_depth[:] = np.float32(2.0 * z_hi)
    elif kind in ("main", "strict"):
        y, x = np.mgrid[0:h, 0:w]
        plane = (z_med * (0.75 + 0.5 * x / w + 0.2 * (y / h - 0.5))).astype(np.float32)
        edge = 2 * w // 3
        keep = x < edge
        board = ((x // 3 + y // 3) % 2) == 0
        keep &= (x < edge - 12) | board
        fg_depth = np.where(keep, plane, np.float32(0)).astype(np.float32)
        ix, iy = w - 2, TILE + 5                                     # second row of tiles, right of the plane: no other foreground
        assert iy < h and ix - ix % TILE >= edge
        fg_depth[iy, ix] = np.float32(z_med)
        if kind == "strict":
            ids = np.unique(np.asarray(flatten_ids))
            z = np.asarray(depths, np.float32)
            m = np.asarray(means2d, np.float32)
            px, py = np.floor(m[ids, 0]).astype(int), np.floor(m[ids, 1]).astype(int)
            ok = (px >= 0) & (px < w) & (py >= 0) & (py < h)
            ids, px, py = ids[ok], px[ok], py[ok]
            order = np.argsort(z[ids], kind="stable")
            seen, n = set(), 0
            for j in order:
                if (px[j], py[j]) in seen:
                    continue
                seen.add((px[j], py[j]))
                fg_depth[py[j], px[j]] = z[ids[j]]
                n += 1
                if n == N_STRICT:
                    break
            assert n == N_STRICT
    else:
        raise ValueError(kind)
    return fg_rgb, fg_depth


def tile_truncation(depths, flatten_ids, offsets, fg_depth, w, h):
    """Per tile (row-major): (full list length, truncated length, open pixels) -- the truncated list ends at the first
    entry whose depth is >= the tile's largest foreground depth; 0 for a tile without foreground."""
    z = np.asarray(depths, np.float32)
    ids = np.asarray(flatten_ids)
    tw, th = tiles_of(w, h)
    flat = np.concatenate([np.asarray(offsets).reshape(-1), [len(ids)]]).astype(np.int64)
    has = has_foreground(fg_depth)
    out = np.zeros((tw * th, 3), np.int64)
    for t in range(tw * th):
        ty, tx = divmod(t, tw)
        sl = (slice(ty * TILE, min(ty * TILE + TILE, h)), slice(tx * TILE, min(tx * TILE + TILE, w)))
        n_open = int(has[sl].sum())
        full = int(flat[t + 1] - flat[t])
        trunc = 0
        if n_open:
            d_max = np.asarray(fg_depth, np.float32)[sl][has[sl]].max()
            trunc = int(np.searchsorted(z[ids[flat[t]:flat[t + 1]]], d_max, side="left"))
        out[t] = (full, trunc, n_open)
    return out


class HybridReference:
    """The statement for ONE camera (module docstring).  feats [n, >= 3]: rgb in the first three columns.
    Attributes: rgb [h,w,3], depth [h,w], t_f [h,w] (and tf_sub, the T_F -= w form), has_fg [h,w], n_front [h,w] (members
    of F), margins [4,h,w], flip_weight [h,w] -- zero / inf / pass-through-free at pixels without foreground, which this
    class leaves at rgb = 0, depth = 0, t_f = 0."""

    def __init__(self, means2d, conics, feats, depths, opacities, flatten_ids, offsets, w, h, fg_rgb, fg_depth,
                 dtype=np.float64, flip_eps=O.EPS_STAGE, record=None):
        self.w, self.h, self.dtype = w, h, dtype
        mu, con, opa = (np.asarray(a, dtype=dtype) for a in (means2d, conics, opacities))
        z32 = np.asarray(depths, np.float32)
        d32 = np.asarray(fg_depth, np.float32)
        self.feats32 = np.asarray(feats, np.float32)[:, :3]
        col = np.concatenate([self.feats32.astype(dtype), z32.astype(dtype)[:, None]], axis=1)      # r, g, b, z
        self.fg_rgb, self.fg_depth = np.asarray(fg_rgb, np.float32), d32
        self.has_fg = has_foreground(d32)
        self.flatten_ids = np.asarray(flatten_ids)
        z_all = [float(z32[np.unique(self.flatten_ids)].max())] if len(self.flatten_ids) else []
        z_all += [float(d32[self.has_fg].max())] if self.has_fg.any() else []
        self.z_max = max(z_all) if z_all else 0.0                   # the largest depth a pixel can be made of
        tw, th = tiles_of(w, h)
        self.offsets = np.asarray(offsets).reshape(th, tw)
        flat = np.concatenate([self.offsets.reshape(-1), [len(self.flatten_ids)]]).astype(np.int64)
        acc_img = np.zeros((h, w, 4), dtype)
        self.t_f, self.tf_sub = np.zeros((h, w), dtype), np.zeros((h, w), dtype)
        self.n_front = np.zeros((h, w), np.int64)
        self.margins = np.full((4, h, w), np.inf)
        self.flip_weight = np.zeros((h, w))
        self.members = {} if record is not None else None          # (x, y) -> list indices of F, in walk order
        fe_a, fe_t, fe_s = flip_eps["alpha"], flip_eps["T"], flip_eps["sigma"]
        half, one = dtype(0.5), dtype(1.0)
        for t in range(tw * th):
            ty, tx = divmod(t, tw)
            s, e = flat[t], flat[t + 1]
            y_lo, y_hi, x_lo, x_hi = ty * TILE, min(ty * TILE + TILE, h), tx * TILE, min(tx * TILE + TILE, w)
            has = self.has_fg[y_lo:y_hi, x_lo:x_hi]
            if not has.any():
                continue
            zt = z32[self.flatten_ids[s:e]]
            assert np.all(zt[1:] >= zt[:-1]), f"tile {t}: the list is not in depth order, F would not be a prefix"
            d = d32[y_lo:y_hi, x_lo:x_hi]
            py, px = np.meshgrid(np.arange(y_lo, y_hi, dtype=dtype) + half, np.arange(x_lo, x_hi, dtype=dtype) + half,
                                 indexing="ij")
            T, tsub = np.ones_like(px), np.ones_like(px)
            C = np.zeros(px.shape + (4,), dtype)
            done = ~has                                              # a pixel without foreground is not walked
            cnt = np.zeros(px.shape, np.int64)
            tm = np.full((4,) + px.shape, np.inf)
            fw, loose, r_acc, sr_acc = (np.zeros(px.shape) for _ in range(4))
            for i in range(s, e):
                g = self.flatten_ids[i]
                with np.errstate(invalid="ignore"):
                    done = done | ~(z32[g] < d)                      # strict, fp32 on the given arrays: at d is behind
                if done.all():
                    break
                dx, dy = mu[g, 0] - px, mu[g, 1] - py
                sigma = half * (con[g, 0] * dx * dx + con[g, 2] * dy * dy) + con[g, 1] * dx * dy
                ov = opa[g] * np.exp(-sigma)
                a = np.minimum(dtype(O.ALPHA_MAX), ov)
                live = ~done
                ok = live & (sigma >= 0) & (a >= dtype(O.ALPHA_MIN))
                Tn = T * (one - a)
                # the conditioned margins and the flip weight of oracle.gs_oracle_np.rasterize, over the live pairs
                S = half * (abs(con[g, 0]) * dx * dx + abs(con[g, 2]) * dy * dy) + abs(con[g, 1] * dx * dy)
                r_amp = np.where(ov >= dtype(O.ALPHA_MAX), 0, a / np.maximum(one - a, dtype(1e-3)))
                cS = dtype(O.SIGMA_ABS) * S
                m_a = np.maximum(np.abs(a * dtype(255.0) - one) - cS, 0)
                m_t = np.maximum(np.abs(Tn / dtype(O.T_STOP) - one) - (cS * r_amp + sr_acc), 0) / np.sqrt((one + r_amp) ** 2 + r_acc)
                with np.errstate(divide="ignore", invalid="ignore"):
                    m_s = np.where(S > 0, np.abs(sigma) / S, np.inf)
                could_count = a >= dtype(0.5 * O.ALPHA_MIN)
                toggle = live & ((m_a < fe_a) | (could_count & (m_s < fe_s)))
                fw += np.where(toggle, a * T, 0)
                loose += np.where(toggle, a, 0)
                fw += np.where(live & could_count & (m_t < fe_t + loose), T, 0)
                tm[0] = np.where(live, np.minimum(tm[0], m_a), tm[0])
                tm[1] = np.where(live & could_count, np.minimum(tm[1], m_t), tm[1])
                tm[2] = np.where(live & could_count, np.minimum(tm[2], m_s), tm[2])
                stop = ok & (Tn <= dtype(O.T_STOP))
                done = done | stop
                acc = ok & ~stop
                r_acc = r_acc + np.where(acc, r_amp * r_amp, 0)
                sr_acc = sr_acc + np.where(acc, cS * r_amp, 0)
                wgt = np.where(acc, a * T, 0).astype(dtype)
                C += wgt[..., None] * col[g][None, None, :]
                T = np.where(acc, Tn, T)
                tsub = (tsub - wgt).astype(dtype)
                cnt += acc
                if self.members is not None:
                    for yy, xx in zip(*np.nonzero(acc)):
                        if (x_lo + xx, y_lo + yy) in record:
                            self.members.setdefault((x_lo + xx, y_lo + yy), []).append(int(i))
            sl = (slice(y_lo, y_hi), slice(x_lo, x_hi))
            acc_img[sl] = np.where(has[..., None], C, 0)
            self.t_f[sl] = np.where(has, T, 0)
            self.tf_sub[sl] = np.where(has, tsub, 0)
            self.n_front[sl] = np.where(has, cnt, 0)
            self.margins[:, y_lo:y_hi, x_lo:x_hi] = np.where(has[None], tm, np.inf)
            self.flip_weight[sl] = np.where(has, fw, 0)
        self.acc = acc_img                                           # sum_F w (r, g, b, z)
        m = self.has_fg
        fg4 = np.concatenate([self.fg_rgb.astype(dtype), np.where(m, d32, 0).astype(dtype)[..., None]], axis=-1)
        out = acc_img + self.t_f[..., None] * np.where(m[..., None], fg4, 0)
        self.rgb, self.depth = out[..., :3], out[..., 3]

    def feat_max(self):
        """[4]: per colour channel the larger of the Gaussians' and the foreground's largest value, and the largest depth
        among the listed Gaussians and the foreground."""
        fm = np.abs(self.feats32.astype(np.float64)).max(axis=0) if len(self.feats32) else np.zeros(3)
        if self.has_fg.any():
            fm = np.maximum(fm, np.abs(self.fg_rgb[self.has_fg].astype(np.float64)).max(axis=0))
        return np.concatenate([fm, [self.z_max]])

def check_hybrid(ref, rgb, depth, visibility, what="hybrid"):
    """THE gate of these files (module docstring), on the pixels with foreground.  Prints and returns check_frame's
    statistics."""
    m = ref.has_fg
    rgb, depth, vis = (np.asarray(a, np.float64) for a in (rgb, depth, visibility))
    assert rgb.shape == (ref.h, ref.w, 3) and depth.shape == (ref.h, ref.w) and vis.shape == (ref.h, ref.w)
    assert np.isfinite(rgb[m]).all() and np.isfinite(depth[m]).all() and np.isfinite(vis[m]).all(), f"{what}: non-finite output"
    got = np.where(m[..., None], np.concatenate([rgb, depth[..., None]], axis=-1), 0.0)
    want = np.concatenate([np.asarray(ref.rgb, np.float64), np.asarray(ref.depth, np.float64)[..., None]], axis=-1)
    st = O.check_frame(got, np.where(m, 1.0 - vis, 0.0), want, np.where(m, 1.0 - np.asarray(ref.t_f, np.float64), 0.0),
                       ref.margins, O.EPS_STAGE, what=what, flip_weight=ref.flip_weight, feat_max=ref.feat_max(),
                       require_flip_bound=True)
    st["open_pixels"] = int(m.sum())
    print(f"\n{what}: {st['open_pixels']} pixels with foreground, could-flip {st['could_flip_frac']:.2e}, over 1e-4 "
          f"{st['over_tol']} (unexplained {st['unexplained']}), max err off flips {st['max_err_nonflip']:.2e}, flip over bound "
          f"{st['flip_over_bound']}")
    return st


def check_pass_through(fg_depth, render, alphas, backdrop, rgb, depth, visibility, what="pass-through"):
    """Byte for byte at every pixel without foreground."""
    m = ~has_foreground(fg_depth)
    want = pass_through(render, alphas, backdrop)
    for name, g_, w_ in zip(("rgb", "depth", "fg_visibility"), (rgb, depth, visibility), want):
        g_, w_ = np.asarray(g_, np.float32), np.asarray(w_, np.float32)
        assert g_.shape == w_.shape, (name, g_.shape, w_.shape)
        same = g_.view(np.uint32) == w_.view(np.uint32)
        same = same.all(axis=-1) if same.ndim == 3 else same
        assert same[m].all(), f"{what}: {int((~same & m).sum())} pixels without foreground differ in {name}"
    return int(m.sum())
