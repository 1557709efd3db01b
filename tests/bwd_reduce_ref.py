"""fp64 restatement of the REDUCE half of the deterministic raster backward (mgs_rasterize_bwd_det: reduce_records_rows_kernel
up to 4 channels, reduce_records_kernel for 5..32; csrc/raster_bwd.hip), with a derived rounding bound per value, an fp32
restatement that follows the kernels' order of operations and takes named deliberate defects, the exact unit tables of the
segmented launch, and hand-placed raster-level inputs.  NumPy only: no GPU, no torch.

The operation.  The record half leaves, per (tile, Gaussian) slot, a flag and a record {s, s_x, s_y, s_xx, s_xy, s_yy,
colour gradients, (absgrad x, y)}: the moments of v_sigma = d loss / d sigma about the TILE CENTRE.  A Gaussian owns the
slots slot_base + row * w + col of its tile rectangle (pair_info = {slot_base, x0, y0, w | h << 16}); a slot EXISTS iff
slot < capacity and COUNTS iff it exists and its flag is non-zero.  Per counted slot, with m = mean - (16 tile + 8):
    P   = m_x s - s_x                      (= sum v_sigma dx)
    Q   = m_y s - s_y
    Vaa = m_x P - (m_x s_x - s_xx)         (= sum v_sigma dx^2)
    Vab = m_y P - (m_x s_y - s_xy)         (= sum v_sigma dx dy)
    Vbb = m_y Q - (m_y s_y - s_yy)
These and s, the colours and the absgrad pair are summed over the Gaussian's counted slots; then, once per Gaussian,
    v_means2d = (a SP + b SQ, b SP + c SQ),  v_conics = (SVaa / 2, SVab, SVbb / 2),  v_opacity = -Ss / opacity (0 if <= 0).
A Gaussian with no counted slot gets exact zeros.

The rounding bound (u = 2^-24, fp32 round to nearest; every term names the kernel operation it comes from).  The mean is
the fp32 value the GPU read and 16 tile + 8 is an integer below 2^24, so the fp64 m is exact and the kernel's
m^ = fl(mean - centre) = m (1 + d), |d| <= u  [the subtraction in row_sum / reduce_records_kernel].
  moments_to_mean, per slot, first order in u, stated in the absolute values of the operands (the nested-difference form:
  products and differences, never the cancelled result):
    P^   = fma(m^x, s, -s_x)             one rounding + d of m^x:   e_P   = u (2 |m_x||s| + |s_x|)
    t^   = fma(m^x, s_x, -s_xx)          likewise:                   e_t   = u (2 |m_x||s_x| + |s_xx|)
    Vaa^ = fma(m^x, P^, -t^)             |m_x| e_P (P^'s error carried) + u |m_x| |P|abs (d of m^x) + e_t
                                         + u |Vaa|abs (the fma's own rounding),
           |P|abs = |m_x||s| + |s_x|,  |t|abs = |m_x||s_x| + |s_xx|,  |Vaa|abs = |m_x| |P|abs + |t|abs
    Vab, Vbb: the same with (m_y, P, m_x s_y - s_xy) and (m_y, Q, m_y s_y - s_yy).
  The sum of K counted terms x_i, in ANY order (rows by column then rows by row, or slot by slot: additions of the exact
  zeros of uncounted slots round nothing): at most K - 1 inexact additions touch a term:  gamma(K - 1) sum |x_i|,
  gamma(k) = k u / (1 - k u)  [rs[] += / acc[] += in both kernels].  With the terms' own errors:
    E_X = sum e_X,i + gamma(K - 1) sum |X_i|abs.
  finish_geo, two terms:  v_x^ = fma(b, SQ^, fl(a SP^)):   |a| E_P + |b| E_Q + 2 u |a| sum|P|abs + u |b| sum|Q|abs
                          v_y^ = fma(c, SQ^, fl(b SP^)):   |b| E_P + |c| E_Q + 2 u |b| sum|P|abs + u |c| sum|Q|abs
                          the halves of v_conics are exact.
  opacity:  fl(-Ss^ / opacity): one division:  (E_s + u sum|s|) / opacity.
  Second order: every first-order term above is multiplied afterwards by at most K + 8 further factors (1 + d): the
  whole bound is scaled by 1 + gamma(K + 8).
  Underflow: each of the at most 16 roundings per slot (and the 8 of the finish) may lose up to 2^-126 (flush to zero
  or a denormal's ulp) which later factors scale by at most max(1, |m|)^2 max(1, |conic|, 1 / opacity):
    floor = 2^-126 * 16 (K + 1) * max(1, |m_x|, |m_y|)^2 * max(1, |a|, |b|, |c|, 1 / opacity).
Nothing here was fitted to what the kernels give; tests/test_gpu_bwd_reduce.py measures the ratio error / bound.
"""
from __future__ import annotations

import numpy as np

U = 2.0 ** -24
F32_MIN = 2.0 ** -126
BIG_PAIRS = 256           # csrc/raster_bwd.hip kBigPairs: rectangles of this many tiles go to the one-wave path
RUN = 16                  # kRun: consecutive Gaussians a wave of the rows kernel owns, a launch of waves apart
UNIT_CLASSES = 32         # kUnitClasses

BUGS = ("no_plus8", "column_major", "ignore_flags", "no_half", "vab_sign", "opacity_no_divide", "opacity_sign",
        "read_past_capacity", "drop_row64", "skip_256")


def padded_channels(channels: int) -> int:
    return channels if channels <= 4 else 8 if channels <= 8 else 16 if channels <= 16 else 32


def record_floats(channels: int, absgrad: bool) -> int:
    return (6 + padded_channels(channels) + (2 if absgrad else 0) + 3) // 4 * 4


def gamma(k):
    k = np.maximum(np.asarray(k, dtype=np.float64), 0.0)
    return k * U / (1.0 - k * U)


# ---- the slots of every rectangle ---------------------------------------------------------------------------------------
def rect_slots(pair_info, column_major=False):
    """All (Gaussian, row, col, slot) of the rectangles, row-major per Gaussian (int64 arrays, Gaussian-major)."""
    pi = np.asarray(pair_info).astype(np.int64)
    w = pi[:, 3] & 0xffff
    h = (pi[:, 3] >> 16) & 0xffff
    cnt = w * h
    g = np.repeat(np.arange(len(pi)), cnt)
    first = np.cumsum(cnt) - cnt
    i = np.arange(int(cnt.sum())) - first[g]
    row, col = i // np.maximum(w[g], 1), i % np.maximum(w[g], 1)
    slot = pi[g, 0] + (col * h[g] + row if column_major else i)
    return g, row, col, slot


def slot_kinds(pair_info, flags, capacity):
    """(flagged, unflagged, non-existent) slot counts of the rectangles."""
    _, _, _, slot = rect_slots(pair_info)
    exist = slot < capacity
    fl = np.zeros(len(slot), dtype=bool)
    fl[exist] = np.asarray(flags)[slot[exist]] != 0
    return int(fl.sum()), int((exist & ~fl).sum()), int((~exist).sum())


# ---- fp64 with the bound --------------------------------------------------------------------------------------------------
def reduce_f64(pair_info, records, flags, capacity, mean, conic, opacity, channels, absgrad):
    """Values and rounding bounds (module docstring) of the five outputs: dict name -> (value, bound), float64 arrays of the
    outputs' shapes, plus "counted" [N]: the number of counted slots per Gaussian."""
    pi = np.asarray(pair_info).astype(np.int64)
    n = len(pi)
    records = np.asarray(records)
    mean = np.asarray(mean, dtype=np.float32).astype(np.float64)
    conic = np.asarray(conic, dtype=np.float32).astype(np.float64)
    opacity = np.asarray(opacity, dtype=np.float32).astype(np.float64)
    cht = padded_channels(channels)
    g, row, col, slot = rect_slots(pi)
    exist = slot < capacity
    on = exist.copy()
    on[exist] = np.asarray(flags)[slot[exist]] != 0
    g, row, col, slot = g[on], row[on], col[on], slot[on]
    r = records[slot].astype(np.float64)
    s, sx, sy, sxx, sxy, syy = (r[:, i] for i in range(6))
    mx = mean[g, 0] - (16.0 * (pi[g, 1] + col) + 8.0)
    my = mean[g, 1] - (16.0 * (pi[g, 2] + row) + 8.0)
    amx, amy = np.abs(mx), np.abs(my)
    a_ = np.abs

    P, Q = mx * s - sx, my * s - sy
    Pabs, Qabs = amx * a_(s) + a_(sx), amy * a_(s) + a_(sy)
    eP, eQ = U * (2 * amx * a_(s) + a_(sx)), U * (2 * amy * a_(s) + a_(sy))

    def second(m, am, X, Xabs, eX, mt, t1, t2):       # V = m X - (mt t1 - t2)
        amt = np.abs(mt)
        t = mt * t1 - t2
        tabs = amt * a_(t1) + a_(t2)
        et = U * (2 * amt * a_(t1) + a_(t2))
        Vabs = am * Xabs + tabs
        return m * X - t, Vabs, am * eX + U * am * Xabs + et + U * Vabs

    Vaa, Vaa_abs, eVaa = second(mx, amx, P, Pabs, eP, mx, sx, sxx)
    Vab, Vab_abs, eVab = second(my, amy, P, Pabs, eP, mx, sy, sxy)
    Vbb, Vbb_abs, eVbb = second(my, amy, Q, Qabs, eQ, my, sy, syy)

    def per_g(x):
        return np.bincount(g, weights=x, minlength=n)

    K = np.bincount(g, minlength=n).astype(np.float64)
    gk = gamma(K - 1)

    def total(x, xabs, ex):
        return per_g(x), per_g(xabs), per_g(ex) + gk * per_g(xabs)

    SP, AP, EP = total(P, Pabs, eP)
    SQ, AQ, EQ = total(Q, Qabs, eQ)
    Saa, _, Eaa = total(Vaa, Vaa_abs, eVaa)
    Sab, _, Eab = total(Vab, Vab_abs, eVab)
    Sbb, _, Ebb = total(Vbb, Vbb_abs, eVbb)
    Ss, As, Es = total(s, a_(s), np.zeros_like(s))
    ca, cb, cc = conic[:, 0], conic[:, 1], conic[:, 2]
    aca, acb, acc = a_(ca), a_(cb), a_(cc)
    has_op = opacity > 0
    inv_op = np.where(has_op, 1.0 / np.where(has_op, opacity, 1.0), 0.0)
    mmax = np.maximum(1.0, np.maximum(np.zeros(n), np.maximum(_gmax(g, amx, n), _gmax(g, amy, n))))
    floor = F32_MIN * 16 * (K + 1) * mmax ** 2 * np.maximum(1.0, np.maximum(np.maximum(aca, acb), np.maximum(acc, inv_op)))
    second_order = 1.0 + gamma(K + 8)
    live = K > 0

    def fin(v, e):
        e = np.where(_b(live, v), _b(second_order, v) * e + _b(floor, v), 0.0)
        return np.where(_b(live, v), v, 0.0), e

    out = {"counted": K.astype(np.int64)}
    vm = np.stack([ca * SP + cb * SQ, cb * SP + cc * SQ], 1)
    em = np.stack([aca * EP + acb * EQ + U * (2 * aca * AP + acb * AQ),
                   acb * EP + acc * EQ + U * (2 * acb * AP + acc * AQ)], 1)
    out["v_means2d"] = fin(vm, em)
    out["v_conics"] = fin(np.stack([0.5 * Saa, Sab, 0.5 * Sbb], 1), np.stack([0.5 * Eaa, Eab, 0.5 * Ebb], 1))
    out["v_opacities"] = fin(-Ss * inv_op, (Es + U * As) * inv_op)
    vf, ef = np.zeros((n, channels)), np.zeros((n, channels))
    for c in range(channels):
        vf[:, c], _, ef[:, c] = total(r[:, 6 + c], a_(r[:, 6 + c]), np.zeros_like(s))
    out["v_feats"] = fin(vf, ef)
    if absgrad:
        vb, eb = np.zeros((n, 2)), np.zeros((n, 2))
        for c in range(2):
            vb[:, c], _, eb[:, c] = total(r[:, 6 + cht + c], a_(r[:, 6 + cht + c]), np.zeros_like(s))
        out["v_means2d_abs"] = fin(vb, eb)
    return out


def _gmax(g, x, n):
    m = np.zeros(n)
    np.maximum.at(m, g, x)
    return m


def _b(x, like):
    return x if like.ndim == 1 else x[:, None]


OUTPUTS = ("v_means2d", "v_conics", "v_feats", "v_opacities", "v_means2d_abs")


def compare(got: dict, ref: dict):
    """got: name -> array (the kernel's or reduce_fp32's outputs).  Returns (worst error / bound per output, list of
    (output, row) that miss: outside the bound, not finite, or non-zero where nothing counted).  No row is excused."""
    worst, bad = {}, []
    for name in OUTPUTS:
        if name not in ref:
            continue
        val, bound = ref[name]
        x = np.asarray(got[name], dtype=np.float64).reshape(val.shape)
        err = np.abs(x - val)
        ok = np.isfinite(x) & (err <= bound)
        rows = np.nonzero(~(ok if ok.ndim == 1 else ok.all(1)))[0]
        bad += [(name, int(i)) for i in rows[:8]]
        with np.errstate(divide="ignore", invalid="ignore"):
            ratio = np.where(bound > 0, err / bound, 0.0)
        ratio = np.where(np.isfinite(ratio), ratio, np.inf)
        worst[name] = float(ratio.max()) if ratio.size else 0.0
        if not ok.all() and not rows.size:
            bad.append((name, -1))
    return worst, bad


# ---- fp32, the kernels' order, with deliberate defects ------------------------------------------------------------------------
def _f32(x):
    return np.asarray(x, dtype=np.float32)


def _fma(a, b, c):
    """fp32 fma: the product of two fp32 is exact in fp64; the sum is rounded to 53 bits and then to 24 (the double rounding
    differs from a true fma in well under one case in 2^28: this restatement checks the bound, it is not bit-exact)."""
    return (a.astype(np.float64) * b.astype(np.float64) + c.astype(np.float64)).astype(np.float32)


def rows_wave_layout(pair_info):
    """Which wave and lane of reduce_records_rows_kernel owns each Gaussian, and the index of its first row within the
    wave's row rounds (runs of 16 consecutive Gaussians dealt a launch of waves apart; big rectangles own no rows)."""
    pi = np.asarray(pair_info).astype(np.int64)
    n = len(pi)
    w, h = pi[:, 3] & 0xffff, (pi[:, 3] >> 16) & 0xffff
    hh = np.where((w == 0) | (w * h >= BIG_PAIRS), 0, h)
    n_waves = 4 * ((n + 255) // 256)
    run = np.arange(n) // RUN
    wave, lane = run % n_waves, (run // n_waves) * RUN + np.arange(n) % RUN
    order = np.lexsort((lane, wave))
    row0 = np.zeros(n, dtype=np.int64)
    cs = np.cumsum(hh[order]) - hh[order]
    wv = wave[order]
    first_of_wave = np.r_[True, wv[1:] != wv[:-1]]
    base = np.maximum.accumulate(np.where(first_of_wave, cs, 0))
    row0[order] = cs - base
    return wave, lane, row0


def reduce_fp32(pair_info, records, flags, capacity, mean, conic, opacity, channels, absgrad, bug=None, order=None):
    """The reduce in NumPy float32, in the kernels' order: order="rows" (up to 4 channels: within a row by column, then
    the rows in row order) or "slots" (5..32 channels: one running sum over the slots, row-major); default by `channels`.
    Outputs start as NaN (the tests' sentinel) and every row is written -- unless `bug` says otherwise.  Slots that do not
    exist read as NaN when a defect reads them; unflagged records are whatever `records` holds (the tests poison them)."""
    assert bug is None or bug in BUGS, bug
    pi = np.asarray(pair_info).astype(np.int64)
    n = len(pi)
    cht = padded_channels(channels)
    nv = 6 + cht + (2 if absgrad else 0)
    order = order or ("rows" if channels <= 4 else "slots")
    records, flags = _f32(records), np.asarray(flags)
    mean, conic, opacity = _f32(mean), _f32(conic), _f32(opacity)
    w, h = pi[:, 3] & 0xffff, (pi[:, 3] >> 16) & 0xffff
    h = np.where(w == 0, 0, h)
    g, row, col, slot = rect_slots(np.c_[pi[:, :3], w | (h << 16)], column_major=bug == "column_major")
    exist = slot < capacity
    safe = np.where(exist, slot, 0)
    on = exist & (flags[safe] != 0)
    if bug == "ignore_flags":
        on = exist
    rec = np.where(on[:, None], records[safe][:, :nv], np.float32(0))
    if bug == "read_past_capacity":
        rec = np.where(exist[:, None], rec, np.float32(np.nan))
    centre = np.float32(0.0 if bug == "no_plus8" else 8.0)
    mx = mean[g, 0] - (_f32((pi[g, 1] + col) * 16) + centre)
    my = mean[g, 1] - (_f32((pi[g, 2] + row) * 16) + centre)
    s, sx, sy, sxx, sxy, syy = (rec[:, i] for i in range(6))
    P, Q = _fma(mx, s, -sx), _fma(my, s, -sy)
    Vaa = _fma(mx, P, -_fma(mx, sx, -sxx))
    Vab = _fma(my, P, -_fma(mx, sy, sxy if bug == "vab_sign" else -sxy))
    Vbb = _fma(my, Q, -_fma(my, sy, -syy))
    terms = np.concatenate([np.stack([P, Q, Vaa, Vab, Vbb, s], 1), rec[:, 6:nv]], 1)       # [slots, nv]

    cnt = w * h
    first = np.cumsum(cnt) - cnt
    acc = np.zeros((n, nv), dtype=np.float32)
    if order == "slots":
        for i in range(int(cnt.max()) if n else 0):
            act = np.nonzero(cnt > i)[0]
            acc[act] = acc[act] + terms[first[act] + i]
    else:
        n_rows = int(h.sum())
        rg = np.repeat(np.arange(n), h)
        rfirst = np.cumsum(h) - h
        rr = np.arange(n_rows) - rfirst[rg]
        rs = np.zeros((n_rows, nv), dtype=np.float32)
        for c in range(int(w.max()) if n else 0):
            act = np.nonzero(w[rg] > c)[0]
            rs[act] = rs[act] + terms[first[rg[act]] + rr[act] * w[rg[act]] + c]
        if bug == "drop_row64":
            _, _, row0 = rows_wave_layout(pi)
            small = cnt[rg] < BIG_PAIRS
            rs[small & ((row0[rg] + rr) % 64 == 63)] = 0
        for r_ in range(int(h.max()) if n else 0):
            act = np.nonzero(h > r_)[0]
            acc[act] = acc[act] + rs[rfirst[act] + r_]
    ca, cb, cc = conic[:, 0], conic[:, 1], conic[:, 2]
    live = cnt > 0
    vx = np.where(live, _fma(cb, acc[:, 1], ca * acc[:, 0]), acc[:, 0])
    vy = np.where(live, _fma(cc, acc[:, 1], cb * acc[:, 0]), acc[:, 1])
    half = np.float32(1.0 if bug == "no_half" else 0.5)
    with np.errstate(divide="ignore", invalid="ignore"):
        ss = acc[:, 5] if bug == "opacity_sign" else -acc[:, 5]
        vo = np.where(opacity > 0, ss if bug == "opacity_no_divide" else ss / opacity, np.float32(0))
    vo = np.where(live, vo, acc[:, 5])
    out = {"v_means2d": np.stack([vx, vy], 1),
           "v_conics": np.stack([np.where(live, acc[:, 2] * half, acc[:, 2]), acc[:, 3], np.where(live, acc[:, 4] * half, acc[:, 4])], 1),
           "v_feats": acc[:, 6:6 + channels].copy(), "v_opacities": vo.astype(np.float32)}
    if absgrad:
        out["v_means2d_abs"] = acc[:, 6 + cht:8 + cht].copy()
    if bug == "skip_256":
        for v in out.values():
            v[cnt == BIG_PAIRS] = np.nan
    return out


# ---- the unit tables of the segmented launch --------------------------------------------------------------------------------
def tile_hi(tile_offsets, last_ids, tile_w, tile_h):
    """Per tile min(max last_id of the tile's pixels, end - 1)."""
    last = np.asarray(last_ids)
    H, W = last.shape
    pad = np.full((tile_h * 16, tile_w * 16), np.iinfo(np.int32).min, dtype=np.int64)
    pad[:H, :W] = last
    mx = pad.reshape(tile_h, 16, tile_w, 16).max(axis=(1, 3)).reshape(-1)
    off = np.asarray(tile_offsets).astype(np.int64)
    return np.minimum(mx, off[1:] - 1)


def unit_tables_ref(tile_offsets, last_ids, shift, tile_w, tile_h):
    """The tables unit_table_kernel must build: dict hi [n_tiles], n_seg [n_tiles], cls [n_tiles] (length class of the last
    segment, -1 where the tile has no unit), counts [1 + 32], whole: set of (tile, segment, start, hi), part: list of 32
    such sets."""
    off = np.asarray(tile_offsets).astype(np.int64)
    start = off[:-1]
    hi = tile_hi(off, last_ids, tile_w, tile_h)
    S = 1 << shift
    has = hi >= start
    n_seg = np.where(has, ((hi - start) >> shift) + 1, 0)
    last_len = np.where(has, ((hi - start) & (S - 1)) + 1, 0)
    cls = np.where(has, ((S - last_len) * UNIT_CLASSES) >> shift, -1)
    whole, part = set(), [set() for _ in range(UNIT_CLASSES)]
    for t in np.nonzero(has)[0]:
        for sg in range(int(n_seg[t]) - 1):
            whole.add((int(t), sg, int(start[t]), int(hi[t])))
        part[int(cls[t])].add((int(t), int(n_seg[t]) - 1, int(start[t]), int(hi[t])))
    counts = np.array([len(whole)] + [len(p) for p in part], dtype=np.int64)
    return {"hi": hi, "n_seg": n_seg, "cls": cls, "counts": counts, "whole": whole, "part": part}


def allowed_slots(pair_info, tile_offsets, flatten_ids, last_ids, tile_w, tile_h):
    """Slots of the (tile, Gaussian) pairs the lists hold at an index no later than the tile's largest last_id."""
    off = np.asarray(tile_offsets).astype(np.int64)
    hi = tile_hi(off, last_ids, tile_w, tile_h)
    n_list = int(off[-1])
    tile = np.repeat(np.arange(tile_w * tile_h), np.diff(off))
    idx = np.arange(n_list)
    keep = idx <= hi[tile]
    tile, gid = tile[keep], np.asarray(flatten_ids).astype(np.int64)[:n_list][keep]
    pi = np.asarray(pair_info).astype(np.int64)
    tx, ty = tile % tile_w, tile // tile_w
    w = pi[gid, 3] & 0xffff
    return np.unique(pi[gid, 0] + (ty - pi[gid, 2]) * w + (tx - pi[gid, 1]))


# ---- hand-placed raster-level inputs ------------------------------------------------------------------------------------------
class Case:
    """One frame's raster-level inputs, placed by hand (no projection): Gaussian i is given the tile rectangle rects[i] =
    (x0, y0, w, h) -- classic bounds, so the binning lists exactly that -- a conic that reaches only part of it with
    alpha >= 1/255 (so flagged and unflagged slots both occur), a low opacity (so the lists stay open) and a depth."""

    def __init__(self, name, tile_w, tile_h, rects, seed, width=None, height=None, opacity=(0.03, 0.3), reach=(0.45, 0.9),
                 anywhere=False, zero_opacity=()):
        rng = np.random.default_rng(seed)
        self.name, self.tile_w, self.tile_h = name, tile_w, tile_h
        self.width, self.height = width or 16 * tile_w, height or 16 * tile_h
        self.rects = np.asarray(rects, dtype=np.int64).reshape(-1, 4)
        n = self.n = len(self.rects)
        x0, y0, w, h = self.rects.T
        empty = (w == 0) | (h == 0)
        jit = rng.uniform(-2.5, 2.5, (n, 2))
        mean = np.stack([16.0 * x0 + 8.0 * w, 16.0 * y0 + 8.0 * h], 1) + jit
        radii = np.stack([8 * w - 4, 8 * h - 4], 0)
        if anywhere:      # rectangles that fill the frame: any mean inside it, radii that clip to the frame on every side
            mean = rng.uniform([0, 0], [self.width, self.height], (n, 2))
            radii = np.full((2, n), 16 * max(tile_w, tile_h) + 16)
        # an empty rectangle: radius 0 on a tile boundary (floor == ceil)
        mean[empty] = np.stack([16.0 * x0[empty], 16.0 * y0[empty]], 1)
        radii[:, empty] = 0
        self.means2d = mean.astype(np.float32)
        self.radii = radii.astype(np.int32)
        op = rng.uniform(opacity[0], opacity[1], n)
        k = np.sqrt(2.0 * np.log(255.0 * op))                 # alpha >= 1/255 within k standard deviations
        fr = rng.uniform(reach[0], reach[1], (n, 2))
        sx = np.maximum(fr[:, 0] * 8.0 * np.maximum(w, 1), 5.0) / k
        sy = np.maximum(fr[:, 1] * 8.0 * np.maximum(h, 1), 5.0) / k
        rho = rng.uniform(-0.5, 0.5, n)
        d = 1.0 - rho * rho
        self.conics = np.stack([1.0 / (sx * sx * d), -rho / (sx * sy * d), 1.0 / (sy * sy * d)], 1).astype(np.float32)
        op[list(zero_opacity)] = 0.0
        self.opacities = op.astype(np.float32)
        self.feats = rng.uniform(0.0, 1.0, (n, 32)).astype(np.float32)
        self.depths = rng.permutation(n).astype(np.float32) + 1.0
        self.seed = seed

    def pair_info(self):
        """What mgs_isect_tiles must report for these rectangles (slot bases ascend with the Gaussian index)."""
        x0, y0, w, h = self.rects.T
        cnt = w * h
        w_, h_ = np.where(cnt > 0, w, 0), np.where(cnt > 0, h, 0)
        return np.stack([np.cumsum(cnt) - cnt, x0, y0, w_ | (h_ << 16)], 1).astype(np.int32)

    def n_isect(self):
        return int((self.rects[:, 2] * self.rects[:, 3]).sum())

    def splats(self, channels):
        s = np.zeros((self.n, 12), dtype=np.float32)
        s[:, 0:2], s[:, 2:5], s[:, 5] = self.means2d, self.conics, self.opacities
        s[:, 6:6 + min(channels, 4)] = self.feats[:, :min(channels, 4)]
        return s

    def cotangents(self, channels):
        rng = np.random.default_rng(self.seed + 1000)
        return (rng.standard_normal((self.height, self.width, channels)).astype(np.float32),
                rng.standard_normal((self.height, self.width)).astype(np.float32))

    def stand_in(self, channels, absgrad, capacity=None):
        """A CPU stand-in for the record half: (records, flags, capacity).  A slot is flagged when the Gaussian reaches the
        tile's nearest pixel centre with alpha >= 1/255 (what the raster's decision comes to while the list is open);
        flagged records are standard normal moments scaled like sums over a tile, every other float is the 0xFF poison."""
        rng = np.random.default_rng(self.seed + 2000)
        pi = self.pair_info()
        cap = self.n_isect() if capacity is None else capacity
        rf = record_floats(channels, absgrad)
        records = np.frombuffer(b"\xff" * (4 * max(cap, 1) * rf), dtype=np.float32).reshape(max(cap, 1), rf).copy()
        flags = np.zeros(max(cap, 1), dtype=np.uint8)
        g, row, col, slot = rect_slots(pi)
        lo_x, lo_y = 16.0 * (pi[g, 1] + col) + 0.5, 16.0 * (pi[g, 2] + row) + 0.5
        dx = self.means2d[g, 0] - np.clip(self.means2d[g, 0], lo_x, lo_x + 15.0)
        dy = self.means2d[g, 1] - np.clip(self.means2d[g, 1], lo_y, lo_y + 15.0)
        a, b, c = (self.conics[g, i].astype(np.float64) for i in range(3))
        sigma = 0.5 * (a * dx * dx + c * dy * dy) + b * dx * dy
        with np.errstate(divide="ignore"):
            reach = (self.opacities[g] > 0) & (self.opacities[g] * np.exp(-sigma) >= 1.0 / 255.0)
        on = reach & (slot < cap)
        flags[slot[on]] = 1
        scale = np.array([1, 8, 8, 64, 64, 64] + [1] * (rf - 6), dtype=np.float32)
        records[slot[on]] = rng.standard_normal((int(on.sum()), rf)).astype(np.float32) * scale
        return records, flags, cap


def _pack(rects_wh, tile_w, tile_h, rng):
    """Place rectangles of the given (w, h) at random positions of the grid (they may overlap)."""
    out = []
    for w, h in rects_wh:
        out.append((int(rng.integers(0, tile_w - w + 1)), int(rng.integers(0, tile_h - h + 1)), w, h) if w and h else
                   (int(rng.integers(0, tile_w)), int(rng.integers(0, tile_h)), 0, 0))
    return out


def case_geometry():
    """Widths 1..9 x slot bases of every residue mod 4 (a leading filler rectangle shifts the base), heights 1..3; empty
    rectangles interleaved."""
    rng = np.random.default_rng(11)
    wh = []
    for w in range(1, 10):
        for res in range(4):
            fill = (res - sum(a * b for a, b in wh)) % 4
            if fill:
                wh.append((fill, 1))
            wh.append((w, int(rng.integers(1, 4))))
            if (w + res) % 3 == 0:
                wh.append((0, 0))
    return Case("geometry", 12, 6, _pack(wh, 12, 6, rng), 11, width=187, height=91)   # (a frame that ends inside its last tiles)


def case_count(n):
    """n Gaussians of mixed small rectangles (n = 1, 15, 16, 17, 63, 64, 65, 255, 256, 257, 1100: the run and wave edges,
    and five workgroups whose runs of 16 interleave)."""
    rng = np.random.default_rng(100 + n)
    wh = [(int(rng.integers(1, 5)), int(rng.integers(1, 4))) if rng.random() > 0.1 else (0, 0) for _ in range(n)]
    wh[0] = (5, 3)
    return Case(f"count{n}", 10, 6, _pack(wh, 10, 6, rng), 100 + n, opacity=(0.02, 0.12), reach=(0.5, 0.5) if n == 1 else (0.3, 0.9))


COUNTS = (1, 15, 16, 17, 63, 64, 65, 255, 256, 257, 1100)


def case_rounds():
    """One wave's rectangles with more than 64 rows: Gaussian 12 (1 x 9) straddles row 64 of the first round, the wave goes
    on through a second and into a third round (rows 0..~150); further runs of the same wave follow 64 Gaussians on."""
    rng = np.random.default_rng(21)
    wh = [(2, 5)] * 12 + [(1, 9)] + [(3, 5)] * 3              # run 0 of wave 0: rows 0..59, 60..68, 69..83
    wh += [(1, 1)] * (16 * 3)                                  # runs of waves 1..3
    wh += [(2, 7)] * 8 + [(1, 6)] * 8                          # run 1 of wave 0 (Gaussians 64..79): rows 84..187
    wh += [(1, 2)] * 20
    return Case("rounds", 6, 10, _pack(wh, 6, 10, rng), 21, opacity=(0.02, 0.12))


def case_big():
    """Rectangles around the 256-tile threshold of the one-wave path on a 17 x 17-tile frame: 255 = 15 x 17 and 17 x 15,
    256 = 16 x 16 (twice), 272 = 16 x 17, 289 = 17 x 17, small and empty ones between them (257 = 257 x 1: case_big_strip)."""
    wh = [(2, 2), (15, 17), (1, 3), (16, 16), (0, 0), (16, 17), (3, 1), (17, 15), (17, 17), (2, 1), (16, 16)]
    rng = np.random.default_rng(31)
    return Case("big", 17, 17, _pack(wh, 17, 17, rng), 31, opacity=(0.02, 0.1))


def case_big_strip():
    """257 = 257 x 1 tiles, 256 = 256 x 1 and 255 = 255 x 1 on a 257 x 1-tile strip (the widest rows: 65 trips)."""
    wh = [(255, 1), (2, 1), (256, 1), (257, 1), (5, 1)]
    rng = np.random.default_rng(32)
    return Case("big_strip", 257, 1, _pack(wh, 257, 1, rng), 32, opacity=(0.02, 0.1))


def case_tall():
    """4 x 66 tiles on a 64 x 1056-pixel frame: a big rectangle with more than 64 rows (two rounds of the big path)."""
    wh = [(1, 2), (4, 66), (2, 30), (4, 65), (3, 66), (1, 1)]
    rng = np.random.default_rng(33)
    return Case("tall", 4, 66, _pack(wh, 4, 66, rng), 33, opacity=(0.02, 0.1))


def case_many_big(n_big=4200):
    """More than 4096 rectangles of 256 tiles (the whole 256 x 256 frame) with small ones between: the second trip of the
    big path's stride loop.  Opacities just above 1/255 keep every list open."""
    rng = np.random.default_rng(41)
    rects = []
    for i in range(n_big):
        rects.append((0, 0, 16, 16))
        if i % 64 == 0:
            rects.append((int(rng.integers(0, 14)), int(rng.integers(0, 15)), 3, 2))
    c = Case("many_big", 16, 16, rects, 41, opacity=(0.0042, 0.0048), anywhere=True)
    # the small ones keep their designed rectangles; the big ones' conics are wide (a third of the frame)
    big = (c.rects[:, 2] * c.rects[:, 3]) >= 256
    small = Case("many_big_small", 16, 16, c.rects[~big], 42, opacity=(0.0042, 0.0048))
    c.means2d[~big], c.radii[:, ~big], c.conics[~big] = small.means2d, small.radii, small.conics
    s = rng.uniform(100.0, 160.0, (int(big.sum()), 2))
    c.conics[big] = np.stack([1.0 / s[:, 0] ** 2, np.zeros(len(s)), 1.0 / s[:, 1] ** 2], 1).astype(np.float32)
    return c


def case_channels():
    """Small rectangles at slot bases of every residue mod 4 (the wide kernel's `lead`), a few dozen Gaussians."""
    rng = np.random.default_rng(51)
    wh = [(int(rng.integers(1, 6)), int(rng.integers(1, 4))) if rng.random() > 0.1 else (0, 0) for _ in range(90)]
    wh[:4] = [(1, 1), (2, 1), (1, 3), (3, 1)]                  # bases 0, 1, 3, 6(=2 mod 4), then 9(=1)...
    return Case("channels", 8, 5, _pack(wh, 8, 5, rng), 51, opacity=(0.03, 0.2))


def case_zero_opacity():
    rng = np.random.default_rng(61)
    wh = [(int(rng.integers(1, 5)), int(rng.integers(1, 4))) for _ in range(40)]
    return Case("zero_opacity", 8, 5, _pack(wh, 8, 5, rng), 61, zero_opacity=(0, 7, 16, 39))


def case_overflow():
    """Lists cut by the capacity: small rectangles, then big ones -- more big ones wholly past the capacity than a big
    list has room for -- see overflow_capacities()."""
    rng = np.random.default_rng(71)
    wh = [(int(rng.integers(1, 7)), int(rng.integers(1, 5))) for _ in range(40)] + [(16, 16)] * 3 + [(3, 2)] * 5
    return Case("overflow", 16, 16, _pack(wh, 16, 16, rng), 71, opacity=(0.02, 0.1), reach=(0.2, 0.9))


def overflow_capacities(case):
    """Capacities that are no multiple of 4 and cut a rectangle mid-row and mid-trip: inside a small rectangle of width
    >= 3 (one past its first row's first slot ... ) and inside the first big one."""
    pi = case.pair_info().astype(np.int64)
    w, h = pi[:, 3] & 0xffff, pi[:, 3] >> 16
    caps = []
    g = int(np.nonzero((w >= 3) & (h >= 2) & (np.arange(len(pi)) > 30))[0][0])
    for c in (pi[g, 0] + w[g] + 1, pi[g, 0] + w[g] + 2):       # second row, second / third slot
        caps.append(int(c))
    gb = int(np.nonzero(w * h >= 256)[0][0])
    caps.append(int(pi[gb, 0] + 16 * 5 + 7))                   # sixth row of the first big rectangle, mid-trip
    return [c if c % 4 else c + 1 for c in caps]


def case_segments(interval):
    """Segmented walk on 17 x 16 = 272 tiles (two table workgroups).  Rows 0 and 1 of the grid hold only: tile (0,0) EMPTY;
    tile (1,0) a stack of exactly `interval` one-tile Gaussians whose farthest one covers every pixel, so the walk ends on
    the LAST entry of a segment; tile (2,0) a stack of interval + 1, so it ends on the FIRST entry of the second segment.
    From row 2 down: stacks of random length up to 2.5 intervals on 30 tiles and rectangles of several tiles across them."""
    rng = np.random.default_rng(81 + interval)
    rects, closers = [], []
    for tx, length in ((1, interval), (2, interval + 1)):
        rects += [(tx, 0, 1, 1)] * length
        closers.append(len(rects) - 1)
    for _ in range(30):
        tx, ty = int(rng.integers(0, 17)), int(rng.integers(2, 16))
        rects += [(tx, ty, 1, 1)] * int(rng.integers(1, int(2.5 * interval)))
    for _ in range(5 * interval):
        w, h = int(rng.integers(2, 7)), int(rng.integers(1, 5))
        rects.append((int(rng.integers(0, 17 - w + 1)), int(rng.integers(2, 16 - h + 1)), w, h))
    c = Case(f"segments{interval}", 17, 16, rects, 81 + interval, opacity=(0.006, 0.012), reach=(0.2, 0.9))
    for j, g in enumerate(closers):       # the farthest of its stack, flat over the tile, strong enough to count everywhere
        c.conics[g] = (1.0 / 1600.0, 0.0, 1.0 / 1600.0)
        c.opacities[g] = 0.3
        c.depths[g] = c.n + 10.0 + j
    return c


# ---- the cases the GPU module runs (tests/test_bwd_reduce_host.py runs the same ones on the stand-in records) -------------------
_BUILT = {}


def built(builder, *args):
    key = (builder.__name__,) + args
    if key not in _BUILT:
        _BUILT[key] = builder(*args)
    return _BUILT[key]


def gpu_cases():
    """(id, builder, builder args, channels, absgrad, capacity index or None, checkpoint interval)."""
    out = [("geometry-c3", case_geometry, (), 3, False, None, 0), ("geometry-c3-abs", case_geometry, (), 3, True, None, 0)]
    out += [(f"count{n}", case_count, (n,), 3, False, None, 0) for n in COUNTS]
    out += [("rounds-c4-abs", case_rounds, (), 4, True, None, 0), ("rounds-c2", case_rounds, (), 2, False, None, 0)]
    out += [("big-c3", case_big, (), 3, False, None, 0), ("big-c4-abs", case_big, (), 4, True, None, 0),
            ("big_strip-c3", case_big_strip, (), 3, False, None, 0), ("tall-c3", case_tall, (), 3, False, None, 0),
            ("many_big-c1", case_many_big, (), 1, False, None, 0)]
    for ch in (1, 2, 3, 4, 5, 12, 20, 32):
        out += [(f"channels-c{ch}", case_channels, (), ch, False, None, 0), (f"channels-c{ch}-abs", case_channels, (), ch, True, None, 0)]
    out += [("zero_opacity-c3", case_zero_opacity, (), 3, False, None, 0), ("zero_opacity-c8", case_zero_opacity, (), 8, False, None, 0)]
    out += [(f"overflow{i}-c3-abs", case_overflow, (), 3, True, i, 0) for i in range(3)]
    out += [("overflow0-c5", case_overflow, (), 5, False, 0, 0), ("overflow2-c12-abs", case_overflow, (), 12, True, 2, 0)]
    out += [("segments64-c3", case_segments, (64,), 3, False, None, 64), ("segments256-c4-abs", case_segments, (256,), 4, True, None, 256)]
    return out


def capacity_of(case, cap_index):
    """The list capacity of a GPU case: a few slots more than the lists need, or one of overflow_capacities()."""
    return case.n_isect() + 5 if cap_index is None else overflow_capacities(case)[cap_index]
