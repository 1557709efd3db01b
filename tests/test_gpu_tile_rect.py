"""The tile rectangles as the kernels run them (robosimgs_amd/csrc/tile_rect.h inside tile_count_kernel, binning.hip, and
inside the seed of project_color_fwd_kernel, projection.hip) against the fp64 reference of tests/tile_rect_ref.py -- the
cases and the sandwich of tests/test_tile_rect_host.py, which holds a g++ build of the same header on the CPU -- and the
rule's contract on those cases: lists from tightened rectangles render and differentiate to the same bits as the classic
ones.  numpy fp64 only; nothing is compiled here.
"""
import numpy as np
import pytest
import torch

import project_color_ref as PR
from guard_bands import guarded_empty, guards_intact as _guards_intact
import tile_rect_ref as R

pytestmark = pytest.mark.gpu

DEV = "cuda"
W, H, TW, TH = 640, 480, 40, 30


def _t(a, dtype=torch.float32):
    return torch.from_numpy(np.ascontiguousarray(a)).to(dtype).to(DEV)


def _np(t):
    return t.detach().cpu().numpy()


def _bits(t):
    return t.contiguous().view(torch.int32)


@pytest.fixture(scope="module")
def ops():
    from robosimgs_amd import ops as _ops
    return _ops


def _radii(z, planar):
    """[N] under the classic rule, planar [2, N] per-axis extents."""
    return _t(np.stack([z["rx"], z["ry"]]), torch.int32) if planar else _t(z["rx"], torch.int32)


def _depths(n, seed):
    return np.random.default_rng(seed).uniform(0.5, 30.0, n).astype(np.float32)


def _isect(ops, z, planar, tw, th, cap, tight=True, **kw):
    m2d, con = _t(np.stack([z["mx"], z["my"]], axis=1)), _t(np.stack([z["a"], z["b"], z["c"]], axis=1))
    more = dict(conics=con, opacities=_t(z["op"])) if tight else {}
    return ops.isect_tiles_raw(m2d, _radii(z, planar), _t(_depths(len(z["mx"]), 3)), tw, th, cap, want_pair_info=True, **more, **kw)


def _rect_of_pair_info(pi):
    pi = pi.astype(np.int64)
    return np.stack([pi[:, 1], pi[:, 2], pi[:, 3] & 0xffff, pi[:, 3] >> 16], axis=1)


def _rect_of_lists(flat, offsets, n, tw):
    """x0, y0, w, h of every Gaussian from the lists themselves, its entry count, and whether its tiles fill that box."""
    tile = np.repeat(np.arange(len(offsets) - 1), np.diff(offsets))
    tx, ty = tile % tw, tile // tw
    big = 1 << 30
    x0, y0, x1, y1 = np.full(n, big), np.full(n, big), np.full(n, -1), np.full(n, -1)
    np.minimum.at(x0, flat, tx), np.minimum.at(y0, flat, ty), np.maximum.at(x1, flat, tx), np.maximum.at(y1, flat, ty)
    cnt = np.bincount(flat, minlength=n)
    has = cnt > 0
    rect = np.where(has[:, None], np.stack([x0, y0, x1 - x0 + 1, y1 - y0 + 1], axis=1), 0)
    return rect, cnt, np.array_equal(cnt, rect[:, 2] * rect[:, 3])


class Stage:
    """One set of cases through the operator path with room to spare: the lists, the rectangles and the counts."""

    def __init__(self, ops, z, planar, tw, th):
        self.z, self.planar, self.tw, self.th, self.n = z, planar, tw, th, len(z["mx"])
        self.classic = R.classic_rects(z)
        self.cap = int((self.classic[:, 2] * self.classic[:, 3]).sum()) + 16
        tl = _isect(ops, z, planar, tw, th, self.cap)
        torch.cuda.synchronize()
        self.tl = tl
        self.n_isect, self.status = int(tl.n_isect.item()), int(tl.status.item())
        self.rect = _rect_of_pair_info(_np(tl.pair_info))
        self.tpg = _np(tl.tiles_per_gauss).astype(np.int64)
        self.flat, self.offsets = _np(tl.flatten_ids)[:self.n_isect].astype(np.int64), _np(tl.tile_offsets).astype(np.int64)


CASES = {"classic": (4096, TW, TH, 11, False), "per_axis": (4096, TW, TH, 12, True),
         "wide": (512, 1023, 2, 13, False), "wide_per_axis": (512, 1023, 2, 14, True)}
_stages = {}


@pytest.fixture(scope="module")
def stage(ops):
    def get(name):
        if name not in _stages:
            n, tw, th, seed, per_axis = CASES[name]
            _stages[name] = Stage(ops, R.cases(n, tw, th, seed, per_axis=per_axis), per_axis, tw, th)
        return _stages[name]
    yield get
    _stages.clear()


@pytest.mark.parametrize("name", list(CASES))
def test_operator_rectangles_meet_the_fp64_sandwich(stage, name):
    """isect_tiles_raw(conics=, opacities=, want_pair_info=True): every Gaussian's rectangle, read from pair_info and
    rebuilt from the lists, is held to the sandwich box(E) <= tight <= box(1.001 E + 0.02) of tests/tile_rect_ref.py, to
    the classic rectangle exactly where the fp32 path falls back and to empty under the opacity gate; n_isect is the sum
    of the counts."""
    s = stage(name)
    assert s.status == 0 and s.n_isect <= s.cap
    cnt = s.rect[:, 2] * s.rect[:, 3]
    assert s.n_isect == cnt.sum() and np.array_equal(s.tpg, cnt) and s.offsets[-1] == s.n_isect
    from_lists, cnt_lists, filled = _rect_of_lists(s.flat, s.offsets, s.n, s.tw)
    assert filled and np.array_equal(cnt_lists, cnt)
    assert np.array_equal(from_lists, s.rect)                    # (pair_info is 0 0 0 0 where the count is 0, like the lists)
    # an empty rectangle leaves pair_info at 0 0 0 0: give the reference's comparison the corner the rule keeps
    rect = np.where((cnt > 0)[:, None], s.rect, np.concatenate([s.classic[:, :2], np.zeros((s.n, 2), np.int64)], axis=1))
    rect[~(s.z["rx"] > 0)] = 0
    fb = R.branches(s.z)["fallback"] & (cnt == 0)
    rect[fb] = np.where((s.classic[fb, 2] * s.classic[fb, 3] == 0)[:, None], s.classic[fb], rect[fb])   # (count 0: extents unseen)
    v = R.sandwich(s.z, rect, s.classic)
    print(f"{name}: n_isect {s.n_isect} of {int((s.classic[:, 2] * s.classic[:, 3]).sum())} classic pairs; "
          + ", ".join(f"{k} {int(v[k].sum())}" for k in ("regular", "fallback", "borderline", "low", "culled")))
    for k in ("bad_inner", "bad_outer", "bad_fallback", "bad_either", "bad_low", "bad_culled"):
        assert not v[k].any(), (k, int(v[k].sum()), np.flatnonzero(v[k])[:10])
    assert v["regular"].sum() > s.n // 2
    if not s.planar:                                             # (the per-axis rule leaves nothing under 1/255 to the rectangle)
        assert v["low"].sum() > s.n // 100 and (cnt[v["low"]] == 0).all()
        assert s.n < 4096 or np.isnan(s.z["op"][v["low"]]).any()
        assert (cnt < (s.classic[:, 2] * s.classic[:, 3])).sum() > s.n // 8


@pytest.mark.parametrize("name", list(CASES))
def test_exact_and_short_capacity(ops, stage, name):
    """Capacity exactly n_isect: the same lists, no overflow.  One less: the overflow status is set, n_isect still reports
    the need, and nothing is written past any buffer of the call (0xA5 guards behind each)."""
    from robosimgs_amd import _lib
    s = stage(name)
    with guarded_empty() as guards:
        tl = _isect(ops, s.z, s.planar, s.tw, s.th, s.n_isect)
    torch.cuda.synchronize()
    assert int(tl.status.item()) == 0 and int(tl.n_isect.item()) == s.n_isect
    assert torch.equal(tl.flatten_ids, s.tl.flatten_ids[:s.n_isect]) and torch.equal(tl.tile_offsets, s.tl.tile_offsets)
    assert torch.equal(tl.pair_info, s.tl.pair_info) and torch.equal(tl.tiles_per_gauss, s.tl.tiles_per_gauss)
    assert len(guards) >= 8 and _guards_intact(guards)
    with guarded_empty() as guards:
        tl = _isect(ops, s.z, s.planar, s.tw, s.th, s.n_isect - 1)
    torch.cuda.synchronize()
    assert int(tl.status.item()) & _lib.MGS_STATUS_ISECT_OVERFLOW and int(tl.n_isect.item()) == s.n_isect
    off = _np(tl.tile_offsets)
    assert off.min() >= 0 and off.max() <= s.n_isect - 1 and np.all(np.diff(off) >= 0)
    assert len(guards) >= 8 and _guards_intact(guards)


@pytest.mark.parametrize("name", ["classic", "per_axis", "wide"])
def test_dropped_tiles_fail_the_alpha_test_in_fp64(stage, name):
    """Every tile in classic \\ tight: the fp64 minimum of sigma over the tile's 16 x 16 pixel centres exceeds
    ln(255 o) (the construction of test_cull_host._rect_min_fp64 on the 16 x 16 rectangle; where that lower bound does not
    decide, the centres themselves).  No tolerance: the rule's slack is at least 0.05."""
    s = stage(name)
    case, tx, ty = R.dropped_pairs(s.classic, s.rect)
    a, b, c, o = (s.z[k].astype(np.float64) for k in ("a", "b", "c", "op"))
    ok = (a > 0) & (c > 0) & (a * c - b * b > 0) & np.isfinite(s.z["mx"]) & np.isfinite(s.z["my"]) & np.isfinite(o) & (o > 0)
    keep = ok[case]
    case, tx, ty = case[keep], tx[keep], ty[keep]
    smin = R.tile_min_sigma_f64(s.z, case, tx, ty)                # over the rectangle the centres span: a lower bound ...
    thr = np.log(255.0 * o[case])
    close = np.flatnonzero(~(smin > thr))                          # ... that a Gaussian between two centres does not meet:
    smin[close] = R.tile_centres_min_sigma_f64(s.z, case[close], tx[close], ty[close])      # the 256 centres one by one
    print(f"{name}: {len(case)} dropped (tile, Gaussian) pairs, {len(close)} of them judged centre by centre, smallest sigma_min - ln(255 o) = {(smin - thr).min():.4f}")
    assert len(case) > 1000 and (smin > thr).all(), np.flatnonzero(~(smin > thr))[:10]
    # what is left out above has nothing dropped at all, but for opacities the raster never evaluates
    rest = ~ok & (s.z["op"] >= R.GATE)
    assert np.array_equal(s.rect[rest, 2] * s.rect[rest, 3], (s.classic[:, 2] * s.classic[:, 3])[rest])


@pytest.mark.parametrize("ch", [3, 4])
def test_tight_and_classic_lists_render_and_differentiate_to_the_same_bits(ops, stage, ch):
    """The contract on the adversarial cases: rasterize_to_pixels and both raster schedules (one wave per tile, one per
    8 x 8 block) give bit-identical render and alpha and the same last Gaussian at every pixel (last_ids themselves are
    list positions) from the classic and from the tightened lists, and the whole-list deterministic backward
    bit-identical gradients (NaN rows of NaN inputs included), up to the sign of a zero."""
    s = stage("classic")
    z, n = s.z, s.n
    classic = _isect(ops, z, False, TW, TH, s.cap, tight=False)
    assert int(classic.status.item()) == 0 and int(classic.n_isect.item()) > s.n_isect
    rng = np.random.default_rng(20 + ch)
    m2d, con = _t(np.stack([z["mx"], z["my"]], axis=1)), _t(np.stack([z["a"], z["b"], z["c"]], axis=1))
    op, col = _t(z["op"]), _t(rng.uniform(0.0, 1.0, (n, ch)).astype(np.float32))
    bg = _t(rng.uniform(0.0, 1.0, ch).astype(np.float32))
    vr, va = _t(rng.normal(size=(H, W, ch)).astype(np.float32)), _t(rng.normal(size=(H, W)).astype(np.float32))
    outs = {}
    for key, tl in (("classic", classic), ("tight", s.tl)):
        k = int(tl.n_isect.item())
        img, alpha = ops.rasterize_to_pixels(m2d[None], con[None], col[None], op[None], W, H, 16,
                                             tl.tile_offsets[:-1].reshape(1, TH, TW), tl.flatten_ids[:k], backgrounds=bg[None])
        res = [img[0], alpha[0, ..., 0]]
        for latency in (False, True):
            r, a, last = ops.rasterize_fwd_raw(m2d, con, col, op, bg, W, H, TW, TH, tl.tile_offsets, tl.flatten_ids, latency=latency)
            res += [r, a, _t(_last_gaussian(last, tl), torch.int32)]
            if not latency:
                grads = ops.rasterize_bwd_det_raw(m2d, con, col, op, bg, W, H, TW, TH, tl, a, last, vr, va, absgrad=True)
        outs[key] = res + list(grads)
    torch.cuda.synchronize()
    names = ("render", "alpha", "render/tile", "alpha/tile", "last_ids/tile", "render/block", "alpha/block", "last_ids/block",
             "v_means2d", "v_conics", "v_colors", "v_opacities", "v_means2d_abs")
    for name, x, y in zip(names, outs["classic"], outs["tight"]):
        # Gradients: the same bits, but for the sign of a zero -- a Gaussian that blends nowhere gets -0 from the empty
        # sums over its classic slots and +0 where the tightened rectangle leaves it no slot at all (422 opacity and one
        # mean gradient of these 4,096 cases; torch.equal, which the rule's other tests use, does not see it either).
        same = _bits(x) == _bits(y)
        if name.startswith("v_"):
            same |= (x == 0) & (y == 0)
        assert bool(same.all()), (name, int((~same).sum()))
    t = outs["tight"]
    assert torch.equal(_bits(t[0]), _bits(t[2])) and torch.equal(_bits(t[1]), _bits(t[3]))
    assert bool((t[1] > 0.9).any()) and int((t[4] >= 0).sum()) > H * W // 2          # (the frame is not empty)
    # threshold opacities do blend: Gaussians at 1/255 +- an ulp are some pixel's last contributor
    last = _np(t[4])
    assert np.array_equal(last, _np(t[7]))
    thr_ids = np.flatnonzero(np.abs(z["op"] - R.T255) <= 1e-9)
    print(f"ch {ch}: {np.isin(last, thr_ids).sum()} pixels end on a Gaussian at 1/255 +- an ulp")


def _last_gaussian(last, tl):
    """last_ids are positions in the sorted lists, which differ between two list flavours: the Gaussian each names, or
    -1 where the position lies outside the pixel's own tile list (no Gaussian blended)."""
    last, off, flat = _np(last).astype(np.int64), _np(tl.tile_offsets).astype(np.int64), _np(tl.flatten_ids).astype(np.int64)
    ys, xs = np.mgrid[0:H, 0:W]
    tile = (ys // 16) * TW + xs // 16
    inside = (last >= off[tile]) & (last < off[tile + 1])
    return np.where(inside, flat[np.clip(last, 0, len(flat) - 1)], -1)


def _behind(case, every=7):
    """The case with every 7th mean mirrored through the camera centre: behind the camera."""
    vm = case["viewmat"].astype(np.float64)
    campos = -vm[:3, :3].T @ vm[:3, 3]
    c = dict(case)
    means = case["means"].astype(np.float64).copy()
    means[::every] = 2.0 * campos - means[::every]
    c["means"] = np.ascontiguousarray(means, dtype=np.float32)
    return c


def _words(a):
    """The 32-bit words of a float32 or int32 tensor, as int64."""
    return _np(a.contiguous()).view(np.uint32).astype(np.int64)


@pytest.mark.parametrize("n", [1, 63, 64, 65, 257])
def test_projection_seed_is_the_operator_rectangle(ops, n):
    """mgs_project_color_fwd's binning seed against the operator path on that call's own means2d / radii / conics and the
    opacity the blend sees (the plain one; opac_out when anti-aliased and when raw), under both radius rules, both
    parameter forms and both seeds: seed_info bit for bit (the rectangle word where pair_info shows it, the count
    everywhere), (kEmptyTileRect, 0) on invisible rows, seed_sums the count sum per 64 rows with nothing written behind
    them, the same lists from the seed as from the arrays, lean=True the same seed / records / depths, and words 0-9 of
    the packed records {x, y, a, b | c, opacity, f0, f1 | f2, f3} (projection.hip) equal to the arrays."""
    tw, th = ops.tile_grid(PR.W, PR.H)
    visible_rows = 0
    for raw in (False, True):
        case = _behind(PR.scene_case("pinhole", raw, n=n, mu=0.1, seed=n))
        dev = {k: _t(case[k]) for k in ("means", "quats", "scales", "opac", "sh", "viewmat")}
        K = _t(case["K"])
        for aa in (False, True):
            for per_axis in (False, True):
                for bin_seed in ("tight", "classic"):
                    call = lambda **kw: ops.project_color_fwd_raw(
                        dev["means"], dev["quats"], dev["scales"], dev["opac"], 3, dev["sh"], dev["viewmat"], K, PR.W, PR.H,
                        PR.EPS2D, PR.NEAR, 1e10, 0.0, aa, True, want_splats=True, bin_seed=bin_seed, per_axis=per_axis, raw=raw, **kw)
                    what = (n, raw, aa, per_axis, bin_seed)
                    with guarded_empty() as guards:
                        radii, m2d, dep, con, opac, feats, splats, (info, sums) = call()
                    torch.cuda.synchronize()
                    assert _guards_intact(guards), what
                    assert sums.numel() == -(-n // 64)
                    used = opac if (aa or raw) else dev["opac"]
                    vis = _np(ops.radii_x(radii)) > 0
                    visible_rows += int(vis.sum())
                    assert not vis[::7].any(), what                           # the rows behind the camera
                    cap = ops._upper_bound_isects(radii, tw, th) + 1
                    more = dict(conics=con, opacities=used) if bin_seed == "tight" else {}
                    tl = ops.isect_tiles_raw(m2d, radii, dep, tw, th, cap, want_pair_info=True, **more)
                    rect = _rect_of_pair_info(_np(tl.pair_info))
                    cnt = rect[:, 2] * rect[:, 3]
                    got = _words(info)
                    assert np.array_equal(got[:, 1], cnt), what
                    shown = cnt > 0
                    assert np.array_equal(got[shown], R.pack(rect)[shown]), what
                    assert (got[~vis] == np.array([R.EMPTY_WORD, 0])).all(), what
                    assert ((got[:, 0] >> 20) >= 1).all() and (cnt[~vis] == 0).all(), what
                    want_sums = np.add.reduceat(cnt, np.arange(0, n, 64))
                    assert np.array_equal(_words(sums), want_sums), what
                    assert int(tl.status.item()) == 0 and int(tl.n_isect.item()) == cnt.sum()
                    # the seed gives the lists the arrays give
                    ts = ops.isect_tiles_raw(None, None, dep, tw, th, cap, want_pair_info=True, seed=(info, sums.clone()))
                    k = int(tl.n_isect.item())
                    assert int(ts.n_isect.item()) == k and int(ts.status.item()) == 0, what
                    assert torch.equal(ts.pair_info, tl.pair_info) and torch.equal(ts.tile_offsets, tl.tile_offsets), what
                    assert torch.equal(ts.flatten_ids[:k], tl.flatten_ids[:k]) and torch.equal(ts.tiles_per_gauss, tl.tiles_per_gauss), what
                    # the packed records: words 0-9 are the arrays, 10-11 zero; invisible rows are not written
                    rec = _words(splats)[vis]
                    want = np.concatenate([_words(m2d), _words(con), _words(used)[:, None], _words(feats)], axis=1)[vis]
                    assert np.array_equal(rec[:, :10], want) and (rec[:, 10:] == 0).all(), what
                    assert np.array_equal(_words(feats)[:, 3], _words(dep)), what
                    # an inference frame: nothing but depths, records and seed, the same bits
                    l_radii, l_m2d, l_dep, l_con, l_opac, l_feats, l_splats, (l_info, l_sums) = call(lean=True)
                    assert l_radii is None and l_m2d is None and l_con is None and l_feats is None
                    assert torch.equal(l_info, info) and torch.equal(l_sums, sums) and torch.equal(_bits(l_dep), _bits(dep)), what
                    assert np.array_equal(_words(l_splats)[vis], rec), what
    assert visible_rows > 0 or n == 1
