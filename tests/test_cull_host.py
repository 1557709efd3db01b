"""CPU test of the raster's cull (robosimgs_amd/csrc/raster_common.h: quadrant_mask for the one-wave-per-tile kernels,
rect_min_sigma for the per-block kernel), compiled with g++ behind shims for the device qualifiers and the rcp / log /
med3 builtins.  Both bounds are taken against fp64 arithmetic on the same fp32 inputs, never against the code under test:

  (a) conservative: a quadrant that holds a pixel centre whose fp32 alpha -- the kernels' own chain, poly_coefs /
      pair_power_poly / exp2 -- is at least 1/255 has its bit set.  Zero exceptions.
  (b) tight: no bit is set where the fp64 minimum of sigma over the quadrant's rectangle of pixel centres exceeds
      lim = ln(255 opacity) + slack by more than 1e-3 relative plus 1e-3 absolute.
"""
import ctypes
import os
import subprocess

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
N = 1 << 20
EDGES = np.array([0.5, 7.5, 8.5, 15.5])


@pytest.fixture(scope="module")
def lib(tmp_path_factory):
    so = tmp_path_factory.mktemp("cull") / "libcull.so"
    subprocess.run(["g++", "-O2", "-std=c++17", "-shared", "-fPIC", "-ffp-contract=off",
                    os.path.join(HERE, "host_harness", "cull_harness.cpp"), "-o", str(so)], check=True)
    return ctypes.CDLL(str(so))


def _cases(n=N, seed=7):
    """(mean, conic, opacity, tile) cases in fp32: means inside, on the edge lines of, and up to 40 px outside the tile;
    conics of eigenvalues up to 1 / 0.3 (the 2D covariance carries eps2d = 0.3) with ratios down to 1e-4; opacities
    uniform, at 1/255 and one ulp to either side, at 0.999, and log-uniform just above the threshold; one case in 512
    has a NaN mean, conic or opacity."""
    rng = np.random.default_rng(seed)
    tile_x = 16.0 * rng.integers(0, 120, n)
    tile_y = 16.0 * rng.integers(0, 68, n)
    kind = rng.integers(0, 10, n)
    ox, oy = rng.uniform(-40.0, 56.0, n), rng.uniform(-40.0, 56.0, n)
    inside = kind < 2
    ox[inside], oy[inside] = rng.uniform(0.0, 16.0, inside.sum()), rng.uniform(0.0, 16.0, inside.sum())
    on_x, on_y, centre = kind == 2, kind == 3, kind == 4
    ox[on_x] = EDGES[rng.integers(0, 4, on_x.sum())]            # on a vertical edge line, any height
    oy[on_y] = EDGES[rng.integers(0, 4, on_y.sum())]
    ox[centre] = rng.integers(0, 16, centre.sum()) + 0.5        # exactly on a pixel centre
    oy[centre] = rng.integers(0, 16, centre.sum()) + 0.5
    mx, my = (tile_x + ox).astype(np.float32), (tile_y + oy).astype(np.float32)
    l1 = 10.0 ** rng.uniform(-3.0, np.log10(1.0 / 0.3), n)
    l2 = l1 * 10.0 ** rng.uniform(-4.0, 0.0, n)
    l2[::5] = l1[::5] * 1e-4                                    # the ratio's end
    th = rng.uniform(0.0, np.pi, n)
    cs, sn = np.cos(th), np.sin(th)
    a, c, b = l1 * cs * cs + l2 * sn * sn, l1 * sn * sn + l2 * cs * cs, (l1 - l2) * cs * sn
    op = rng.uniform(0.0, 1.0, n).astype(np.float32)
    ok = rng.integers(0, 10, n)
    t = np.float32(1.0 / 255.0)
    op[ok == 0] = t
    op[ok == 1] = np.nextafter(t, np.float32(0.0))
    op[ok == 2] = np.nextafter(t, np.float32(1.0))
    op[ok == 3] = np.float32(0.999)
    near = ok == 4
    op[near] = (10.0 ** rng.uniform(np.log10(1.0 / 255.0), np.log10(0.02), near.sum())).astype(np.float32)
    f = lambda v: np.ascontiguousarray(v, dtype=np.float32)
    mx, my, a, b, c = f(mx), f(my), f(a), f(b), f(c)
    for i, v in enumerate((mx, my, a, b, c, op)):
        v[512 * np.arange(n // 3072) * 6 + 512 * i] = np.nan
    return dict(mx=f(mx), my=f(my), a=f(a), b=f(b), c=f(c), op=f(op), tile_x=f(tile_x), tile_y=f(tile_y))


def _call(fn, z):
    n = len(z["mx"])
    out = np.zeros(n, np.uint8)
    p = lambda v: v.ctypes.data_as(ctypes.c_void_p)
    fn(n, *(p(z[k]) for k in ("mx", "my", "a", "b", "c", "op", "tile_x", "tile_y")), p(out))
    return out


def _rect_min_fp64(z):
    """fp64 minimum of 0.5 (a dx^2 + c dy^2) + b dx dy over each quadrant's rectangle of pixel centres, [n, 4]: zero when
    the mean lies inside, otherwise on an edge -- the clamped minimiser of the quadratic along that edge."""
    d = {k: v.astype(np.float64) for k, v in z.items()}
    out = np.empty((len(d["mx"]), 4))

    def edge(e, wu, wv, lo, hi):
        with np.errstate(all="ignore"):
            v = np.clip(-d["b"] * e / wv, lo, hi)
        return 0.5 * (wu * e * e + wv * v * v) + d["b"] * e * v

    for k in range(4):
        x0 = d["tile_x"] + 8.0 * (k & 1) + 0.5 - d["mx"]
        y0 = d["tile_y"] + 8.0 * (k >> 1) + 0.5 - d["my"]
        x1, y1 = x0 + 7.0, y0 + 7.0
        s = np.minimum(np.minimum(edge(x0, d["a"], d["c"], y0, y1), edge(x1, d["a"], d["c"], y0, y1)),
                       np.minimum(edge(y0, d["c"], d["a"], x0, x1), edge(y1, d["c"], d["a"], x0, x1)))
        out[:, k] = np.where((x0 <= 0) & (x1 >= 0) & (y0 <= 0) & (y1 >= 0), 0.0, s)
    return out


def _lim_fp64(z):
    d = {k: v.astype(np.float64) for k, v in z.items()}
    fx = np.maximum(np.abs(d["tile_x"] - d["mx"]), np.abs(d["tile_x"] + 16.0 - d["mx"]))
    fy = np.maximum(np.abs(d["tile_y"] - d["my"]), np.abs(d["tile_y"] + 16.0 - d["my"]))
    slack = 0.05 + 4e-6 * (np.abs(d["a"]) + np.abs(d["c"]) + 2.0 * np.abs(d["b"])) * (fx * fx + fy * fy)
    with np.errstate(all="ignore"):
        return np.log(255.0 * d["op"]) + slack


@pytest.fixture(scope="module")
def reference(lib):
    """The cases and what both bounds are taken against, computed once."""
    z = _cases()
    return dict(z=z, reached=_call(lib.ch_reached, z), smin=_rect_min_fp64(z), lim=_lim_fp64(z))


@pytest.mark.parametrize("which", ["ch_quadrant_mask", "ch_block_mask"])
def test_cull_is_conservative_and_tight(lib, reference, which):
    z, reached, smin, lim = (reference[k] for k in ("z", "reached", "smin", "lim"))
    mask = _call(getattr(lib, which), z)
    assert len(mask) >= 1_000_000
    # the cases do exercise both answers, the threshold opacities and the needle conics
    frac = np.array([(mask >> k & 1).mean() for k in range(4)])
    assert (frac > 0.1).all() and (frac < 0.9).all(), frac
    assert ((reached != 0) & (z["op"] < 0.0040)).sum() > 1000
    # NaN: a NaN mean or conic keeps every quadrant (the pixel test then rejects the pair), a NaN opacity reaches nothing,
    # and neither does one well below 1/255
    nan_geo = np.isnan(z["mx"]) | np.isnan(z["my"]) | np.isnan(z["a"]) | np.isnan(z["b"]) | np.isnan(z["c"])
    assert nan_geo.sum() > 500 and np.isnan(z["op"]).sum() > 100
    assert (mask[nan_geo & (z["op"] >= np.float32(1.0 / 255.0))] == 15).all()
    assert ((reached & ~mask)[z["op"] < np.float32(1.0 / 255.0)] == 0).all()    # an ulp below 1/255 the blend can still count
    assert (mask[np.isnan(z["op"])] == 0).all()
    assert (mask[z["op"] < np.float32(0.9 / 255.0)] == 0).all() and (z["op"] < np.float32(0.9 / 255.0)).sum() > 1000
    # (a) zero exceptions
    missed = reached & ~mask
    print(f"{which}: {int((reached != 0).sum())} cases reach a quadrant, {int((missed != 0).sum())} missed")
    assert not missed.any(), np.flatnonzero(missed)[:10]
    # (b) a set bit means the exact minimum is within 1e-3 relative + 1e-3 absolute of lim
    for k in range(4):
        bit = (mask >> k & 1).astype(bool) & ~nan_geo          # (no minimum to hold a NaN case to)
        over = smin[bit, k] - (lim[bit] + 1e-3 * np.abs(lim[bit]) + 1e-3)
        print(f"{which}: quadrant {k}: {int(bit.sum())} set, largest excess over the bound {over.max():.3e}")
        assert (over <= 0).all(), (k, over.max())


def test_closed_quadrants_are_skipped_and_change_no_other_bit(lib):
    """quadrant_mask(..., live) == quadrant_mask(...) & live for every set of open quadrants."""
    z = {k: v[:65536] for k, v in _cases(65536, seed=3).items()}
    full = _call(lib.ch_quadrant_mask, z)
    p = lambda v: v.ctypes.data_as(ctypes.c_void_p)
    for live in range(16):
        out = np.full(len(full), 255, np.uint8)
        lib.ch_quadrant_mask_live(len(full), *(p(z[k]) for k in ("mx", "my", "a", "b", "c", "op", "tile_x", "tile_y")), live, p(out))
        assert np.array_equal(out, full & live), live
