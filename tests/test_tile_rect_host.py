"""CPU test of the tile rectangles (robosimgs_amd/csrc/tile_rect.h: tile_rect, tighten_rect, pack_tile_rect), compiled
with g++ behind shims for the device qualifiers, __logf, uint2 and min / max (tests/host_harness/tile_rect_harness.cpp).
A tile the tightened rectangle drops is never seen by any later check, so the rule is held from both sides, each bound
against fp64 arithmetic on the same fp32 inputs (tests/tile_rect_ref.py), never against the code under test:

  (a) conservative, zero exceptions: every tile of the classic rectangle that holds a pixel centre whose fp32 alpha -- the
      kernels' own chain, poly_coefs about the tile centre / pair_power_poly / exp2 -- is at least 1/255 lies inside the
      tightened rectangle;
  (b) the fp64 sandwich box(E) <= tight <= box(1.001 E + 0.02), the classic rectangle exactly where the fp32 path falls
      back, either within 1e-6 relative of the determinant's branch point;
  (c) empty under the opacity gate (the raster's own, 0.95 / 255: an ulp under 1/255 the blend still counts) and for a
      NaN opacity;
  (d) the packing;  (e) the classic rectangle against the oracle, bit for bit;  (f) the cases are adversarial.
"""
import ctypes
import os
import subprocess
import time

import numpy as np
import pytest

import tile_rect_ref as R
from oracle import gs_oracle_np as O

HERE = os.path.dirname(os.path.abspath(__file__))
T0 = time.perf_counter()


@pytest.fixture(scope="module")
def lib(tmp_path_factory):
    so = tmp_path_factory.mktemp("tile_rect") / "libtile_rect.so"
    subprocess.run(["g++", "-O2", "-std=c++17", "-shared", "-fPIC", "-ffp-contract=off",
                    os.path.join(HERE, "host_harness", "tile_rect_harness.cpp"), "-o", str(so)], check=True)
    return ctypes.CDLL(str(so))


def _p(v):
    return v.ctypes.data_as(ctypes.c_void_p)


def _classic(lib, z, overload):
    out = np.zeros((len(z["mx"]), 4), np.int32)
    lib.tr_classic(len(out), *(_p(z[k]) for k in ("mx", "my", "rx", "ry", "tile_w", "tile_h")), overload, _p(out))
    return out.astype(np.int64)


def _tight(lib, z):
    n = len(z["mx"])
    rect, packed = np.zeros((n, 4), np.int32), np.zeros((n, 2), np.uint32)
    lib.tr_tight(n, *(_p(z[k]) for k in R.FIELDS + ("rx", "ry", "tile_w", "tile_h")), _p(rect), _p(packed))
    return rect.astype(np.int64), packed


def _reached(lib, z, classic, brute=0):
    n = len(z["mx"])
    bbox, evals = np.zeros((n, 4), np.int32), ctypes.c_longlong(0)
    rect = np.ascontiguousarray(classic, dtype=np.int32)
    lib.tr_reached(n, *(_p(z[k]) for k in R.FIELDS), _p(rect), brute, _p(bbox), ctypes.byref(evals))
    return bbox.astype(np.int64), evals.value


def all_cases():
    """2^18 + 14,336 cases: the 40 x 30 grid under the classic and the per-axis radius rule, and the grids at the
    packing's and the clamps' ends."""
    return R.concat([R.cases(3 << 16, 40, 30, 1), R.cases(1 << 16, 40, 30, 2, per_axis=True),
                     R.cases(4096, 1, 1, 3), R.cases(4096, 1023, 2, 4), R.cases(4096, 1023, 2, 5, per_axis=True),
                     R.cases(2048, 2, 1023, 6, giant_every=512)])


@pytest.fixture(scope="module")
def ref(lib):
    """The cases, the reference rectangles and what the harness makes of them, computed once and left unchanged."""
    z = all_cases()
    classic = R.classic_rects(z)
    t = time.perf_counter()
    reached, evals = _reached(lib, z, classic)
    print(f"reached_tiles: {len(z['mx'])} cases, {evals} pixels evaluated, {time.perf_counter() - t:.1f} s")
    tight, packed = _tight(lib, z)
    return dict(z=z, classic=classic, reached=reached, tight=tight, packed=packed, s=R.sandwich(z, tight, classic))


def test_classic_rectangle_matches_the_oracle_bit_for_bit(lib, ref):
    """(e) both tile_rect overloads == oracle.gs_oracle_np.tile_rects(dtype=float32) on every case with a finite mean (the
    oracle's float-to-int conversion of a NaN is numpy's, not the device's; such a rectangle has width 0 on either), and
    the reference module's own statement of the rule equals both."""
    z = ref["z"]
    fin = np.isfinite(z["mx"]) & np.isfinite(z["my"])
    assert (~fin).sum() > 100
    for overload, radii in ((1, z["rx"]), (2, np.stack([z["rx"], z["ry"]], axis=1))):
        got = _classic(lib, z, overload)
        mine = R.classic_rects(z, per_axis=overload == 2)
        vis = z["rx"] > 0
        assert np.array_equal(got[vis], mine[vis])              # (the bare function does not know about culled rows)
        for tw, th in {(int(w), int(h)) for w, h in zip(z["tile_w"], z["tile_h"])}:
            sel = fin & (z["tile_w"] == tw) & (z["tile_h"] == th)
            with np.errstate(invalid="ignore"):
                x0, x1, y0, y1 = O.tile_rects(np.stack([z["mx"][sel], z["my"][sel]], axis=1), radii[sel], 16, tw, th,
                                              dtype=np.float32)
            assert np.array_equal(mine[sel], np.stack([x0, y0, x1 - x0, y1 - y0], axis=1)), (overload, tw, th)
        nan_x = np.isnan(z["mx"]) & vis
        assert (got[nan_x, 2] == 0).all() and (got[np.isnan(z["my"]) & vis, 3] == 0).all()


def test_reached_tiles_accelerators_change_no_answer(lib, ref):
    """The row interval and the skip of tiles inside the box found so far (tile_rect_harness.cpp) against the plain walk
    over every pixel of the classic rectangle, on every 16th case."""
    z = R.take(ref["z"], slice(None, None, 16))
    classic = ref["classic"][::16]
    fast, e_fast = _reached(lib, z, classic)
    plain, e_plain = _reached(lib, z, classic, brute=1)
    print(f"{len(classic)} cases: {e_plain} pixels evaluated by the plain walk, {e_fast} with the accelerators")
    assert np.array_equal(fast, plain)
    assert np.array_equal(fast, ref["reached"][::16])


def test_tightened_rectangle_is_conservative(lib, ref):
    """(a) zero exceptions, and (c)'s interplay with it."""
    z, reached, tight = ref["z"], ref["reached"], ref["tight"]
    r_ok = reached[:, 2] > reached[:, 0]
    t, t_ok = R.corners(tight)
    missed = ~R._inside(reached, r_ok, t, t_ok)
    below = ~(z["op"] >= R.T255) & (z["rx"] > 0)
    print(f"{int(r_ok.sum())} cases reach a tile, {int(missed.sum())} missed; {int((r_ok & below).sum())} reach one under 1/255")
    # An ulp under 1/255 -- and further down -- the blend still counts: its fp32 alpha, exp2f(log2f(o) + ...), comes out at
    # 1/255 on a pixel centre the mean sits on, exactly as tests/test_cull_host.py documents for the quadrant cull, whose
    # gate (cull_opacity_ok, 0.95 / 255) is therefore the rule's gate too: a rectangle emptied at 1/255 missed 1,324 of
    # these cases.  Under the gate no kernel evaluates the pair, and reached_tiles reports nothing.
    assert (r_ok & below).sum() > 1000
    assert lib.tr_cull_opacity_ok(ctypes.c_float(float(R.GATE))) == 1
    assert lib.tr_cull_opacity_ok(ctypes.c_float(float(np.nextafter(R.GATE, np.float32(0))))) == 0
    assert not r_ok[~(z["op"] >= R.GATE)].any()
    assert not missed.any(), np.flatnonzero(missed)[:10]


def test_tightened_rectangle_sandwich(ref):
    """(b) and (c)."""
    z, s, tight, packed = ref["z"], ref["s"], ref["tight"], ref["packed"]
    n = len(z["mx"])
    for k in ("regular", "fallback", "borderline", "low", "culled"):
        print(f"{k}: {int(s[k].sum())} cases")
    share = s["borderline"].sum() / n
    print(f"borderline share {100 * share:.4f} %")
    assert 0 < share <= 1e-3
    for k in ("bad_inner", "bad_outer", "bad_fallback", "bad_either", "bad_low", "bad_culled"):
        assert not s[k].any(), (k, int(s[k].sum()), np.flatnonzero(s[k])[:10])
    # (c): count 0, width 0 (stored as 1) under the gate and for a NaN opacity; at the gate and above, never
    x0, y0, w, cnt = R.unpack(packed)
    low = s["low"]
    assert np.isnan(z["op"][low]).sum() > 50 and (z["op"][low] == np.nextafter(R.GATE, np.float32(0))).sum() > 1000
    at = (z["op"] == R.GATE) & s["regular"] & s["inner_ok"]
    assert at.sum() > 1000 and (cnt[at] > 0).all()
    assert (cnt[low] == 0).all() and (w[low] == 1).all() and (tight[low, 2:] == 0).all()


def test_how_tight(ref):
    """The largest observed ratio of the tightened extent to E, read off the tiles: the smallest s of a ladder for which
    every regular case lies inside box(s E + 0.01).  Printed for profiles/tile_rect/README.md; the code's own factor is
    1.0001, and (b) holds 1.001."""
    z, s, tight = ref["z"], ref["s"], ref["tight"]
    _, ex, ey, _ = R.extents_f64(z)
    t, t_ok = R.corners(tight)
    for scale in (1.0, 1.0001, 1.00011, 1.0002, 1.001):
        o, o_ok = R.box(z, s["classic"], scale * ex + 0.01, scale * ey + 0.01)
        out = ~R._inside(t, t_ok, o, o_ok) & s["regular"]
        print(f"outside box({scale} E + 0.01): {int(out.sum())} cases")
    assert not out.any()


def test_packing(lib, ref):
    """(d)"""
    z, tight, packed = ref["z"], ref["tight"], ref["packed"]
    assert lib.tr_empty_word() == R.EMPTY_WORD == 1 << 20
    x0, y0, w, cnt = R.unpack(packed)
    vis = z["rx"] > 0
    assert np.array_equal(packed.astype(np.int64)[vis], R.pack(tight)[vis])
    assert (packed[~vis] == np.array([R.EMPTY_WORD, 0], np.uint32)).all() and (~vis).sum() > 1000
    assert np.array_equal(x0[vis], tight[vis, 0]) and np.array_equal(y0[vis], tight[vis, 1])
    assert np.array_equal(w[vis], np.maximum(tight[vis, 2], 1)) and np.array_equal(cnt, tight[:, 2] * tight[:, 3])
    assert (w >= 1).all() and (cnt[w != np.maximum(tight[:, 2], 1)] == 0).all()
    # the ends the cases reach ...
    assert tight[:, 0].max() == 1023 and tight[:, 1].max() == 1023 and tight[:, 2].max() == 1023
    assert cnt.max() == 2 * 1023                                # (the height is not stored: it is in the count)
    # ... and the packing's own, whatever rectangle it is given
    rng = np.random.default_rng(0)
    rect = rng.integers(0, 1024, (4096, 4)).astype(np.int32)
    rect[0], rect[1], rect[2], rect[3] = (1023, 1023, 1023, 1023), (1023, 0, 1023, 1), (0, 1023, 0, 1023), (1023, 1023, 0, 0)
    out = np.zeros((len(rect), 2), np.uint32)
    lib.tr_pack(len(rect), _p(rect), _p(out))
    px, py, pw, pc = R.unpack(out)
    assert np.array_equal(px, rect[:, 0]) and np.array_equal(py, rect[:, 1])
    assert np.array_equal(pw, np.maximum(rect[:, 2], 1)) and np.array_equal(pc, rect[:, 2].astype(np.int64) * rect[:, 3])


def test_cases_are_adversarial(ref):
    """(f), measured on the reference alone."""
    z, s, classic, reached = ref["z"], ref["s"], ref["classic"], ref["reached"]
    n = len(z["mx"])
    assert n >= 1 << 18
    c_ok = (classic[:, 2] > 0) & (classic[:, 3] > 0)
    ob, ob_ok = s["outer_box"], s["outer_ok"]
    judged = s["regular"] & c_ok
    smaller = judged & (~ob_ok | ((ob[:, 2] - ob[:, 0]) * (ob[:, 3] - ob[:, 1]) < classic[:, 2] * classic[:, 3]))
    empty = judged & ~ob_ok
    thr_reach = (reached[:, 2] > reached[:, 0]) & (z["op"] < 0.0040)
    f = np.float32
    with np.errstate(invalid="ignore"):
        tx, ty, rx, ry = z["mx"] / f(16), z["my"] / f(16), z["rx"].astype(f) / f(16), z["ry"].astype(f) / f(16)
        vis = z["rx"] > 0
        clamped = {"left": vis & (np.floor(tx - rx) < 0), "right": vis & (np.ceil(tx + rx) > z["tile_w"]),
                   "top": vis & (np.floor(ty - ry) < 0), "bottom": vis & (np.ceil(ty + ry) > z["tile_h"])}
    print(f"{n} cases: the outer box is smaller than the classic rectangle in {int(smaller.sum())} ({100 * smaller.sum() / n:.1f} %), "
          f"empty with a positive radius and an opacity >= 1/255 in {int(empty.sum())}; {int(thr_reach.sum())} threshold-opacity cases "
          f"reach a tile; {int(s['fallback'].sum())} fall back; clamped "
          + ", ".join(f"{k} {int(v.sum())}" for k, v in clamped.items()))
    print(f"host test so far: {time.perf_counter() - T0:.1f} s")
    assert smaller.sum() > 0.30 * n
    assert empty.sum() > 1000 and thr_reach.sum() > 1000 and s["fallback"].sum() > 1000
    for k, v in clamped.items():
        assert v.sum() > 1000, k
