"""Lifting masks onto Gaussians without a GPU: include/mgs_lift.h <-> libmgs.so / libmgs_debug.so <-> the fifth ctypes table
(_lib.LIFT_EXPORTS), the argument checks of both entry points, the fp64 reference of tests/lift_gates.py against fp64
autograd, and the gate shown to pass a plain fp32 walk on every scene and mask tests/test_gpu_lift.py uses and to fail on
eight vote bugs.

Measured here (NumPy, the two FRAMES scenes projected and binned by the oracle, fp32 stand-in: fp32 weights, fp32 tile
sums, Q32 integer accumulation): undecided Gaussians 0.8 - 1.4 % (tiles) and 2.3 - 2.9 % (ragged) on the capped masks, up to
4 % on the others; no decided Gaussian with another class, no vote over the bound, worst error / bound 0.004, largest
vote 85, largest vote error 1.7e-6.
"""
import ctypes
import os
import re
import subprocess

import numpy as np
import pytest

import lift_gates as LF
from feature_channel_gates import FRAMES, TILE, BackwardReference, scene, tiles_of
from oracle import gs_oracle_np as O

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "mgs_lift.h")


def _code(path=HEADER):
    return re.sub(r"/\*.*?\*/", "", open(path).read(), flags=re.S)


def _declared(path=HEADER):
    decls = re.findall(r"\b(?:int|void|size_t|const char \*)\s*\*?\s*(mgs_\w+)\s*\(([^;]*?)\)\s*;", _code(path), flags=re.S)
    return {name: 0 if args.strip() == "void" else len([a for a in args.split(",") if a.strip()]) for name, args in decls}


def test_lift_header_symbols_are_exported_and_bound_in_both_libraries():
    from robosimgs_amd import _lib
    decl = _declared()
    assert sorted(decl) == sorted(_lib.LIFT_EXPORTS) == ["mgs_lift_assign", "mgs_raster_votes"]
    others = (_lib.EXPORTS, _lib.OPTIM_EXPORTS, _lib.REFINE_EXPORTS, _lib.LABEL_EXPORTS)
    assert not set(_lib.LIFT_EXPORTS) & set().union(*map(set, others))
    assert len(_lib.EXPORTS) == 29                                        # include/mgs.h's table is untouched
    # the parameter lists as the header spells them: mgs_raster_labels' with (mask) for (class_ids), and
    # (row_offset, n_rows, votes) for (labels, label_weights)
    assert decl == {"mgs_raster_votes": 18, "mgs_lift_assign": 7}
    for L in (_lib.lib(), _lib.debug_lib()):
        for name, nargs in decl.items():
            assert len(getattr(L, name).argtypes) == nargs, name
        assert L.mgs_lift_assign.argtypes[3] is ctypes.c_float
    nm = lambda path: subprocess.run(["nm", "-D", "--defined-only", path], capture_output=True, text=True).stdout
    for path in (_lib.LIB_PATH, _lib.DEBUG_LIB_PATH):
        assert all(name in nm(path) for name in decl), path
    assert "MGS_VERSION" not in _code() and "#define" not in _code().replace("#define MGS_LIFT_H_", "")


def _raster_votes(n_classes=3, mask=0x1000, votes=0x2000, splats=0x3000, means2d=None, conics=None, opacities=None, width=32,
                  height=16, tile_w=2, tile_h=1, offsets=0x4000, flatten=0x5000, n_rows=10, n=10):
    """mgs_raster_votes on made-up addresses: every case here must be refused before anything is launched."""
    from robosimgs_amd import _lib
    L = _lib.lib()
    rc = L.mgs_raster_votes(n, means2d, conics, opacities, splats, mask, n_classes, width, height, tile_w, tile_h, offsets, flatten,
                            None, 0, n_rows, votes, None)
    return rc, L.mgs_last_error_string()


@pytest.mark.parametrize("kw,word", [
    (dict(n_classes=0), b"n_classes 0 outside 1..32"),
    (dict(n_classes=33), b"n_classes 33 outside 1..32"),
    (dict(n_classes=-1), b"n_classes"),
    (dict(mask=None), b"mask is null"),
    (dict(votes=None), b"votes is null"),
    (dict(n_rows=-1), b"n_rows -1 is negative"),
    (dict(splats=None), b"neither packed records"),
    (dict(splats=None, means2d=0x6000, conics=0x7000), b"neither packed records"),
    (dict(n=-1), b"bad sizes"),
    (dict(width=0, tile_w=0), b"bad sizes"),
    (dict(tile_w=3), b"tile grid"),
    (dict(tile_h=2), b"tile grid"),
    (dict(offsets=None), b"null tile lists"),
    (dict(flatten=None), b"null tile lists"),
])
def test_raster_votes_argument_errors_are_reported_without_a_gpu(kw, word):
    rc, msg = _raster_votes(**kw)
    assert rc == -1 and word in msg and msg.startswith(b"raster_votes:"), (rc, msg)


@pytest.mark.parametrize("kw,word", [
    (dict(n_rows=-1), b"n_rows -1 is negative"),
    (dict(n_classes=0), b"n_classes 0 outside 1..32"),
    (dict(n_classes=33), b"n_classes 33 outside 1..32"),
    (dict(votes=None), b"votes is null"),
    (dict(class_ids=None), b"class_ids is null"),
    (dict(min_vote=-1.0), b"min_vote"),
    (dict(min_vote=float("nan")), b"min_vote"),
    (dict(min_vote=float("inf")), b"min_vote"),
    (dict(min_vote=3e9), b"min_vote"),
])
def test_lift_assign_argument_errors_are_reported_without_a_gpu(kw, word):
    from robosimgs_amd import _lib
    L = _lib.lib()
    a = dict(n_rows=10, n_classes=3, votes=0x1000, min_vote=0.0, class_ids=0x2000)
    a.update(kw)
    rc = L.mgs_lift_assign(a["n_rows"], a["n_classes"], a["votes"], a["min_vote"], a["class_ids"], None, None)
    msg = L.mgs_last_error_string()
    assert rc == -1 and word in msg and msg.startswith(b"lift_assign:"), (rc, msg)


def test_lift_assign_of_no_rows_launches_nothing():
    from robosimgs_amd import _lib
    assert _lib.lib().mgs_lift_assign(0, 3, 0x1000, 0.0, 0x2000, None, None) == 0


# ---- the gate on the CPU -------------------------------------------------------------------------------------------------
f32 = lambda a: np.asarray(a, np.float32)


class _Frame:
    """One FRAMES scene projected and binned by the oracle (fp64 projection rounded to the fp32 a kernel would read), its
    fp64 vote reference for every mask of LF.CASES, and the fp32 stand-in."""

    def __init__(self, name, theta=None):
        from robosimgs_amd import camera_ring
        spec = FRAMES[name]
        self.g, self.w, self.h = scene(spec), spec["w"], spec["h"]
        cam = camera_ring(1, self.w, self.h, thetas=[spec["theta"] if theta is None else theta])[0]
        p = O.project(self.g.means, self.g.quats, self.g.scales, f32(cam.viewmat()).astype(np.float64),
                      f32(cam.K).astype(np.float64), self.w, self.h)
        self.m2d, self.con, self.opac = f32(p["means2d"]), f32(p["conics"]), f32(self.g.opacities)
        tw, th = tiles_of(self.w, self.h)
        _, keys, self.ids = O.isect_tiles(self.m2d, p["radii"], f32(p["depths"]), TILE, tw, th, dtype=np.float32)
        self.offs = O.isect_offsets(keys, 1, tw, th)[0]
        self.n = len(self.g)
        self.masks = LF.masks_for(self.w, self.h)
        self.args = (self.m2d, self.con, self.opac, self.ids, self.offs, self.w, self.h)
        self.ref = LF.VoteReference(*self.args, self.masks)
        self.standin = LF.walk(*self.args, self.masks, dtype=np.float32)


@pytest.fixture(scope="module")
def frames():
    cache = {}

    def get(name, theta=None):
        if (name, theta) not in cache:
            cache[(name, theta)] = _Frame(name, theta)
        return cache[(name, theta)]
    return get


def test_masks_are_what_the_cases_say(frames):
    fr = frames("ragged")
    for (kind, k), (m, _) in fr.masks.items():
        assert m.shape == (fr.h, fr.w) and m.dtype == np.uint8
        valid = m[m < k]
        assert set(np.unique(valid)) == set(range(k)), (kind, k)
        if kind in ("stripes", "checker"):
            assert (m < k).all()
        if kind == "ignore":
            assert set(np.unique(m[m >= k])) == {LF.IGNORE} and 0.25 < (m == LF.IGNORE).mean() < 0.45
        if kind == "high":
            assert set(np.unique(m[m >= k])) == set(range(k, 255)), "every value in K..254 occurs"
    tw, th = tiles_of(fr.w, fr.h)
    per_tile = lambda m: [len(np.unique(m[y:y + 16, x:x + 16])) for y in range(0, fr.h, 16) for x in range(0, fr.w, 16)]
    assert max(per_tile(fr.masks[("checker", 32)][0])) == 16       # 4x4 cells of 4x4 pixels: the present-class loop's longest
    cut = per_tile(fr.masks[("stripes", 7)][0])
    assert min(cut) == 1 and max(cut) == 2                                      # whole tiles and cut tiles


@pytest.mark.parametrize("frame", list(FRAMES))
def test_gate_passes_the_fp32_walk_on_every_mask(frames, frame):
    fr = frames(frame)
    for case in LF.CASES:
        votes = fr.standin[case][0]
        cls, conf = LF.assign(votes)
        st = LF.check_votes(fr.ref.V(case), fr.ref.bound(case), votes, cls, conf, capped=case in LF.CAPPED,
                            what=f"{frame} {case[0]} K={case[1]} fp32 stand-in")
        assert st["ok"] and st["max_ratio"] < 0.1, st                          # measured: 0.004
        assert st["voted"] > 0.9 * fr.n and st["max_vote"] > 5
        if case in LF.CAPPED:
            assert st["undecided"] <= LF.UNDECIDED_CAP * fr.n
        assert len(set(cls.tolist()) - {-1}) == case[1] or case[1] == 32, (case, set(cls.tolist()))
    # the same stripes under holes: no pixel of a hole votes, whatever value marks it
    a, b = fr.standin[("ignore", 7)][0], fr.standin[("high", 7)][0]
    assert np.array_equal(a, b) and (a <= fr.standin[("stripes", 7)][0]).all() and a.sum() < 0.8 * fr.standin[("stripes", 7)][0].sum()
    assert fr.ref.could_flip < 50
    # min_vote: the gate follows it
    votes = fr.standin[("stripes", 7)][0]
    cls, conf = LF.assign(votes, 0.5)
    st = LF.check_votes(fr.ref.V(("stripes", 7)), fr.ref.bound(("stripes", 7)), votes, cls, conf, min_vote=0.5,
                        what=f"{frame} stripes K=7 min_vote 0.5")
    assert st["ok"] and (cls == -1).sum() > (LF.assign(votes)[0] == -1).sum()


def test_reference_walk_equals_fp64_autograd(frames):
    """V = v_feats of the fp64 blend with features ones [N,K] and cotangent one-hot(mask), to 1e-9."""
    fr = frames("ragged")
    back = BackwardReference(fr.m2d, fr.con, np.ones((fr.n, 32)), fr.opac, fr.ids, fr.offs, fr.w, fr.h)
    for case in (("checker", 32), ("ignore", 7)):
        mask, k = fr.masks[case]
        cot = np.zeros((fr.h, fr.w, 32))
        ok = mask < k
        cot[np.nonzero(ok)[0], np.nonzero(ok)[1], mask[ok]] = 1.0
        v_feats = back.grads(k, cot, None)[2]
        assert v_feats.shape == (fr.n, k)
        err = float(np.abs(v_feats - fr.ref.V(case)).max())
        print(f"\n{case}: walk against autograd, largest difference {err:.2e}")
        assert err <= 1e-9
    # counted pixels: a vote needs one, and a counted pixel's weight is at least 1/255 * 1e-4
    V, cnt = fr.ref.V(("checker", 32)), fr.ref.count(("checker", 32))
    assert ((V > 0) == (cnt > 0)).all() and (V <= cnt).all()


def test_gate_fails_on_each_vote_bug(frames):
    """Every corrupted fp32 walk is refused on the ragged frame (about 500 pixels close early); which part of the gate
    catches it is printed.  The cap (c) is not what fails them: (a) or (b) is."""
    fr = frames("ragged")
    for bug in LF.BUGS:
        case = ("ignore", 7) if bug == "ignore_as_zero" else ("stripes", 7)
        votes = LF.walk(*fr.args, {case: fr.masks[case]}, dtype=np.float32, bug=bug)[case][0]
        cls, conf = LF.assign(votes)
        st = LF.check_votes(fr.ref.V(case), fr.ref.bound(case), votes, cls, conf, what=bug, raise_on_fail=False)
        assert not st["ok"] and (st["over"] or st["wrong_class"] or st["nonzero_at_zero_bound"]), (bug, st)


def test_gate_fails_on_votes_overwritten_across_two_cameras(frames):
    a, b = frames("ragged"), frames("ragged", 1.3)
    case = ("stripes", 7)
    V, B = a.ref.V(case) + b.ref.V(case), a.ref.bound(case) + b.ref.bound(case)
    both = a.standin[case][0] + b.standin[case][0]
    st = LF.check_votes(V, B, both, *LF.assign(both), capped=True, what="two cameras accumulated")
    assert st["ok"]
    last = b.standin[case][0]
    st = LF.check_votes(V, B, last, *LF.assign(last), what="two cameras, the second overwrites", raise_on_fail=False)
    assert not st["ok"] and st["over"] > 1000


def test_q32_round_trip():
    """Sums of rint(w 2^32) equal the float64 sums to n 2^-33; a tile's fp32 sum times 2^32 is an integer from 2^-8 up."""
    rng = np.random.default_rng(0)
    for n in (1, 7, 256, 100_000):
        w = rng.random(n).astype(np.float32).astype(np.float64)
        q = np.rint(w * LF.Q32).astype(np.int64)
        assert abs(int(q.sum()) / LF.Q32 - w.sum()) <= n * 2.0 ** -33
    s = np.float32(1 / 255) * np.float32(1e-4)                     # the smallest weight that is ever counted
    assert np.rint(np.float64(s) * LF.Q32) > 1000
    big = np.float32(256.0)                                        # a tile's largest sum: 41 bits
    assert int(np.rint(np.float64(big) * LF.Q32)) * (1 << 16) < 2 ** 63             # 2^16 tiles of 256 pixels: 2^24 pixels
    cls, conf = LF.assign(np.array([[5, 5, 0], [0, 0, 0], [1, 2, 3]], np.int64))
    assert cls.tolist() == [0, -1, 2] and conf.tolist() == [0.5, 0.0, 0.5]          # ties to the lowest class; no vote: -1
