"""The part-label output without a GPU: include/mgs_labels.h <-> libmgs.so / libmgs_debug.so <-> the fourth ctypes table
(_lib.LABEL_EXPORTS), the argument checks of both entry points, and the gate of tests/label_gates.py shown to pass a plain
fp32 blend on every scene and class assignment tests/test_gpu_labels.py uses and to fail on five label bugs.

Measured here (NumPy, the two FRAMES scenes projected and binned by the oracle): the fp32 oracle as a stand-in leaves 0 - 3
of ~8,000 pixels undecided and its largest weight error is 2e-7 .. 4e-7.  On the ragged frame with 7 random classes a
plain fp32 blend that counts the closing Gaussian, or that ignores the stop rule, changes NO decided label but breaks the
weight bound at 46 and 105 pixels (error 2.1e-3) -- which is why label_weights is part of the gate; shifted class ids break
the label check at all 8,051 pixels, a forgotten T at 3,697, "class of the first contributor" at 5,270.
"""
import ctypes
import os
import re
import subprocess

import numpy as np
import pytest

import label_gates as LG
from feature_channel_gates import FRAMES, TILE, scene, tiles_of
from oracle import gs_oracle_np as O

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "mgs_labels.h")
CORRUPTIONS = ("count_closing", "no_stop", "shift", "stale_T", "first")


def _code(path=HEADER):
    return re.sub(r"/\*.*?\*/", "", open(path).read(), flags=re.S)


def _declared(path=HEADER):
    decls = re.findall(r"\b(?:int|void|size_t|const char \*)\s*\*?\s*(mgs_\w+)\s*\(([^;]*?)\)\s*;", _code(path), flags=re.S)
    return {name: 0 if args.strip() == "void" else len([a for a in args.split(",") if a.strip()]) for name, args in decls}


def test_label_header_symbols_are_exported_and_bound_in_both_libraries():
    from robosimgs_amd import _lib
    decl = _declared()
    assert sorted(decl) == sorted(_lib.LABEL_EXPORTS) == ["mgs_raster_labels", "mgs_render_frames_labeled"]
    assert not set(_lib.LABEL_EXPORTS) & (set(_lib.EXPORTS) | set(_lib.OPTIM_EXPORTS) | set(_lib.REFINE_EXPORTS))
    assert decl["mgs_raster_labels"] == 17
    # mgs_render_frames' parameter list with the four label arguments in front of the workspace
    frames = _declared(os.path.join(ROOT, "include", "mgs.h"))["mgs_render_frames"]
    assert decl["mgs_render_frames_labeled"] == frames + 4
    for L in (_lib.lib(), _lib.debug_lib()):
        for name, nargs in decl.items():
            assert len(getattr(L, name).argtypes) == nargs, name
        a, b = L.mgs_render_frames.argtypes, L.mgs_render_frames_labeled.argtypes
        assert b[:len(a) - 3] == a[:-3] and b[-3:] == a[-3:]
        assert b[len(a) - 3:-3] == [ctypes.c_void_p, ctypes.c_int, ctypes.c_void_p, ctypes.c_void_p]
    nm = lambda path: subprocess.run(["nm", "-D", "--defined-only", path], capture_output=True, text=True).stdout
    for path in (_lib.LIB_PATH, _lib.DEBUG_LIB_PATH):
        assert all(name in nm(path) for name in decl), path
    define = lambda name: int(re.search(rf"#define\s+{name}\s+(\d+)", _code()).group(1))
    assert define("MGS_LABEL_NONE") == _lib.LABEL_NONE == LG.NONE == 255
    assert define("MGS_LABELS_MAX_CLASSES") == _lib.LABELS_MAX_CLASSES == LG.BASE == 32
    assert "MGS_VERSION" not in _code()                                   # the version is mgs.h's alone


def _raster_labels(n_classes=3, class_ids=0x1000, labels=0x2000, splats=0x3000, means2d=None, conics=None, opacities=None,
                   width=32, height=16, tile_w=2, tile_h=1, offsets=0x4000, flatten=0x5000):
    """mgs_raster_labels on made-up addresses: every case here must be refused before anything is launched."""
    from robosimgs_amd import _lib
    L = _lib.lib()
    rc = L.mgs_raster_labels(10, means2d, conics, opacities, splats, class_ids, n_classes, width, height, tile_w, tile_h, offsets,
                             flatten, None, labels, None, None)
    return rc, L.mgs_last_error_string()


@pytest.mark.parametrize("kw,word", [
    (dict(n_classes=0), b"n_classes 0 outside 1..32"),
    (dict(n_classes=33), b"n_classes 33 outside 1..32"),
    (dict(n_classes=-1), b"n_classes"),
    (dict(class_ids=None), b"class_ids is null"),
    (dict(labels=None), b"labels is null"),
    (dict(splats=None), b"neither packed records"),
    (dict(splats=None, means2d=0x6000, conics=0x7000), b"neither packed records"),
    (dict(tile_w=3), b"tile grid"),
    (dict(offsets=None), b"null tile lists"),
])
def test_raster_labels_argument_errors_are_reported_without_a_gpu(kw, word):
    rc, msg = _raster_labels(**kw)
    assert rc == -1 and word in msg and msg.startswith(b"raster_labels:"), (rc, msg)


@pytest.mark.parametrize("kw,word", [
    (dict(n_classes=0), b"render_frames_labeled: n_classes 0 outside 1..32"),
    (dict(n_classes=33), b"render_frames_labeled: n_classes 33 outside 1..32"),
    (dict(class_ids=None), b"render_frames_labeled: class_ids is null"),
    (dict(labels=None), b"render_frames_labeled: labels is null"),
    (dict(channels=5), b"render_frames: channels"),                 # mgs_render_frames' own checks, under its name
])
def test_render_frames_labeled_argument_errors_are_reported_without_a_gpu(kw, word):
    from robosimgs_amd import _lib
    L = _lib.lib()
    a = dict(n_classes=3, class_ids=0x1000, labels=0x2000, channels=4)
    a.update(kw)
    nbytes = ctypes.c_size_t(1 << 30)
    rc = L.mgs_render_frames_labeled(10, None, None, None, None, 0, 1, None, 1, None, None, 32, 16, 0.3, 0.01, 1e10, 0.0, 0,
                                     a["channels"], 0, None, 4096, None, None, None, None, None, None, 0, None, a["class_ids"],
                                     a["n_classes"], a["labels"], None, 0x10000, ctypes.byref(nbytes), None)
    msg = L.mgs_last_error_string()
    assert rc == -1 and word in msg, (rc, msg)


def test_render_frames_labeled_size_query_is_render_frames():
    """The label frames live in the caller's buffers and the kernel reads the workspace's records and lists: no byte more."""
    from robosimgs_amd import _lib
    L = _lib.lib()
    head = [4099, None, None, None, None, 3, 16, None, 2, None, None, 97, 83, 0.3, 0.01, 1e10, 0.0, 0, 4, 0, None, 50000, None,
            None, None, None, None, None, 0, None]
    a, b = ctypes.c_size_t(0), ctypes.c_size_t(0)
    assert L.mgs_render_frames(*head, None, ctypes.byref(a), None) == 0
    assert L.mgs_render_frames_labeled(*head, 0x1000, 7, 0x2000, None, None, ctypes.byref(b), None) == 0
    assert a.value == b.value > 0


# ---- the gate on the CPU -------------------------------------------------------------------------------------------------
f32 = lambda a: np.asarray(a, np.float32)


class _Frame:
    """One FRAMES scene projected and binned by the oracle (fp64 projection rounded to the fp32 a kernel would read)."""

    def __init__(self, name):
        from robosimgs_amd import camera_ring
        spec = FRAMES[name]
        self.g, self.w, self.h = scene(spec), spec["w"], spec["h"]
        cam = camera_ring(1, self.w, self.h, thetas=[spec["theta"]])[0]
        p = O.project(self.g.means, self.g.quats, self.g.scales, f32(cam.viewmat()).astype(np.float64),
                      f32(cam.K).astype(np.float64), self.w, self.h)
        self.m2d, self.con, self.opac = f32(p["means2d"]), f32(p["conics"]), f32(self.g.opacities)
        tw, th = tiles_of(self.w, self.h)
        _, keys, self.ids = O.isect_tiles(self.m2d, p["radii"], f32(p["depths"]), TILE, tw, th, dtype=np.float32)
        self.offs = O.isect_offsets(keys, 1, tw, th)[0]
        self.n = len(self.g)
        self._refs, self._standins = {}, {}

    def base(self, kind):
        return LG.base_classes(kind, self.n, self.g.means)

    def ref(self, kind):
        key = "spatial" if kind == "spatial" else "random"
        if key not in self._refs:
            self._refs[key] = LG.LabelReference(self.m2d, self.con, self.opac, self.ids, self.offs, self.w, self.h, self.base(key))
        return self._refs[key]

    def standin(self, kind):
        """The fp32 oracle's frame [h,w,32] for the base one-hot features."""
        key = "spatial" if kind == "spatial" else "random"
        if key not in self._standins:
            self._standins[key] = O.rasterize(self.m2d, self.con, LG.one_hot(self.base(key)), self.opac, self.ids, self.offs,
                                              self.w, self.h, TILE, dtype=np.float32)[0]
        return self._standins[key]


@pytest.fixture(scope="module")
def frames():
    cache = {}

    def get(name):
        if name not in cache:
            cache[name] = _Frame(name)
        return cache[name]
    return get


def _labels_of(W):
    """What the kernel's epilogue makes of class weights [h,w,K]: ascending scan with a strict >, 255 where all are 0."""
    W = np.asarray(W)
    lab = W.argmax(axis=-1).astype(np.uint8)
    top = W.max(axis=-1)
    lab[top <= 0] = LG.NONE
    return lab, top


@pytest.mark.parametrize("frame", list(FRAMES))
def test_gate_passes_the_fp32_blend_on_every_assignment(frames, frame):
    fr = frames(frame)
    for kind, k in LG.CASES:
        ref = fr.ref(kind)
        lab, top = _labels_of(LG.fold_columns(fr.standin(kind), LG.fold(kind, k), k))
        st = LG.check_labels(ref.weights(kind, k), ref.flip_weight, lab, top, what=f"{frame} {kind} K={k} fp32 stand-in")
        assert st["ok"] and st["undecided"] <= LG.UNDECIDED_CAP * st["pixels"]
        assert st["max_weight_err"] < 5e-6, st          # fp32 rounding: measured 2e-7 .. 6e-7
        if kind == "ignore":                            # the ignored third occludes and is reported for no class
            plain = ref.weights("random", k)
            assert float((plain.sum(-1) - ref.weights(kind, k).sum(-1)).max()) > 0.1
        # the labels are not trivial: several classes own pixels
        assert len(set(np.unique(lab)) - {LG.NONE}) >= min(k, 5), (kind, k, np.unique(lab))


def test_folded_reference_equals_the_literal_one_hot_call(frames):
    """One oracle run at 32 base classes serves every assignment: columns summed over m^-1(k) against O.rasterize on the
    assignment's own one-hot features (a base class mapped to -1 is a zeroed row)."""
    fr = frames("ragged")
    ref = fr.ref("ignore")
    for kind, k in (("ignore", 7), ("random", 2)):
        ids = LG.class_ids(kind, k, fr.base(kind))
        assert (ids.min() == -1) == (kind == "ignore") and ids.max() == k - 1
        lit = O.rasterize(fr.m2d, fr.con, LG.one_hot(ids), fr.opac, fr.ids, fr.offs, fr.w, fr.h, TILE)[0]
        np.testing.assert_allclose(ref.weights(kind, k), lit[..., :k], rtol=0, atol=1e-12)
        assert float(np.abs(lit[..., k:]).max()) == 0.0


def _corrupt_blends(fr, cls, K):
    """kind -> (labels, weights): a plain fp32 blend of the lists with one label bug each ("ok": none), in one walk."""
    flat = np.concatenate([fr.offs.reshape(-1), [len(fr.ids)]]).astype(int)
    tw, th = tiles_of(fr.w, fr.h)
    kinds = ("ok",) + CORRUPTIONS
    W = {kd: np.zeros((fr.h, fr.w, K), np.float32) for kd in kinds}
    first = np.full((fr.h, fr.w), LG.NONE, np.uint8)
    one, half = np.float32(1), np.float32(0.5)
    for t in range(tw * th):
        ty, tx = divmod(t, tw)
        y0, y1, x0, x1 = ty * 16, min(ty * 16 + 16, fr.h), tx * 16, min(tx * 16 + 16, fr.w)
        py, px = np.meshgrid(np.arange(y0, y1, dtype=np.float32) + half, np.arange(x0, x1, dtype=np.float32) + half, indexing="ij")
        T, done = np.ones_like(px), np.zeros(px.shape, bool)
        T_ns = np.ones_like(px)                                    # "no_stop": its own transmittance, never finished
        acc_w = {kd: np.zeros(px.shape + (K,), np.float32) for kd in kinds}
        fst = np.full(px.shape, LG.NONE, np.uint8)
        for i in range(flat[t], flat[t + 1]):
            g = fr.ids[i]
            dx, dy = fr.m2d[g, 0] - px, fr.m2d[g, 1] - py
            sig = half * (fr.con[g, 0] * dx * dx + fr.con[g, 2] * dy * dy) + fr.con[g, 1] * dx * dy
            a = np.minimum(np.float32(0.999), fr.opac[g] * np.exp(-sig)).astype(np.float32)
            hit = (sig >= 0) & (a >= np.float32(1 / 255))
            ok = hit & ~done
            Tn = T * (one - a)
            stop = ok & (Tn <= np.float32(1e-4))
            acc = ok & ~stop
            c = int(cls[g])
            w = np.where(acc, a * T, 0).astype(np.float32)
            acc_w["ok"][..., c] += w
            acc_w["first"][..., c] += w
            acc_w["shift"][..., (c + 1) % K] += w
            acc_w["count_closing"][..., c] += np.where(ok, a * T, 0).astype(np.float32)
            acc_w["stale_T"][..., c] += np.where(acc, a, 0).astype(np.float32)
            acc_w["no_stop"][..., c] += np.where(hit, a * T_ns, 0).astype(np.float32)
            T_ns = np.where(hit, T_ns * (one - a), T_ns)
            fst = np.where((fst == LG.NONE) & acc, np.uint8(c), fst)
            T = np.where(acc, Tn, T)
            done |= stop
        for kd in kinds:
            W[kd][y0:y1, x0:x1] = acc_w[kd]
        first[y0:y1, x0:x1] = fst
    out = {kd: _labels_of(W[kd]) for kd in kinds}
    out["first"] = (first, out["first"][1])
    return out


def test_gate_fails_on_each_label_bug(frames):
    """The ragged frame (about 500 pixels close early), 7 random classes."""
    fr = frames("ragged")
    kind, K = "random", 7
    ref = fr.ref(kind)
    W = ref.weights(kind, K)
    blends = _corrupt_blends(fr, LG.class_ids(kind, K, fr.base(kind)), K)
    st = LG.check_labels(W, ref.flip_weight, *blends["ok"], what="plain fp32 blend")
    assert st["ok"]
    stats = {}
    for kd in CORRUPTIONS:
        stats[kd] = LG.check_labels(W, ref.flip_weight, *blends[kd], what=kd, raise_on_fail=False)
        assert not stats[kd]["ok"], kd
    # the closing Gaussian and the stop rule show in the weights, where nearly no label moves: the weight output is what
    # makes the kernel testable for them
    for kd in ("count_closing", "no_stop"):
        assert stats[kd]["weight_over"] >= 20 and stats[kd]["wrong_labels"] <= 5, (kd, stats[kd])
    for kd in ("shift", "stale_T", "first"):
        assert stats[kd]["wrong_labels"] >= 1000, (kd, stats[kd])
