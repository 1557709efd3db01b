"""The exact mesh-over-splat composite without a GPU: the fp64 statement of tests/hybrid_ref.py at its two limits, its
prefix property, the case that motivates the operator (with the numbers composite_over's rule gets wrong), the gate of
tests/test_gpu_hybrid.py shown to pass an fp32 emulation of the walk on every one of its cases, and include/mgs_hybrid.h
<-> libmgs.so / libmgs_debug.so <-> the ctypes table (_lib.HYBRID_EXPORTS) with the entry point's refusals.

Measured here (NumPy, the scenes projected and binned by the oracle): the fp32 emulation leaves 0 unexplained pixels on all
ten cases, the could-flip share is 0 .. 1.3e-4 of a frame, and the largest error off a could-flip pixel is 1e-6 .. 4.4e-6
(the depth channel, of values up to 11).  The pane case: the exact composite keeps 0.3 of the pane's red over the blue foreground, composite_over's
rule returns the bare foreground -- 0.3 apart in two channels.
"""
import ctypes
import os
import re
import subprocess

import numpy as np
import pytest

import hybrid_ref as HR
from feature_channel_gates import FRAMES, MULTI, TILE, features, multi_cameras, scene, tiles_of
from oracle import gs_oracle_np as O

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "mgs_hybrid.h")
f32 = lambda a: np.asarray(a, np.float32)


# ---- the header, the libraries, the binding ----------------------------------------------------------------------------
def _code(path=HEADER):
    return re.sub(r"/\*.*?\*/", "", open(path).read(), flags=re.S)


def _declared(path=HEADER):
    decls = re.findall(r"\b(?:int|void|size_t|const char \*)\s*\*?\s*(mgs_\w+)\s*\(([^;]*?)\)\s*;", _code(path), flags=re.S)
    return {name: 0 if args.strip() == "void" else len([a for a in args.split(",") if a.strip()]) for name, args in decls}


def test_hybrid_header_symbol_is_exported_and_bound_in_both_libraries():
    from robosimgs_amd import _lib
    from robosimgs_amd.csrc import build
    decl = _declared()
    assert decl == {"mgs_raster_over_opaque": 23} and _lib.HYBRID_EXPORTS == ["mgs_raster_over_opaque"]
    others = (_lib.EXPORTS, _lib.OPTIM_EXPORTS, _lib.REFINE_EXPORTS, _lib.LABEL_EXPORTS, _lib.LIFT_EXPORTS, _lib.HINGE_EXPORTS,
              _lib.POSE_EXPORTS, _lib.DEFORM_EXPORTS, _lib.DEFORM_SH_EXPORTS, _lib.MESH_EXPORTS)
    assert not set(_lib.HYBRID_EXPORTS) & set().union(*map(set, others))
    assert "hybrid.hip" in build.SOURCES
    for L in (_lib.lib(), _lib.debug_lib()):
        assert len(L.mgs_raster_over_opaque.argtypes) == 23
    nm = lambda path: subprocess.run(["nm", "-D", "--defined-only", path], capture_output=True, text=True).stdout
    for path in (_lib.LIB_PATH, _lib.DEBUG_LIB_PATH):
        assert "mgs_raster_over_opaque" in nm(path), path
    assert "MGS_VERSION" not in _code()                                   # the version is mgs.h's alone


_ARGS = ("n", "means2d", "conics", "opacities", "feats", "feat_stride", "depths", "fg_rgb", "fg_depth", "render", "alphas",
         "backdrop", "width", "height", "tile_w", "tile_h", "offsets", "flatten", "order", "out_rgb", "out_depth", "vis", "stream")


def _over_opaque(**kw):
    """mgs_raster_over_opaque on made-up addresses: every case here must be refused before anything is launched."""
    from robosimgs_amd import _lib
    L = _lib.lib()
    a = dict(n=10, means2d=0x1000, conics=0x2000, opacities=0x3000, feats=0x4000, feat_stride=4, depths=0x5000, fg_rgb=0x6000,
             fg_depth=0x7000, render=0x8000, alphas=0x9000, backdrop=None, width=32, height=16, tile_w=2, tile_h=1,
             offsets=0xA000, flatten=0xB000, order=None, out_rgb=0xC000, out_depth=0xD000, vis=None, stream=None)
    assert set(kw) <= set(a)
    a.update(kw)
    rc = L.mgs_raster_over_opaque(*[a[k] for k in _ARGS])
    return rc, L.mgs_last_error_string()


@pytest.mark.parametrize("kw,word", [
    (dict(n=-1), b"bad sizes"),
    (dict(width=0), b"bad sizes"),
    (dict(height=-3), b"bad sizes"),
    (dict(feat_stride=2), b"feature stride 2 below 3"),
    (dict(tile_w=3), b"tile grid 3x1 does not match 32x16"),
    (dict(tile_h=2), b"tile grid"),
    (dict(width=33), b"tile grid"),
    (dict(means2d=None), b"means2d, conics or opacities is null"),
    (dict(conics=None), b"means2d, conics or opacities is null"),
    (dict(opacities=None), b"means2d, conics or opacities is null"),
    (dict(feats=None), b"feats or depths is null"),
    (dict(depths=None), b"feats or depths is null"),
    (dict(fg_rgb=None), b"null foreground"),
    (dict(fg_depth=None), b"null foreground"),
    (dict(render=None), b"null frame"),
    (dict(alphas=None), b"null frame"),
    (dict(offsets=None), b"null tile lists"),
    (dict(flatten=None), b"null tile lists"),
    (dict(out_rgb=None), b"null output"),
    (dict(out_depth=None), b"null output"),
    (dict(render=0x8004), b"16-byte aligned"),
])
def test_raster_over_opaque_argument_errors_are_reported_without_a_gpu(kw, word):
    rc, msg = _over_opaque(**kw)
    assert rc == -1 and word in msg and msg.startswith(b"raster_over_opaque:"), (rc, msg)


# ---- scenes on the CPU -------------------------------------------------------------------------------------------------
class _Camera:
    """One camera of a scene projected and binned by the oracle (fp64 projection rounded to the fp32 a kernel would read),
    with random colours."""

    def __init__(self, g, cam, w, h):
        self.w, self.h = w, h
        p = O.project(g.means, g.quats, g.scales, f32(cam.viewmat()).astype(np.float64), f32(cam.K).astype(np.float64), w, h)
        self.m2d, self.con, self.opac, self.z = f32(p["means2d"]), f32(p["conics"]), f32(g.opacities), f32(p["depths"])
        tw, th = tiles_of(w, h)
        _, keys, self.ids = O.isect_tiles(self.m2d, p["radii"], self.z, TILE, tw, th, dtype=np.float32)
        self.offs = O.isect_offsets(keys, 1, tw, th)[0]
        self.rgb = features(len(g))[0][:, :3]
        self._refs = {}

    def fg(self, kind):
        return HR.foreground(kind, self.w, self.h, self.m2d, self.z, self.ids)

    def ref(self, fg_rgb, fg_depth, dtype=np.float64, **kw):
        return HR.HybridReference(self.m2d, self.con, self.rgb, self.z, self.opac, self.ids, self.offs, self.w, self.h,
                                  fg_rgb, fg_depth, dtype=dtype, **kw)

    def case(self, kind, dtype=np.float64):
        if (kind, dtype) not in self._refs:
            self._refs[(kind, dtype)] = self.ref(*self.fg(kind), dtype=dtype)
        return self._refs[(kind, dtype)]


@pytest.fixture(scope="module")
def cameras():
    cache = {}

    def get(name, setup=None, c=0):
        key = (name, setup if c == 2 else None, c)                  # the setups share cameras 0 and 1
        if key not in cache:
            from robosimgs_amd import camera_ring
            if name == "tiles":
                spec = FRAMES[name]
                cam = camera_ring(1, spec["w"], spec["h"], thetas=[spec["theta"]])[0]
            else:
                spec = MULTI
                cam = multi_cameras(setup)[c]
            cache[key] = _Camera(scene(spec), cam, spec["w"], spec["h"])
        return cache[key]
    return get


def test_limit_beyond_every_depth_is_the_oracles_frame(cameras):
    cam = cameras("tiles")
    fg_rgb, d = cam.fg("far")
    ref = cam.case("far")
    col = np.concatenate([cam.rgb, cam.z[:, None]], axis=1)
    img, alpha, _, _ = O.rasterize(cam.m2d, cam.con, col, cam.opac, cam.ids, cam.offs, cam.w, cam.h, TILE)
    assert ref.has_fg.all() and d.min() > cam.z[np.unique(cam.ids)].max()
    np.testing.assert_allclose(ref.rgb, img[..., :3] + (1.0 - alpha)[..., None] * fg_rgb, rtol=0, atol=1e-12)
    np.testing.assert_allclose(ref.t_f, 1.0 - alpha, rtol=0, atol=1e-12)
    np.testing.assert_allclose(ref.depth, img[..., 3] + (1.0 - alpha) * d, rtol=0, atol=1e-12)
    np.testing.assert_allclose(ref.tf_sub, ref.t_f, rtol=0, atol=1e-12)          # the two forms of T_F, in fp64
    assert float(alpha.max()) > 0.99 and float(alpha.min()) < 0.5                # the frame is neither empty nor closed


def test_limit_below_every_depth_is_the_foreground_exactly(cameras):
    cam = cameras("tiles")
    fg_rgb, d = cam.fg("near")
    ref = cam.case("near")
    assert d.max() < cam.z[np.unique(cam.ids)].min()
    assert np.array_equal(ref.rgb, fg_rgb.astype(np.float64)) and np.array_equal(ref.depth, d.astype(np.float64))
    assert np.array_equal(ref.t_f, np.ones_like(ref.t_f)) and int(ref.n_front.max()) == 0
    emu = cam.case("near", np.float32)
    assert np.array_equal(emu.rgb, fg_rgb) and np.array_equal(emu.depth, d) and emu.rgb.dtype == np.float32


def test_raising_d_only_appends_to_F(cameras):
    cam = cameras("tiles")
    pixels = {(5, 7), (37, 41), (60, 20), (111, 79), (80, 64)}
    z = np.sort(cam.z[np.unique(cam.ids)])
    prev, grew = {p: [] for p in pixels}, 0
    for q in (0.0, 0.1, 0.3, 0.5, 0.7, 0.9, 1.0):
        d = np.zeros((cam.h, cam.w), np.float32)
        for x, y in pixels:
            d[y, x] = np.nextafter(z[int(q * (len(z) - 1))], np.float32(np.inf))       # just behind that Gaussian
        ref = cam.ref(np.zeros((cam.h, cam.w, 3), np.float32), d, record=pixels)
        for p in pixels:
            cur = ref.members.get(p, [])
            assert cur[:len(prev[p])] == prev[p], f"pixel {p}: raising d to quantile {q} changed the front of F"
            assert len(cur) == int(ref.n_front[p[1], p[0]]) and cur == sorted(cur)
            grew += len(cur) > len(prev[p])
            prev[p] = cur
    assert grew >= 10 and max(len(v) for v in prev.values()) >= 5


def test_pane_in_front_of_the_foreground_keeps_its_tint():
    """A pane at alpha ~ 0.3 (depth 2), a foreground plane (depth 4), an opaque wall (depth 6), one 16 x 16 tile."""
    w = h = 16
    m2d = f32([[8.0, 8.0], [8.0, 8.0]])
    con = f32([[1e-4, 0.0, 1e-4], [1e-4, 0.0, 1e-4]])               # 100 px wide: flat over the tile
    opac, z = f32([0.3, 0.999]), f32([2.0, 6.0])
    rgb = f32([[1.0, 0.0, 0.0], [0.0, 1.0, 0.0]])                   # a red pane, a green wall
    ids, offs = np.array([0, 1], np.int32), np.zeros((1, 1), np.int32)
    fg_rgb = np.zeros((h, w, 3), np.float32)
    fg_rgb[..., 2] = 1.0                                             # a blue foreground
    d = np.full((h, w), 4.0, np.float32)
    ref = HR.HybridReference(m2d, con, rgb, z, opac, ids, offs, w, h, fg_rgb, d)
    # by hand: two terms
    py, px = np.mgrid[0:h, 0:w] + 0.5
    sig = 0.5 * (np.float64(con[0, 0]) * (8.0 - px) ** 2 + np.float64(con[0, 2]) * (8.0 - py) ** 2)
    a = np.float64(opac[0]) * np.exp(-sig)
    hand = a[..., None] * rgb[0].astype(np.float64) + (1.0 - a)[..., None] * fg_rgb
    np.testing.assert_allclose(ref.rgb, hand, rtol=0, atol=1e-12)
    np.testing.assert_allclose(ref.t_f, 1.0 - a, rtol=0, atol=1e-12)
    np.testing.assert_allclose(ref.depth, a * 2.0 + (1.0 - a) * 4.0, rtol=0, atol=1e-12)
    assert int(ref.n_front.min()) == int(ref.n_front.max()) == 1
    # composite_over's rule (include/mgs.h, "Compositing") on the finished frame, restated
    col = np.concatenate([rgb, z[:, None]], axis=1)
    img, alpha, _, _ = O.rasterize(m2d, con, col, opac, ids, offs, w, h, TILE)
    bg_rgb, bg_depth = img[..., :3], img[..., 3] / np.maximum(alpha, 1e-10)
    has_fg = (d > 0) & (d < np.inf)
    front = has_fg & (~(alpha > 0) | (d <= bg_depth))
    old = np.where(front[..., None], fg_rgb, bg_rgb + (1.0 - alpha)[..., None] * fg_rgb)
    gap = np.abs(ref.rgb - old).max(axis=-1)
    print(f"\npane: expected depth {bg_depth.min():.3f} .. {bg_depth.max():.3f} against the foreground at 4: composite_over puts "
          f"the foreground {'in front' if front.all() else 'behind'}; exact red {ref.rgb[..., 0].min():.3f} .. "
          f"{ref.rgb[..., 0].max():.3f}, composite_over's {old[..., 0].max():.3f}; largest gap {gap.max():.3f}")
    assert front.all() and float(old[..., 0].max()) == 0.0          # the pane is dropped entirely
    assert float(gap.min()) > 0.1 and float(ref.rgb[..., 0].min()) > 0.29


# ---- the gate on the CPU -----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,setup,c,kind", HR.CASES)
def test_gate_passes_the_fp32_emulation_on_every_gpu_case(cameras, name, setup, c, kind):
    cam = cameras(name, setup, c)
    ref, emu = cam.case(kind), cam.case(kind, np.float32)
    assert emu.rgb.dtype == np.float32 and emu.t_f.dtype == np.float32
    if kind == "none":
        assert not ref.has_fg.any() and float(np.abs(ref.rgb).max()) == 0.0
        return
    st = HR.check_hybrid(ref, emu.rgb, emu.depth, emu.tf_sub, what=f"{name} {setup} camera {c} {kind}: fp32 emulation")
    assert st["unexplained"] == 0 and st["flip_over_bound"] == 0 and st["could_flip_frac"] <= 0.05
    assert st["max_err_nonflip"] < 2e-5, st                         # fp32 rounding, depth channel included
    if kind in ("main", "strict"):                                  # the plane cuts the image and the scene
        front = ref.n_front[ref.has_fg]
        assert int(front.min()) < int(front.max()) and int(front.max()) >= 5 and 0.3 < ref.has_fg.mean() < 0.7
    if kind == "strict":                                            # the chosen Gaussians are behind their own depth
        plain = cam.case("main")
        moved = ref.fg_depth != plain.fg_depth
        assert int(moved.sum()) == HR.N_STRICT
        nxt = cam.ref(ref.fg_rgb, np.where(moved, np.nextafter(ref.fg_depth, np.float32(np.inf)), 0).astype(np.float32))
        assert (nxt.n_front[moved] >= ref.n_front[moved]).all() and int((nxt.n_front[moved] > ref.n_front[moved]).sum()) >= 16


def test_cases_reach_the_kernels_paths(cameras):
    """From the offsets: a truncated list of more than two queue batches, a truncated list that is empty while the full one
    is not, and a tile with foreground but no list."""
    long_, emptied, listless = 0, 0, 0
    for name, setup, c, kind in HR.CASES:
        cam = cameras(name, setup, c)
        t = HR.tile_truncation(cam.z, cam.ids, cam.offs, cam.fg(kind)[1], cam.w, cam.h)
        long_ += int((t[:, 1] > 2 * HR.QUEUE).sum())
        emptied += int(((t[:, 1] == 0) & (t[:, 0] > 0) & (t[:, 2] > 0)).sum())
        listless += int(((t[:, 0] == 0) & (t[:, 2] > 0)).sum())
    assert long_ > 0 and emptied > 0 and listless > 0, (long_, emptied, listless)
