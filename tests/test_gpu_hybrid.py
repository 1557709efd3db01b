"""The exact mesh-over-splat composite on the GPU (include/mgs_hybrid.h, csrc/hybrid.hip): raster_over_opaque_kernel
against the fp64 statement of tests/hybrid_ref.py, on the GPU's own projection, lists and frame, through every layer that
hands it out -- ops.raster_over_opaque_raw, ops.rasterize_over_opaque, rasterization(foreground=...) on the feature path
and on the SH path -- and once with rasterize_mesh as the producer of the foreground.

The foregrounds are built from the GPU's own projected depths (hybrid_ref.foreground), so every comparison is made at the
GPU's own inputs to this stage.  tests/test_hybrid_host.py shows on the CPU that the gate passes an fp32 emulation of the
walk on every case of hybrid_ref.CASES.  Every case is at most 112x80 pixels and 4,000 Gaussians, the fp64 references are
cached per module, and nothing here is captured in a graph.
"""
import numpy as np
import pytest
import torch

import hybrid_ref as HR
from feature_channel_gates import FRAMES, MULTI, camera_lists, features, multi_cameras, scene, tiles_of
from oracle import gs_oracle_np as O

pytestmark = pytest.mark.gpu
DEV = "cuda"
CANARY = 0xA5
GUARD = 1 << 14
C = MULTI["n_cams"]
W, H = MULTI["w"], MULTI["h"]


def _t(a):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32)).to(DEV)


def _np(x):
    return x.detach().cpu().numpy()


def _same(a, b):
    """Byte for byte (torch.equal calls NaN unequal and -0 equal to 0)."""
    return a.shape == b.shape and torch.equal(a.contiguous().view(torch.int32), b.contiguous().view(torch.int32))


@pytest.fixture(scope="module")
def ops():
    from robosimgs_amd import ops as _ops
    return _ops


class _Guarded:
    """The three output frames with 0xA5 bytes in front of and behind each."""

    def __init__(self, h, w):
        self.raw, self.out = [], []
        for shape in ((h, w, 3), (h, w), (h, w)):
            n = int(np.prod(shape))
            raw = torch.full((4 * (n + 2 * GUARD),), CANARY, dtype=torch.uint8, device=DEV)
            self.raw.append((raw, n))
            self.out.append(raw.view(torch.float32)[GUARD:GUARD + n].view(shape))

    def intact(self):
        torch.cuda.synchronize()
        return all(bool((raw[:4 * GUARD] == CANARY).all()) and bool((raw[4 * (GUARD + n):] == CANARY).all())
                   for raw, n in self.raw)

    def written(self):
        return all(not bool((raw[4 * GUARD:4 * (GUARD + n)].view(torch.int32) == -0x5A5A5A5B).any()) for raw, n in self.raw)


# ---- 1. the stage, one camera -------------------------------------------------------------------------------------------
class _Stage:
    """FRAMES["tiles"] projected with its depth channel (mgs_project_color_fwd), binned and blended ("RGB+ED") by the HIP
    kernels, and the fp64 references on those very values and lists."""

    def __init__(self, ops):
        from robosimgs_amd import camera_ring
        spec = FRAMES["tiles"]
        self.w, self.h = spec["w"], spec["h"]
        self.tw, self.th = tiles_of(self.w, self.h)
        g = scene(spec)
        cam = camera_ring(1, self.w, self.h, thetas=[spec["theta"]])[0]
        self.vm, self.K = _t(cam.viewmat()), _t(cam.K)
        t = g.to_torch(DEV, 0)
        self.opac = t["opacities"]
        radii, self.m2d, self.z, self.con, _, self.feats, _ = ops.project_color_fwd_raw(
            t["means"], t["quats"], t["scales"], t["opacities"], 0, t["colors"], self.vm, self.K, self.w, self.h, 0.3, 0.01,
            1e10, 0.0, False, True, want_splats=True)
        assert tuple(self.feats.shape) == (len(g), 4) and torch.equal(self.feats[:, 3], self.z)
        cap = ops._upper_bound_isects(radii, self.tw, self.th) + 1
        self.tl = ops.isect_tiles_raw(self.m2d, radii, self.z, self.tw, self.th, cap)
        assert int(self.tl.status.item()) == 0
        self.n_isect = int(self.tl.n_isect.item())
        self.render, self.alphas, _ = ops.rasterize_fwd_raw(self.m2d, self.con, self.feats, self.opac, None, self.w, self.h,
                                                            self.tw, self.th, self.tl.tile_offsets, self.tl.flatten_ids,
                                                            track_last=False, expected_last=True)
        self.ids, self.offs = _np(self.tl.flatten_ids[:self.n_isect]), _np(self.tl.tile_offsets[:-1])
        self._fg, self._refs = {}, {}

    def fg(self, kind):
        if kind not in self._fg:
            self._fg[kind] = HR.foreground(kind, self.w, self.h, _np(self.m2d), _np(self.z), self.ids)
        return self._fg[kind]

    def ref(self, kind, fg=None):
        if fg is not None or kind not in self._refs:
            fg_rgb, fg_depth = fg if fg is not None else self.fg(kind)
            r = HR.HybridReference(_np(self.m2d), _np(self.con), _np(self.feats), _np(self.z), _np(self.opac), self.ids, self.offs,
                                   self.w, self.h, fg_rgb, fg_depth)
            if fg is not None:
                return r
            self._refs[kind] = r
        return self._refs[kind]

    def run(self, ops, fg, backdrop=None, order=True, out=None, visibility=True):
        return ops.raster_over_opaque_raw(self.tl, self.m2d, self.con, self.opac, self.feats, self.z, _t(fg[0]), _t(fg[1]),
                                          self.render, self.alphas, self.w, self.h, backdrop=backdrop, out=out,
                                          return_visibility=visibility, use_group_order=order)


@pytest.fixture(scope="module")
def stage(ops):
    return _Stage(ops)


def test_no_foreground_is_the_frame_byte_for_byte(ops, stage):
    """Zeros, a NaN, an inf and a negative depth: no pixel has foreground, every output byte is the pass-through rule's."""
    fg = stage.fg("none")
    assert np.isnan(fg[1]).sum() == 1 and np.isinf(fg[1]).sum() == 1 and (fg[1] < 0).sum() == 1
    for backdrop in (None, _t(HR.BACKDROP)):
        guarded = _Guarded(stage.h, stage.w)
        rgb, depth, vis = stage.run(ops, fg, backdrop=backdrop, out=tuple(guarded.out))
        assert guarded.intact() and guarded.written(), "the kernel wrote outside its frames, or not all of them"
        n = HR.check_pass_through(fg[1], _np(stage.render), _np(stage.alphas), None if backdrop is None else HR.BACKDROP,
                                  _np(rgb), _np(depth), _np(vis))
        assert n == stage.w * stage.h
        if backdrop is None:
            assert _same(rgb, stage.render[..., :3].contiguous())
    a = _np(stage.alphas)
    assert np.isinf(_np(depth)[a == 0]).all() and np.isfinite(_np(depth)[a > 0]).all()


def test_plane_nearer_than_every_gaussian_is_the_foreground_bit_for_bit(ops, stage):
    fg = stage.fg("near")
    rgb, depth, vis = stage.run(ops, fg, backdrop=_t(HR.BACKDROP))
    assert _same(rgb, _t(fg[0])) and _same(depth, _t(fg[1])) and bool((vis == 1).all())


def test_plane_beyond_every_gaussian_is_the_whole_blend(ops, stage):
    """The gate against the reference; and the reference's sum over F of w c against rasterize_to_pixels' own frame."""
    fg = stage.fg("far")
    ref = stage.ref("far")
    rgb, depth, vis = stage.run(ops, fg)
    HR.check_hybrid(ref, _np(rgb), _np(depth), _np(vis), what="tiles far")
    offs = stage.tl.tile_offsets[:-1].view(1, stage.th, stage.tw)
    frame, alphas = ops.rasterize_to_pixels(stage.m2d[None], stage.con[None], stage.feats[None], stage.opac[None], stage.w,
                                            stage.h, 16, offs, stage.tl.flatten_ids[:stage.n_isect])
    st = O.check_frame(_np(frame[0]), _np(alphas[0, ..., 0]), ref.acc, 1.0 - ref.t_f, ref.margins, O.EPS_STAGE,
                       what="tiles far: sum over F against rasterize_to_pixels", flip_weight=ref.flip_weight,
                       feat_max=ref.feat_max(), require_flip_bound=True)
    print(f"\nsum over F against the operator's frame: over 1e-4 {st['over_tol']}, max err off flips {st['max_err_nonflip']:.2e}")
    # fg_visibility against the frame's own 1 - alpha: the two forms of T (T -= w here, fma(-alpha, T, T) there)
    gap = float((vis - (1.0 - alphas[0, ..., 0])).abs().max())
    print(f"fg_visibility against 1 - alpha of the frame: largest difference {gap:.2e}")
    assert gap <= 1e-5


@pytest.mark.parametrize("kind", ("main", "strict"))
def test_slanted_plane_through_the_scene(ops, stage, kind):
    """Tiles that mix open and closed pixels, a tile maximum far from most pixels' d, an isolated foreground pixel -- and
    (strict) 32 pixels whose d is a Gaussian's own depth.  Gate, pass-through bytes, determinism, launch order."""
    fg = stage.fg(kind)
    ref = stage.ref(kind)
    bd = _t(HR.BACKDROP)
    guarded = _Guarded(stage.h, stage.w)
    rgb, depth, vis = stage.run(ops, fg, backdrop=bd, out=tuple(guarded.out))
    assert guarded.intact() and guarded.written()
    HR.check_hybrid(ref, _np(rgb), _np(depth), _np(vis), what=f"tiles {kind}")
    n = HR.check_pass_through(fg[1], _np(stage.render), _np(stage.alphas), HR.BACKDROP, _np(rgb), _np(depth), _np(vis))
    assert 0.3 * stage.w * stage.h < n < 0.7 * stage.w * stage.h
    again = stage.run(ops, fg, backdrop=bd)
    unordered = stage.run(ops, fg, backdrop=bd, order=False)
    for a, b, c in zip((rgb, depth, vis), again, unordered):
        assert _same(a, b), "two runs differ"
        assert _same(a, c), "the launch order changes a byte"
    only = stage.run(ops, fg, backdrop=bd, visibility=False)
    assert only[2] is None and _same(only[0], rgb) and _same(only[1], depth)                  # fg_visibility is nullable
    if kind == "strict":
        moved = fg[1] != stage.fg("main")[1]
        assert int(moved.sum()) == HR.N_STRICT
        # one ulp further back the Gaussian is in front: the strict comparison is what keeps it out
        nxt = stage.ref(None, fg=(fg[0], np.where(moved, np.nextafter(fg[1], np.float32(np.inf)), 0).astype(np.float32)))
        assert int((nxt.n_front[moved] > ref.n_front[moved]).sum()) >= 16
        assert float(np.abs(nxt.t_f[moved] - ref.t_f[moved]).max()) > 0.01


def test_raster_over_opaque_raw_refuses_lists_the_kernel_cannot_read(ops, stage):
    """The lists reach the kernel as raw pointers: a short, an int64 or a strided one is a ValueError that names it, raised
    before anything is launched; the same call with good lists afterwards gives the bytes it gave before."""
    assert stage.tw * stage.th >= 2
    fg = tuple(_t(x) for x in stage.fg("main"))
    tl = stage.tl

    def call(lists, **kw):
        return ops.raster_over_opaque_raw(lists, stage.m2d, stage.con, stage.opac, stage.feats, stage.z, *fg, stage.render,
                                          stage.alphas, stage.w, stage.h, **kw)

    def lists(**changed):
        out = ops.TileLists()
        for name in ("flatten_ids", "tile_offsets", "group_order"):
            setattr(out, name, changed.get(name, getattr(tl, name)))
        return out

    before = call(tl)
    doubled = torch.stack([tl.tile_offsets, tl.tile_offsets], dim=1)
    for bad_tl, kw, word in ((tl, dict(tile_offsets=tl.tile_offsets[1:]), "tile_offsets"),
                             (lists(tile_offsets=tl.tile_offsets[1:]), {}, "tile_offsets"),
                             (lists(flatten_ids=tl.flatten_ids.long()), {}, "flatten_ids"),
                             (tl, dict(tile_offsets=doubled[:, 0]), "tile_offsets"),
                             (lists(tile_offsets=tl.tile_offsets.long()), {}, "tile_offsets"),
                             (lists(group_order=tl.group_order.long()), {}, "group_order")):
        with pytest.raises(ValueError, match="^" + word):
            call(bad_tl, **kw)
    for a, b in zip(call(tl), before):
        assert _same(a, b)


def test_real_producer_rasterize_mesh(ops, stage):
    """The open box, scaled to three units at the world origin, rendered by rasterize_mesh from the stage's camera: its
    outputs go straight in."""
    import mesh_scenes as MS
    from robosimgs_amd import Mesh, rasterize_mesh
    box = MS.openbox()
    v = box["verts"].astype(np.float64)
    v = (v - 0.5 * (v.min(0) + v.max(0))) * (3.0 / (v.max(0) - v.min(0)).max())
    col = np.random.default_rng(4).random((len(v), 3)).astype(np.float32)
    mesh = Mesh(v.astype(np.float32), box["faces"].astype(np.int64), vertex_colors=col).to(DEV)
    fg_rgb, fg_depth, _ = rasterize_mesh(mesh, stage.vm[None], stage.K[None], stage.w, stage.h, headlight=True)
    assert tuple(fg_rgb.shape) == (1, stage.h, stage.w, 3) and tuple(fg_depth.shape) == (1, stage.h, stage.w)
    fg = (_np(fg_rgb[0]), _np(fg_depth[0]))
    covered = HR.has_foreground(fg[1])
    z_lo, _, z_hi = HR.listed_depth_range(_np(stage.z), stage.ids)
    assert 0.02 < covered.mean() < 0.9 and z_lo < fg[1][covered].min() and fg[1][covered].max() < z_hi
    rgb, depth, vis = ops.raster_over_opaque_raw(stage.tl, stage.m2d, stage.con, stage.opac, stage.feats, stage.z, fg_rgb[0],
                                                 fg_depth[0], stage.render, stage.alphas, stage.w, stage.h)
    ref = stage.ref(None, fg=fg)
    HR.check_hybrid(ref, _np(rgb), _np(depth), _np(vis), what="tiles, the open box by rasterize_mesh")
    HR.check_pass_through(fg[1], _np(stage.render), _np(stage.alphas), None, _np(rgb), _np(depth), _np(vis))
    v_in = _np(vis)[covered]
    print(f"the box covers {int(covered.sum())} pixels, fg_visibility there {v_in.min():.3f} .. {v_in.max():.3f}")
    assert v_in.max() - v_in.min() > 0.2                            # the box is neither in front of the scene nor behind it


# ---- 2. three cameras: the operator and rasterization's feature path ------------------------------------------------------
@pytest.fixture(scope="module")
def multi():
    g = scene(MULTI)
    return g, features(len(g))[0][:, :3]


class _Multi:
    """MULTI under one setup through the stage operators: projection, lists, the "RGB+ED" frame."""

    def __init__(self, ops, g, rgb, setup):
        self.N = len(g)
        cams = multi_cameras(setup)
        self.vm, self.Ks = _t(np.stack([c.viewmat() for c in cams])), _t(np.stack([c.K for c in cams]))
        tw, th = tiles_of(W, H)
        radii, self.m2d, self.z, self.con, _ = ops.fully_fused_projection(_t(g.means), None, _t(g.quats), _t(g.scales), self.vm,
                                                                         self.Ks, W, H)
        _, keys, self.flat = ops.isect_tiles(self.m2d, radii, self.z, 16, tw, th)
        self.offs = ops.isect_offset_encode(keys, C, tw, th)
        self.opac = _t(g.opacities)[None].expand(C, self.N).contiguous()
        self.feats = torch.cat([_t(rgb)[None].expand(C, self.N, 3), self.z[..., None]], dim=-1).contiguous()
        frame, alphas = ops.rasterize_to_pixels(self.m2d, self.con, self.feats, self.opac, W, H, 16, self.offs, self.flat)
        self.render = torch.cat([frame[..., :3], frame[..., 3:] / alphas.clamp(min=1e-10)], dim=-1)
        self.alphas = alphas
        self.lists = [camera_lists(_np(self.flat), _np(self.offs), c, self.N) for c in range(C)]

    def fg(self, kind):
        per = [HR.foreground(kind, W, H, _np(self.m2d[c]), _np(self.z[c]), self.lists[c][0]) for c in range(C)]
        return np.stack([p[0] for p in per]), np.stack([p[1] for p in per])

    def ref(self, c, fg_rgb, fg_depth):
        ids, offs = self.lists[c]
        return HR.HybridReference(_np(self.m2d[c]), _np(self.con[c]), _np(self.feats[c]), _np(self.z[c]), _np(self.opac[c]), ids,
                                  offs, W, H, fg_rgb[c], fg_depth[c])


@pytest.mark.parametrize("setup", ("ring", "empty_tail"))
def test_operator_and_feature_path_three_cameras(ops, multi, setup):
    from robosimgs_amd import rasterization
    g, rgb = multi
    m = _Multi(ops, g, rgb, setup)
    cases = [(c, kind) for name, s, c, kind in HR.CASES if name == "multi" and s == setup]
    for kind in sorted({k for _, k in cases}):
        fg_rgb, fg_depth = m.fg(kind)
        out = ops.rasterize_over_opaque(m.m2d, m.con, m.feats, m.z, m.opac, _t(fg_rgb), _t(fg_depth), m.render, m.alphas, W, H, 16,
                                        m.offs, m.flat, backdrop=HR.BACKDROP, return_visibility=True)
        assert [tuple(o.shape) for o in out] == [(C, H, W, 3), (C, H, W), (C, H, W)]
        two = ops.rasterize_over_opaque(m.m2d, m.con, m.feats, m.z, m.opac, _t(fg_rgb), _t(fg_depth), m.render, m.alphas[..., 0],
                                        W, H, 16, m.offs, m.flat, backdrop=HR.BACKDROP)
        assert len(two) == 2 and _same(two[0], out[0]) and _same(two[1], out[1])
        for c in range(C):
            HR.check_pass_through(fg_depth[c], _np(m.render[c]), _np(m.alphas[c]), HR.BACKDROP, _np(out[0][c]), _np(out[1][c]),
                                  _np(out[2][c]), what=f"{setup} camera {c} {kind}")
            if (c, kind) in cases:
                HR.check_hybrid(m.ref(c, fg_rgb, fg_depth), _np(out[0][c]), _np(out[1][c]), _np(out[2][c]),
                                what=f"{setup} camera {c} {kind}")
        if kind != "main":
            continue
        # rasterization(foreground=...) with per-Gaussian colours: the operator's bytes, the frame untouched
        args = (_t(g.means), _t(g.quats), _t(g.scales), _t(g.opacities), _t(rgb), m.vm, m.Ks, W, H)
        plain = rasterization(*args, render_mode="RGB+ED")
        got = rasterization(*args, render_mode="RGB+ED", foreground=(_t(fg_rgb), _t(fg_depth)), backdrop=HR.BACKDROP)
        assert _same(plain[0], got[0]) and _same(plain[1], got[1]) and _same(plain[0], m.render)
        new = {"hybrid_rgb", "hybrid_depth", "fg_visibility"}
        assert not new & set(plain[2]) and set(plain[2]) | new == set(got[2])
        for key, want in zip(("hybrid_rgb", "hybrid_depth", "fg_visibility"), out):
            assert _same(got[2][key], want) and not got[2][key].requires_grad, key
    if setup == "empty_tail":                                       # the last camera's right and bottom tiles have no list
        per_tile = np.diff(np.concatenate([m.lists[2][1].reshape(-1), [len(m.lists[2][0])]]))
        assert (per_tile == 0).sum() >= 20


# ---- 3. the SH path ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("aa", ("classic", "antialiased"))
def test_sh_path_gives_the_stage_operators_bytes(ops, multi, aa):
    """rasterization(sh_degree=0, foreground=...) per camera: the raw call on that camera's own arrays, lists and frame
    (colours from the same projection call), one camera held to the reference; with gradients wanted on both training
    paths; the refusals."""
    from robosimgs_amd import rasterization
    g, _ = multi
    t = g.to_torch(DEV, 0)
    cams = multi_cameras("ring")
    vm, Ks = _t(np.stack([c.viewmat() for c in cams])), _t(np.stack([c.K for c in cams]))
    args = (t["means"], t["quats"], t["scales"], t["opacities"], t["colors"], vm, Ks, W, H)
    kw = dict(sh_degree=0, render_mode="RGB+ED", rasterize_mode=aa)
    plain = rasterization(*args, **kw)
    lists = [(_np(tl.flatten_ids[:int(n)]), _np(tl.tile_offsets[:-1])) for tl, n in zip(plain[2]["tile_lists"], plain[2]["n_isects"])]
    per = [HR.foreground("main", W, H, _np(plain[2]["means2d"][c]), _np(plain[2]["depths"][c]), lists[c][0]) for c in range(C)]
    fg_rgb, fg_depth = _t(np.stack([p[0] for p in per])), _t(np.stack([p[1] for p in per]))
    got = rasterization(*args, foreground=(fg_rgb, fg_depth), backdrop=HR.BACKDROP, **kw)
    assert _same(plain[0], got[0]) and _same(plain[1], got[1])
    new = {"hybrid_rgb", "hybrid_depth", "fg_visibility"}
    assert not new & set(plain[2]) and set(plain[2]) | new == set(got[2])
    for key in ("means2d", "conics", "radii", "depths", "opacities", "n_isects", "isect_offsets"):
        assert torch.equal(plain[2][key], got[2][key]), key
    meta, bd = got[2], _t(HR.BACKDROP)
    for c in range(C):
        feats = ops.project_color_fwd_raw(t["means"], t["quats"], t["scales"], t["opacities"], 0, t["colors"], vm[c], Ks[c], W, H,
                                          0.3, 0.01, 1e10, 0.0, aa == "antialiased", True, want_splats=True, bin_seed="tight")[5]
        opac = meta["opacities"][c].contiguous()                    # the opacity the raster saw: anti-aliased where the frame is
        want = ops.raster_over_opaque_raw(meta["tile_lists"][c], meta["means2d"][c], meta["conics"][c], opac, feats,
                                          meta["depths"][c], fg_rgb[c], fg_depth[c], got[0][c], got[1][c, ..., 0].contiguous(),
                                          W, H, backdrop=bd)
        for key, w_ in zip(("hybrid_rgb", "hybrid_depth", "fg_visibility"), want):
            assert _same(meta[key][c], w_), (key, c)
        if c == 1:
            ref = HR.HybridReference(_np(meta["means2d"][c]), _np(meta["conics"][c]), _np(feats), _np(meta["depths"][c]), _np(opac),
                                     *lists[c], W, H, *per[c])
            HR.check_hybrid(ref, *(_np(meta[k][c]) for k in ("hybrid_rgb", "hybrid_depth", "fg_visibility")),
                            what=f"SH path {aa} camera {c}")
            HR.check_pass_through(per[c][1], _np(got[0][c]), _np(got[1][c]), HR.BACKDROP,
                                  *(_np(meta[k][c]) for k in ("hybrid_rgb", "hybrid_depth", "fg_visibility")))
    if aa == "antialiased":
        assert not torch.equal(meta["opacities"][0], t["opacities"])
        return
    for cap in (None, 200_000):                                     # gradients wanted: per camera, and the one-call training path
        means = t["means"].clone().requires_grad_(True)
        col, _, m2 = rasterization(means, *args[1:], foreground=(fg_rgb, fg_depth), backdrop=HR.BACKDROP, isect_capacity=cap, **kw)
        for key in new:
            assert _same(m2[key], meta[key]) and not m2[key].requires_grad, (key, cap)
        col.sum().backward()
        assert bool(torch.isfinite(means.grad).all())
    for bad, word in ((dict(render_mode="RGB"), "RGB\\+ED"), (dict(lean_meta=True, isect_capacity=200_000), "lean_meta"),
                      (dict(dataset_out=(None, None, None, True)), "dataset_out")):
        with pytest.raises(ValueError, match=word):
            rasterization(*args, foreground=(fg_rgb, fg_depth), **{**kw, **bad})
    with pytest.raises(ValueError, match="foreground must be"):
        rasterization(*args, foreground=(fg_rgb[0], fg_depth[0]), **kw)
    with pytest.raises(ValueError, match="backdrop given without foreground"):
        rasterization(*args, backdrop=HR.BACKDROP, **kw)


# ---- 4. the cases reach the kernel's paths ----------------------------------------------------------------------------------
def test_cases_reach_the_kernels_paths(ops, stage, multi):
    """From the GPU's own offsets and depths: a truncated list of more than two batches of the walk's queue, a truncated
    list that is empty while the full one is not, a tile with foreground pixels and no list at all."""
    g, rgb = multi
    long_, emptied, listless = 0, 0, 0
    tables = [HR.tile_truncation(_np(stage.z), stage.ids, stage.offs, stage.fg(kind)[1], stage.w, stage.h) for kind in HR.FOREGROUNDS]
    for setup in ("ring", "empty_tail"):
        m = _Multi(ops, g, rgb, setup)
        for c, kind in [(c, kind) for name, s, c, kind in HR.CASES if name == "multi" and s == setup]:
            tables.append(HR.tile_truncation(_np(m.z[c]), *m.lists[c], m.fg(kind)[1][c], W, H))
    for t in tables:
        long_ += int((t[:, 1] > 2 * HR.QUEUE).sum())
        emptied += int(((t[:, 1] == 0) & (t[:, 0] > 0) & (t[:, 2] > 0)).sum())
        listless += int(((t[:, 0] == 0) & (t[:, 2] > 0)).sum())
    print(f"\ntiles with a truncated list over {2 * HR.QUEUE} entries: {long_}; emptied by the truncation: {emptied}; with "
          f"foreground and no list: {listless}")
    assert long_ > 0 and emptied > 0 and listless > 0
