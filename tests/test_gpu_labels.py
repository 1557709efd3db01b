"""Part labels on the GPU (include/mgs_labels.h, csrc/labels.hip): raster_labels_kernel against the fp64 class weights of
tests/label_gates.py, on the GPU's own projection and lists, through every layer that hands labels out --
ops.raster_labels_raw, ops.rasterize_labels, rasterization(class_ids=...) on its three paths, FrameRenderer.

tests/test_labels_host.py shows on the CPU that the gate passes a plain fp32 blend on these scenes and assignments and
fails on five label bugs.  Every case is at most 112x80 pixels and 4,000 Gaussians; the fp64 references are cached per
module (one oracle run per set of lists serves every class count: label_gates.LabelReference).
"""
import math

import numpy as np
import pytest
import torch

import label_gates as LG
from feature_channel_gates import FRAMES, MULTI, camera_lists, multi_cameras, scene, tiles_of

pytestmark = pytest.mark.gpu
DEV = "cuda"
CANARY = 0xA5
GUARD = 1 << 16
C = MULTI["n_cams"]
W, H = MULTI["w"], MULTI["h"]


def _t(a):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32)).to(DEV)


def _ids(a):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.int32)).to(DEV)


def _np(x):
    return x.detach().cpu().numpy()


@pytest.fixture(scope="module")
def ops():
    from robosimgs_amd import ops as _ops
    return _ops


class _Guarded:
    """A label frame and a weight frame with 0xA5 bytes in front of and behind each."""

    def __init__(self, shape):
        n = int(np.prod(shape))
        self.lab_all = torch.full((n + 2 * GUARD,), CANARY, dtype=torch.uint8, device=DEV)
        self.w_all = torch.full((4 * (n + 2 * GUARD),), CANARY, dtype=torch.uint8, device=DEV)
        self.labels = self.lab_all[GUARD:GUARD + n].view(shape)
        self.weights = self.w_all.view(torch.float32)[GUARD:GUARD + n].view(shape)
        self.n = n

    def intact(self):
        torch.cuda.synchronize()
        return (bool((self.lab_all[:GUARD] == CANARY).all()) and bool((self.lab_all[GUARD + self.n:] == CANARY).all())
                and bool((self.w_all[:4 * GUARD] == CANARY).all()) and bool((self.w_all[4 * (GUARD + self.n):] == CANARY).all()))


# ---- 1. the stage -----------------------------------------------------------------------------------------------------------
class _Stage:
    """One FRAMES scene projected (mgs_project_color_fwd: arrays AND packed records of the same projection) and binned by the
    HIP kernels, and the fp64 references on those very values and lists."""

    def __init__(self, ops, name):
        from robosimgs_amd import camera_ring
        spec = FRAMES[name]
        self.name, self.w, self.h = name, spec["w"], spec["h"]
        self.tw, self.th = tiles_of(self.w, self.h)
        self.g = scene(spec)
        cam = camera_ring(1, self.w, self.h, thetas=[spec["theta"]])[0]
        t = self.g.to_torch(DEV, 0)
        self.n, self.opac = len(self.g), t["opacities"]
        radii, self.m2d, dep, self.con, _, _, self.splats = ops.project_color_fwd_raw(
            t["means"], t["quats"], t["scales"], t["opacities"], 0, t["colors"], _t(cam.viewmat()), _t(cam.K), self.w, self.h,
            0.3, 0.01, 1e10, 0.0, False, False, want_splats=True)
        cap = ops._upper_bound_isects(radii, self.tw, self.th) + 1
        self.tl = ops.isect_tiles_raw(self.m2d, radii, dep, self.tw, self.th, cap)
        assert int(self.tl.status.item()) == 0
        self.n_isect = int(self.tl.n_isect.item())
        self._refs = {}

    def base(self, kind):
        return LG.base_classes(kind, self.n, self.g.means)

    def ref(self, kind):
        key = "spatial" if kind == "spatial" else "random"
        if key not in self._refs:
            self._refs[key] = LG.LabelReference(_np(self.m2d), _np(self.con), _np(self.opac), _np(self.tl.flatten_ids[:self.n_isect]),
                                                _np(self.tl.tile_offsets[:-1]), self.w, self.h, self.base(key))
        return self._refs[key]

    def run(self, ops, cls, k, records, order, out=None):
        kw = dict(splats=self.splats) if records else dict(means2d=self.m2d, conics=self.con, opacities=self.opac)
        return ops.raster_labels_raw(self.tl, cls, k, self.w, self.h, out=out, use_group_order=order, **kw)


@pytest.fixture(scope="module")
def stages(ops):
    cache = {}

    def get(name):
        if name not in cache:
            cache[name] = _Stage(ops, name)
        return cache[name]
    return get


@pytest.mark.parametrize("frame", list(FRAMES))
@pytest.mark.parametrize("kind,k", LG.CASES)
def test_stage_matches_fp64_class_weights(ops, stages, kind, k, frame):
    """From means2d / conics / opacities and from the packed records, with and without tile_group_order: the same bytes,
    held to the fp64 class weights; nothing written outside the two frames."""
    st = stages(frame)
    lens = st.tl.tile_offsets[1:] - st.tl.tile_offsets[:-1]
    if frame == "ragged":
        assert st.w % 16 and st.h % 16 and int(lens.max()) > 3 * 64, int(lens.max())       # partial tiles, lists of several batches
    ids_np = LG.class_ids(kind, k, st.base(kind))
    assert (ids_np.min() == -1) == (kind == "ignore")
    cls = _ids(ids_np)
    guarded = _Guarded((st.h, st.w))
    first = st.run(ops, cls, k, records=False, order=True, out=(guarded.labels, guarded.weights))
    assert guarded.intact(), "the label kernel wrote outside its frames"
    assert not bool((guarded.w_all[4 * GUARD:4 * (GUARD + guarded.n)] == CANARY).all())
    for records, order in ((False, False), (True, True), (True, False)):
        lab, wts = st.run(ops, cls, k, records, order)
        assert torch.equal(lab, first[0]) and torch.equal(wts, first[1]), f"records={records} order={order} changes a byte"
    only, none = st.run(ops, cls, k, True, True, out=(torch.empty_like(first[0]), None))
    assert none is None and torch.equal(only, first[0])                                     # label_weights is nullable
    ref = st.ref(kind)
    LG.check_labels(ref.weights(kind, k), ref.flip_weight, _np(first[0]), _np(first[1]), what=f"{frame} {kind} K={k}")
    lab = _np(first[0])
    assert lab[lab != LG.NONE].max() < k and bool((first[1][first[0] == LG.NONE] == 0).all())


def test_raster_labels_raw_refuses_lists_the_kernel_cannot_read(ops, stages):
    """The lists reach the kernel as raw pointers: a short, an int64 or a strided one is a ValueError that names it, raised
    before anything is launched; the same call with good lists afterwards gives the bytes it gave before."""
    st = stages("ragged")
    assert st.tw * st.th >= 2
    cls = _ids(LG.class_ids("random", 7, st.base("random")))
    before = st.run(ops, cls, 7, records=True, order=True)

    def lists(**changed):
        tl = ops.TileLists()
        for name in ("flatten_ids", "tile_offsets", "group_order"):
            setattr(tl, name, changed.get(name, getattr(st.tl, name)))
        return tl

    doubled = torch.stack([st.tl.tile_offsets, st.tl.tile_offsets], dim=1)
    for bad_tl, kw, word in ((st.tl, dict(tile_offsets=st.tl.tile_offsets[1:]), "tile_offsets"),
                             (lists(tile_offsets=st.tl.tile_offsets[1:]), {}, "tile_offsets"),
                             (lists(flatten_ids=st.tl.flatten_ids.long()), {}, "flatten_ids"),
                             (st.tl, dict(tile_offsets=doubled[:, 0]), "tile_offsets"),
                             (lists(tile_offsets=st.tl.tile_offsets.long()), {}, "tile_offsets"),
                             (lists(group_order=st.tl.group_order.long()), {}, "group_order")):
        with pytest.raises(ValueError, match="^" + word):
            ops.raster_labels_raw(bad_tl, cls, 7, st.w, st.h, splats=st.splats, **kw)
    with pytest.raises(ValueError, match="^means2d must be a contiguous float32 tensor"):      # the votes call's array checks
        ops.raster_labels_raw(st.tl, cls, 7, st.w, st.h, means2d=st.m2d[:, :1], conics=st.con, opacities=st.opac)
    with pytest.raises(ValueError, match="^splats"):
        ops.raster_labels_raw(st.tl, cls, 7, st.w, st.h, splats=st.splats[:, :8])
    after = st.run(ops, cls, 7, records=True, order=True)
    assert torch.equal(after[0], before[0]) and torch.equal(after[1].view(torch.int32), before[1].view(torch.int32))


# ---- 2. against the feature operator --------------------------------------------------------------------------------------
@pytest.mark.parametrize("frame", list(FRAMES))
@pytest.mark.parametrize("k", (7, 32))
def test_labels_are_the_argmax_of_one_hot_features(ops, stages, k, frame):
    """rasterize_to_pixels on one-hot [1,N,K] features blends with the same weights in the same order: labels equal its
    argmax wherever its two largest channels differ by more than 1e-6, weights within 1e-6 of its largest channel."""
    st = stages(frame)
    ids_np = LG.class_ids("random", k, st.base("random"))
    feats = torch.from_numpy(LG.one_hot(ids_np, k)).to(DEV)
    offs = st.tl.tile_offsets[:-1].view(1, st.th, st.tw)
    flat = st.tl.flatten_ids[:st.n_isect]
    render, _ = ops.rasterize_to_pixels(st.m2d[None], st.con[None], feats[None], st.opac[None], st.w, st.h, 16, offs, flat)
    lab, wts = ops.rasterize_labels(st.m2d[None], st.con[None], st.opac[None], _ids(ids_np), k, st.w, st.h, 16, offs, flat,
                                    return_weights=True)
    assert lab.shape == (1, st.h, st.w) and lab.dtype == torch.uint8 and wts.shape == (1, st.h, st.w)
    top2 = render.topk(2, dim=-1).values
    clear = (top2[..., 0] - top2[..., 1]) > 1e-6
    arg = render.argmax(dim=-1)
    differ = int(((lab.long() != arg) & clear).sum())
    werr = float((wts - top2[..., 0]).abs().max())
    print(f"\n{frame} K={k}: {differ} clear pixels differ from the operator's argmax, largest weight difference {werr:.2e}, "
          f"{int((~clear).sum())} unclear pixels")
    assert differ == 0 and werr <= 1e-6
    assert torch.equal(ops.rasterize_labels(st.m2d[None], st.con[None], st.opac[None], _ids(ids_np).long(), k, st.w, st.h, 16,
                                            offs, flat), lab)                                  # any integer type, weights optional


# ---- 3. three cameras, every path of rasterization ---------------------------------------------------------------------------
K3 = 7


@pytest.fixture(scope="module")
def multi():
    g = scene(MULTI)
    base = LG.base_classes("random", len(g))
    return g, base, LG.class_ids("random", K3, base)


@pytest.fixture(scope="module")
def camera_refs():
    """fp64 references by (camera's projected inputs and lists): setups and paths share what is bit-identical."""
    return {}


def _gate_cameras(camera_refs, base, m2d, con, opac, lists, labels, weights, what):
    """lists[c] = (ids local to camera c, offsets from 0).  A camera without a list: 255 and weight 0 everywhere."""
    n_empty = 0
    for c in range(len(lists)):
        ids_c, offs_c = lists[c]
        lab, wts = _np(labels[c]), _np(weights[c])
        if len(ids_c) == 0:
            assert (lab == LG.NONE).all() and (wts == 0).all(), f"{what} camera {c}: no list, but labels"
            n_empty += 1
            continue
        key = (m2d[c].tobytes(), con[c].tobytes(), opac[c].tobytes(), ids_c.tobytes(), offs_c.tobytes())
        if key not in camera_refs:
            camera_refs[key] = LG.LabelReference(m2d[c], con[c], opac[c], ids_c, offs_c, W, H, base)
        ref = camera_refs[key]
        LG.check_labels(ref.weights("random", K3), ref.flip_weight, lab, wts, what=f"{what} camera {c}")
    return n_empty


@pytest.mark.parametrize("setup", ("empty_tail", "blind_middle"))
def test_operator_and_feature_path_three_cameras(ops, multi, camera_refs, setup):
    from robosimgs_amd import rasterization
    g, base, ids_np = multi
    N = len(g)
    cams = multi_cameras(setup)
    vm, Ks = _t(np.stack([c.viewmat() for c in cams])), _t(np.stack([c.K for c in cams]))
    tw, th = tiles_of(W, H)
    radii, m2d, dep, con, _ = ops.fully_fused_projection(_t(g.means), None, _t(g.quats), _t(g.scales), vm, Ks, W, H)
    _, keys, flat = ops.isect_tiles(m2d, radii, dep, 16, tw, th)
    offs = ops.isect_offset_encode(keys, C, tw, th)
    opac = _t(g.opacities)[None].expand(C, N).contiguous()
    lab, wts = ops.rasterize_labels(m2d, con, opac, _ids(ids_np), K3, W, H, 16, offs, flat, return_weights=True)
    assert lab.shape == (C, H, W) and wts.shape == (C, H, W)
    lists = [camera_lists(_np(flat), _np(offs), c, N) for c in range(C)]
    n_empty = _gate_cameras(camera_refs, base, _np(m2d), _np(con), _np(opac), lists, lab, wts, f"{setup} operator")
    assert n_empty == (1 if setup == "blind_middle" else 0)
    if setup == "empty_tail":             # most of the last camera's tiles are empty, and pixels inside listed tiles are too
        per_tile = np.diff(np.concatenate([_np(offs)[2].reshape(-1), [len(_np(flat))]]))
        assert (per_tile == 0).sum() >= 20
        none = _np(lab[2]) == LG.NONE
        listed = np.repeat(np.repeat(per_tile.reshape(th, tw) > 0, 16, 0), 16, 1)[:H, :W]
        assert (none & ~listed).sum() > 0 and (none & listed).sum() > 0 and bool((wts[2][lab[2] == LG.NONE] == 0).all())
    # rasterization(class_ids=...) with per-Gaussian features: the operator's labels, colours untouched
    feats = _t(np.random.default_rng(3).random((N, 5)))
    args = (_t(g.means), _t(g.quats), _t(g.scales), _t(g.opacities), feats, vm, Ks, W, H)
    plain = rasterization(*args)
    got = rasterization(*args, class_ids=_ids(ids_np).long(), n_classes=K3)
    assert torch.equal(plain[0], got[0]) and torch.equal(plain[1], got[1])
    assert torch.equal(got[2]["labels"], lab) and torch.equal(got[2]["label_weights"], wts)
    assert "labels" not in plain[2] and set(plain[2]) | {"labels", "label_weights"} == set(got[2])
    auto = rasterization(*args, class_ids=_ids(ids_np))                       # n_classes = max + 1, read back once
    assert torch.equal(auto[2]["labels"], lab)


@pytest.mark.parametrize("setup", ("empty_tail", "blind_middle"))
def test_sh_path_and_lean_path_three_cameras(ops, multi, camera_refs, setup):
    """The SH path on each camera's records and lists, the lean path inside the one C call: labels held to the fp64 class
    weights of the path's own projection, lean == non-lean byte for byte, colours and alphas those of the call without."""
    from robosimgs_amd import rasterization
    g, base, ids_np = multi
    t = g.to_torch(DEV, 0)
    cams = multi_cameras(setup)
    vm, Ks = _t(np.stack([c.viewmat() for c in cams])), _t(np.stack([c.K for c in cams]))
    args = (t["means"], t["quats"], t["scales"], t["opacities"], t["colors"], vm, Ks, W, H)
    cls = _ids(ids_np)
    for mode, aa in (("RGB", "classic"), ("RGB+ED", "antialiased")):
        kw = dict(sh_degree=0, render_mode=mode, rasterize_mode=aa)
        plain = rasterization(*args, **kw)
        got = rasterization(*args, class_ids=cls, n_classes=K3, **kw)
        assert torch.equal(plain[0], got[0]) and torch.equal(plain[1], got[1])
        meta = got[2]
        assert set(plain[2]) | {"labels", "label_weights"} == set(meta)
        for key in ("means2d", "conics", "radii", "depths", "opacities", "n_isects", "isect_offsets"):
            assert torch.equal(plain[2][key], meta[key]), key
        lab, wts = meta["labels"], meta["label_weights"]
        assert lab.shape == (C, H, W) and lab.dtype == torch.uint8 and wts.shape == (C, H, W) and wts.dtype == torch.float32
        counts = [int(x) for x in meta["n_isects"].tolist()]
        lists = [(_np(tl.flatten_ids[:n]), _np(tl.tile_offsets[:-1])) for tl, n in zip(meta["tile_lists"], counts)]
        # (the opacity the raster read: anti-aliased where the frame is)
        n_empty = _gate_cameras(camera_refs, base, _np(meta["means2d"]), _np(meta["conics"]), _np(meta["opacities"]), lists, lab,
                                wts, f"{setup} SH {mode} {aa}")
        assert n_empty == (1 if setup == "blind_middle" else 0)
        cap = max(counts) + 1000
        fixed = rasterization(*args, class_ids=cls, n_classes=K3, isect_capacity=cap, **kw)
        lean_plain = rasterization(*args, isect_capacity=cap, lean_meta=True, **kw)
        lean = rasterization(*args, class_ids=cls, n_classes=K3, isect_capacity=cap, lean_meta=True, **kw)
        assert set(lean[2]) == set(lean_plain[2]) | {"labels", "label_weights"} and "means2d" not in lean[2]
        assert torch.equal(lean[0], lean_plain[0]) and torch.equal(lean[1], lean_plain[1])
        assert torch.equal(lean[0], plain[0]) and torch.equal(lean[1], plain[1])
        for other in (fixed, lean):
            assert torch.equal(other[2]["labels"], lab) and torch.equal(other[2]["label_weights"], wts)
        assert int(lean[2]["isect_status"].max()) == 0


def test_labels_with_gradients_wanted_and_under_capture(ops, multi):
    """The training paths (per camera and one C call) hand out the same labels; n_classes=None is refused under capture."""
    from robosimgs_amd import rasterization
    g, base, ids_np = multi
    t = g.to_torch(DEV, 0)
    cams = multi_cameras("empty_tail")
    vm, Ks = _t(np.stack([c.viewmat() for c in cams])), _t(np.stack([c.K for c in cams]))
    cls = _ids(ids_np)
    args = (t["quats"], t["scales"], t["opacities"], t["colors"], vm, Ks, W, H)
    want = rasterization(t["means"], *args, sh_degree=0, class_ids=cls, n_classes=K3)[2]
    for cap in (None, 200_000):
        means = t["means"].clone().requires_grad_(True)
        col, _, meta = rasterization(means, *args, sh_degree=0, class_ids=cls, n_classes=K3, isect_capacity=cap)
        assert torch.equal(meta["labels"], want["labels"]) and torch.equal(meta["label_weights"], want["label_weights"])
        assert not meta["labels"].requires_grad and not meta["label_weights"].requires_grad
        col.sum().backward()
        assert bool(torch.isfinite(means.grad).all())
    with pytest.raises(ValueError, match="n_classes"):
        rasterization(t["means"], *args, sh_degree=0, class_ids=cls, n_classes=33)
    with pytest.raises(ValueError, match="integer"):
        rasterization(t["means"], *args, sh_degree=0, class_ids=cls.float(), n_classes=K3)
    s = torch.cuda.Stream()
    with torch.cuda.stream(s):
        rasterization(t["means"], *args, sh_degree=0, class_ids=cls, n_classes=K3, isect_capacity=200_000, lean_meta=True)
        torch.cuda.synchronize()
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph, stream=s):
            with pytest.raises(ValueError, match="graph capture"):
                rasterization(t["means"], *args, sh_degree=0, class_ids=cls, isect_capacity=200_000, lean_meta=True)
            _, _, meta = rasterization(t["means"], *args, sh_degree=0, class_ids=cls, n_classes=K3, isect_capacity=200_000,
                                       lean_meta=True)
        graph.replay()
    torch.cuda.synchronize()
    assert torch.equal(meta["labels"], want["labels"]) and torch.equal(meta["label_weights"], want["label_weights"])


# ---- 4. FrameRenderer, static scene --------------------------------------------------------------------------------------
def _eager(fr_t, cam, cls, k, **kw):
    """rasterization with per-camera intermediates on the renderer's own copy: (labels [H,W], weights, meta)."""
    from robosimgs_amd import rasterization
    _, _, meta = rasterization(fr_t["means"], fr_t["quats"], fr_t["scales"], fr_t["opacities"], fr_t["colors"],
                               _t(cam.viewmat())[None], _t(cam.K)[None], W, H, sh_degree=fr_t["sh_degree"], class_ids=cls,
                               n_classes=k, **kw)
    return meta["labels"][0], meta["label_weights"][0], meta


def _gate_eager(meta, base_or_ids, k, labels, weights, what, kind="random"):
    """Gate `labels` against the fp64 class weights of the eager frame's own projection and lists.  base_or_ids: base
    classes (kind "random") or, for kind None, the class ids themselves (< 32: they are their own base classes)."""
    n = int(meta["n_isects"][0])
    tl = meta["tile_lists"][0]
    ref = LG.LabelReference(_np(meta["means2d"][0]), _np(meta["conics"][0]), _np(meta["opacities"][0]), _np(tl.flatten_ids[:n]),
                            _np(tl.tile_offsets[:-1]), W, H, base_or_ids)
    Wk = ref.weights(kind, k) if kind else ref.blend.img[..., :k]
    return LG.check_labels(Wk, ref.flip_weight, _np(labels), _np(weights), what=what)


@pytest.mark.parametrize("reorder", (None, "morton"))
def test_frame_renderer_static_scene(multi, reorder):
    """Three frames in flight, six cameras: every fetched label frame is its own camera's (a slot never returns the
    previous replay's buffer), on both schedules -- a lone submit, then bursts."""
    from robosimgs_amd import FrameRenderer, camera_ring
    g, base, ids_np = multi
    t = g.to_torch(DEV, 0)
    cams = camera_ring(6, W, H)
    fr = FrameRenderer(t, W, H, frames_in_flight=3, isect_capacity=200_000, reorder=reorder, class_ids=_ids(ids_np).long(),
                       n_classes=K3)
    assert (fr.order is None) == (reorder is None)
    order = _np(fr.order) if fr.order is not None else np.arange(len(g))
    assert torch.equal(fr.class_ids, _ids(ids_np[order])) and fr.class_ids.dtype == torch.int32
    got, variants = [], []

    def take(tk):
        f = fr.fetch(tk)
        assert f["labels"].shape == (H, W) and f["labels"].dtype == torch.uint8 and f["label_weights"].shape == (H, W)
        got.append((f["labels"].clone(), f["label_weights"].clone()))
        fr.release(tk)

    tk = fr.submit(cams[0].viewmat(), cams[0].K)                 # alone: the latency schedule's graph
    variants.append(fr._slots[tk]["variant"])
    take(tk)
    tickets = []
    for cam in cams[1:]:
        if len(tickets) == 3:
            take(tickets.pop(0))
        tickets.append(fr.submit(cam.viewmat(), cam.K))
        variants.append(fr._slots[tickets[-1]]["variant"])
    for tk in tickets:
        take(tk)
    assert fr.isect_status_max() == 0 and {"latency", "throughput"} <= set(variants), variants
    for i, cam in enumerate(cams):
        lab, wts, meta = _eager(fr.t, cam, fr.class_ids, K3)
        assert torch.equal(got[i][0], lab) and torch.equal(got[i][1], wts), f"camera {i}: not this camera's label frame"
        if i in (0, 5):               # the lone frame and the last of a burst against fp64, on the renderer's own copy
            _gate_eager(meta, base[order], K3, got[i][0], got[i][1], f"FrameRenderer reorder={reorder} camera {i}")
    for i in range(1, 6):
        assert not torch.equal(got[i][0], got[i - 1][0])
    one = fr.render(cams[2].viewmat(), cams[2].K)
    assert torch.equal(one["labels"], got[2][0]) and torch.equal(one["label_weights"], got[2][1])


# ---- 5. FrameRenderer, dynamic scene ---------------------------------------------------------------------------------------
def _rot_z(a):
    c, s = math.cos(a), math.sin(a)
    return np.array([[c, -s, 0.0], [s, c, 0.0], [0.0, 0.0, 1.0]])


def test_frame_renderer_dynamic_scene_labels_the_groups(multi):
    """group_ids with two groups, labels=True: class = group id + 1, static Gaussians class 0; one group rotated per frame.
    The reference is built on transform_gaussians' posed output.  The dataset output changes no label byte."""
    from robosimgs_amd import FrameRenderer, camera_ring, transform_gaussians
    g, _, _ = multi
    t = g.to_torch(DEV, 0)
    # groups cut by world z: the ring cameras look across the z axis, so every one of them sees the bottom slab (group 0),
    # the static middle and the top slab (group 1) side by side.  (Cut by world x, the scene being opaque, the slab on the
    # far side of a camera is hidden behind the other two and its class is nowhere the largest.)
    z = g.means[:, 2]
    gid_np = np.where(z < np.quantile(z, 0.3), 0, np.where(z > np.quantile(z, 0.7), 1, -1)).astype(np.int32)
    cams = camera_ring(3, W, H)
    poses = [([_rot_z(0.5 * i), np.eye(3)], [np.zeros(3), np.zeros(3)]) for i in range(3)]
    kw = dict(render_mode="RGB+ED", frames_in_flight=3, isect_capacity=200_000, group_ids=_ids(gid_np), n_groups=2, labels=True)
    fr = FrameRenderer(t, W, H, **kw)
    ds = FrameRenderer(t, W, H, dataset_output=torch.float16, dataset_K=cams[0].K, dataset_keep_float=False, **kw)
    assert fr.n_classes == 3 and torch.equal(fr.class_ids, fr.group_ids + 1)
    frames = []
    for r in (fr, ds):
        tickets = [r.submit(cam.viewmat(), cam.K, rotations=Rs, translations=ts) for cam, (Rs, ts) in zip(cams, poses)]
        out = []
        for tk in tickets:
            f = r.fetch(tk)
            out.append((f["labels"].clone(), f["label_weights"].clone(), f.get("rgba") is not None, f["colors"] is None))
            r.release(tk)
        frames.append(out)
    for i, (cam, (Rs, ts)) in enumerate(zip(cams, poses)):
        posed = transform_gaussians(fr.t, Rs, ts, group_ids=fr.group_ids)
        posed["sh_degree"] = fr.t["sh_degree"]
        lab, wts, meta = _eager(posed, cam, fr.class_ids, 3, render_mode="RGB+ED")
        assert torch.equal(frames[0][i][0], lab) and torch.equal(frames[0][i][1], wts)
        if i == 2:
            _gate_eager(meta, _np(fr.class_ids), 3, lab, wts, f"dynamic scene frame {i}", kind=None)
        seen = set(np.unique(_np(lab)).tolist())
        assert {0, 1, 2} <= seen, seen                  # class 0: only static Gaussians seen there
        assert frames[1][i][2] and frames[1][i][3]      # the dataset renderer wrote RGBA8 and no float frame
        assert torch.equal(frames[1][i][0], lab) and torch.equal(frames[1][i][1], wts), "dataset output changed a label"
    with pytest.raises(ValueError):
        FrameRenderer(t, W, H, isect_capacity=1000, labels=True)                          # no group_ids to take classes from


# ---- 6. an overflowed capacity ------------------------------------------------------------------------------------------------
def test_overflowed_capacity_returns_and_stays_inside_the_label_frames(ops, multi):
    g, _, ids_np = multi
    t = g.to_torch(DEV, 0)
    cams = multi_cameras("ring")
    vm, Ks = _t(np.stack([c.viewmat() for c in cams])), _t(np.stack([c.K for c in cams]))
    guarded = _Guarded((C, H, W))
    _, _, n_isects, status = ops.render_frames_raw(
        t["means"], t["quats"], t["scales"], t["opacities"], 0, t["colors"], vm, Ks, W, H, 0.3, 0.01, 1e10, 0.0, False, False, 64,
        labels=(_ids(ids_np), K3, guarded.labels, guarded.weights))
    assert guarded.intact(), "the label kernel wrote outside its frames"
    assert int(status.min()) == 1 and int(n_isects.min()) > 64
    lab = _np(guarded.labels)
    assert ((lab < K3) | (lab == LG.NONE)).all() and bool(torch.isfinite(guarded.weights).all())
