"""2D masks lifted onto Gaussians on the GPU (include/mgs_lift.h, csrc/lift.hip): raster_votes_kernel and lift_assign_kernel
against the fp64 votes of tests/lift_gates.py, on the GPU's own projection and lists, through every layer --
ops.raster_votes_raw, ops.rasterize_votes, ops.assign_classes, lift_labels.

tests/test_lift_host.py shows on the CPU that the gate passes a plain fp32 walk on these scenes and masks and fails on
eight vote bugs.  Every case is at most 112x80 pixels and 4,000 Gaussians; the fp64 references are cached per module (one
blend and one walk per set of lists serve every mask).
"""
import numpy as np
import pytest
import torch

import lift_gates as LF
from feature_channel_gates import FRAMES, MULTI, MULTI_SETUPS, camera_lists, multi_cameras, scene, tiles_of
from label_gates import WEIGHT_TOL
from lens_ref import MILD

pytestmark = pytest.mark.gpu
DEV = "cuda"
CANARY = 0xA5
GUARD = 1 << 16
C = MULTI["n_cams"]
W, H = MULTI["w"], MULTI["h"]
K3 = 7


def _t(a):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32)).to(DEV)


def _u8(a):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.uint8)).to(DEV)


def _np(x):
    return x.detach().cpu().numpy()


@pytest.fixture(scope="module")
def ops():
    from robosimgs_amd import ops as _ops
    return _ops


def _zeros(n, k):
    return torch.zeros(n, k, dtype=torch.int64, device=DEV)


class _Guarded:
    """A tensor of `shape` and `dtype` with 0xA5 bytes in front of and behind it."""

    def __init__(self, shape, dtype):
        size = torch.empty(0, dtype=dtype).element_size()
        self.n = int(np.prod(shape)) * size
        self.all = torch.full((self.n + 2 * GUARD,), CANARY, dtype=torch.uint8, device=DEV)
        self.t = self.all[GUARD:GUARD + self.n].view(dtype).view(shape)

    def intact(self):
        torch.cuda.synchronize()
        return bool((self.all[:GUARD] == CANARY).all()) and bool((self.all[GUARD + self.n:] == CANARY).all())


# ---- 1. the stage -----------------------------------------------------------------------------------------------------------
class _Stage:
    """One FRAMES scene projected (mgs_project_color_fwd: arrays AND packed records of the same projection) and binned by the
    HIP kernels, and the fp64 vote reference on those very values and lists."""

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
        self.tl = ops.isect_tiles_raw(self.m2d, radii, dep, self.tw, self.th, cap, want_pair_info=True)
        assert int(self.tl.status.item()) == 0
        self.n_isect = int(self.tl.n_isect.item())
        self.masks_np = LF.masks_for(self.w, self.h)
        self.masks = {case: _u8(m) for case, (m, _) in self.masks_np.items()}
        self._ref = None

    @property
    def ref(self):
        if self._ref is None:
            self._ref = LF.VoteReference(_np(self.m2d), _np(self.con), _np(self.opac), _np(self.tl.flatten_ids[:self.n_isect]),
                                         _np(self.tl.tile_offsets[:-1]), self.w, self.h, self.masks_np)
        return self._ref

    def run(self, ops, case, records=False, order=True, votes=None, mask=None):
        kw = dict(splats=self.splats) if records else dict(means2d=self.m2d, conics=self.con, opacities=self.opac)
        votes = _zeros(self.n, case[1]) if votes is None else votes
        return ops.raster_votes_raw(self.tl, self.masks[case] if mask is None else mask, case[1], self.w, self.h, votes,
                                    use_group_order=order, **kw)


@pytest.fixture(scope="module")
def stages(ops):
    cache = {}

    def get(name):
        if name not in cache:
            cache[name] = _Stage(ops, name)
        return cache[name]
    return get


@pytest.mark.parametrize("frame", list(FRAMES))
@pytest.mark.parametrize("kind,k", LF.CASES)
def test_stage_matches_fp64_votes(ops, stages, kind, k, frame):
    """From means2d / conics / opacities and from the packed records: the same bits, held to the fp64 votes; the classes
    and confidences of assign_classes held to the reference's; nothing written outside the vote buffer."""
    st = stages(frame)
    case = (kind, k)
    if frame == "ragged":
        lens = st.tl.tile_offsets[1:] - st.tl.tile_offsets[:-1]
        assert st.w % 16 and st.h % 16 and int(lens.max()) > 3 * 64, int(lens.max())       # partial tiles, lists of several batches
    guarded = _Guarded((st.n, k), torch.int64)
    guarded.t.zero_()
    votes = st.run(ops, case, votes=guarded.t)
    assert guarded.intact(), "the vote kernel wrote outside its buffer"
    records = st.run(ops, case, records=True)
    assert torch.equal(votes, records), "packed records and separate arrays give different votes"
    cls, conf = ops.assign_classes(votes)
    assert cls.dtype == torch.int32 and conf.dtype == torch.float32 and cls.shape == conf.shape == (st.n,)
    LF.check_votes(st.ref.V(case), st.ref.bound(case), _np(votes), _np(cls), _np(conf), capped=case in LF.CAPPED,
                   what=f"{frame} {kind} K={k}")
    want_cls, want_conf = LF.assign(_np(votes))
    assert np.array_equal(_np(cls), want_cls) and np.allclose(_np(conf), want_conf, rtol=0, atol=1e-7)
    assert int(cls.max()) < k and bool((conf[cls < 0] == 0).all()) and bool((conf[cls >= 0] > 0).all())
    cls5, conf5 = ops.assign_classes(votes, 0.5)
    LF.check_votes(st.ref.V(case), st.ref.bound(case), _np(votes), _np(cls5), _np(conf5), min_vote=0.5,
                   what=f"{frame} {kind} K={k} min_vote 0.5")
    if kind == "high":                                    # values K..254 vote for nothing: the ignore mask's votes
        assert torch.equal(votes, st.run(ops, ("ignore", k)))


# ---- 2. integers ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("frame", list(FRAMES))
def test_votes_are_bit_reproducible_and_accumulate(ops, stages, frame):
    st = stages(frame)
    for case in (("stripes", 7), ("checker", 32)):
        first = st.run(ops, case)
        assert int(first.sum()) > 0
        assert torch.equal(first, st.run(ops, case)), "two runs differ"
        assert torch.equal(first, st.run(ops, case, order=False)), "the launch order changes a vote"
        assert torch.equal(first, st.run(ops, case, records=True, order=False))
        twice = st.run(ops, case, votes=first.clone())
        assert torch.equal(twice, 2 * first), "a second call into the same buffer is not an exact doubling"
        nothing = torch.full((st.h, st.w), LF.IGNORE, dtype=torch.uint8, device=DEV)
        kept = st.run(ops, case, votes=first.clone(), mask=nothing)
        assert torch.equal(kept, first), "an all-255 mask changed the votes"
        high = torch.full((st.h, st.w), case[1], dtype=torch.uint8, device=DEV)          # the first value that is no class
        assert torch.equal(st.run(ops, case, votes=first.clone(), mask=high), first)


def test_raster_votes_raw_refuses_buffers_the_kernel_cannot_read(ops, stages):
    st = stages("ragged")
    case = ("stripes", 7)
    good = dict(means2d=st.m2d, conics=st.con, opacities=st.opac)
    for bad, word in ((dict(conics=st.con.double()), "conics"), (dict(means2d=st.m2d[:-1]), "must be a contiguous float32 tensor"),
                      (dict(opacities=st.opac[::2]), "opacities"), (dict(conics=None), "needs splats")):
        with pytest.raises(ValueError, match=word):
            ops.raster_votes_raw(st.tl, st.masks[case], 7, st.w, st.h, _zeros(st.n, 7), **{**good, **bad})
    with pytest.raises(ValueError, match="splats"):
        ops.raster_votes_raw(st.tl, st.masks[case], 7, st.w, st.h, _zeros(st.n, 7), splats=st.splats[:, :8])
    with pytest.raises(ValueError, match="votes"):
        ops.raster_votes_raw(st.tl, st.masks[case], 7, st.w, st.h, _zeros(st.n, 7).int(), **good)
    with pytest.raises(ValueError, match="mask"):
        ops.raster_votes_raw(st.tl, st.masks[case][:-1], 7, st.w, st.h, _zeros(st.n, 7), **good)
    with pytest.raises(ValueError, match="tile_offsets"):
        ops.raster_votes_raw(st.tl, st.masks[case], 7, st.w, st.h, _zeros(st.n, 7), tile_offsets=st.tl.tile_offsets[1:], **good)


# ---- 3. against the record backward ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("frame", list(FRAMES))
@pytest.mark.parametrize("kind,k", (("stripes", 1), ("stripes", 7), ("checker", 32)))
def test_votes_equal_v_feats_of_the_record_backward(ops, stages, kind, k, frame):
    """The same lists, the same decisions bit for bit -- no flip budget: v_feats of rasterize_bwd_det_raw with features ones
    [N,K], v_render one-hot(mask), v_alphas None, no background, within test_backward_matches_fp64_autograd's 1e-4 of the
    largest entry."""
    st = stages(frame)
    feats = torch.ones(st.n, k, device=DEV)
    out = ops.rasterize_fwd_raw(st.m2d, st.con, feats, st.opac, None, st.w, st.h, st.tw, st.th, st.tl.tile_offsets,
                                st.tl.flatten_ids)
    v_render = torch.nn.functional.one_hot(st.masks[(kind, k)].long(), k).float().contiguous()
    v_feats = ops.rasterize_bwd_det_raw(st.m2d, st.con, feats, st.opac, None, st.w, st.h, st.tw, st.th, st.tl, out[1], out[2],
                                        v_render, None)[2]
    votes = ops.votes_to_float(st.run(ops, (kind, k)))
    assert votes.dtype == torch.float64
    err, scale = float((votes - v_feats.double()).abs().max()), float(v_feats.abs().max())
    print(f"\n{frame} {kind} K={k}: largest difference from the backward's v_feats {err:.2e} at a largest entry of {scale:.1f}")
    assert scale > 5 and err <= 1e-4 * scale


# ---- 4. conservation ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("frame", list(FRAMES))
def test_votes_of_a_class_sum_to_the_alpha_under_its_mask(ops, stages, frame):
    st = stages(frame)
    feats = torch.ones(st.n, 1, device=DEV)
    alphas = ops.rasterize_fwd_raw(st.m2d, st.con, feats, st.opac, None, st.w, st.h, st.tw, st.th, st.tl.tile_offsets,
                                   st.tl.flatten_ids)[1].double()
    for case in (("stripes", 7), ("checker", 32), ("ignore", 7)):
        votes = ops.votes_to_float(st.run(ops, case))
        for k in range(case[1]):
            under = st.masks[case] == k
            got, want, pixels = float(votes[:, k].sum()), float(alphas[under].sum()), int(under.sum())
            assert pixels > 0 and abs(got - want) <= WEIGHT_TOL * pixels, (case, k, got, want, pixels)


# ---- 5./6. three cameras: the operator ------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def multi(ops):
    """MULTI's scene under each setup, projected and binned by the operators."""
    g = scene(MULTI)
    cache = {}

    def get(setup):
        if setup not in cache:
            cams = multi_cameras(setup)
            vm, Ks = _t(np.stack([c.viewmat() for c in cams])), _t(np.stack([c.K for c in cams]))
            tw, th = tiles_of(W, H)
            radii, m2d, dep, con, _ = ops.fully_fused_projection(_t(g.means), None, _t(g.quats), _t(g.scales), vm, Ks, W, H)
            _, keys, flat = ops.isect_tiles(m2d, radii, dep, 16, tw, th)
            offs = ops.isect_offset_encode(keys, C, tw, th)
            opac = _t(g.opacities)[None].expand(C, len(g)).contiguous()
            cache[setup] = dict(m2d=m2d, con=con, opac=opac, flat=flat, offs=offs, vm=vm, Ks=Ks)
        return g, cache[setup]
    return get


def _camera_masks():
    """Three different masks of K3 classes: stripes, ignore, checker."""
    return np.stack([LF.make_mask(kind, K3, W, H) for kind in ("stripes", "ignore", "checker")])


@pytest.mark.parametrize("setup", MULTI_SETUPS)
def test_operator_is_the_sum_of_its_cameras_and_stays_inside_its_buffers(ops, multi, setup):
    g, m = multi(setup)
    N = len(g)
    masks = _u8(_camera_masks())
    votes, cls, conf = _Guarded((N, K3), torch.int64), _Guarded((N,), torch.int32), _Guarded((N,), torch.float32)
    votes.t.zero_()
    got = ops.rasterize_votes(m["m2d"], m["con"], m["opac"], masks, K3, W, H, 16, m["offs"], m["flat"], votes=votes.t)
    ops.assign_classes(got, out=(cls.t, conf.t))
    assert votes.intact() and cls.intact() and conf.intact(), "written outside votes, class_ids or confidence"
    assert got.data_ptr() == votes.t.data_ptr() and int(cls.t.max()) == K3 - 1 and int(cls.t.min()) >= -1
    fresh = ops.rasterize_votes(m["m2d"], m["con"], m["opac"], masks, K3, W, H, 16, m["offs"], m["flat"])
    assert torch.equal(fresh, got) and fresh.shape == (N, K3) and fresh.dtype == torch.int64
    # camera by camera on its own lists, ids local to the camera
    total, per_cam = _zeros(N, K3), []
    for c in range(C):
        ids_c, offs_c = camera_lists(_np(m["flat"]), _np(m["offs"]), c, N)
        if len(ids_c) == 0:                       # a camera that sees nothing has no list to hand over
            per_cam.append(0)
            continue
        tl = ops.TileLists()
        tl.flatten_ids = torch.from_numpy(ids_c).to(DEV)
        tl.tile_offsets = torch.from_numpy(np.concatenate([offs_c.reshape(-1), [len(ids_c)]]).astype(np.int32)).to(DEV)
        one = ops.raster_votes_raw(tl, masks[c], K3, W, H, _zeros(N, K3), means2d=m["m2d"][c].contiguous(),
                                   conics=m["con"][c].contiguous(), opacities=m["opac"][c].contiguous())
        per_cam.append(int(one.sum()))
        total += one
    assert torch.equal(total, got), "the operator is not the sum of its cameras"
    assert (per_cam[1] == 0) == (setup == "blind_middle") and per_cam[0] > 0 and per_cam[2] > 0, per_cam
    # a window of rows: ids outside it are skipped, never written
    lo, rows = N // 3, N // 2
    window = _Guarded((rows, K3), torch.int64)
    window.t.zero_()
    tl = ops.TileLists()
    tl.flatten_ids = m["flat"].to(torch.int32).contiguous()
    offsets = torch.cat([m["offs"].reshape(-1).to(torch.int32), torch.tensor([tl.flatten_ids.numel()], dtype=torch.int32, device=DEV)])
    n_tiles = m["offs"][0].numel()
    for c in range(C):
        ops.raster_votes_raw(tl, masks[c], K3, W, H, window.t, means2d=m["m2d"].view(C * N, 2), conics=m["con"].view(C * N, 3),
                             opacities=m["opac"].view(C * N), row_offset=c * N + lo, use_group_order=False,
                             tile_offsets=offsets[c * n_tiles:])
    assert window.intact() and torch.equal(window.t, got[lo:lo + rows])


# ---- 7. lift_labels ---------------------------------------------------------------------------------------------------------
VARIANTS = {"pinhole": dict(), "antialiased": dict(rasterize_mode="antialiased"), "opacity_aware": dict(radius_rule="opacity_aware"),
            "fisheye": dict(camera_model="fisheye", distortion=MILD)}


def _reference_of(debug, masks_np, name):
    """(V, B) summed over the cameras of a lift_labels call, on that call's own projected inputs and lists."""
    V = B = 0
    for d, mask in zip(debug, masks_np):
        n = int(d["lists"].n_isect.item())
        assert int(d["lists"].status.item()) == 0
        if n == 0:
            continue
        ref = LF.VoteReference(_np(d["means2d"]), _np(d["conics"]), _np(d["opacities"]), _np(d["lists"].flatten_ids[:n]),
                               _np(d["lists"].tile_offsets[:-1]), W, H, {name: (mask, K3)})
        V, B = V + ref.V(name), B + ref.bound(name)
    return V, B


@pytest.mark.parametrize("variant", list(VARIANTS))
def test_lift_labels_end_to_end(multi, variant):
    """Two ring cameras, stripes and ignore masks: votes, classes and confidences held to the fp64 walk of the call's own
    projection and lists; the second camera continued through votes= gives the same bits as one call."""
    from robosimgs_amd import lift_labels
    g, m = multi("ring")
    t = g.to_torch(DEV, 0)
    masks_np = _camera_masks()[:2]
    masks = _u8(masks_np)
    args = (t["means"], t["quats"], t["scales"], t["opacities"])
    kw = VARIANTS[variant]
    debug = []
    res = lift_labels(*args, m["vm"][:2], m["Ks"][:2], W, H, masks, K3, _debug=debug, **kw)
    assert res.votes.shape == (len(g), K3) and res.class_ids.shape == res.confidence.shape == (len(g),) and len(debug) == 2
    if variant == "antialiased":
        assert bool((debug[0]["opacities"] < t["opacities"]).any())
    V, B = _reference_of(debug, masks_np, "m")
    st = LF.check_votes(V, B, _np(res.votes), _np(res.class_ids), _np(res.confidence), capped=True, what=f"lift_labels {variant}")
    assert st["voted"] > 0.8 * len(g)
    first = lift_labels(*args, m["vm"][:1], m["Ks"][:1], W, H, masks[:1], K3, **kw)
    assert not torch.equal(first.votes, res.votes)
    both = lift_labels(*args, m["vm"][1:2], m["Ks"][1:2], W, H, masks[1:2].cpu(), K3, votes=first.votes,
                       **kw)                                                         # (a host mask is uploaded by the call)
    assert both.votes.data_ptr() == first.votes.data_ptr()
    assert torch.equal(both.votes, res.votes) and torch.equal(both.class_ids, res.class_ids)
    assert torch.equal(both.confidence, res.confidence)
    strict = lift_labels(*args, m["vm"][:2], m["Ks"][:2], W, H, masks, K3, min_vote=2.0, **kw)
    LF.check_votes(V, B, _np(strict.votes), _np(strict.class_ids), _np(strict.confidence), min_vote=2.0,
                   what=f"lift_labels {variant} min_vote 2")
    assert int((strict.class_ids < 0).sum()) > int((res.class_ids < 0).sum())


def test_lift_labels_refuses_what_it_cannot_lift(multi):
    from robosimgs_amd import lift_labels
    g, m = multi("ring")
    t = g.to_torch(DEV, 0)
    args = (t["means"], t["quats"], t["scales"], t["opacities"], m["vm"], m["Ks"], W, H)
    masks = _u8(_camera_masks())
    with pytest.raises(ValueError, match="masks"):
        lift_labels(*args, masks[:2], K3)
    with pytest.raises(ValueError, match="masks"):
        lift_labels(*args, masks.float(), K3)
    with pytest.raises(ValueError, match="n_classes"):
        lift_labels(*args, masks, 33)
    with pytest.raises(ValueError, match="votes"):
        lift_labels(*args, masks, K3, votes=_zeros(len(g), K3 + 1))
    with pytest.raises(ValueError, match="distortion"):
        lift_labels(*args, masks, K3, distortion=MILD)


# ---- 8. graph capture -----------------------------------------------------------------------------------------------------
def test_assign_classes_replays_in_a_graph(ops, stages):
    st = stages("ragged")
    a, b = st.run(ops, ("stripes", 7)), st.run(ops, ("checker", 7))
    want_a, want_b = ops.assign_classes(a, 0.25), ops.assign_classes(b, 0.25)
    assert not torch.equal(want_a[0], want_b[0])
    votes = a.clone()
    cls = torch.empty(st.n, dtype=torch.int32, device=DEV)
    conf = torch.empty(st.n, dtype=torch.float32, device=DEV)
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        ops.assign_classes(votes, 0.25, out=(cls, conf))
        torch.cuda.synchronize()
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph, stream=s):
            ops.assign_classes(votes, 0.25, out=(cls, conf))
        graph.replay()
        torch.cuda.synchronize()
        assert torch.equal(cls, want_a[0]) and torch.equal(conf, want_a[1])
        votes.copy_(b)
        graph.replay()
    torch.cuda.synchronize()
    assert torch.equal(cls, want_b[0]) and torch.equal(conf, want_b[1])


# ---- 9. round trip ----------------------------------------------------------------------------------------------------------
def test_round_trip_label_frames_lifted_back(multi):
    """Label frames of rasterization(class_ids=spatial classes) on MULTI's ring, lifted back: the votes satisfy gate (a)
    against the fp64 walk with those label frames as masks.  The recovered share is printed, not asserted: a Gaussian's
    votes follow the pixels' majority label, which is not its own class at mixed pixels."""
    from robosimgs_amd import lift_labels, rasterization
    g, m = multi("ring")
    t = g.to_torch(DEV, 0)
    z = g.means[:, 2]
    true_np = np.searchsorted(np.quantile(z, [1 / 3, 2 / 3]), z).astype(np.int32)       # three slabs along world z
    true = torch.from_numpy(true_np).to(DEV)
    args = (t["means"], t["quats"], t["scales"], t["opacities"])
    meta = rasterization(*args, t["colors"], m["vm"], m["Ks"], W, H, sh_degree=0, class_ids=true, n_classes=3)[2]
    labels = meta["labels"]
    assert labels.shape == (C, H, W) and labels.dtype == torch.uint8 and {0, 1, 2} <= set(np.unique(_np(labels))) <= {0, 1, 2, 255}
    debug = []
    res = lift_labels(*args, m["vm"], m["Ks"], W, H, labels, 3, _debug=debug)
    labels_np = _np(labels)
    V = B = 0
    for d, mask in zip(debug, labels_np):
        n = int(d["lists"].n_isect.item())
        ref = LF.VoteReference(_np(d["means2d"]), _np(d["conics"]), _np(d["opacities"]), _np(d["lists"].flatten_ids[:n]),
                               _np(d["lists"].tile_offsets[:-1]), W, H, {"labels": (mask, 3)})
        V, B = V + ref.V("labels"), B + ref.bound("labels")
    LF.check_votes(V, B, _np(res.votes), what="round trip")
    voted = res.class_ids >= 0
    same = (res.class_ids == true) & voted
    sure = voted & (res.confidence >= 0.9)
    print(f"\nround trip: {int(voted.sum())} of {len(g)} Gaussians voted, {float(same.sum()) / max(1, int(voted.sum())):.3f} of them "
          f"recover their class, {float((same & sure).sum()) / max(1, int(sure.sum())):.3f} of the {int(sure.sum())} at confidence >= 0.9")
    assert int(voted.sum()) > 0.8 * len(g)
