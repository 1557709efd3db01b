"""The blend stage at every `with_channels` instantiation (csrc/mgs_common.h: CHT = 1, 2, 3, 4, 8, 16, 32) against fp64.

Counts of 5..32 run in the next bucket up behind `c < channels` guards, in kernels that share no blend body with the
3- and 4-channel ones (no lane-mask PixelState, no per-block kernel, the whole-list backward walk only,
reduce_records_kernel).  Each count in feature_channel_gates.CHANNELS goes through mgs_rasterize_fwd (training and
inference variant), mgs_rasterize_bwd (atomics) and mgs_rasterize_bwd_det (records) on two frames -- a whole number of
tiles and one ragged in both axes -- on identical inputs: the scene projected and binned once by the HIP kernels, features
and background from a seeded generator.

Forward: O.check_frame against O.rasterize in fp64 (tolerance 1e-4, zero unexplained pixels, flip bound required), the
numbers of test_gpu_forward.py::test_rasterize_matches_oracle.  Backward: fp64 autograd through OT.rasterize on the same
lists, through grad_gate.compare at the parameters of test_gpu_backward.py::test_rasterize_backward (row_tol 2e-3,
bad_frac 5e-3, cosine 0.9999).  tests/test_feature_channels_host.py shows on the CPU that these gates pass a plain fp32
blend and fail on channel bugs.
"""
import numpy as np
import pytest
import torch

from feature_channel_gates import (CHANNELS, FRAMES, MAX_CH, BackwardReference, BlendReference, check_forward, cotangents,
                                   features, scene, tiles_of)
from grad_gate import compare

pytestmark = pytest.mark.gpu
DEV = "cuda"
WIDE = tuple(ch for ch in CHANNELS if ch > 4)
GRAD_NAMES = ("v_means2d", "v_conics", "v_feats", "v_opacities")
CANARY = 0xA5
GUARD_FLOATS = 1 << 16


def _t(a):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32)).to(DEV)


class _Inputs:
    """One frame's blend inputs on the device (projected by mgs_projection_fwd, binned by mgs_isect_tiles with the record
    slots) and, built on first use, the fp64 references on the very same fp32 values and lists."""

    def __init__(self, ops, name):
        from robosimgs_amd import camera_ring
        spec = FRAMES[name]
        self.name, self.w, self.h = name, spec["w"], spec["h"]
        self.tw, self.th = tiles_of(self.w, self.h)
        g = scene(spec)
        cam = camera_ring(1, self.w, self.h, thetas=[spec["theta"]])[0]
        t = g.to_torch(DEV, 0)
        self.n, self.opac = len(g), t["opacities"]
        radii, self.m2d, dep, self.con, _ = ops.projection_fwd_raw(t["means"], t["quats"], t["scales"], _t(cam.viewmat()),
                                                                    _t(cam.K), self.w, self.h, 0.3, 0.01, 1e10, 0.0, False)
        cap = ops._upper_bound_isects(radii, self.tw, self.th) + 1
        self.tl = ops.isect_tiles_raw(self.m2d, radii, dep, self.tw, self.th, cap, want_pair_info=True)
        assert int(self.tl.status.item()) == 0
        self.n_isect = int(self.tl.n_isect.item())
        self.feats_np, self.bg_np = features(self.n)
        self.vr_np, self.va_np = cotangents(self.w, self.h)
        self.va = _t(self.va_np)
        self._ref = self._bref = None

    def lists(self):
        return (self.m2d.cpu().numpy(), self.con.cpu().numpy(), self.feats_np, self.opac.cpu().numpy(),
                self.tl.flatten_ids[:self.n_isect].cpu().numpy(), self.tl.tile_offsets[:-1].cpu().numpy(), self.w, self.h)

    @property
    def ref(self):
        if self._ref is None:
            self._ref = BlendReference(*self.lists())
        return self._ref

    @property
    def bref(self):
        if self._bref is None:
            self._bref = BackwardReference(*self.lists())
        return self._bref

    def feats(self, ch):
        return _t(self.feats_np[:, :ch])

    def bg(self, ch):
        return _t(self.bg_np[:ch])

    def vr(self, ch):
        return _t(self.vr_np[..., :ch])

    def fwd(self, ops, ch, bg=True, **kw):
        return ops.rasterize_fwd_raw(self.m2d, self.con, self.feats(ch), self.opac, self.bg(ch) if bg else None, self.w, self.h,
                                     self.tw, self.th, self.tl.tile_offsets, self.tl.flatten_ids, **kw)

    def bwd_atomic(self, ops, ch, out, bg=True, vr=None, **kw):
        return ops.rasterize_bwd_raw(self.m2d, self.con, self.feats(ch), self.opac, self.bg(ch) if bg else None, self.w, self.h,
                                     self.tw, self.th, self.tl.tile_offsets, self.tl.flatten_ids, out[1], out[2],
                                     self.vr(ch) if vr is None else vr, self.va, **kw)

    def bwd_det(self, ops, ch, out, bg=True, va="given", **kw):
        return ops.rasterize_bwd_det_raw(self.m2d, self.con, self.feats(ch), self.opac, self.bg(ch) if bg else None, self.w,
                                         self.h, self.tw, self.th, self.tl, out[1], out[2], self.vr(ch),
                                         self.va if isinstance(va, str) else va, **kw)


@pytest.fixture(scope="module")
def ops():
    from robosimgs_amd import ops as _ops
    return _ops


@pytest.fixture(scope="module")
def inputs(ops):
    cache = {}

    def get(name):
        if name not in cache:
            cache[name] = _Inputs(ops, name)
        return cache[name]
    return get


def _same_bits(a, b, what):
    for x, y, name in zip(a, b, ("render", "alphas", "last_ids")):
        if x is not None and y is not None:
            assert torch.equal(x, y), f"{what}: {name} differs in {int((x != y).sum())} values"


def _gate(inp, ch, got, bg, ed=False, form=""):
    """got: (v_means2d, v_conics, v_feats, v_opacities, ...) of one backward form against the fp64 autograd of the same loss."""
    ref = inp.bref.grads(ch, inp.vr_np, inp.va_np, inp.bg_np if bg else None, ed)
    assert tuple(got[2].shape) == (inp.n, ch), tuple(got[2].shape)
    stats = {}
    for name, x, r in zip(GRAD_NAMES, got, ref):
        st = compare(f"{name} {form}", x, r, bad_frac=5e-3)
        stats[name] = st
        print(f"{inp.name} ch={ch} bg={bg} ed={ed} {form} {name}: {st['rows_over_tol']} of {st['rows']} rows over 2e-3, "
              f"cosine {st['cosine']:.7f}")
    return stats


@pytest.mark.parametrize("frame", list(FRAMES))
@pytest.mark.parametrize("ch", CHANNELS)
def test_forward_matches_fp64_oracle(ops, inputs, ch, frame):
    """Training and inference variant bit-identical; render, alpha and last_ids held to the fp64 blend with and without a
    background, and with the expected last channel (the epilogue's divide at a run-time last channel inside a wider bucket)."""
    inp = inputs(frame)
    alpha0 = None
    for bg in (True, False):
        for ed in (False, True):
            what = f"{frame} ch={ch} bg={bg} ed={ed}"
            train = inp.fwd(ops, ch, bg, expected_last=ed)
            infer = inp.fwd(ops, ch, bg, expected_last=ed, track_last=False)
            assert infer[2] is None
            _same_bits(train, infer, what + " inference vs training")
            if alpha0 is None:
                alpha0 = train[1:]
            _same_bits((None,) + tuple(alpha0), train, what + " alpha / last_ids across variants")
            check_forward(inp.ref, ch, train[0].cpu().numpy(), train[1].cpu().numpy(), train[2].cpu().numpy(),
                          inp.bg_np if bg else None, ed, what=what)
    assert inp.ref.contribs > 0 and float(alpha0[0].max()) > 0.999


@pytest.mark.parametrize("frame", list(FRAMES))
@pytest.mark.parametrize("ch", CHANNELS)
def test_latency_flag_changes_no_bit(ops, inputs, ch, frame):
    """MGS_RASTER_LATENCY: the per-block kernel exists up to 4 channels (test_raster_schedules_give_identical_bits feeds it
    3 and 4); above that the flag must be accepted and the per-tile kernel give the same bits."""
    inp = inputs(frame)
    for bg in (True, False):
        for kw in (dict(), dict(expected_last=True), dict(track_last=False)):
            a = inp.fwd(ops, ch, bg, latency=False, **kw)
            b = inp.fwd(ops, ch, bg, latency=True, **kw)
            _same_bits(a, b, f"{frame} ch={ch} bg={bg} {kw} latency")


@pytest.mark.parametrize("frame", list(FRAMES))
@pytest.mark.parametrize("ch", (1, 2) + WIDE)
def test_forward_checkpoints_change_no_bit_and_stay_inside_their_buffer(ops, inputs, ch, frame):
    """mgs_rasterize_fwd writes (1 + channels) * 256 floats per checkpoint unit at ANY channel count: frame bit-identical to
    the run without, and 0xA5 bytes in front of and behind the buffer untouched."""
    inp = inputs(frame)
    lens = inp.tl.tile_offsets[1:] - inp.tl.tile_offsets[:-1]
    assert int(lens.max()) > 3 * 64, int(lens.max())              # tiles of several segments
    n_ck = ops.checkpoint_buffer(inp.tl.capacity, inp.tw, inp.th, ch, 64, DEV).numel()
    big = torch.full((4 * (n_ck + 2 * GUARD_FLOATS),), CANARY, dtype=torch.uint8, device=DEV)
    ck = big.view(torch.float32)[GUARD_FLOATS:GUARD_FLOATS + n_ck]
    plain = inp.fwd(ops, ch)
    with_ck = inp.fwd(ops, ch, checkpoints=ck, checkpoint_interval=64)
    torch.cuda.synchronize()
    _same_bits(plain, with_ck, f"{frame} ch={ch} checkpoints")
    assert bool((big[:4 * GUARD_FLOATS] == CANARY).all()), "the forward wrote in front of its checkpoint buffer"
    assert bool((big[4 * (GUARD_FLOATS + n_ck):] == CANARY).all()), "the forward wrote past its checkpoint buffer"
    assert not bool((big[4 * GUARD_FLOATS:4 * (GUARD_FLOATS + n_ck)] == CANARY).all())      # ... and it did write checkpoints


@pytest.mark.parametrize("frame", list(FRAMES))
@pytest.mark.parametrize("ch", CHANNELS)
def test_backward_matches_fp64_autograd(ops, inputs, ch, frame):
    """Both backward forms against fp64 autograd of <v_render, frame> + <v_alphas, alpha>, with and without a background;
    absgrad; the det form bit-reproducible and v_alphas=None equal to an explicit zero frame."""
    inp = inputs(frame)
    for bg in (True, False):
        out = inp.fwd(ops, ch, bg)
        atomic = inp.bwd_atomic(ops, ch, out, bg, absgrad=True)
        det = inp.bwd_det(ops, ch, out, bg, absgrad=True)
        again = inp.bwd_det(ops, ch, out, bg, absgrad=True)
        for name, x, y in zip(GRAD_NAMES + ("v_means2d_abs",), det, again):
            assert torch.equal(x, y), f"{name}: two runs of the record backward differ"
        _gate(inp, ch, atomic, bg, form="atomic")
        _gate(inp, ch, det, bg, form="det")
        for form, got in (("atomic", atomic), ("det", det)):
            g2d, gabs = got[0], got[4]
            assert tuple(gabs.shape) == (inp.n, 2) and bool(torch.isfinite(gabs).all())
            # |sum| <= sum |.| up to rounding: the inequality of test_rasterize_absgrad
            assert bool((gabs * (1 + 2e-5) + 2e-6 >= g2d.abs()).all()), (form, float((g2d.abs() - gabs).max()))
        # the two forms: the same sums up to float re-association (test_deterministic_backward_many_channels' 1e-4)
        for name, x, y in zip(GRAD_NAMES + ("v_means2d_abs",), atomic, det):
            scale = float(x.abs().max()) + 1e-20
            assert float((x - y).abs().max()) / scale < 1e-4, (name, float((x - y).abs().max()) / scale)
    # include/mgs.h: v_alphas NULL = a zero cotangent on alpha
    none = inp.bwd_det(ops, ch, out, False, va=None)
    zero = inp.bwd_det(ops, ch, out, False, va=torch.zeros_like(inp.va))
    for name, x, y in zip(GRAD_NAMES, none, zero):
        assert torch.equal(x, y), f"{name}: v_alphas=None differs from a zero frame"


@pytest.mark.parametrize("frame", list(FRAMES))
@pytest.mark.parametrize("ch", [1, 2, 5, 32])
@pytest.mark.parametrize("bg", [True, False])
def test_backward_through_the_expected_last_channel(ops, inputs, bg, ch, frame):
    """Forward with MGS_RASTER_EXPECTED_LAST, the record backward handed its frame as expected_render: gradients of
    <v_render, frame> + <v_alphas, alpha> where frame[..., -1] = sum / clamp(alpha, 1e-10)."""
    inp = inputs(frame)
    out = inp.fwd(ops, ch, bg, expected_last=True)
    det = inp.bwd_det(ops, ch, out, bg, expected_render=out[0])
    again = inp.bwd_det(ops, ch, out, bg, expected_render=out[0])
    for name, x, y in zip(GRAD_NAMES, det, again):
        assert torch.equal(x, y), name
    _gate(inp, ch, det, bg, ed=True, form="det expected_render")


@pytest.mark.parametrize("frame", list(FRAMES))
@pytest.mark.parametrize("ch", (1, 2) + WIDE)
def test_backward_with_checkpoints(ops, inputs, ch, frame):
    """Checkpoints + render_out handed to the record backward.  Up to 4 channels the segmented walk runs: other bits than
    the whole-list walk, held to the fp64 oracle like it.  Above 4 channels the host falls back to the whole-list walk
    (workspace still sized for segments): bit-identical gradients.  0xA5 bytes behind the workspace survive either way."""
    inp = inputs(frame)
    ck = ops.checkpoint_buffer(inp.tl.capacity, inp.tw, inp.th, ch, 64, DEV)
    plain = inp.fwd(ops, ch)
    out = inp.fwd(ops, ch, checkpoints=ck, checkpoint_interval=64)
    _same_bits(plain, out, f"{frame} ch={ch} checkpoints")
    whole = inp.bwd_det(ops, ch, plain, absgrad=True)
    seg = inp.bwd_det(ops, ch, out, absgrad=True, render_out=out[0], checkpoints=ck, checkpoint_interval=64,
                      canary_bytes=1 << 20)
    torch.cuda.synchronize()
    assert bool((seg[5] == CANARY).all()), "the backward wrote past its workspace"
    if ch > 4:
        for name, x, y in zip(GRAD_NAMES + ("v_means2d_abs",), whole, seg):
            assert torch.equal(x, y), f"{name}: checkpoints changed the whole-list walk's bits at {ch} channels"
    else:
        assert any(not torch.equal(x, y) for x, y in zip(whole[:4], seg[:4])), "the segmented walk did not run"
        _gate(inp, ch, seg, True, form="det segmented")
