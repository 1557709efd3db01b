"""The batch phase of the one-wave-per-tile forward raster (robosimgs_amd/csrc/raster_fwd.hip): the cull over the
eight edge lines of a tile's four quadrants, the quadrant masks of a batch as lane masks in SGPRs, and the walk of the
queued entries four per trip.  None of it may change a bit of a frame:

  * with and without the cull, and in both schedules, the same bits (3, 4 and 7 channels, frames whose edges are no
    multiples of 16);
  * one tile holding exactly 1, 3, 4, 5, 63, 64, 65 and 129 Gaussians -- the unrolled walk's remainders and the batch
    edges -- against the fp64 oracle;
  * a quadrant that closes in the middle of a batch whose later entries still reach it and its neighbours, with the
    hand-written body and, through a needle-like conic and an opacity above 0.998 in the batch, the generic one;
  * the backward, which shares the cull: whole-list and segmented gradients repeat bit for bit and stay within the
    row tolerance of the fp64 autograd oracle.
"""
import math

import numpy as np
import pytest
import torch

from oracle import gs_oracle_np as O
from robosimgs_amd import camera_ring, synthetic_scene

pytestmark = pytest.mark.gpu

DEV = "cuda"
FRAMES = [(96, 80, 3000, 0.15), (333, 207, 4000, 0.1)]


def _t(a, dtype=torch.float32):
    return torch.from_numpy(np.ascontiguousarray(a)).to(dtype).to(DEV)


@pytest.fixture(scope="module")
def ops():
    from robosimgs_amd import ops as _ops
    return _ops


@pytest.fixture(scope="module")
def listed(ops):
    """Projected Gaussians and tile lists of the two frames, made once: {(w, h): dict}."""
    out = {}
    for w, h, n, mu in FRAMES:
        g = synthetic_scene(n, math.log(mu), 0, 3)
        rng = np.random.default_rng(4)
        g.log_scales[::5, 0] += math.log(30.0)                       # needles among them
        g.opacity_logits[::7] = rng.uniform(-6.5, -5.0, size=len(g.opacity_logits[::7]))   # around 1/255
        cam = camera_ring(1, w, h, thetas=[0.3])[0]
        t = g.to_torch(DEV, 0)
        radii, m2d, dep, con, _, _ = ops.project_color_fwd_raw(t["means"], t["quats"], t["scales"], t["opacities"], 0,
                                                               t["colors"], _t(cam.viewmat()), _t(cam.K), w, h, 0.3, 0.01,
                                                               1e10, 0.0, False, True)
        tw, th = -(-w // 16), -(-h // 16)
        tl = ops.isect_tiles_raw(m2d, radii, dep, tw, th, ops._upper_bound_isects(radii, tw, th) + 1)
        feats = torch.rand(n, 7, device=DEV, generator=torch.Generator(DEV).manual_seed(9))
        out[(w, h)] = dict(m2d=m2d, con=con, op=t["opacities"], feats=feats, tl=tl, tw=tw, th=th)
    return out


@pytest.mark.parametrize("w,h", [f[:2] for f in FRAMES])
@pytest.mark.parametrize("ch", [3, 4, 7])
def test_cull_and_schedule_change_no_bit(ops, listed, w, h, ch):
    from robosimgs_amd import _lib
    s = listed[(w, h)]
    feats = s["feats"][:, :ch].contiguous()
    bg = torch.linspace(0.1, 0.7, ch, device=DEV)

    def frame(**kw):
        return ops.rasterize_fwd_raw(s["m2d"], s["con"], feats, s["op"], bg, w, h, s["tw"], s["th"], s["tl"].tile_offsets,
                                     s["tl"].flatten_ids, **kw)

    shipped = {lat: frame(latency=lat) for lat in (False, True)}
    inference = frame(track_last=False)
    assert float(shipped[False][1].max()) > 0.5
    with _lib.use_debug_lib() as dbg:
        try:
            for lat in (False, True):
                dbg.mgs_debug_set_raster_cull(1)
                on = frame(latency=lat)
                dbg.mgs_debug_set_raster_cull(0)
                off = frame(latency=lat)
                for x, y, z, name in zip(on, off, shipped[lat], ("render", "alphas", "last_ids")):
                    assert torch.equal(x, y), f"{name}: the cull changed {int((x != y).sum())} values (latency={lat})"
                    assert torch.equal(x, z), f"{name}: debug and shipped builds differ (latency={lat})"
        finally:
            dbg.mgs_debug_set_raster_cull(1)
    for x, y, name in zip(shipped[False], shipped[True], ("render", "alphas", "last_ids")):
        assert torch.equal(x, y), f"{name}: per-tile and per-block schedules differ"
    assert torch.equal(inference[0], shipped[False][0]) and torch.equal(inference[1], shipped[False][1])


def _one_tile(ops, w, h, tile, mean, conic, opac, feats, bg=None, **kw):
    """A frame whose only list is `tile`'s: every Gaussian given, in the order given.  Returns the raw outputs and the
    arguments the oracle needs."""
    tw, th = -(-w // 16), -(-h // 16)
    n = len(mean)
    offsets = np.zeros(tw * th + 1, np.int32)
    offsets[tile + 1:] = n
    args = dict(m2d=_t(mean), con=_t(conic), feats=_t(feats), op=_t(opac), offs=_t(offsets, torch.int32),
                ids=_t(np.arange(n, dtype=np.int32), torch.int32), tw=tw, th=th, w=w, h=h, bg=bg)
    return args


def _render(ops, a, **kw):
    return ops.rasterize_fwd_raw(a["m2d"], a["con"], a["feats"], a["op"], a["bg"], a["w"], a["h"], a["tw"], a["th"], a["offs"],
                                 a["ids"], **kw)


def _check_against_oracle(a, out, what):
    bg = None if a["bg"] is None else a["bg"].cpu().numpy()
    feats = a["feats"].cpu().numpy()
    ref_img, ref_alpha, ref_last, stats = O.rasterize(
        a["m2d"].cpu().numpy(), a["con"].cpu().numpy(), feats, a["op"].cpu().numpy(), a["ids"].cpu().numpy(),
        a["offs"][:-1].cpu().numpy().reshape(a["th"], a["tw"]), a["w"], a["h"], 16, background=bg, margins=True,
        flip_eps=O.EPS_STAGE)
    fmax = np.abs(feats).max(0) if bg is None else np.maximum(np.abs(feats).max(0), np.abs(bg))
    O.check_frame(out[0].cpu().numpy(), out[1].cpu().numpy(), ref_img, ref_alpha, stats["margins"], O.EPS_STAGE, what=what,
                  flip_weight=stats["flip_weight"], feat_max=fmax, require_flip_bound=True, max_explained=1.0)
    return ref_last


@pytest.mark.parametrize("count", [1, 3, 4, 5, 63, 64, 65, 129])
def test_walk_boundaries_one_tile(ops, count):
    """One tile of a 96x80 frame holds exactly `count` faint Gaussians strewn over and around it: none closes a pixel, so
    every queued entry is walked; the cull takes some quadrants off most of them."""
    w, h, tile = 96, 80, 2 * 6 + 3
    rng = np.random.default_rng(100 + count)
    mean = np.stack([16.0 * 3 + rng.uniform(-4.0, 20.0, count), 16.0 * 2 + rng.uniform(-4.0, 20.0, count)], 1)
    sig = rng.uniform(1.0, 4.0, count)
    conic = np.stack([1.0 / sig ** 2, rng.uniform(-0.3, 0.3, count) / sig ** 2, 1.0 / sig ** 2], 1)
    a = _one_tile(ops, w, h, tile, mean, conic, rng.uniform(0.02, 0.2, count), rng.random((count, 4)))
    out = _render(ops, a, expected_last=False)
    _check_against_oracle(a, out, f"one tile of {count}")
    assert float(out[1].max()) > 0.01 and float(out[1].max()) < 0.9999
    inf = _render(ops, a, track_last=False)
    blk = _render(ops, a, latency=True)
    assert torch.equal(inf[0], out[0]) and torch.equal(inf[1], out[1])
    assert all(torch.equal(x, y) for x, y in zip(out, blk))
    inside = torch.zeros(h, w, dtype=torch.bool, device=DEV)
    inside[32:48, 48:64] = True
    assert float(out[1][~inside].abs().max()) == 0.0                 # no other tile has a list


@pytest.mark.parametrize("ch", [3, 4])
@pytest.mark.parametrize("unsafe", [False, True])
def test_quadrant_closing_inside_a_batch(ops, ch, unsafe):
    """An opaque stack over quadrant 0 closes all 64 of its pixels within the first 32 entries of a 64-entry batch; the
    rest of the batch keeps reaching that quadrant and its neighbours.  unsafe: entry 5 is a needle-like conic and
    entry 7 has an opacity above 0.998, so the batch is walked by the generic body, on the same masks."""
    from robosimgs_amd import _lib
    w, h, tile = 96, 80, 1 * 6 + 2
    x0, y0 = 32.0, 16.0
    rng = np.random.default_rng(5 + ch)
    n = 100
    mean = np.stack([x0 + rng.uniform(2.0, 14.0, n), y0 + rng.uniform(2.0, 14.0, n)], 1)
    sig = rng.uniform(2.0, 5.0, n)
    conic = np.stack([1.0 / sig ** 2, np.zeros(n), 1.0 / sig ** 2], 1)
    opac = rng.uniform(0.05, 0.3, n)
    # the stack: nearly opaque, centred on quadrant 0 -- alpha >= 0.3 on all of it (0.7^32 < 1e-4), about 0.01 at the
    # middle of the far quadrant and below 1/255 at its far corner
    mean[:32] = [x0 + 4.0, y0 + 4.0] + rng.uniform(-0.5, 0.5, (32, 2))
    conic[:32] = [0.06, 0.0, 0.06]
    opac[:32] = 0.9
    if unsafe:
        conic[5] = [3.0, 0.0, 1e-4]
        opac[7] = 0.9995
    bg = torch.linspace(0.2, 0.5, ch, device=DEV)
    a = _one_tile(ops, w, h, tile, mean, conic, opac, rng.random((n, ch)), bg=bg)
    out = _render(ops, a)
    ref_last = _check_against_oracle(a, out, f"closing quadrant ch={ch} unsafe={unsafe}")
    last = out[2].cpu().numpy()
    q0 = last[16:24, 32:40]
    # quadrant 0 closed inside the first batch: entries 32..99 reach it too, and none of them is the last one blended
    assert q0.max() < 40
    assert last[28:32, 44:48].min() > 64                                     # the far quadrant's far block is still open in the second batch
    assert (last == ref_last).mean() > 0.999
    with _lib.use_debug_lib() as dbg:
        try:
            dbg.mgs_debug_set_raster_cull(0)
            off = _render(ops, a)
        finally:
            dbg.mgs_debug_set_raster_cull(1)
    blk, inf = _render(ops, a, latency=True), _render(ops, a, track_last=False)
    for x, y, z in zip(out, off, blk):
        assert torch.equal(x, y) and torch.equal(x, z)
    assert torch.equal(inf[0], out[0]) and torch.equal(inf[1], out[1])


def test_backward_shares_the_cull():
    """96x80, lists of a few hundred entries: the whole-list walk and the 64-entry segments each give the same bits when
    the call is repeated, and the blend's four gradients stay within the row tolerance of the fp64 autograd oracle."""
    from grad_gate import compare, oracle_budgets
    from robosimgs_amd import rasterization
    w, h, deg, mode = 96, 80, 1, "RGB+ED"
    g = synthetic_scene(5000, math.log(0.07), deg, 0)
    cam = camera_ring(1, w, h, thetas=[0.3])[0]
    t = g.to_torch(DEV, deg)
    vm, K = _t(cam.viewmat()[None]), _t(cam.K[None])
    names = ("means", "quats", "scales", "opacities", "colors")
    rng = np.random.default_rng(2)
    wr, wa = rng.normal(size=(h, w, 4)), rng.normal(size=(h, w))

    def run(segment):
        p = {k: t[k].detach().clone().requires_grad_(True) for k in names}
        c, al, meta = rasterization(p["means"], p["quats"], p["scales"], p["opacities"], p["colors"], vm, K, w, h,
                                    sh_degree=deg, render_mode=mode, backward_segment=segment)
        ((c[0] * _t(wr)).sum() + (al[0, ..., 0] * _t(wa)).sum()).backward()
        return [p[k].grad for k in names], meta

    f32 = lambda m: np.asarray(m, dtype=np.float32)
    info = oracle_budgets(g, f32(cam.viewmat()), f32(cam.K), w, h, deg, mode, wr, wa, O.EPS_PATH_GRAD)
    for segment in (0, 64):
        g1, meta = run(segment)
        g2, _ = run(segment)
        lens = meta["tile_lists"][0].tile_offsets[1:] - meta["tile_lists"][0].tile_offsets[:-1]
        assert int(lens.max()) > 128
        for k, x, y in zip(names, g1, g2):
            assert torch.equal(x, y), (segment, k)
        bg = meta["blend_grads"][0]
        for name, got, ref, b in (("means2d", bg[0], info["g_means2d"], info["budget"][:, 0]),
                                  ("conics", bg[1], info["g_conics"], info["budget"][:, 1]),
                                  ("feats", bg[2], info["g_feats"], info["budget"][:, 2]),
                                  ("opacities", bg[3], info["g_opacities"].reshape(-1, 1), info["budget"][:, 3])):
            compare(f"segment {segment}: blend v_{name}", got, ref, row_tol=5e-3, bad_frac=1e-2, cos_min=0.999, budget=b)
