"""The scalar side of the hand-written blend body (robosimgs_amd/csrc/raster_fwd.hip: MGS_SAFE_BODY): EXEC set from
`alive` and restored once per queue entry, the closing lanes as vcc & ~exec, `quad` emptied by one s_cselect on the SCC
of the `alive` update.  The cases are the ones those instructions can get wrong:

  1. lanes outside the image: frames of 20x12 and 17x9, the tile whose quadrants lie partly or wholly outside, opaque
     Gaussians centred outside the image so that their exponent is largest on the dead lanes;
  2. a Gaussian that counts for closed pixels only (its body runs with vcc = 0) while its quadrant stays open;
  3. quadrant 0's last pixel closes at entry 10 of batch 0 and quadrant 3's at entry 40 of batch 1 while quadrants 1
     and 2 stay open to the end -- with every batch safe, and with batch 1 walked by the generic body (a needle conic
     with opacity 0.9995 in it);
  4. the whole tile closes inside the first batch: nothing after the closing entry changes a pixel or a last_id.

Every case runs for 3 and 4 channels, as inference and with track_last, and asserts: the per-tile render equals the
per-block one bit for bit; the shipped library equals the debug library with the cull off; the fp64 oracle's
check_frame on the per-tile render.  The helpers follow tests/test_gpu_raster_batch.py.
"""
import numpy as np
import pytest
import torch

from oracle import gs_oracle_np as O

pytestmark = pytest.mark.gpu

DEV = "cuda"
QUADS = [(slice(0, 8), slice(0, 8)), (slice(0, 8), slice(8, 16)), (slice(8, 16), slice(0, 8)), (slice(8, 16), slice(8, 16))]
VARIANTS = [(3, False), (3, True), (4, False), (4, True)]


def _t(a, dtype=torch.float32):
    return torch.from_numpy(np.ascontiguousarray(a)).to(dtype).to(DEV)


@pytest.fixture(scope="module")
def ops():
    from robosimgs_amd import ops as _ops
    return _ops


def _one_tile(w, h, tile, mean, conic, opac, feats, bg=None):
    """A frame whose only list is `tile`'s: every Gaussian given, in the order given."""
    tw, th = -(-w // 16), -(-h // 16)
    n = len(mean)
    offsets = np.zeros(tw * th + 1, np.int32)
    offsets[tile + 1:] = n
    return dict(m2d=_t(mean), con=_t(conic), feats=_t(feats), op=_t(opac), offs=_t(offsets, torch.int32),
                ids=_t(np.arange(n, dtype=np.int32), torch.int32), tw=tw, th=th, w=w, h=h, bg=bg)


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


def _render_and_check(ops, a, track, what):
    """The three assertions of every case; returns the per-tile outputs (last_ids None for an inference render)."""
    from robosimgs_amd import _lib
    out = _render(ops, a, track_last=track)
    blk = _render(ops, a, track_last=track, latency=True)
    with _lib.use_debug_lib() as dbg:
        try:
            dbg.mgs_debug_set_raster_cull(0)
            off = {lat: _render(ops, a, track_last=track, latency=lat) for lat in (False, True)}
        finally:
            dbg.mgs_debug_set_raster_cull(1)
    names = ("render", "alphas", "last_ids") if track else ("render", "alphas")
    for i, name in enumerate(names):
        assert torch.equal(out[i], blk[i]), f"{what}: {name}: per-tile and per-block schedules differ"
        assert torch.equal(out[i], off[False][i]), f"{what}: {name}: per-tile, shipped against debug build with the cull off"
        assert torch.equal(blk[i], off[True][i]), f"{what}: {name}: per-block, shipped against debug build with the cull off"
    ref_last = _check_against_oracle(a, out, what)
    assert bool(torch.isfinite(out[0]).all()) and bool(torch.isfinite(out[1]).all()), f"{what}: NaN or inf in the frame"
    return out, ref_last


def _feats(rng, n, ch):
    return rng.random((n, ch))


def _bg(ch):
    return torch.linspace(0.2, 0.5, ch, device=DEV)


# ---- 1. lanes outside the image --------------------------------------------------------------------------------------

@pytest.mark.parametrize("ch,track", VARIANTS)
@pytest.mark.parametrize("w,h", [(20, 12), (17, 9)])
def test_lanes_outside_the_image(ops, w, h, ch, track):
    """Tile 1 of a two-tile frame: quadrant 0 and 2 have columns (and rows) outside the image, quadrants 1 and 3 lie
    outside altogether.  24 Gaussians of opacity 0.99 centred right of and below the image: alpha is largest on lanes
    that have no pixel."""
    rng = np.random.default_rng(10 * w + h)
    n = 24
    mean = np.stack([rng.uniform(w + 1.0, 31.0, n), rng.uniform(h - 2.0, 15.0, n)], 1)
    sig = rng.uniform(3.0, 7.0, n)
    conic = np.stack([1.0 / sig ** 2, rng.uniform(-0.2, 0.2, n) / sig ** 2, 1.0 / sig ** 2], 1)
    a = _one_tile(w, h, 1, mean, conic, np.full(n, 0.99), _feats(rng, n, ch), bg=_bg(ch))
    out, _ = _render_and_check(ops, a, track, f"{w}x{h} ch={ch} track={track}")
    alphas = out[1].cpu().numpy()
    assert alphas[:, 16:].max() > 0.5                                  # the Gaussians do reach the pixels that exist
    assert alphas[:, :16].max() == 0.0                                 # tile 0 has no list


# ---- 2. a Gaussian no open pixel counts for --------------------------------------------------------------------------

SMALL = 40                      # the list index of the late, small Gaussian


def _scene_closed_under_small(ch):
    rng = np.random.default_rng(20 + ch)
    n = 70
    mean = np.stack([rng.uniform(0.0, 16.0, n), rng.uniform(0.0, 16.0, n)], 1)
    sig = rng.uniform(2.0, 4.0, n)
    conic = np.stack([1.0 / sig ** 2, np.zeros(n), 1.0 / sig ** 2], 1)
    opac = rng.uniform(0.01, 0.04, n)
    # eight opaque splats close the four pixels around (4, 4): alpha >= 0.95 exp(-0.5 * 0.16 * 0.5) = 0.91 there,
    # 0.95 exp(-0.08 * 24.5) = 0.13 at the quadrant's corners, which stay open
    mean[:8] = [4.0, 4.0]
    conic[:8] = [0.16, 0.0, 0.16]
    opac[:8] = 0.95
    # the small one: sigma = 0.52, opacity 0.3 -- alpha >= 1/255 within r^2 <= 2.35, i.e. on those four pixels only
    # (the next ring of pixel centres is at r^2 = 2.5)
    mean[SMALL] = [4.0, 4.0]
    conic[SMALL] = [1.0 / 0.52 ** 2, 0.0, 1.0 / 0.52 ** 2]
    opac[SMALL] = 0.3
    return mean, conic, opac, _feats(rng, n, ch)


@pytest.mark.parametrize("ch,track", VARIANTS)
def test_gaussian_no_open_pixel_counts_for(ops, ch, track):
    mean, conic, opac, feats = _scene_closed_under_small(ch)
    # what the scene is built for, from the numbers themselves: the small Gaussian counts exactly on the four pixels
    ys, xs = np.mgrid[0:16, 0:16] + 0.5
    r2 = (xs - 4.0) ** 2 + (ys - 4.0) ** 2
    counted = opac[SMALL] * np.exp(-0.5 * conic[SMALL, 0] * r2) >= 1.0 / 255.0
    assert counted.sum() == 4 and counted[3:5, 3:5].all()
    a = _one_tile(16, 16, 0, mean, conic, opac, feats, bg=_bg(ch))
    out, ref_last = _render_and_check(ops, a, track, f"closed under a small Gaussian ch={ch} track={track}")
    with_small = out
    # the image must not move: the same list with the small Gaussian's opacity at zero gives the same bits
    opac0 = opac.copy()
    opac0[SMALL] = 0.0
    b = _one_tile(16, 16, 0, mean, conic, opac0, feats, bg=_bg(ch))
    without = _render(ops, b, track_last=track)
    assert torch.equal(with_small[0], without[0]) and torch.equal(with_small[1], without[1])
    if track:
        last = out[2].cpu().numpy()
        assert torch.equal(with_small[2], without[2])
        assert (last[counted] < 8).all()                               # closed by the opaque splats, before the small one
        assert (last != SMALL).all()
        q0 = last[QUADS[0]]
        assert (q0 > SMALL).sum() >= 32                                # later entries of the batch still reach the quadrant
        assert (last == ref_last).mean() > 0.99


# ---- 3. a quadrant's last pixel closes mid-batch, then another one's in the next batch ----------------------------------

def _scene_two_closings(ch, unsafe):
    rng = np.random.default_rng(11)
    n = 130
    mean = np.stack([rng.uniform(0.0, 16.0, n), rng.uniform(0.0, 16.0, n)], 1)
    sig = rng.uniform(2.0, 4.0, n)
    conic = np.stack([1.0 / sig ** 2, np.zeros(n), 1.0 / sig ** 2], 1)
    opac = rng.uniform(0.01, 0.03, n)
    # ten splats of opacity 0.9 over a quadrant leave T = 0.45^10 = 3.4e-4 at its four corners (alpha = 0.9 exp(-0.02 * 24.5)
    # = 0.55 there; every other pixel of the quadrant closes earlier); the eleventh, opacity 0.99 and nearly flat, takes
    # T (1 - alpha) to 2e-5 there: the quadrant's last pixels close at that entry
    for first, centre in ((0, 4.0), (94, 12.0)):
        mean[first:first + 11] = [centre, centre]
        conic[first:first + 10] = [0.04, 0.0, 0.04]
        opac[first:first + 10] = 0.9
        conic[first + 10] = [0.004, 0.0, 0.004]
        opac[first + 10] = 0.99
    if unsafe:
        # batch 1 goes through the generic body: a needle right of the tile (it counts, faintly, for the last column)
        mean[70] = [17.0, 8.0]
        conic[70] = [3.0, 0.0, 1e-4]
        opac[70] = 0.9995
    return mean, conic, opac, _feats(rng, n, ch)


@pytest.mark.parametrize("ch,track", VARIANTS)
@pytest.mark.parametrize("unsafe", [False, True])
def test_two_quadrants_close_in_two_batches(ops, ch, track, unsafe):
    mean, conic, opac, feats = _scene_two_closings(ch, unsafe)
    a = _one_tile(16, 16, 0, mean, conic, opac, feats, bg=_bg(ch))
    out, ref_last = _render_and_check(ops, a, track, f"two closings ch={ch} track={track} unsafe={unsafe}")
    ref = np.asarray(ref_last)
    # the oracle's own last ids say what the scene is built for (whatever the render under test does)
    assert ref[QUADS[0]].max() == 9 and (ref[QUADS[0]] == 9).sum() == 4        # quadrant 0: the corners close at entry 10
    assert ref[QUADS[3]].max() == 103 and ref[QUADS[3]].min() >= 10           # quadrant 3: its last pixel closes at 64 + 40
    assert (ref[QUADS[1]] > 104).sum() >= 8 and (ref[QUADS[2]] > 104).sum() >= 8   # quadrants 1 and 2 are open to the end
    if track:
        last = out[2].cpu().numpy()
        assert last[QUADS[0]].max() == 9 and last[QUADS[3]].max() == 103
        assert (last[QUADS[1]] > 104).sum() >= 8 and (last[QUADS[2]] > 104).sum() >= 8
        assert (last == ref).mean() > 0.99
    alphas = out[1].cpu().numpy()
    assert alphas[QUADS[0]].min() > 0.98 and alphas[QUADS[3]].min() > 0.98        # (a closing pixel keeps the T it had)


# ---- 4. the whole tile closes inside a batch -------------------------------------------------------------------------

@pytest.mark.parametrize("ch,track", VARIANTS)
def test_whole_tile_closes_inside_a_batch(ops, ch, track):
    """64 opaque Gaussians over the whole tile (alpha >= 0.9 exp(-0.001 * 112.5) = 0.8 everywhere: every pixel is closed
    by the seventh), then 64 more of the same kind."""
    rng = np.random.default_rng(40 + ch)
    n = 128
    mean = 8.0 + rng.uniform(-0.5, 0.5, (n, 2))
    conic = np.tile([0.002, 0.0, 0.002], (n, 1))
    opac = rng.uniform(0.9, 0.95, n)
    feats = _feats(rng, n, ch)
    a = _one_tile(16, 16, 0, mean, conic, opac, feats, bg=_bg(ch))
    out, ref_last = _render_and_check(ops, a, track, f"whole tile closes ch={ch} track={track}")
    # nothing after the closing entry changes a pixel: the first eight entries alone give the same bits
    b = _one_tile(16, 16, 0, mean[:8], conic[:8], opac[:8], feats[:8], bg=_bg(ch))
    head = _render(ops, b, track_last=track)
    assert torch.equal(out[0], head[0]) and torch.equal(out[1], head[1])
    assert float(out[1].min()) > 0.99                                  # (a closing pixel keeps the T it had)
    if track:
        assert torch.equal(out[2], head[2])
        assert int(out[2].max()) < 7
        assert (out[2].cpu().numpy() == ref_last).mean() > 0.99
