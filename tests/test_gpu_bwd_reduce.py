"""The REDUCE half of mgs_rasterize_bwd_det held to fp64 on its own (tests/bwd_reduce_ref.py): every case bins hand-placed
Gaussians (mgs_isect_tiles with pair_info), renders them (mgs_rasterize_fwd with last_ids) and makes ONE backward call into
a workspace pre-filled with 0xFF bytes (every unwritten record is NaN) and outputs pre-filled with NaN.  The GPU's own
records and flags, read back out of that workspace, are the reference's input: every row of every output must lie inside
the derived rounding bound of their fp64 sum -- no row excused -- rows with no counted slot must be exact zeros, every
output element finite, and every flagged slot one of the lists' (tile, Gaussian) pairs at an index the tile's walk reaches.
The figures are printed before they are asserted (pytest -s); profiles/bwd_reduce/README.md keeps the measured ones."""
import numpy as np
import pytest
import torch

import bwd_reduce_ref as R

pytestmark = pytest.mark.gpu
DEV = "cuda"
CASES = {c[0]: c for c in R.gpu_cases()}
NAMES = ("v_means2d", "v_conics", "v_feats", "v_opacities", "v_means2d_abs")


def _t(a, dtype=np.float32):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=dtype)).to(DEV)


class _Frame:
    """A case on the device: binned and rendered once (the lists, alphas and last_ids are shared by its backward calls)."""

    def __init__(self, ops, case, ch, cap, interval=0, annotate=False):
        self.case, self.ch, self.cap, self.interval = case, ch, cap, interval
        self.tw, self.th, self.w, self.h = case.tile_w, case.tile_h, case.width, case.height
        self.m2d, self.con, self.opac = _t(case.means2d), _t(case.conics), _t(case.opacities)
        self.feats = _t(case.feats[:, :ch])
        self.splats = _t(case.splats(ch)) if ch <= 4 else None
        self.tl = ops.isect_tiles_raw(self.m2d, _t(case.radii, np.int32), _t(case.depths), self.tw, self.th, cap,
                                      want_pair_info=True, splats=self.splats if annotate else None)
        self.overflowed = int(self.tl.status.item()) != 0
        assert int(self.tl.n_isect.item()) == case.n_isect()
        self.pair_info = self.tl.pair_info.cpu().numpy()
        want = case.pair_info().astype(np.int64)
        got = self.pair_info.astype(np.int64)
        some = (want[:, 3] & 0xffff) * (want[:, 3] >> 16) > 0
        assert np.array_equal(got[some], want[some]), "the binning lists other rectangles than the case designed"
        assert ((got[~some, 3] & 0xffff) * (got[~some, 3] >> 16) == 0).all()
        self.ck = ops.checkpoint_buffer(cap, self.tw, self.th, ch, interval, DEV) if interval else None
        self.render, self.alphas, self.last = ops.rasterize_fwd_raw(
            self.m2d, self.con, self.feats, self.opac, None, self.w, self.h, self.tw, self.th, self.tl.tile_offsets,
            self.tl.flatten_ids, checkpoints=self.ck, checkpoint_interval=interval)
        vr, va = case.cotangents(ch)
        self.vr, self.va = _t(vr), _t(va)
        off = self.tl.tile_offsets.cpu().numpy().astype(np.int64)
        self.offsets = np.minimum(off, cap)                  # (a cut list ends at the capacity)
        self.flatten = self.tl.flatten_ids.cpu().numpy()
        self.last_np = self.last.cpu().numpy()

    def backward(self, ops, absgrad, source="arrays", segmented=False, canary=0, tl=None, splats=None):
        """One call: 0xFF workspace, NaN outputs.  Returns dict of numpy arrays (outputs, records, flags, tables)."""
        n, ch, iv = self.case.n, self.ch, self.interval if segmented else 0
        need = ops.rasterize_bwd_det_workspace_bytes(ch, absgrad, self.cap, self.tw, self.th, iv)
        ws = torch.full((need + 256 + canary,), 0xFF, dtype=torch.uint8, device=DEV)
        out = tuple(torch.full(s, float("nan"), device=DEV) for s in ((n, 2), (n, 3), (n, ch), (n,))) + \
            ((torch.full((n, 2), float("nan"), device=DEV),) if absgrad else (None,))
        kw = dict(render_out=self.render, checkpoints=self.ck, checkpoint_interval=iv) if segmented else {}
        use_splats = splats if splats is not None else (self.splats if source == "splats" else None)
        res = ops.rasterize_bwd_det_raw(self.m2d, self.con, self.feats, self.opac, None, self.w, self.h, self.tw, self.th,
                                        tl or self.tl, self.alphas, self.last, self.vr, self.va, absgrad=absgrad,
                                        splats=use_splats, canary_bytes=canary, out=out, workspace=ws, **kw)
        torch.cuda.synchronize()
        assert all(a is b for a, b in zip(res[:5], out)), "out= buffers are returned as they are"
        v = ops.rasterize_bwd_det_workspace_views(ws, ch, absgrad, self.cap, self.tw, self.th, iv)
        got = {k: v[k].cpu().numpy() for k in v}
        got.update({name: o.cpu().numpy() for name, o in zip(NAMES, out) if o is not None})
        if canary:
            got["canary"] = res[5].cpu().numpy()
        got["absgrad"] = absgrad
        return got

    def check(self, got, label):
        """The four assertions of the module docstring on one call's results; prints the figures first."""
        absgrad, case = got["absgrad"], self.case
        ref = R.reduce_f64(self.pair_info, got["records"], got["flags"], self.cap, case.means2d, case.conics, case.opacities,
                           self.ch, absgrad)
        worst, bad = R.compare(got, ref)
        kinds = R.slot_kinds(self.pair_info, got["flags"], self.cap)
        print(f"\n[bwd_reduce] {label}: n={case.n} slots flagged/unflagged/non-existent={kinds} "
              f"rows with counted slots={int((ref['counted'] > 0).sum())} worst error/bound: " +
              " ".join(f"{k}={x:.3f}" for k, x in worst.items()))
        for name in NAMES:
            if name in got:
                assert np.isfinite(got[name]).all(), f"{label}: {name} has rows no path wrote (or summed a poisoned record)"
        assert not bad, f"{label}: rows outside the bound (output, row): {bad}"
        dead = ref["counted"] == 0
        for name in NAMES:
            if name in got:
                assert (got[name][dead] == 0).all(), f"{label}: {name} is not exactly zero where nothing counted"
        flagged = np.nonzero(got["flags"])[0]
        allowed = R.allowed_slots(self.pair_info, self.offsets, self.flatten, self.last_np, self.tw, self.th)
        assert np.isin(flagged, allowed).all(), f"{label}: a flagged slot is no pair of the lists within the tile's walk"
        # not degenerate: a real share of the slots that exist is flagged, and a real share is not (an overflowed binning
        # keeps only `capacity` of the list entries, so the shares are of the existing slots, not of the rectangles')
        exist = kinds[0] + kinds[1]
        assert kinds[0] >= 0.05 * exist and kinds[1] >= 0.05 * exist, f"{label}: degenerate case {kinds}"
        return worst


@pytest.fixture(scope="module")
def ops():
    from robosimgs_amd import ops as _ops
    return _ops


def _frame(ops, name, **kw):
    _, builder, args, ch, absgrad, cap_index, interval = CASES[name]
    case = R.built(builder, *args)
    return _Frame(ops, case, ch, R.capacity_of(case, cap_index), interval, **kw), absgrad


PLAIN = [n for n, c in CASES.items() if c[5] is None and not c[6]]


@pytest.mark.parametrize("name", PLAIN)
def test_reduce_against_fp64_on_its_own_records(ops, name):
    """Rectangle geometry (widths 1..9 x slot bases mod 4, empty rectangles between), the Gaussian counts around the run
    and wave edges, the row rounds, the big rectangles (255 / 256 / 257 / 272 / 289 tiles, more than 64 rows, more than
    4096 of them), channels 1..4 on the rows kernel and 5..32 on the per-Gaussian one with and without absgrad, opacity
    exactly 0."""
    f, absgrad = _frame(ops, name)
    assert not f.overflowed
    f.check(f.backward(ops, absgrad), name)


def test_zero_opacity_rows_are_zero(ops):
    f, _ = _frame(ops, "zero_opacity-c3")
    got = f.backward(ops, False)
    zero = f.case.opacities == 0
    assert zero.sum() == 4
    for name in ("v_means2d", "v_conics", "v_feats", "v_opacities"):
        assert (got[name][zero] == 0).all(), name


@pytest.mark.parametrize("ch", [1, 2, 3, 4])
@pytest.mark.parametrize("absgrad", [False, True])
def test_arrays_and_splat_records_and_splat_slots_give_the_same_bits(ops, ch, absgrad):
    """The source of mean, conic and opacity (arrays or the packed splat records) and the source of the record slot
    (pair_info or the records' annotation, MGS_RASTER_BWD_SPLAT_SLOTS) change no bit of the outputs or the flags."""
    case = R.built(R.case_channels)
    f = _Frame(ops, case, ch, case.n_isect() + 5, annotate=True)
    assert ops._splat_slots_valid(f.tl, f.splats)
    arrays = f.backward(ops, absgrad, source="arrays")
    slots_on = f.backward(ops, absgrad, source="splats")
    slots_off = f.backward(ops, absgrad, splats=f.splats.clone())      # another tensor object: pair_info gives the slots
    assert not ops._splat_slots_valid(f.tl, f.splats.clone())
    f.check(slots_on, f"splat records + slots c{ch} absgrad={absgrad}")
    for other, what in ((slots_on, "arrays vs splat records"), (slots_off, "splat slots on vs off")):
        assert np.array_equal(arrays["flags"], other["flags"]), what
        for name in NAMES:
            if name in arrays:
                assert np.array_equal(arrays[name].view(np.uint32), other[name].view(np.uint32)), (what, name)


OVERFLOW = [n for n, c in CASES.items() if c[5] is not None]


@pytest.mark.parametrize("name", OVERFLOW)
def test_overflowed_lists_sum_the_slots_that_exist(ops, name):
    """Capacity (no multiple of 4) cut inside a rectangle, mid-row and mid-trip; big rectangles wholly past it, more of
    them than a big list has room for.  include/mgs.h: a slot at or past the capacity does not exist, every row is still
    written.  Nothing is written past the workspace (canary)."""
    f, absgrad = _frame(ops, name)
    assert f.overflowed and f.cap % 4 != 0
    got = f.backward(ops, absgrad, canary=1 << 16)
    assert (got["canary"] == 0xA5).all(), "the backward wrote past its workspace"
    f.check(got, name)
    assert R.slot_kinds(f.pair_info, got["flags"], f.cap)[2] > 0


@pytest.mark.parametrize("name", ["segments64-c3", "segments256-c4-abs"])
def test_segmented_walk_tables_flags_and_reduce(ops, name):
    """Intervals 64 and 256: the reduce assertion on the segmented walk's own records; the unit tables in the workspace
    equal the integer reference (counts as numbers, entries as sets) with an empty tile, a walk that ends on the last
    entry of a segment, one that ends on the first, and two table workgroups; the flags are those of the whole walk."""
    f, absgrad = _frame(ops, name)
    S, shift = f.interval, f.interval.bit_length() - 1
    assert f.tw * f.th > 256
    seg = f.backward(ops, absgrad, segmented=True)
    ref = R.unit_tables_ref(f.offsets, f.last_np, shift, f.tw, f.th)
    start = f.offsets[:-1]
    assert ref["n_seg"][0] == 0 and f.offsets[1] == f.offsets[0], "tile 0 is empty"
    assert ref["n_seg"][1] == 1 and ref["hi"][1] - start[1] + 1 == S and ref["cls"][1] == 0, "tile 1 ends a segment"
    assert ref["n_seg"][2] == 2 and ref["hi"][2] - start[2] == S and ref["cls"][2] == 31, "tile 2 starts a segment"
    counts = seg["unit_counts"][:33].astype(np.int64)
    print(f"\n[bwd_reduce] {name}: unit counts {list(counts)}")
    assert np.array_equal(counts, ref["counts"])
    assert counts[0] > 0 and (counts[1:] > 0).sum() >= 4
    assert {tuple(int(x) for x in e) for e in seg["unit_whole"][:counts[0]]} == ref["whole"]
    for c in range(32):
        assert {tuple(int(x) for x in e) for e in seg["unit_part"][c, :counts[1 + c]]} == ref["part"][c], c
    f.check(seg, name + " segmented")
    whole = f.backward(ops, absgrad, segmented=False)
    f.check(whole, name + " whole walk")
    assert np.array_equal(seg["flags"], whole["flags"]), "mgs.h: same records and slots -- the flags differ"


@pytest.mark.parametrize("name", ["count1100", "big-c4-abs", "channels-c12-abs", "segments64-c3"])
def test_second_call_gives_the_same_bits(ops, name):
    f, absgrad = _frame(ops, name)
    a = f.backward(ops, absgrad, segmented=bool(f.interval))
    b = f.backward(ops, absgrad, segmented=bool(f.interval))
    assert np.array_equal(a["records"].view(np.uint32), b["records"].view(np.uint32))
    assert np.array_equal(a["flags"], b["flags"])
    for name_ in NAMES:
        if name_ in a:
            assert np.array_equal(a[name_].view(np.uint32), b[name_].view(np.uint32)), name_
