"""The reduce stage's references checked on the host (tests/bwd_reduce_ref.py): the fp64 restatement against a direct
per-pixel evaluation, the fp32 restatement against the derived bound on the GPU module's own inputs -- clean, and with
each named defect -- the unit-table reference against a brute-force walk, the Python workspace views against the C size
query, and the argument errors of rasterize_bwd_det_raw(out=, workspace=).  No GPU."""
import itertools

import numpy as np
import pytest
import torch

import bwd_reduce_ref as R

CASES = R.gpu_cases()
IDS = [c[0] for c in CASES]


def _stand_in(spec):
    _, builder, args, ch, absgrad, cap_index, _ = spec
    case = R.built(builder, *args)
    cap = R.capacity_of(case, cap_index)
    records, flags, cap = case.stand_in(ch, absgrad, cap)
    return case, records, flags, cap


def _run(spec, bug=None):
    _, _, _, ch, absgrad, _, _ = spec
    case, records, flags, cap = _stand_in(spec)
    pi = case.pair_info()
    ref = R.reduce_f64(pi, records, flags, cap, case.means2d, case.conics, case.opacities, ch, absgrad)
    got = R.reduce_fp32(pi, records, flags, cap, case.means2d, case.conics, case.opacities, ch, absgrad, bug=bug)
    return R.compare(got, ref), ref


def test_f64_reduce_equals_the_per_pixel_sums():
    """Records formed in fp64 from a synthetic v_sigma field over the tiles of each rectangle: reduce_f64 must give the
    direct sums over PIXELS of v_sigma dx, v_sigma dx^2, ... with dx = mean - (pixel + 0.5), conic applied per Gaussian.
    Proves the moment algebra and the tile-centre convention (16 tile + 8) with no kernel involved."""
    rng = np.random.default_rng(5)
    rects = [(1, 0, 3, 2), (0, 2, 1, 1), (2, 1, 4, 3), (5, 0, 2, 4)]
    case = R.Case("pixels", 8, 5, rects, 5)
    pi = case.pair_info()
    cap = case.n_isect()
    ch = 3
    rf = R.record_floats(ch, True)
    records = np.zeros((cap, rf))
    flags = np.zeros(cap, dtype=np.uint8)
    direct = {k: np.zeros(s) for k, s in (("v_means2d", (4, 2)), ("v_conics", (4, 3)), ("v_feats", (4, ch)), ("v_opacities", 4),
                                          ("v_means2d_abs", (4, 2)))}
    scale = np.zeros(4)
    mean = case.means2d.astype(np.float64)
    for g, (x0, y0, w, h) in enumerate(rects):
        sums = np.zeros(6)
        for r_, c_ in itertools.product(range(h), range(w)):
            slot = pi[g, 0] + r_ * w + c_
            if (r_ or c_) and rng.random() < 0.25:
                continue                                   # an unflagged slot: its record (zeros here) must not matter
            flags[slot] = 1
            v = rng.standard_normal((16, 16))
            vf = rng.standard_normal((16, 16, ch))
            va = np.abs(rng.standard_normal((16, 16, 2)))
            py, px = np.mgrid[0:16, 0:16]
            X, Y = px + 0.5 - 8.0, py + 0.5 - 8.0           # pixel centre about the tile centre
            records[slot, :6] = [v.sum(), (v * X).sum(), (v * Y).sum(), (v * X * X).sum(), (v * X * Y).sum(), (v * Y * Y).sum()]
            records[slot, 6:6 + ch] = vf.sum((0, 1))
            records[slot, 6 + ch:8 + ch] = va.sum((0, 1))
            dx = mean[g, 0] - (16 * (x0 + c_) + px + 0.5)
            dy = mean[g, 1] - (16 * (y0 + r_) + py + 0.5)
            sums += [(v * dx).sum(), (v * dy).sum(), (v * dx * dx).sum(), (v * dx * dy).sum(), (v * dy * dy).sum(), v.sum()]
            direct["v_feats"][g] += vf.sum((0, 1))
            direct["v_means2d_abs"][g] += va.sum((0, 1))
            scale[g] += np.abs(v).sum() * (np.abs(dx).max() + np.abs(dy).max() + 16) ** 2
        a, b, c = case.conics[g].astype(np.float64)
        direct["v_means2d"][g] = [a * sums[0] + b * sums[1], b * sums[0] + c * sums[1]]
        direct["v_conics"][g] = [0.5 * sums[2], sums[3], 0.5 * sums[4]]
        direct["v_opacities"][g] = -sums[5] / float(case.opacities[g])
    records[flags == 0] = np.nan                            # ... and poisoned, it must not be read
    ref = R.reduce_f64(pi, records, flags, cap, case.means2d, case.conics, case.opacities, ch, True)
    amp = np.maximum(1.0, np.abs(case.conics).max(1) + 1.0 / case.opacities)
    for name, want in direct.items():
        got = ref[name][0]
        # 1e-12 relative to the sum of the operands' absolute values (the sums cancel: |want| alone is no scale)
        tol = 1e-12 * (scale * amp).reshape((-1,) + (1,) * (want.ndim - 1))
        assert np.all(np.abs(got - want) <= tol), (name, np.abs(got - want).max())
    assert (ref["counted"] > 0).all()


@pytest.mark.parametrize("spec", CASES, ids=IDS)
def test_clean_fp32_restatement_is_inside_the_bound_and_the_case_is_not_degenerate(spec, record_property):
    """On every GPU case's inputs (records from the CPU stand-in): the fp32 restatement in the kernels' order passes the
    derived bound on every row, and the case holds a real share of flagged and of unflagged slots (and of non-existent
    ones where the capacity cuts the lists) -- no case sums nothing."""
    (worst, bad), ref = _run(spec)
    case, records, flags, cap = _stand_in(spec)
    flagged, unflagged, missing = R.slot_kinds(case.pair_info(), flags, cap)
    total = flagged + unflagged + missing
    print(f"{spec[0]}: n={case.n} slots={total} flagged={flagged} unflagged={unflagged} non-existent={missing} "
          f"worst error/bound {max(worst.values()):.3f}")
    record_property("worst_ratio", max(worst.values()))
    assert not bad, bad
    assert max(worst.values()) <= 1.0
    exist = flagged + unflagged
    assert flagged >= 0.05 * exist and unflagged >= 0.05 * exist, (flagged, unflagged, missing)
    if spec[5] is not None:
        assert missing >= 0.05 * total, (flagged, unflagged, missing)
    else:
        assert missing == 0
    live = ref["counted"] > 0
    assert live.any()
    if (case.rects[:, 2] * case.rects[:, 3] == 0).any():
        assert (~live).any()                                # rows with no counted slot (exact zeros) are in the case too


# which case must catch which deliberate defect (each also fails others; profiles/bwd_reduce/README.md has the matrix)
CATCHES = {"no_plus8": "geometry-c3", "column_major": "geometry-c3", "ignore_flags": "channels-c12", "no_half": "channels-c3-abs",
           "vab_sign": "geometry-c3-abs", "opacity_no_divide": "count64", "opacity_sign": "channels-c5",
           "read_past_capacity": "overflow0-c3-abs", "drop_row64": "rounds-c4-abs", "skip_256": "big-c3"}


@pytest.mark.parametrize("bug", R.BUGS)
def test_each_named_defect_fails_the_bound(bug):
    assert set(CATCHES) == set(R.BUGS)
    spec = CASES[IDS.index(CATCHES[bug])]
    (worst, bad), _ = _run(spec, bug=bug)
    assert bad, f"{bug} passes {spec[0]}: worst error/bound {worst}"


def test_wave_layout_of_the_rounds_case():
    """The rounds case is what its docstring says: wave 0 owns Gaussians 0..15 and 64..79, its rows pass 64 and 128, and
    Gaussian 12 straddles row 64 of the first round."""
    case = R.built(R.case_rounds)
    wave, lane, row0 = R.rows_wave_layout(case.pair_info())
    assert list(np.nonzero(wave == 0)[0][:32]) == list(range(16)) + list(range(64, 80))
    assert row0[12] < 63 < row0[12] + 9 - 1 and row0[12] + 9 > 64
    h = case.rects[:, 3]
    assert row0[79] + h[79] > 128 and lane[64] == 16


def test_designed_edges_are_in_the_cases():
    """Widths 1..9 at slot bases of every residue mod 4 (both flag words of a trip, rows that end on and off a trip
    boundary), every residue for the wide kernel's `lead`, the big sizes, and the cut capacities."""
    pi = R.built(R.case_geometry).pair_info().astype(np.int64)
    w = pi[:, 3] & 0xffff
    assert {(int(a), int(b) % 4) for a, b in zip(w, pi[:, 0]) if a} >= {(a, b) for a in range(1, 10) for b in range(4)}
    assert (w == 0).sum() >= 8
    pi = R.built(R.case_channels).pair_info().astype(np.int64)
    assert {int(b) % 4 for b, x in zip(pi[:, 0], pi[:, 3]) if x} == {0, 1, 2, 3}
    sizes = lambda c: sorted(int(a * b) for _, _, a, b in c.rects)
    assert {255, 256, 272, 289} <= set(sizes(R.built(R.case_big))) and {255, 256, 257} <= set(sizes(R.built(R.case_big_strip)))
    assert any(h > 64 and w_ * h >= 256 for _, _, w_, h in R.built(R.case_tall).rects)
    assert sum(s >= 256 for s in sizes(R.built(R.case_many_big))) > 4096
    case = R.built(R.case_overflow)
    pi = case.pair_info().astype(np.int64)
    for cap in R.overflow_capacities(case):
        g = int(np.nonzero(pi[:, 0] <= cap)[0][-1])
        wg = int(pi[g, 3] & 0xffff)
        off = cap - int(pi[g, 0])
        assert cap % 4 and 0 < off % wg and off < wg * int(pi[g, 3] >> 16), (cap, g)     # inside a rectangle, mid-row
        # the case lists more big rectangles than one big list has room for at this capacity (capacity / 256 + 1), and some
        # of them lie wholly past it
        big = (pi[:, 3] & 0xffff) * (pi[:, 3] >> 16) >= 256
        assert big.sum() > cap // 256 + 1 and (big & (pi[:, 0] >= cap)).sum() >= 2


def _brute_tables(tile_offsets, last_ids, shift, tile_w, tile_h):
    H, W = last_ids.shape
    S = 1 << shift
    whole, part = set(), [set() for _ in range(32)]
    for t in range(tile_w * tile_h):
        tx, ty = t % tile_w, t // tile_w
        start, end = int(tile_offsets[t]), int(tile_offsets[t + 1])
        hi = None
        for y in range(16 * ty, min(16 * ty + 16, H)):
            for x in range(16 * tx, min(16 * tx + 16, W)):
                hi = int(last_ids[y, x]) if hi is None else max(hi, int(last_ids[y, x]))
        hi = min(hi, end - 1)
        segs = {}
        for idx in range(start, hi + 1):                    # walk the entries the backward visits
            segs.setdefault((idx - start) // S, []).append(idx)
        if not segs:
            continue
        last = max(segs)
        for sg in segs:
            if sg != last:
                assert len(segs[sg]) == S
                whole.add((t, sg, start, hi))
        part[(S - len(segs[last])) * 32 // S].add((t, last, start, hi))
    return whole, part


@pytest.mark.parametrize("shift", [6, 8])
def test_unit_table_reference_against_a_brute_force_walk(shift):
    rng = np.random.default_rng(shift)
    tw, th, W, H = 5, 4, 75, 60
    S = 1 << shift
    lens = rng.integers(0, 3 * S, tw * th)
    lens[[0, 1, 2, 3, 4]] = [0, S, S + 1, 2 * S, 1]          # empty; ends on a segment's last entry; on a first entry
    off = np.r_[0, np.cumsum(lens)]
    last = np.zeros((H, W), dtype=np.int32)
    for t in range(tw * th):
        tx, ty = t % tw, t // tw
        blk = last[16 * ty:16 * ty + 16, 16 * tx:16 * tx + 16]
        lo, hi = off[t], max(off[t + 1], off[t] + 1)
        blk[...] = rng.integers(lo, hi, blk.shape) if t % 7 else 0      # (some tiles nothing reached: last_ids stay 0)
        if t in (1, 2, 3) and blk.size:
            blk[0, 0] = off[t + 1] - 1                       # the walk goes to the list's end
        if t == 6:
            blk[...] = off[t + 1] + 40                       # past the end (a cut list): clamped to end - 1
    ref = R.unit_tables_ref(off, last, shift, tw, th)
    whole, part = _brute_tables(off, last, shift, tw, th)
    assert ref["whole"] == whole and ref["part"] == part
    assert list(ref["counts"]) == [len(whole)] + [len(p) for p in part]
    assert ref["n_seg"][0] == 0 and ref["cls"][1] == 0 and ref["n_seg"][1] == 1 and ref["cls"][2] == 31 and ref["n_seg"][2] == 2


def test_workspace_views_rest_on_the_offsets_of_the_size_query():
    """rasterize_bwd_det_workspace_layout (what the Python views use, what include/mgs.h documents) against the library's own
    size query: the totals agree for every shape, so a change of BwdDetWs cannot leave the views behind unnoticed."""
    from robosimgs_amd import ops
    for (tw, th), cap, ch, absg, iv in itertools.product(((120, 68), (4, 3), (17, 17)), (0, 1, 7, 255, 256, 257, 65_536, 1_000_003),
                                                         (1, 2, 3, 4, 5, 8, 12, 20, 32), (False, True), (0, 64, 256)):
        lay = ops.rasterize_bwd_det_workspace_layout(ch, absg, cap, tw, th, iv)
        assert lay["total"] == ops.rasterize_bwd_det_workspace_bytes(ch, absg, cap, tw, th, iv), (tw, th, cap, ch, absg, iv)
        assert lay["record_floats"] == R.record_floats(ch, absg)
        assert lay["flags"] % 256 == 0 and lay["flags"] >= max(cap, 1) * lay["record_floats"] * 4 > lay["flags"] - 256
        assert lay["counters"] == lay["flags"] + (max(cap, 1) + 255) // 256 * 256 and lay["order"] == lay["counters"] + 256
    ws = torch.zeros(ops.rasterize_bwd_det_workspace_bytes(3, True, 1000, 4, 3, 64) + 256, dtype=torch.uint8)
    v = ops.rasterize_bwd_det_workspace_views(ws, 3, True, 1000, 4, 3, 64)
    assert tuple(v["records"].shape) == (1000, 12) and tuple(v["flags"].shape) == (1000,)
    assert tuple(v["unit_whole"].shape) == ((1000 >> 6) + 12 + 1, 4) and tuple(v["unit_part"].shape) == (32, 12, 4)
    base = ws.data_ptr() + (-ws.data_ptr() % 256)
    lay = ops.rasterize_bwd_det_workspace_layout(3, True, 1000, 4, 3, 64)
    assert v["records"].data_ptr() == base and v["flags"].data_ptr() == base + lay["flags"]
    assert v["unit_counts"].data_ptr() == base + lay["order"] and v["unit_whole"].data_ptr() == base + lay["order"] + 256


def test_argument_errors_of_out_and_workspace():
    from robosimgs_amd import ops
    n, ch = 5, 3
    m2d, con, feats, op = torch.zeros(n, 2), torch.zeros(n, 3), torch.zeros(n, ch), torch.zeros(n)
    tl = ops.TileLists()
    tl.capacity, tl.tile_offsets, tl.flatten_ids, tl.pair_info, tl.group_order, tl.splat_slots = 100, None, None, None, None, False
    frame = (torch.zeros(16, 16), torch.zeros(16, 16, dtype=torch.int32), torch.zeros(16, 16, ch), torch.zeros(16, 16))

    def call(**kw):
        return ops.rasterize_bwd_det_raw(m2d, con, feats, op, None, 16, 16, 1, 1, tl, *frame, **kw)

    good = (torch.zeros(n, 2), torch.zeros(n, 3), torch.zeros(n, ch), torch.zeros(n), None)
    for bad in (good[:4],                                                          # four instead of five
                (torch.zeros(n, 3),) + good[1:],                                   # a wrong shape
                good[:2] + (torch.zeros(n, ch, dtype=torch.float64),) + good[3:],  # a wrong type
                good[:3] + (torch.zeros(2 * n)[::2],) + good[4:],                  # not contiguous
                good[:4] + (torch.zeros(n, 2),)):                                  # an absgrad buffer without absgrad
        with pytest.raises(ValueError, match="out"):
            call(out=bad)
    with pytest.raises(ValueError, match="out"):
        call(out=good, absgrad=True)                                               # absgrad without its buffer
    need = ops.rasterize_bwd_det_workspace_bytes(ch, False, 100, 1, 1)
    with pytest.raises(ValueError, match="workspace"):
        call(out=good, workspace=torch.zeros(need + 256, dtype=torch.float32))
    with pytest.raises(ValueError, match="workspace"):
        call(out=good, workspace=torch.zeros(need - 1, dtype=torch.uint8))
    with pytest.raises(ValueError, match="workspace"):
        call(out=good, workspace=torch.zeros(need + 256, dtype=torch.uint8), canary_bytes=4096)
    with pytest.raises(ValueError, match="workspace"):
        ops.rasterize_bwd_det_workspace_views(torch.zeros(need - 1, dtype=torch.uint8), ch, False, 100, 1, 1)
