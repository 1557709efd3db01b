"""The per-tile depth sort (robosimgs_amd/csrc/tile_sort.hip) held to the stable sort at the edges of its paths: list
lengths around every LDS list and unit count, units over the units' LDS list, more heavy buckets than the stack holds,
bucket sizes at each threshold, windows of the generic loop, digits below / at / above the key's lowest bit, ids-only
levels, every bit pattern of a depth key, and too small a capacity behind guard bands.

The cases and the model that says which path each one takes are tests/tile_sort_ref.py (preconditions are asserted when a
case is built; tests/test_tile_sort_ref_host.py builds them all without a GPU).  The expected result is always
oracle.gs_oracle_np.isect_tiles / isect_offsets, bit for bit -- no tolerance anywhere.  Every case runs under the radix
partition (debug knob 4: the order the model assumes) and under the shipped direct partition (knob 0) on libmgs_debug.so;
one case per family runs once more on libmgs.so itself.
"""
import numpy as np
import pytest
import torch

import tile_sort_ref as T
from guard_bands import forget_workspaces, guarded_empty, guards_intact, workspace_slack_intact
from oracle import gs_oracle_np as O

pytestmark = pytest.mark.gpu

DEV = "cuda"
SHIPPED = "shipped"                                  # libmgs.so, no knob


@pytest.fixture(scope="module")
def ops():
    from robosimgs_amd import ops as _ops
    return _ops


class Built:
    """A case's scene on the device and its stable sort, built once for all knobs."""

    def __init__(self, scene):
        means, radii, bits, self.tw, self.th, self.cap = scene
        self.n_tiles = self.tw * self.th
        self.args = (torch.from_numpy(means).to(DEV), torch.from_numpy(radii).to(DEV),
                     torch.from_numpy(bits.view(np.float32)).to(DEV))
        _, self.ids, self.flat = O.isect_tiles(means, radii, bits.view(np.float32), 16, self.tw, self.th, dtype=np.float32)
        self.total = len(self.flat)
        self.offsets = np.concatenate([O.isect_offsets(self.ids, 1, self.tw, self.th).reshape(-1), [self.total]])


_built = {}


@pytest.fixture(scope="module")
def built():
    def get(name, scene_fn):
        if name not in _built:
            _built[name] = Built(scene_fn())
        return _built[name]
    yield get
    _built.clear()


def _call(ops, b, knob, cap, **kw):
    """isect_tiles_raw under a knob of libmgs_debug.so, or on libmgs.so."""
    from robosimgs_amd import _lib
    if knob == SHIPPED:
        return ops.isect_tiles_raw(*b.args, b.tw, b.th, cap, **kw)
    with _lib.use_debug_lib() as lib:
        lib.mgs_debug_set_sort_opts(knob)
        try:
            return ops.isect_tiles_raw(*b.args, b.tw, b.th, cap, **kw)
        finally:
            lib.mgs_debug_set_sort_opts(0)


def _np(t):
    return t.cpu().numpy()


RUNS = [(name, knob) for name in T.CASES for knob in (4, 0)] + [(name, SHIPPED) for name in T.SHIPPED]


@pytest.mark.parametrize("name,knob", RUNS, ids=[f"{n}-{k}" for n, k in RUNS])
def test_lists_are_the_stable_sort(ops, built, name, knob):
    """flatten_ids, isect_ids, tile_ids, tile_offsets and n_isect bit for bit, status 0.  (Building the case asserts the
    model's precondition for the order knob 4 delivers; the other runs take the same input.)"""
    b = built(name, lambda: T.CASES[name][1]()[0])
    tl = _call(ops, b, knob, b.cap, want_isect_ids=True)
    assert int(tl.n_isect.item()) == b.total and int(tl.status.item()) == 0
    np.testing.assert_array_equal(_np(tl.tile_offsets), b.offsets)
    np.testing.assert_array_equal(_np(tl.flatten_ids[:b.total]), b.flat)
    np.testing.assert_array_equal(_np(tl.isect_ids[:b.total]), b.ids)
    np.testing.assert_array_equal(_np(tl.tile_ids[:b.total]), (b.ids >> 32).astype(np.int32))


# buffers one isect_tiles_raw call allocates: n_isect, status, tile_ids, flatten_ids, tile_offsets, tiles_per_gauss,
# group_order, and (after forget_workspaces) the workspace
N_BUFFERS = 8


@pytest.mark.parametrize("knob", [4, 0])
@pytest.mark.parametrize("short_by", ["0.45", "one"])
@pytest.mark.parametrize("name", ["biased", "bigmix"])
def test_deferred_lists_with_too_small_a_capacity_stay_inside_guarded_buffers(ops, built, name, short_by, knob):
    """C's biased-sample list (a unit over the units' LDS list) and B's mix of lists below and at / above kBigList with a
    capacity of 0.45 n_isect and of n_isect - 1: the overflow is flagged, n_isect reports the need, every offset lies
    inside the capacity, the lists that fit whole are the stable sort's, and nothing is written behind any buffer of the
    call, the workspace's unused quarter included (the collect and the units' kernels store at list offsets)."""
    from robosimgs_amd import _lib
    b = built("H_" + name, lambda: T.overflow_scenes()[name])
    cap = int(b.total * 0.45) if short_by == "0.45" else b.total - 1
    assert T.variant(cap, b.n_tiles) == "long"
    forget_workspaces()
    try:
        with guarded_empty() as guards:
            for _ in range(2):                              # (the second call finds the first one's tables in the workspace)
                tl = _call(ops, b, knob, cap)
                torch.cuda.synchronize()
                assert guards_intact(guards) and workspace_slack_intact()
                assert int(tl.n_isect.item()) == b.total and int(tl.status.item()) & _lib.MGS_STATUS_ISECT_OVERFLOW
                off, got = _np(tl.tile_offsets), _np(tl.flatten_ids)
                assert off.min() >= 0 and off.max() <= cap and np.all(np.diff(off) >= 0)
                whole = 0
                for t in range(b.n_tiles):
                    if b.offsets[t + 1] <= cap and off[t] == b.offsets[t] and off[t + 1] == b.offsets[t + 1]:
                        np.testing.assert_array_equal(got[off[t]:off[t + 1]], b.flat[off[t]:off[t + 1]])
                        whole += off[t + 1] > off[t]
        assert len(guards) >= 2 * N_BUFFERS - 1
        print(f"{name} capacity {cap} of {b.total}: {whole} lists whole")
    finally:
        forget_workspaces()
