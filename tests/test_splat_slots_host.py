"""Which splat records rasterize_bwd_det_raw trusts to carry a binning's record slots (ops._splat_slots_valid): the very
tensor object that binning annotated, until another binning annotates it.  The tagging is host-side bookkeeping, so CPU
tensors stand in for the device records here: no GPU."""
import gc

import torch

from robosimgs_amd import ops


def _binned(splats):
    tl = ops.TileLists()
    ops._tag_splat_slots(tl, splats)
    return tl


def test_only_the_annotated_tensor_object_is_trusted_and_only_by_its_latest_binning():
    s1 = torch.zeros(64, 12)
    first = _binned(s1)
    assert ops._splat_slots_valid(first, s1)
    assert not ops._splat_slots_valid(first, None)
    # binned again: the slot words now belong to the second binning
    second = _binned(s1)
    assert ops._splat_slots_valid(second, s1) and not ops._splat_slots_valid(first, s1)
    # other tensor objects over the same or copied records carry nobody's slots
    for other in (s1.clone(), s1.view(64, 12), s1[:], torch.zeros(64, 12)):
        assert not ops._splat_slots_valid(second, other)
    # lists that never annotated anything, and the train-state lists (their own state's records)
    assert not ops._splat_slots_valid(ops.TileLists(), s1)
    unannotated = ops.TileLists()
    unannotated.splat_slots = False
    assert not ops._splat_slots_valid(unannotated, s1)
    train = ops.TileLists()
    train.splat_slots = True
    assert ops._splat_slots_valid(train, s1)


def test_a_tensor_allocated_after_the_annotated_one_was_freed_is_not_trusted():
    s1 = torch.empty(4096, 12)
    tl = _binned(s1)
    addr = s1.data_ptr()
    del s1
    gc.collect()
    s2 = torch.empty(4096, 12)         # on CPU too the allocator may hand the same block straight back: that must not matter
    assert not ops._splat_slots_valid(tl, s2), f"same address: {s2.data_ptr() == addr}"
    assert not ops._splat_slots_valid(tl, s2.clone())
