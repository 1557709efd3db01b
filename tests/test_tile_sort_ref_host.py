"""tests/tile_sort_ref.py without a GPU: the constants it reads out of tile_sort.hip, its model of the main kernel's
splitters, and the precondition of every case of tests/test_gpu_tile_sort.py -- a case that does not sit on the edge it
is named after fails here, before any kernel runs.  numpy only.
"""
import numpy as np
import pytest

import tile_sort_ref as T


def test_every_constant_is_found_in_the_source():
    assert set(T.K) == set(T.CONSTANT_NAMES) and all(isinstance(v, int) and v > 0 for v in T.K.values())
    # the relations the cases lean on (they hold for any sensible retuning; a constant read from the wrong line breaks them)
    assert T.kFastShort < T.kFastMid < T.kFastLong <= T.kUnit < T.kFastUnit < T.kBigList
    assert T.kAdapt < T.kSmall < T.kSmallLong < T.kFastShort and T.kStack * (T.kSmall + 1) > T.kFastLong
    assert T.kSamplePerUnit < T.kSample and T.kUnitSample < T.BUCKETS_UNIT and T.kMaxUnits * 2 <= T.kSample
    assert 0 < T.SHORT_AVG < T.MID_AVG < T.kFastShort
    assert T.BUCKETS_UNIT < T.BUCKETS_MAIN["short"] == T.BUCKETS_MAIN["mid"] == T.BUCKETS_MAIN["long"]
    assert all(b & (b - 1) == 0 for b in (T.BUCKETS_UNIT, T.BUCKETS_MAIN["short"]))
    assert T.window(T.kFastShort, True) >= 64 and T.window(T.kFastUnit, False) >= 64
    with pytest.raises(LookupError):
        T._const("kNoSuchConstant")


def test_variant_follows_the_capacity_average():
    for nt in (1, 7, 32):
        assert T.variant(T.SHORT_AVG * nt, nt) == "short" and T.variant(T.SHORT_AVG * nt + 1, nt) == "mid"
        assert T.variant(T.MID_AVG * nt, nt) == "mid" and T.variant(T.MID_AVG * nt + 1, nt) == "long"
    # the rule tests/test_gpu_forward.py asserts by hand for its two-full-tiles cases
    assert T.variant(2 * 9_000 + 16, 32) == "short" and T.variant(2 * 12_000 + 16, 32) == "mid" and T.variant(2 * 12_000 + 16, 8) == "long"


@pytest.mark.parametrize("n", [T.kFastMid + 1, T.kUnit, T.kUnit + 1, 2 * T.kUnit + 1, T.kBigList, 12_000, 70_001,
                               T.kMaxUnits * T.kUnit + 1])
@pytest.mark.parametrize("kind", ["uniform", "equal", "sorted"])
def test_units_sum_to_the_list_and_none_is_empty(n, kind):
    rng = np.random.default_rng(n)
    bits = {"uniform": T.uniform_keys(n, rng), "equal": T.equal_keys(n), "sorted": np.sort(T.uniform_keys(n, rng))}[kind]
    c = T.composites(bits, rng.permutation(3 * n)[:n] if kind == "uniform" else np.arange(n))
    st, ns_all, nb, sub, ns = T.sample_plan(n)
    assert nb == min(-(-n // T.kUnit), T.kMaxUnits) and 2 * nb <= ns_all <= T.kSample and nb <= ns
    assert T.sample_positions(n).max() < n
    sizes = T.units_ungrouped(c)
    assert len(sizes) == nb and sizes.sum() == n and sizes.min() >= 1
    # a unit is an interval of the total order: sorting by (unit, composite) is sorting by composite
    u, _ = T.unit_of(c)
    assert np.array_equal(np.lexsort((c, u)), np.argsort(c, kind="stable"))


def test_the_issue_example_of_a_biased_sample():
    """12,000 entries: the sample's positions are the multiples of 72; a low band there leaves the last unit with every
    other entry and the others with about 28 each."""
    assert np.array_equal(T.sample_positions(12_000), np.arange(167) * 72)
    bits = T.biased_sample_keys(12_000, lambda m: np.full(m, T.BASE, np.uint32))
    sizes = T.units_ungrouped(T.composites(bits, np.arange(12_000)))
    assert len(sizes) == 6 and sizes[-1] > T.kFastUnit and sizes[:-1].max() <= 28 and sizes.sum() == 12_000


def test_walk_counts_levels_and_the_buckets_past_the_stack():
    rng = np.random.default_rng(3)
    c = T.composites(T.cluster_keys([T.kSmall + 1] * (T.kStack + 2), rng), np.arange((T.kStack + 2) * (T.kSmall + 1)))
    w = T.walk(c, 1024, T.kSmall)
    assert w["brute"] == 2 and w["sizes"][T.kSmall + 1] == T.kStack + 2
    c = T.composites(T.cluster_keys([T.kSmall] * (T.kStack + 2), rng), np.arange((T.kStack + 2) * T.kSmall))
    w = T.walk(c, 1024, T.kSmall)
    assert w["brute"] == 0 and w["levels"] == 1


@pytest.mark.parametrize("name", [n for n in T.CASES if not n.startswith("D_")])
def test_case_preconditions(name):
    """build() asserts what the model says about its scene; here also: the capacity holds the pairs and the grid is tiny."""
    scene, facts = T.CASES[name][1]()
    means, radii, bits, tw, th, cap = scene
    assert means.dtype == np.float32 and radii.dtype == np.int32 and bits.dtype == np.uint32
    assert len(means) == len(radii) == len(bits) and tw * th <= 32
    total = T.n_isect(scene)
    assert 0 < total <= cap and facts["variant"] == T.variant(cap, tw * th)
    print(name, facts)


@pytest.mark.parametrize("name", ["D_clamp", "D_pigeonhole"])
def test_case_preconditions_of_the_two_large_lists(name):
    scene, facts = T.CASES[name][1]()
    assert len(scene[2]) == scene[5] == facts["n"] and facts["units"] == T.kMaxUnits
    assert (name == "D_clamp") == (facts["n"] <= T.kMaxUnits * T.kFastUnit)
    print(name, facts)


def test_overflow_scenes_and_the_shipped_selection():
    sc = T.overflow_scenes()
    assert set(sc) == {"biased", "bigmix"}
    lens = sorted(len(l) for l in T.tile_lists(sc["bigmix"]) if len(l))
    assert lens[0] < T.kFastShort and any(T.kFastLong < n < T.kBigList for n in lens) and lens[-1] >= T.kBigList
    assert {T.CASES[n][0] for n in T.SHIPPED} == {T.CASES[n][0] for n in T.CASES} == set("ABCDEFG")
