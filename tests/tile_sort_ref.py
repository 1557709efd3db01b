"""Cases for the per-tile depth sort (robosimgs_amd/csrc/tile_sort.hip) at the edges of its paths, and a model of which
path an input takes.  numpy only: tests/test_tile_sort_ref_host.py checks every case's precondition without a GPU,
tests/test_gpu_tile_sort.py runs the cases.

The EXPECTED RESULT of every case is the stable sort of oracle.gs_oracle_np.isect_tiles, bit for bit.  Nothing in this
module is ever an expected result: the model only says where an input goes (which instantiation, how many units and of what
size under the radix partition, which bucket sizes the bit-field levels see, whether the stack of heavy buckets overflows),
so that a case can assert it really sits on the edge it is named after.

Every constant is read out of tile_sort.hip: a changed constant moves the shapes with it.

A scene is the tuple (means2d [N,2] f32, radii [N] i32, depth bits [N] u32, tile_w, tile_h, capacity).  Depths are bit
patterns (view them as float32 to hand them over: no conversion, no NaN canonicalisation).  Every Gaussian either covers
every tile of a tiny grid (`cover_scene`) or sits inside one tile (`inside_scene`: a few full tiles among empty ones, so
that the AVERAGE the capacity allows picks the short and mid instantiations while a list is still long).

Under debug knob 4 the binning's radix partition is stable, so a tile's list reaches the sort in Gaussian-index order and
the main kernel's sample -- list positions i * sub * st -- is known: `units_ungrouped` is deterministic.  The grouped
(shipped) path scatters in an order the hardware picks; only the result is asserted there.
"""
import os
import re
from collections import Counter

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = open(os.path.join(ROOT, "robosimgs_amd", "csrc", "tile_sort.hip")).read()

CONSTANT_NAMES = ("kFastShort", "kFastMid", "kFastLong", "kUnit", "kFastUnit", "kMaxUnits", "kBigList", "kSample",
                  "kSamplePerUnit", "kSmall", "kSmallLong", "kStack", "kAdapt", "kUnitSample")


def _const(name):
    """`constexpr <type> ..., name = <int>` on one line of tile_sort.hip."""
    m = re.search(r"^constexpr\s+\w+\s+.*?\b%s\s*=\s*(\d+)\s*[,;]" % name, SRC, re.M)
    if m is None:
        raise LookupError(f"tile_sort.hip: no constexpr {name}")
    return int(m.group(1))


def _search(pattern, what):
    m = re.search(pattern, SRC, re.S)
    if m is None:
        raise LookupError(f"tile_sort.hip: {what} not found")
    return [int(g) for g in m.groups()]


K = {name: _const(name) for name in CONSTANT_NAMES}
kFastShort, kFastMid, kFastLong, kUnit, kFastUnit, kMaxUnits, kBigList = (K[n] for n in CONSTANT_NAMES[:7])
kSample, kSamplePerUnit, kSmall, kSmallLong, kStack, kAdapt, kUnitSample = (K[n] for n in CONSTANT_NAMES[7:])
# buckets_for(fast): `return fast > A ? B : C;`
_BUCKET_EDGE, _BUCKETS_OVER, _BUCKETS_UPTO = _search(r"buckets_for\(int fast\)\s*\{\s*return\s+fast\s*>\s*(\d+)\s*\?\s*(\d+)\s*:\s*(\d+)\s*;",
                                                     "buckets_for")
# entries per tile the capacity allows on average: up to SHORT_AVG the short form, up to MID_AVG the mid form
SHORT_AVG, = _search(r"bool capacity_says_short_lists\([^)]*\)\s*\{[^}]*?\*\s*(\d+)\s*;", "capacity_says_short_lists")
MID_AVG, = _search(r"const bool mid_lists\s*=[^;]*?\*\s*(\d+)\s*;", "mid_lists")

KFAST = {"short": kFastShort, "mid": kFastMid, "long": kFastLong}


def buckets_for(fast):
    return _BUCKETS_OVER if fast > _BUCKET_EDGE else _BUCKETS_UPTO


BUCKETS_MAIN = {v: buckets_for(f) for v, f in KFAST.items()}
BUCKETS_UNIT = buckets_for(kFastUnit)


def window(fast, own_offsets):
    """kWin of the generic loop: the LDS list less a bucket's reach on either side, less the offsets kept in its tail
    (the short form keeps them in an array of their own)."""
    ksm = kSmallLong if fast == kFastUnit else kSmall
    return fast - (0 if own_offsets else buckets_for(fast) // 2) - 2 * ksm


def variant(capacity, n_tiles):
    """Which instantiation of the main kernel a launch takes: tile_depth_sort's rule on the average list length the
    capacity allows.  The short form sorts every list itself; the other two defer lists over their LDS list to units."""
    if capacity <= n_tiles * SHORT_AVG:
        return "short"
    return "mid" if capacity <= n_tiles * MID_AVG else "long"


def max_units_for(capacity, n_tiles):
    return capacity // kUnit + n_tiles + 1


def composites(bits, ids):
    return (np.asarray(bits, np.uint64) << np.uint64(32)) | np.asarray(ids, np.uint64)


def sample_plan(n):
    """The main kernel's sampling of a deferred list of n entries (ungrouped): st, ns_all, nb, sub, ns."""
    st = -(-n // kSample)
    ns_all = min(-(-n // st), kSample)
    nb = min(-(-n // kUnit), kMaxUnits)
    nb = min(nb, ns_all // 2 if ns_all > 2 else 1)
    sub = max(ns_all // (kSamplePerUnit * nb), 1)
    ns = -(-ns_all // sub)
    return st, ns_all, nb, sub, ns


def sample_positions(n):
    st, _, _, sub, ns = sample_plan(n)
    return np.arange(ns, dtype=np.int64) * sub * st


def unit_of(list_composites):
    """Unit of every entry of a deferred list given in the order the sort receives it (ungrouped): splitter q is the
    sample's element of rank floor(q ns / nb), an entry's unit the number of splitters at or below it."""
    c = np.asarray(list_composites, np.uint64)
    n = len(c)
    _, _, nb, _, ns = sample_plan(n)
    ranked = np.sort(c[sample_positions(n)])
    split = ranked[(np.arange(1, nb, dtype=np.int64) * ns) // nb]
    return np.searchsorted(split, c, side="right"), nb


def units_ungrouped(list_composites):
    """Unit sizes the main kernel's splitters give a deferred list under the radix partition (knob 4)."""
    u, nb = unit_of(list_composites)
    return np.bincount(u, minlength=nb)


def level_buckets(c, n_buckets):
    """Bucket sizes, in bucket order, of one bit-field level over the composites c (two at least, distinct)."""
    c = np.asarray(c, np.uint64)
    hb = int(c.min() ^ c.max()).bit_length() - 1
    bits = n_buckets.bit_length() - 1
    shift = max(hb - (bits - 1), 0)
    return np.bincount(((c >> np.uint64(shift)) & np.uint64(n_buckets - 1)).astype(np.int64), minlength=n_buckets), shift


def walk(c, n_buckets, ksm, lds=0):
    """The bit-field levels a segment goes through in the generic loop (and in lds_level without splitters): bucket sizes
    do not depend on the order of the entries, so the walk is exact.  Returns the number of levels, the sizes of every
    bucket met (Counter), the segments popped off the stack (sizes), the buckets found past the stack's room (kBrute;
    brute_lds: those of them found by a popped segment of up to `lds` entries, i.e. inside lds_level in the units' kernel)
    and the level-0 shift."""
    stack = [np.asarray(c, np.uint64)]
    out = dict(levels=0, sizes=Counter(), popped=[], brute=0, brute_lds=0, brute_sizes=[], shift0=None)
    while stack:
        seg = stack.pop()
        out["popped"].append(len(seg))
        if len(seg) <= ksm:
            continue
        sizes, shift = level_buckets(seg, n_buckets)
        if out["shift0"] is None:
            out["shift0"] = shift
        out["levels"] += 1
        out["sizes"].update(int(s) for s in sizes if s)
        d = ((seg >> np.uint64(shift)) & np.uint64(n_buckets - 1)).astype(np.int64)
        base = len(stack)
        for k, b in enumerate(np.flatnonzero(sizes > ksm)):
            if base + k < kStack:
                stack.append(seg[d == b])
            else:
                out["brute"] += 1
                out["brute_lds"] += len(out["popped"]) > 1 and len(seg) <= lds
                out["brute_sizes"].append(int(sizes[b]))
    return out


def straddled_windows(c, n_buckets, win):
    """Level 0 over c: for every window edge k * win inside the segment, the size of the bucket that lies across it (0 where
    the edge falls between two buckets)."""
    sizes, _ = level_buckets(c, n_buckets)
    ends = np.cumsum(sizes)
    starts = ends - sizes
    out = []
    for edge in range(win, len(c), win):
        b = int(np.searchsorted(ends, edge, side="right"))
        out.append(int(sizes[b]) if starts[b] < edge < ends[b] else 0)
    return out


# ---- scenes ---------------------------------------------------------------------------------------------------------
TILE = 16


def inside_scene(lists, tw, th, capacity, tiles=None, stride=1):
    """Every key array of `lists` becomes the list of one tile (tiles[k], default k + 1; tile 0 stays empty), in that
    order; stride > 1 puts stride - 1 culled Gaussians (radius 0) behind every visible one, so that the ids are
    multiples of it.  Radius 3 around a mean within 2 px of the tile's centre: one tile."""
    tiles = list(range(1, len(lists) + 1)) if tiles is None else list(tiles)
    assert len(tiles) == len(lists) and max(tiles) < tw * th and len(set(tiles)) == len(tiles)
    tile = np.concatenate([np.full(len(l), t, np.int64) for l, t in zip(lists, tiles)] + [np.zeros(0, np.int64)])
    bits = np.concatenate([np.asarray(l, np.uint32) for l in lists] + [np.zeros(0, np.uint32)])
    n = len(bits)
    i = np.arange(n)
    means = np.stack([(tile % tw) * TILE + 8.0 + (i * 7 % 5 - 2), (tile // tw) * TILE + 8.0 + (i * 3 % 5 - 2)], axis=1)
    radii = np.full(n, 3, np.int32)
    if stride > 1:
        m, r, b = np.zeros((n * stride, 2)), np.zeros(n * stride, np.int32), np.zeros(n * stride, np.uint32)
        m[::stride], r[::stride], b[::stride] = means, radii, bits
        b[1::stride] = 0x3f800000                           # (the culled ones lie in front of everything: never listed)
        means, radii, bits = m, r, b
    return means.astype(np.float32), radii, bits, tw, th, int(capacity)


def cover_scene(bits, tw, th, capacity=None):
    """Every Gaussian covers every tile: tw * th lists of all of them."""
    bits = np.asarray(bits, np.uint32)
    n = len(bits)
    i = np.arange(n)
    means = np.stack([TILE * tw / 2.0 + (i * 7 % 5 - 2), TILE * th / 2.0 + (i * 3 % 5 - 2)], axis=1).astype(np.float32)
    radii = np.full(n, TILE * max(tw, th) + TILE, np.int32)
    return means, radii, bits, tw, th, int(n * tw * th + 16 if capacity is None else capacity)


def tile_lists(scene):
    """Per tile: the composites of its list in Gaussian-index order -- what the sort receives under knob 4."""
    from oracle import gs_oracle_np as O
    means, radii, bits, tw, th, _ = scene
    x0, x1, y0, y1 = O.tile_rects(means, radii, TILE, tw, th, np.float32)
    ids = np.arange(len(bits))
    out = []
    for t in range(tw * th):
        tx, ty = t % tw, t // tw
        m = (x0 <= tx) & (tx < x1) & (y0 <= ty) & (ty < y1)
        out.append(composites(bits[m], ids[m]))
    return out


def n_isect(scene):
    return sum(len(l) for l in tile_lists(scene))


# ---- depth keys -----------------------------------------------------------------------------------------------------
LOW, BASE, STEP = 0x40000000, 0x40100000, 1 << 16          # the biased sample's low band; clusters at BASE + j * STEP


def uniform_keys(n, rng):
    return rng.uniform(0.5, 20.0, size=n).astype(np.float32).view(np.uint32)


def equal_keys(n):
    return np.full(n, 0x40500000, np.uint32)                # 3.25


def cluster_keys(sizes, rng, jitter=0, base=BASE, step=STEP):
    """Cluster j: sizes[j] depths at base + j * step + 16, bit-identical (jitter 0) or within +-jitter ulps; shuffled."""
    k = np.concatenate([np.full(s, base + j * step + 16, np.int64) for j, s in enumerate(sizes)])
    if jitter:
        k = k + rng.integers(-jitter, jitter + 1, size=len(k))
    return rng.permutation(k).astype(np.uint32)


def filler_keys(n, rng, base, span=1 << 20):
    """n distinct keys in [base, base + span), shuffled."""
    return (base + rng.permutation(span)[:n]).astype(np.uint32)


def biased_sample_keys(n, high, low=LOW):
    """A list of n entries whose sample (ungrouped) holds nothing but a narrow low band: the entries at the sample's
    positions are low + 0, 1, ...; all others take `high(count)` in order, every one above the band.  The last unit
    then holds every one of those and the top samples, the other units some two dozen entries each."""
    pos = sample_positions(n)
    bits = np.empty(n, np.uint32)
    mask = np.zeros(n, bool)
    mask[pos] = True
    bits[mask] = low + np.arange(len(pos), dtype=np.uint32)
    hi = np.asarray(high(n - len(pos)), np.uint32)
    assert len(hi) == n - len(pos) and (len(hi) == 0 or int(hi.min()) > low + len(pos))
    bits[~mask] = hi
    return bits


PLANTED = (0x00000000, 0x00000001, 0x007fffff, 0x7f7fffff, 0x7f800000, 0x80000000, 0xff800000, 0xffffffff)


def any_bits_keys(n, rng, top=5):
    """Keys drawn from all of uint32 (negative numbers, denormals, infinities and NaNs included) with every PLANTED
    pattern put in twice; the last `top` entries are 0xffffffff."""
    k = rng.integers(0, 1 << 32, size=n, dtype=np.uint64).astype(np.uint32)
    at = rng.permutation(n - top)[:2 * len(PLANTED)]
    k[at] = np.repeat(np.array(PLANTED, np.uint32), 2)
    k[n - top:] = 0xffffffff
    return k


# ---- the cases ------------------------------------------------------------------------------------------------------
# name -> (family, build).  build() returns (scene, facts): `facts` is what the model says about the scene -- asserted
# inside build, so a case whose precondition does not hold cannot be built -- kept for the record
# (profiles/tile_sort_edges/README.md).
CASES = {}


def case(name, family):
    def deco(fn):
        CASES[name] = (family, fn)
        return fn
    return deco


def _rng(name):
    return np.random.default_rng(sum(name.encode()) * 7919 + len(name))


def _grid_for(v, lists):
    """A grid and a capacity AT THE EDGE of variant v's rule for lists in tiles 1..: the short form at exactly SHORT_AVG
    per tile, the mid form at exactly MID_AVG, the long form one entry over it."""
    tw, th = 4, 3
    nt = tw * th
    assert nt > len(lists)
    cap = {"short": SHORT_AVG * nt, "mid": MID_AVG * nt, "long": MID_AVG * nt + 1}[v]
    assert cap >= sum(lists) and variant(cap, nt) == v
    return tw, th, cap


def _a(v, equal):
    name = f"A_{v}_{'equal' if equal else 'uniform'}"

    @case(name, "A")
    def build():
        f = KFAST[v]
        lens = [1, 2, 63, 64, 65, f - 1, f, f + 1]                       # (and 0: tile 0 and the tiles behind the lists)
        rng = _rng(name)
        tw, th, cap = _grid_for(v, lens)
        sc = inside_scene([equal_keys(n) if equal else uniform_keys(n, rng) for n in lens], tw, th, cap)
        got = [len(l) for l in tile_lists(sc)]
        assert got == [0] + lens + [0] * (tw * th - 1 - len(lens))
        path = "its own generic loop" if v == "short" else "one unit"
        return sc, dict(variant=v, lists=got, path=f"lists up to kFast = {f}: lds_level; {f + 1} entries: {path}")


for _v in KFAST:
    for _e in (False, True):
        _a(_v, _e)


def _mid_or_long_grid(v, total):
    """(tw, th) whose average at capacity == total picks variant v."""
    tw, th = (8, 4) if v == "mid" else (4, 2)
    assert variant(total, tw * th) == v and variant(total + 16, tw * th) == v
    return tw, th


def _b(v, tight):
    name = f"B_{v}_{'tight' if tight else 'lengths'}"

    @case(name, "B")
    def build():
        f = KFAST[v]
        lens = ([kBigList - 1, kBigList, f + 1, kBigList + kUnit + 1, 3, kBigList] if tight else
                [f + 1, kUnit, kUnit + 1, 2 * kUnit, 2 * kUnit + 1, kBigList - 1, kBigList])
        rng = _rng(name)
        total = sum(lens)
        tw, th = _mid_or_long_grid(v, total)
        cap = total if tight else total + 16
        sc = inside_scene([uniform_keys(n, rng) for n in lens], tw, th, cap)
        lists = tile_lists(sc)
        assert [len(l) for l in lists[1:len(lens) + 1]] == lens and variant(cap, tw * th) == v
        units = [(n, units_ungrouped(l).tolist()) for n, l in zip(lens, lists[1:]) if n > f]
        for n, u in units:
            assert len(u) == min(-(-n // kUnit), kMaxUnits) and sum(u) == n and min(u) >= 1 and max(u) <= kFastUnit
        big = sum(len(u) for n, u in units if n >= kBigList)
        small = sum(len(u) for n, u in units if n < kBigList)
        room = max_units_for(cap, tw * th)
        assert big > 0 and small > 0 and big + small <= room
        if tight:
            assert cap == n_isect(sc)
        return sc, dict(variant=v, lists=lens, units=[(n, len(u)) for n, u in units], from_bottom=big, from_top=small,
                        table=room, max_unit=max(max(u) for _, u in units))


for _v in ("mid", "long"):
    for _t in (False, True):
        _b(_v, _t)


def _oversized(name, n, high, want=None):
    """A cover scene (2 x 1 tiles, long form) of one biased-sample list; the model's units and the walk of the last one."""
    bits = biased_sample_keys(n, high)
    sc = cover_scene(bits, 2, 1)
    assert variant(sc[5], 2) == "long"
    lists = tile_lists(sc)
    assert len(lists[0]) == n and np.array_equal(lists[0], lists[1])
    u, nb = unit_of(lists[0])
    sizes = np.bincount(u, minlength=nb)
    assert sizes.sum() == n and sizes.min() >= 1 and sizes.argmax() == nb - 1 and sizes[-1] > kFastUnit
    w = walk(lists[0][u == nb - 1], BUCKETS_UNIT, kSmallLong, lds=kFastUnit)
    facts = dict(variant="long", n=n, units=nb, max_unit=int(sizes[-1]), other_units_max=int(sizes[:-1].max()),
                 levels=w["levels"], brute=w["brute"], brute_in_lds_level=w["brute_lds"],
                 popped_max=max(w["popped"][1:], default=0))
    return sc, lists[0][u == nb - 1], w, facts


@case("C_biased", "C")
def _c_biased():
    rng = _rng("C_biased")
    sc, _, w, facts = _oversized("C_biased", 12_000, lambda m: filler_keys(m, rng, BASE))
    assert sample_plan(12_000)[0] * sample_plan(12_000)[3] == 72
    return sc, facts


@case("C_stack", "C")           # (also E's first bullet inside a unit)
def _c_stack():
    rng = _rng("C_stack")
    n_cl = kStack + 4
    high = lambda m: np.concatenate([cluster_keys([kSmallLong + 1] * n_cl, rng, jitter=1),
                                     filler_keys(m - n_cl * (kSmallLong + 1), rng, BASE + 128 * STEP)])
    sc, _, w, facts = _oversized("C_stack", n_cl * (kSmallLong + 1) + 600, high)
    assert w["brute"] >= 4 and min(w["brute_sizes"]) > kSmallLong       # more than kStack heavy buckets at one level
    return sc, facts


@case("C_stack_deep", "C")
def _c_stack_deep():
    """The stack is full when a popped bucket that fits the LDS list is bucketed again: each of the kStack + 4 level-0
    buckets holds three clusters of kSmallLong + 1 depths 4,096 apart, heavy again one level down -- lds_level (mode 0)
    finds them with stack_base = kStack - 1 and marks all but the first kBrute."""
    rng = _rng("C_stack_deep")
    n_cl, m = kStack + 4, kSmallLong + 1

    def high(count):
        k = np.concatenate([np.full(m, BASE + j * STEP + 16 + t * 4096, np.int64) for j in range(n_cl) for t in range(3)])
        k = rng.permutation(k + rng.integers(-1, 2, size=len(k))).astype(np.uint32)
        return np.concatenate([k, filler_keys(count - len(k), rng, BASE + 128 * STEP)])
    sc, _, w, facts = _oversized("C_stack_deep", 3 * n_cl * m + 700, high)
    assert w["brute"] - w["brute_lds"] >= 4 and w["brute_lds"] >= 2 and w["sizes"][3 * m] == n_cl
    return sc, facts


@case("C_reentry", "C")
def _c_reentry():
    rng = _rng("C_reentry")
    sizes = [kFastUnit - 1, kFastUnit + 1, kFastUnit + 1, kFastUnit - 1, kFastUnit]
    high = lambda m: np.concatenate([cluster_keys(sizes, rng, jitter=1), filler_keys(m - sum(sizes), rng, BASE + 128 * STEP)])
    sc, _, w, facts = _oversized("C_reentry", sum(sizes) + 700, high)
    # popped buckets on both sides of the lds_level re-entry (kSmallLong, kFastUnit]
    assert {kFastUnit - 1, kFastUnit, kFastUnit + 1} <= set(w["popped"])
    facts["popped"] = sorted(p for p in w["popped"] if p > kSmallLong)[-6:]
    return sc, facts


def _d(name, n, pigeonhole):
    @case(name, "D")
    def build():
        rng = _rng(name)
        sc = cover_scene(uniform_keys(n, rng), 1, 1, capacity=n)
        assert variant(n, 1) == "long" and sample_plan(n)[2] == kMaxUnits and n > kMaxUnits * kUnit
        facts = dict(variant="long", n=n, units=kMaxUnits)
        if pigeonhole:
            assert n > kMaxUnits * kFastUnit                             # some unit exceeds the LDS list whatever the sample
        sizes = units_ungrouped(composites(sc[2], np.arange(n)))
        assert sizes.sum() == n and sizes.min() >= 1 and (not pigeonhole or sizes.max() > kFastUnit)
        facts.update(max_unit=int(sizes.max()), units_over_lds=int((sizes > kFastUnit).sum()))
        return sc, facts


_d("D_clamp", kMaxUnits * kUnit + 1, False)
_d("D_pigeonhole", kMaxUnits * kFastUnit + 257, True)


def _short_scene(keys_lists):
    """Lists inside tiles 1.. of an 8 x 4 grid at the short form's edge (capacity = SHORT_AVG per tile exactly)."""
    cap = SHORT_AVG * 32
    assert sum(len(k) for k in keys_lists) <= cap and variant(cap, 32) == "short"
    sc = inside_scene(keys_lists, 8, 4, cap)
    return sc, tile_lists(sc)[1:len(keys_lists) + 1]


_SIZES = [kSmall, kSmall + 1, kSmallLong, kSmallLong + 1, kAdapt, kAdapt + 1]


@case("E_stack_short", "E")
def _e_stack_short():
    rng = _rng("E_stack_short")
    sc, (l,) = _short_scene([cluster_keys([kSmall + 1] * (kStack + 4), rng, jitter=1)])
    w = walk(l, BUCKETS_MAIN["short"], kSmall)
    assert len(l) > kFastShort and w["brute"] >= 4 and min(w["brute_sizes"]) > kSmall
    return sc, dict(variant="short", n=len(l), levels=w["levels"], brute=w["brute"], path="generic loop")


@case("E_sizes_short", "E")
def _e_sizes_short():
    rng = _rng("E_sizes_short")
    sc, (a, b) = _short_scene([cluster_keys(_SIZES, rng), cluster_keys(_SIZES + _SIZES, rng)])
    wa, wb = walk(a, BUCKETS_MAIN["short"], kSmall), walk(b, BUCKETS_MAIN["short"], kSmall)
    assert len(a) <= kFastShort < len(b)
    for w, mult in ((wa, 1), (wb, 2)):                                   # level 0: every cluster alone in its bucket
        assert all(w["sizes"][s] >= mult for s in _SIZES)
    return sc, dict(variant="short", lists=[len(a), len(b)], bucket_sizes=sorted(set(wa["sizes"]))[-6:],
                    path="lds_level (first list), generic loop (second)")


@case("E_sizes_units", "E")
def _e_sizes_units():
    rng = _rng("E_sizes_units")
    sizes = _SIZES * 3
    high = lambda m: np.concatenate([cluster_keys(sizes, rng), filler_keys(m - sum(sizes), rng, BASE + 128 * STEP)])
    sc, _, w, facts = _oversized("E_sizes_units", kFastUnit + sum(sizes) + 500, high)
    assert all(w["sizes"][s] >= 3 for s in _SIZES)
    assert {kSmallLong + 1} <= set(w["popped"]) and kSmallLong not in w["popped"][1:]
    return sc, facts


def _adapt_list(n, cluster, rng):
    """n entries: evenly spaced distinct keys but for `cluster` bit-identical ones in the middle."""
    k = (BASE + np.arange(n, dtype=np.int64) * 4096).astype(np.uint32)
    k[n // 2:n // 2 + cluster] = k[n // 2]
    return rng.permutation(k)


def _fullest_bucket(l):
    u, nb = unit_of(l)
    assert nb == 2 and np.bincount(u).max() <= kFastUnit
    return max(int(level_buckets(l[u == j], BUCKETS_UNIT)[0].max()) for j in range(nb))


def _adapt_list_for(n, target, tile, seed):
    """_adapt_list whose fullest bit-field bucket over its units holds exactly `target` entries (the cluster shares its
    bucket with a few of the evenly spaced keys: the cluster is shortened by that many)."""
    for cluster in range(target, target - 8, -1):
        keys = _adapt_list(n, cluster, np.random.default_rng(seed))
        # (the list's ids are those of its place in the scene: tile 1's Gaussians come first)
        if _fullest_bucket(composites(keys, np.arange(n) + (tile - 1) * n)) == target:
            return keys
    raise AssertionError(f"no cluster leaves a fullest bucket of {target}")


@case("E_adapt_units", "E")
def _e_adapt_units():
    """Two deferred lists of two units each: the fullest bit-field bucket of any unit holds exactly kAdapt entries in
    the first (no splitters) and kAdapt + 1 in the second (the unit switches to splitters)."""
    n = kFastLong + 100
    sc = inside_scene([_adapt_list_for(n, kAdapt, 1, 11), _adapt_list_for(n, kAdapt + 1, 2, 12)], 2, 2, 2 * n + 16)
    assert variant(sc[5], 4) == "long"
    fullest = [_fullest_bucket(l) for l in tile_lists(sc)[1:3]]
    assert fullest == [kAdapt, kAdapt + 1]
    return sc, dict(variant="long", lists=[n, n], fullest_bucket=fullest, path="units' lds_level: bit field / splitters")


def _window_sizes(ksm, n_clusters):
    return [ksm - (0, 3, 1, 8, 5)[j % 5] for j in range(n_clusters)]


@case("E_window_short", "E")
def _e_window_short():
    rng = _rng("E_window_short")
    sc, (l,) = _short_scene([cluster_keys(_window_sizes(kSmall, 40), rng, jitter=1)])
    win = window(kFastShort, True)
    across = straddled_windows(l, BUCKETS_MAIN["short"], win)
    w = walk(l, BUCKETS_MAIN["short"], kSmall)
    assert len(l) > 4 * win and w["levels"] == 1 and len(across) >= 4 and min(across) >= kSmall - 8
    return sc, dict(variant="short", n=len(l), window=win, straddling_buckets=across, path="generic loop, windows")


@case("E_window_units", "E")
def _e_window_units():
    rng = _rng("E_window_units")
    sizes = _window_sizes(kSmallLong, 40)
    sc, unit, w, facts = _oversized("E_window_units", sum(sizes) + 400, lambda m: np.concatenate(
        [cluster_keys(sizes, rng, jitter=1), filler_keys(m - sum(sizes), rng, BASE + 128 * STEP)]))
    win = window(kFastUnit, False)
    across = straddled_windows(unit, BUCKETS_UNIT, win)
    assert len(unit) > 2 * win and w["levels"] == 1 and len(across) >= 2 and min(across) >= kSmallLong - 8
    facts.update(window=win, straddling_buckets=across)
    return sc, facts


def _outlier_clusters(rng, size):
    k = np.concatenate([np.full(size, 0x40800100 + 0x4000 * j, np.int64) + rng.integers(-1, 2, size=size) for j in range(4)])
    return rng.permutation(k).astype(np.uint32)


@case("E_outliers_short", "E")
def _e_outliers_short():
    rng = _rng("E_outliers_short")
    k = np.concatenate([[0x00000001], _outlier_clusters(rng, 300), [0x7f7fffff]]).astype(np.uint32)
    sc, (l,) = _short_scene([k])
    w = walk(l, BUCKETS_MAIN["short"], kSmall)
    assert len(l) > kFastShort and w["levels"] >= 3 and max(w["popped"][1:]) == 1200       # the clusters share a bucket
    return sc, dict(variant="short", n=len(l), levels=w["levels"], path="generic loop, a level per ten bits")


@case("E_outliers_units", "E")
def _e_outliers_units():
    rng = _rng("E_outliers_units")
    high = lambda m: np.concatenate([_outlier_clusters(rng, (m - 1) // 4), filler_keys((m - 1) % 4, rng, 0x41000000),
                                     [0x7f7fffff]]).astype(np.uint32)
    bits_fn = lambda n: biased_sample_keys(n, high, low=0x00000100)
    n = 9_000
    sc = cover_scene(bits_fn(n), 2, 1)
    l = tile_lists(sc)[0]
    u, nb = unit_of(l)
    sizes = np.bincount(u, minlength=nb)
    w = walk(l[u == nb - 1], BUCKETS_UNIT, kSmallLong)
    assert sizes[-1] > kFastUnit and w["levels"] >= 3
    return sc, dict(variant="long", n=n, units=nb, max_unit=int(sizes[-1]), levels=w["levels"])


def _f_bits(v, b):
    name = f"F_low{b}_{v}"

    @case(name, "F")
    def build():
        rng = _rng(name)
        f = KFAST[v]
        lens = [f, 2 * f + 3]
        keys = [(0x40000000 | rng.integers(0, 1 << b, size=n)).astype(np.uint32) for n in lens]
        for k in keys:
            k[:2] = 0x40000000, 0x40000000 | ((1 << b) - 1)              # the whole field is used
        if v == "short":
            sc = inside_scene(keys, 4, 2, SHORT_AVG * 8)
        else:
            sc = inside_scene(keys, 2, 2, sum(lens) + 16)
        assert variant(sc[5], sc[3] * sc[4]) == v
        lists = tile_lists(sc)[1:3]
        shifts = [level_buckets(l, BUCKETS_MAIN[v])[1] for l in lists]
        assert all(int(l.min() ^ l.max()) >> 32 == (1 << b) - 1 for l in lists)
        facts = dict(variant=v, lists=lens, low_bits=b, shift_main=shifts[0])
        if v == "long":                                                 # the second list is deferred: its units' shifts
            u, nb = unit_of(lists[1])
            facts["shift_units"] = sorted({level_buckets(lists[1][u == j], BUCKETS_UNIT)[1] for j in range(nb)})
        return sc, facts


for _v in ("short", "long"):
    for _b_ in (1, 5, 9, 10):
        _f_bits(_v, _b_)


def _f_ids(v, high):
    name = f"F_ids_{'high' if high else 'low'}_{v}"

    @case(name, "F")
    def build():
        f = KFAST[v]
        # all depths equal.  high: ids are multiples of 128 (everything between is culled); low: the first list's ids are
        # 0 .. 299 (they differ below the digit: the shift clamps at 0), the second's two neighbours
        lens = [f - 24, f + 476, 2 * f + 100] if high else [300, 2, f + 176]
        stride = 128 if high else 1
        keys = [equal_keys(n) for n in lens]
        if v == "short":
            sc = inside_scene(keys, 4, 2, SHORT_AVG * 8, stride=stride)
        else:
            sc = inside_scene(keys, 2, 2, max(sum(lens) + 16, MID_AVG * 4 + 1), stride=stride)
        assert variant(sc[5], sc[3] * sc[4]) == v
        lists = tile_lists(sc)[1:4]
        assert [len(l) for l in lists] == lens
        x = [int(l.min() ^ l.max()) for l in lists]
        assert all(d < (1 << 32) for d in x)                             # the depths are alike: the ids decide
        if high:
            assert all(int(l[0] | np.bitwise_or.reduce(l)) & 127 == 0 for l in lists)
        else:
            assert x[0] < 512 and x[1] == 1
        return sc, dict(variant=v, lists=lens, id_stride=stride, shifts=[level_buckets(l, BUCKETS_MAIN[v])[1] for l in lists])


for _v in ("short", "long"):
    for _h in (True, False):
        _f_ids(_v, _h)


def _g(v):
    name = f"G_keys_{v}"

    @case(name, "G")
    def build():
        rng = _rng(name)
        f = KFAST[v]
        lens = [f, 3 * f + 5]
        keys = [any_bits_keys(n, rng) for n in lens]
        tw, th = {"short": (4, 2), "mid": (4, 2), "long": (2, 2)}[v]
        cap = SHORT_AVG * tw * th if v == "short" else sum(lens) + 16
        sc = inside_scene(keys, tw, th, cap)
        assert variant(cap, tw * th) == v and cap >= sum(lens)
        for l in tile_lists(sc)[1:3]:
            assert set(PLANTED) <= set((l >> np.uint64(32)).astype(np.uint32).tolist())
        assert (sc[2][-5:] == 0xffffffff).all()                          # the Gaussians of highest index
        return sc, dict(variant=v, lists=lens, path="lds_level; " + ("generic loop" if v == "short" else "units"))


for _v in KFAST:
    _g(_v)


# ---- H: the same lists with too small a capacity ------------------------------------------------------------------------
def overflow_scenes():
    """name -> scene with room to spare (the test shrinks the capacity): C's biased-sample list, and B's mix of lists
    below and at / above kBigList."""
    return {"biased": CASES["C_biased"][1]()[0], "bigmix": CASES["B_long_tight"][1]()[0]}


# one case per family also runs on the shipped library, no knob
SHIPPED = ("A_short_uniform", "B_mid_tight", "C_stack", "D_pigeonhole", "E_sizes_units", "F_low9_long", "G_keys_long")
