"""register_points on the GPU (include/mgs_register.h, csrc/register.hip, robosimgs_amd/registration.py) against the fp64
statement of tests/register_ref.py.

Correspondences are compared EXACTLY.  What makes that fair is the separation condition every case asserts first, on the
statement alone: for each source point and each iteration the fp64 gap between the best and the second-best distinct
distance, and between the best distance and max_distance, exceeds 1e-5, while the kernel's fp32 difference form is off by
under 1e-6 at these coordinate magnitudes (|x| <= 4: test_gpu_hinge.py's count) plus one rounding of p' (2.4e-7 per
coordinate).  A point inside either gap is "undecided": it may receive any of its near-tied candidates, and a case allows at
most 0.5 % of them (the seeds below give none where a count is compared).  distance2 is held to the counted bound
2 max_distance (sqrt(3) 2^-22) + 4 * 2^-24 max_distance^2: p' a rounding apart, and the three roundings of the form.  The
transform, rmse and history are held to 1e-9, the project's bound for fp64 moments about a pivot (both sides read the same
fp32 points; only summation order and the 3x3 solver differ).
"""
import os
import re

import numpy as np
import pytest
import torch

import register_ref as RR

pytestmark = pytest.mark.gpu
DEV = "cuda"
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = open(os.path.join(ROOT, "robosimgs_amd", "csrc", "register.hip")).read()
G = int(re.search(r"constexpr\s+int\s+kRegisterGroup\s*=\s*(\d+)\s*;", SRC).group(1))
MAX_CELLS = 1 << int(re.search(r"constexpr\s+int\s+kRegisterMaxCells\s*=\s*1\s*<<\s*(\d+)\s*;", SRC).group(1))
TOL = 1e-9


@pytest.fixture(scope="module")
def reg():
    from robosimgs_amd import registration
    return registration


def rot(axis, degrees):
    a = np.asarray(axis, np.float64) / np.linalg.norm(axis)
    K = np.array([[0, -a[2], a[1]], [a[2], 0, -a[0]], [-a[1], a[0], 0]])
    t = np.radians(degrees)
    return np.eye(3) + np.sin(t) * K + (1 - np.cos(t)) * K @ K


def inverse(T, X):
    s, R, t = T
    return ((np.asarray(X, np.float64) - t) @ R) / s


def d2_bound(md):
    return 2 * md * np.sqrt(3.0) * 2.0**-22 + 4 * 2.0**-24 * md * md


def run(reg, P, Q, md, **kw):
    """One call with correspondences; everything read back."""
    r = reg.register_points(torch.from_numpy(np.ascontiguousarray(P)).to(DEV), torch.from_numpy(np.ascontiguousarray(Q)).to(DEV),
                            md, return_correspondence=True, **kw)
    return r, r.correspondence.cpu().numpy(), r.distance2.cpu().numpy()


def check_matching(ref_c, ref_d2, T, P, Q, md, c, d2, what):
    """Decided points exactly, undecided ones among their candidates; returns the number of undecided points."""
    undecided, cand = RR.separation(T, P, Q, md)
    n_und = int(undecided.sum())
    assert n_und <= 0.005 * len(P), f"{what}: {n_und} of {len(P)} source points are undecided: another seed"
    dec = ~undecided
    wrong = int((c[dec] != ref_c[dec]).sum())
    both = dec & (ref_c >= 0) & (c >= 0)
    err = float(np.abs(d2[both].astype(np.float64) - ref_d2[both].astype(np.float64)).max()) if both.any() else 0.0
    print(f"\n{what}: {int((ref_c >= 0).sum())} inliers of {len(P)}, {n_und} undecided, {wrong} wrong, distance2 error {err:.2e} "
          f"(bound {d2_bound(md):.2e})")
    assert wrong == 0
    assert err <= d2_bound(md)
    assert np.isinf(d2[c < 0]).all() and (d2[c >= 0] <= RR.limit2_of(md)).all()
    for i in np.flatnonzero(undecided):
        assert int(c[i]) in cand[int(i)], (i, c[i], cand[int(i)])
    return n_und


# ---- 1. matching only ---------------------------------------------------------------------------------------------------------
T0 = (1.04, rot([0.2, 1.0, -0.4], 6.0), np.array([0.11, -0.07, 0.05]))
MD_SMALL, MD_ONE = 0.03, 0.3


def matching_case(n_s, n_t, seed):
    """(P, Q, max_distance, init).  n_t = 4099: targets fill [-3.2, 3.2]^3 and max_distance 0.03 asks for 214^3 cells, more
    than the table has, so the edge grows (asserted); sources are given in the frame T0 maps onto the target's.  n_t = 1, 2: a
    one-cell grid, identity init, and for 2 the same point twice.  The source pool, in the target's frame: points planted
    within 1.5 max_distance of a target (two thirds inliers), points at random, and -- from 63 sources up -- two outside the
    grid on each of its six sides (by 0.4 and by 2 max_distance beyond the extreme target), points on cell faces of each
    axis, points next to a duplicated target, and two non-finite rows."""
    rng = np.random.default_rng(seed)
    if n_t == 4099:
        md, init = MD_SMALL, T0
        Q = rng.uniform(-3.2, 3.2, (n_t, 3))
        Q[100] = Q[50]
        Q[4098] = Q[50]                                      # three copies: index 50 must win
        Q[2000] = Q[1999]
        Q = Q.astype(np.float32)
        Q[7, 0], Q[3000, 2], Q[4097, 1] = np.nan, np.inf, -np.inf
    else:
        md, init = MD_ONE, None
        Q = np.repeat(rng.uniform(-1.0, 1.0, (1, 3)), n_t, 0).astype(np.float32)
    fin = np.flatnonzero(RR.finite_rows(Q))
    Qd = Q[fin].astype(np.float64)

    def near(rows, lo=0.0, hi=1.5):
        d = rng.normal(size=(len(rows), 3))
        d *= (rng.uniform(lo, hi, len(rows)) * md / np.linalg.norm(d, axis=1))[:, None]
        return Qd[rows] + d

    special = []
    if n_s >= 63:
        for a in range(3):
            for row, sign in ((int(np.argmin(Qd[:, a])), -1.0), (int(np.argmax(Qd[:, a])), 1.0)):
                for by in (0.4, 2.0):
                    p = Qd[row].copy()
                    p[a] += sign * by * md
                    special.append(p)
        grid = RR.grid_make(Q, md, MAX_CELLS)
        for a in range(3):
            for k in (1, grid.dims[a] // 2, grid.dims[a]):
                p = near(rng.integers(0, len(Qd), 1), 0.0, 0.8)[0]
                p[a] = grid.origin[a] + k * grid.h
                special.append(p)
        if n_t == 4099:
            dup = np.searchsorted(fin, [50, 50, 1999, 50])
            special += list(near(dup, 0.05, 0.6))
    pool = np.array(special).reshape(-1, 3)
    n_rest = n_s - len(pool)
    n_planted = (2 * n_rest + 2) // 3
    pool = np.concatenate([pool, near(rng.integers(0, len(Qd), n_planted)),
                           rng.uniform(Qd.min(0) - 3 * md, Qd.max(0) + 3 * md, (n_rest - n_planted, 3))])
    pool = pool[rng.permutation(n_s)]
    P = (pool if init is None else inverse(init, pool)).astype(np.float32)
    if n_s >= 63:
        P[5, 1], P[n_s - 2, 0] = np.nan, np.inf
    return P, Q, md, init


MATCH_SEED = 2          # with it no case has an undecided point (asserted)
MATCH_SHAPES = [(n_s, n_t) for n_s in (1, 63, 65, G + 1, 1000) for n_t in (1, 2, 4099)]


@pytest.mark.parametrize("n_s,n_t", MATCH_SHAPES)
def test_matching_only(reg, n_s, n_t):
    P, Q, md, init = matching_case(n_s, n_t, seed=MATCH_SEED + 1000 * n_s + n_t)
    assert np.abs(P[np.isfinite(P)]).max() <= 4.0 and np.abs(Q[np.isfinite(Q)]).max() <= 4.0
    ref = RR.icp(P, Q, md, iterations=0, init=init)
    r, c, d2 = run(reg, P, Q, md, iterations=0, init=None if init is None else (init[1], init[2], init[0]))
    n_und = check_matching(ref.correspondence, ref.distance2, ref.T, P, Q, md, c, d2, f"{n_s} x {n_t}")
    assert r.iterations == 0 and not r.converged and r.history.shape == (0, 4)
    assert r.flags == ref.flags == (RR.FLAG_NONFINITE if (n_s >= 63 or n_t == 4099) else 0)
    assert n_und == 0                                      # the seeds: so that the counts can be compared
    assert r.n_inliers == ref.n_inliers == int((c >= 0).sum()) and r.fitness == ref.fitness
    assert abs(r.rmse - ref.rmse) <= TOL
    assert r.scale == ref.scale and np.array_equal(r.rotation, ref.rotation) and np.array_equal(r.translation, ref.translation)
    grid = RR.grid_make(Q, md, MAX_CELLS)
    assert r.grid_dims == grid.dims and r.cell_edge == grid.h and np.array_equal(r._host()[23:], np.zeros(9))
    if n_t == 4099:
        assert r.cell_edge > 1.2 * md and ref.n_inliers > 0.3 * n_s       # the cap set the edge; the search still finds them
        if n_s >= 63:
            assert (c == 50).any() and (c == 1999).any() and not np.isin(c, [100, 4098, 2000, 7, 3000, 4097]).any()
    else:
        assert r.grid_dims == (1, 1, 1) and (c <= 0).all()              # a duplicate: the lowest index, exactly


def test_a_source_with_no_target_in_reach(reg):
    P, Q, md, init = matching_case(1000, 4099, seed=77)
    P = (P + np.float32(0.5)).astype(np.float32)
    P[:, 0] = np.float32(3.9)                                # a sheet beyond the targets' bounds (3.2) by 23 radii
    ref = RR.icp(P, Q, md, iterations=3)
    assert ref.n_inliers == 0 and ref.flags == RR.FLAG_NONFINITE | RR.FLAG_UNDETERMINED and ref.iterations == 1
    r, c, d2 = run(reg, P, Q, md, iterations=3)
    assert (c == -1).all() and np.isinf(d2).all()
    assert r.n_inliers == 0 and r.fitness == 0.0 and r.rmse == 0.0 and r.flags == ref.flags and r.iterations == 1
    assert np.array_equal(r.matrix(), np.eye(4)) and not r.converged
    assert np.array_equal(r.history, [[0.0, 0.0, 1.0, 0.0]])


# ---- 2. one update from planted correspondences --------------------------------------------------------------------------------
PLANT = (1.03, rot([0.3, -0.5, 0.8], 10.0), np.array([0.05, -0.02, 0.03]))


RIGID_PLANT = (1.0, PLANT[1], PLANT[2])


def planted_case(kind, plant=PLANT, seed=5, n=300):
    """Targets that are the images of the sources under `plant`, rounded to fp32 and shuffled; `init` is the plant, so that
    every source meets its own image (1e-7 away, the next target 0.01 or more)."""
    rng = np.random.default_rng(seed)
    if kind == "volume":
        P = rng.uniform(-2.0, 2.0, (n, 3))
    elif kind == "coplanar":
        P = np.c_[rng.uniform(-2.0, 2.0, (n, 2)), np.full(n, 0.75)]
    elif kind == "collinear":
        P = np.array([1.0, -0.5, 0.25]) + np.outer(np.linspace(-1.5, 1.5, n), [0.6, 0.64, -0.48])
    elif kind == "two":
        P = rng.uniform(-2.0, 2.0, (n, 3))
    P = P.astype(np.float32)
    Q = RR.apply(plant, P).astype(np.float32)
    if kind == "two":
        Q[2:] += np.float32(0.5)                             # all but two images are out of reach
    order = rng.permutation(n)
    return P, Q[order], order


@pytest.mark.parametrize("kind", ["volume", "coplanar"])
@pytest.mark.parametrize("with_scale", [False, True])
def test_one_update_from_planted_correspondences(reg, kind, with_scale):
    plant = PLANT if with_scale else RIGID_PLANT        # a rigid fit of a rigid plant, a similarity fit of a similarity
    P, Q, order = planted_case(kind, plant)
    md = 0.01
    ref = RR.icp(P, Q, md, iterations=1, with_scale=with_scale, init=plant)
    und, _ = RR.separation(plant, P, Q, md)
    assert not und.any() and np.array_equal(order[ref.matchings[0]], np.arange(len(P)))     # each source met its own image
    assert ref.iterations == 1 and ref.flags == 0
    r, c, d2 = run(reg, P, Q, md, iterations=1, with_scale=with_scale, init=(plant[1], plant[2], plant[0]))
    err = dict(R=np.abs(r.rotation - ref.rotation).max(), t=np.abs(r.translation - ref.translation).max(), s=abs(r.scale - ref.scale),
               rmse0=abs(r.history[0, 1] - ref.history[0, 1]))
    print(f"\n{kind}, with_scale {with_scale}: " + ", ".join(f"{k} {v:.2e}" for k, v in err.items()) + f", scale {r.scale:.9f}")
    assert max(err.values()) <= TOL
    R = r.rotation
    assert abs(np.linalg.det(R) - 1.0) <= 1e-12 and np.abs(R @ R.T - np.eye(3)).max() <= 1e-12      # proper, coplanar included
    assert r.iterations == 1 and r.flags == 0 and not r.converged and r.history.shape == (1, 4)
    assert r.history[0, 0] == len(P) and r.history[0, 2] == plant[0] and r.history[0, 3] == 0.0
    assert (r.scale == 1.0) if not with_scale else abs(r.scale - PLANT[0]) < 1e-6
    assert np.abs(r.rotation - plant[1]).max() < 1e-6 and np.abs(r.translation - plant[2]).max() < 1e-6
    und1, _ = RR.separation(ref.T, P, Q, md)
    assert not und1.any() and np.array_equal(c, ref.correspondence) and r.n_inliers == len(P)


@pytest.mark.parametrize("kind", ["collinear", "two"])
def test_an_undetermined_rotation_sets_the_flag_and_leaves_the_transform(reg, kind):
    P, Q, order = planted_case(kind)
    md = 0.01
    init = (PLANT[1], PLANT[2], PLANT[0])
    ref = RR.icp(P, Q, md, iterations=4, with_scale=True, init=PLANT)
    assert ref.flags == RR.FLAG_UNDETERMINED and ref.iterations == 1 and ref.n_inliers == (2 if kind == "two" else len(P))
    sentinel = torch.full((4, 4), -7.0, dtype=torch.float64, device=DEV)
    result = reg.register_icp_raw(torch.from_numpy(P).to(DEV), torch.from_numpy(Q).to(DEV), md, 4, True, 1e-6,
                                  torch.from_numpy(reg.pack_init(init)).to(DEV), history=sentinel)
    r = reg.Registration(result, sentinel)
    assert r.flags == 1 and r.iterations == 1 and not r.converged and r.n_inliers == ref.n_inliers
    assert np.array_equal(r._host()[:13], reg.pack_init(init))                     # T as it was, bit for bit
    h = sentinel.cpu().numpy()
    assert (h[1:] == -7.0).all() and h[0, 0] == ref.n_inliers and abs(h[0, 1] - ref.history[0, 1]) <= TOL
    assert abs(r.rmse - ref.rmse) <= TOL


# ---- 3. a full run ---------------------------------------------------------------------------------------------------------------
def l_solid_surface(rng, n):
    """n points on the surface of an L-shaped solid with a step on one arm (no symmetry): the union of three boxes, sampled
    per box face by area, points inside another box dropped."""
    boxes = np.array([[[0.0, 0.0, 0.0], [2.4, 0.8, 0.7]], [[0.0, 0.8, 0.0], [0.8, 2.0, 0.7]], [[1.6, 0.0, 0.7], [2.4, 0.8, 1.1]]])
    out = []
    while sum(map(len, out)) < n:
        b = boxes[rng.integers(0, len(boxes))]
        ext = b[1] - b[0]
        areas = np.array([ext[1] * ext[2], ext[0] * ext[2], ext[0] * ext[1]])
        a = rng.choice(3, p=areas / areas.sum())
        p = b[0] + rng.random(3) * ext
        p[a] = b[rng.integers(0, 2)][a]
        inside = [(p > o[0] + 1e-9).all() and (p < o[1] - 1e-9).all() for o in boxes]
        if not any(inside):
            out.append(p[None])
    return np.concatenate(out)[:n] - [1.2, 1.0, 0.5]


FULL_MD, FULL_SIZE = 0.5, 2.9
FULL_SEEDS = {True: 20, False: 73}        # per with_scale: seeds whose run has no undecided point at any iteration (asserted)


def full_case(seed):
    """3,000 target points on the L-shaped solid (6.96 x 5.8 x 3.19) and 2,000 source points: 1,400 of them are target points
    seen again with noise 0.002, 600 lie on a patch the target does not have; the source is PLANT's pre-image (10 degrees,
    0.05, 1.03).  The size matters: the chance that a point sits within 1e-5 of a tie between two targets falls with it."""
    rng = np.random.default_rng(seed)
    Q = l_solid_surface(rng, 3000) * FULL_SIZE
    shared = Q[rng.permutation(3000)[:1400]] + rng.normal(0, 0.002, (1400, 3))
    extra = np.c_[rng.uniform(-2.0, 2.0, (600, 2)), np.full(600, 3.0)] + rng.normal(0, 0.002, (600, 3))
    world = np.concatenate([shared, extra])[rng.permutation(2000)]
    return inverse(PLANT, world).astype(np.float32), Q.astype(np.float32)


@pytest.fixture(scope="module")
def full():
    """{with_scale: (P, Q, the statement's run of 30 iterations at tol 1e-6)}"""
    out = {}
    for ws, seed in FULL_SEEDS.items():
        P, Q = full_case(seed)
        out[ws] = (P, Q, RR.icp(P, Q, FULL_MD, iterations=30, with_scale=ws, tol=1e-6))
    return out


@pytest.mark.parametrize("with_scale", [False, True])
def test_full_run_follows_the_statement_at_every_iteration(reg, full, with_scale):
    P, Q, ref = full[with_scale]
    assert np.abs(P).max() <= 4.0 and np.abs(Q).max() <= 4.0
    for k, T in enumerate(ref.transforms):
        und, _ = RR.separation(T, P, Q, FULL_MD)
        assert not und.any(), f"pass {k}: {int(und.sum())} undecided points: another seed"
    sentinel = torch.full((30, 4), -7.0, dtype=torch.float64, device=DEV)
    tp, tq = torch.from_numpy(P).to(DEV), torch.from_numpy(Q).to(DEV)
    c = torch.empty(len(P), dtype=torch.int32, device=DEV)
    d2 = torch.empty(len(P), dtype=torch.float32, device=DEV)
    r = reg.Registration(reg.register_icp_raw(tp, tq, FULL_MD, 30, with_scale, 1e-6, None, c, d2, sentinel), sentinel, c, d2)
    m = ref.iterations
    err = dict(R=np.abs(r.rotation - ref.rotation).max(), t=np.abs(r.translation - ref.translation).max(), s=abs(r.scale - ref.scale),
               rmse=abs(r.rmse - ref.rmse), history=np.abs(r.history - ref.history[:m]).max())
    print(f"\nwith_scale {with_scale}: {m} iterations, converged {ref.converged}, inliers {ref.history[0, 0]:.0f} -> {ref.n_inliers}, "
          f"rmse {ref.history[0, 1]:.4f} -> {ref.rmse:.4f}, scale {ref.scale:.5f}; " + ", ".join(f"{k} {v:.2e}" for k, v in err.items()))
    assert r.iterations == m and r.converged == ref.converged and r.flags == ref.flags == 0
    assert np.array_equal(r.history[:, 0], ref.history[:m, 0])                 # the inlier count of every iteration
    assert (sentinel.cpu().numpy()[m:] == -7.0).all()
    assert max(err.values()) <= TOL
    assert r.n_inliers == ref.n_inliers and r.fitness == ref.fitness
    assert np.array_equal(c.cpu().numpy(), ref.correspondence)
    # the matching of every iteration: a call of k iterations ends with the pass under T_k
    for k in range(m):
        rk, ck, _ = run(reg, P, Q, FULL_MD, iterations=k, with_scale=with_scale, tol=1e-6)
        assert rk.iterations == k and np.array_equal(ck, ref.matchings[k]), k
    # and the alignment itself: the planted similarity, as well as 1,400 noisy points against 3,000 others show it
    ang = np.degrees(np.arccos(np.clip((np.trace(r.rotation @ PLANT[1].T) - 1) / 2, -1, 1)))
    print(f"against the plant: {ang:.3f} degrees, translation {np.abs(r.translation - PLANT[2]).max():.4f}, scale {r.scale:.4f}")
    if with_scale:
        assert ang < 1.0 and np.abs(r.translation - PLANT[2]).max() < 0.02 and abs(r.scale - PLANT[0]) < 0.01


# ---- 4. early stop ---------------------------------------------------------------------------------------------------------------
def test_early_stop_is_the_shorter_run_bit_for_bit(reg, full):
    P, Q, _ = full[True]
    tol = 0.12                                               # the rmse falls by 11 % in the second iteration and by more after it
    ref = RR.icp(P, Q, FULL_MD, iterations=30, with_scale=True, tol=tol)
    m = ref.iterations
    assert ref.converged and 2 <= m < 30
    prev, last = ref.history[m - 2, 1], ref.history[m - 1, 1]
    assert abs(abs(last - prev) - tol * prev) > 1e-6 * prev                    # the stop rule itself is decided by a margin
    for T in ref.transforms:
        assert not RR.separation(T, P, Q, FULL_MD)[0].any()
    tp, tq = torch.from_numpy(P).to(DEV), torch.from_numpy(Q).to(DEV)

    def call(iterations):
        hist = torch.full((iterations, 4), -7.0, dtype=torch.float64, device=DEV)
        c = torch.empty(len(P), dtype=torch.int32, device=DEV)
        d2 = torch.empty(len(P), dtype=torch.float32, device=DEV)
        res = reg.register_icp_raw(tp, tq, FULL_MD, iterations, True, tol, None, c, d2, hist)
        return res.cpu().numpy(), hist.cpu().numpy(), c.cpu().numpy(), d2.cpu().numpy()
    long, short = call(30), call(m)
    assert long[0][16] == m and long[0][17] == 1.0 and short[0][16] == m
    assert (long[1][m:] == -7.0).all() and np.abs(long[1][:m] - ref.history[:m]).max() <= TOL
    assert long[0].tobytes() == short[0].tobytes() and long[1][:m].tobytes() == short[1].tobytes()
    assert np.array_equal(long[2], short[2]) and long[3].tobytes() == short[3].tobytes()
    assert np.array_equal(long[2], ref.correspondence)


# ---- 5. the same bytes -----------------------------------------------------------------------------------------------------------
def test_two_runs_are_the_same_bytes_and_a_permuted_target_permutes(reg, full):
    P, Q, _ = full[True]
    kw = dict(iterations=12, with_scale=True, tol=0.0)
    r1, c1, d1 = run(reg, P, Q, FULL_MD, **kw)
    r2, c2, d2 = run(reg, P, Q, FULL_MD, **kw)
    assert torch.equal(r1.result, r2.result) and torch.equal(r1.history_rows, r2.history_rows)
    assert torch.equal(r1.correspondence, r2.correspondence) and torch.equal(r1.distance2, r2.distance2)
    assert r1.iterations == 12 and r1.n_inliers > 1000
    assert len(np.unique(Q, axis=0)) == len(Q)                                  # no duplicated target: no tie to break by index
    perm = np.random.default_rng(8).permutation(len(Q))
    rp, cp, dp = run(reg, P, Q[perm], FULL_MD, **kw)
    assert torch.equal(rp.distance2, r1.distance2) and torch.equal(rp.result, r1.result)
    assert torch.equal(rp.history_rows, r1.history_rows)
    assert np.array_equal(np.where(cp >= 0, perm[np.maximum(cp, 0)], -1), c1)


# ---- 6. graph capture ------------------------------------------------------------------------------------------------------------
def test_register_icp_raw_replays_in_a_graph(reg, full):
    P, Q, _ = full[True]
    P2 = inverse((0.99, rot([1.0, 0.2, 0.1], 3.0), np.array([0.02, 0.01, -0.03])), RR.apply(PLANT, P)).astype(np.float32)
    its, n = 6, len(P)
    eager = []
    for src in (P, P2):
        r, c, d = run(reg, src, Q, FULL_MD, iterations=its, with_scale=True, tol=0.0)
        eager.append((r._host().copy(), r.history.copy(), c, d))
    assert eager[0][0].tobytes() != eager[1][0].tobytes()
    tp, tq = torch.from_numpy(P).to(DEV), torch.from_numpy(Q).to(DEV)
    c = torch.empty(n, dtype=torch.int32, device=DEV)
    d2 = torch.empty(n, dtype=torch.float32, device=DEV)
    hist = torch.zeros((its, 4), dtype=torch.float64, device=DEV)
    result = torch.empty(reg.RESULT_DOUBLES, dtype=torch.float64, device=DEV)
    ws = reg.register_workspace(n, len(Q), its, DEV)
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        args = (tp, tq, FULL_MD, its, True, 0.0, None, c, d2, hist, result)
        reg.register_icp_raw(*args, workspace=ws)
        torch.cuda.synchronize()
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph, stream=s):
            reg.register_icp_raw(*args, workspace=ws)
        for k in (1, 0):
            tp.copy_(torch.from_numpy((P, P2)[k]).to(DEV))
            ws.fill_(0x5A)                          # nothing in the workspace outlives a call
            graph.replay()
            torch.cuda.synchronize()
            assert result.cpu().numpy().tobytes() == eager[k][0].tobytes(), k
            assert hist.cpu().numpy().tobytes() == eager[k][1].tobytes()
            assert np.array_equal(c.cpu().numpy(), eager[k][2]) and d2.cpu().numpy().tobytes() == eager[k][3].tobytes()
    torch.cuda.synchronize()


# ---- 7. Registration.apply -------------------------------------------------------------------------------------------------------
def test_registration_apply_is_transform_gaussians(reg, full):
    from robosimgs_amd import transform_gaussians
    P, Q, _ = full[True]
    r, _, _ = run(reg, P, Q, FULL_MD, iterations=5, with_scale=True)
    n = len(P)
    gen = torch.Generator(device=DEV).manual_seed(3)
    quats = torch.nn.functional.normalize(torch.randn(n, 4, device=DEV, generator=gen), dim=1)
    tensors = dict(means=torch.from_numpy(P).to(DEV), quats=quats, scales=torch.rand(n, 3, device=DEV, generator=gen) * 0.05,
                   opacities=torch.full((n,), 0.5, device=DEV), colors=torch.rand(n, 4, 3, device=DEV, generator=gen), sh_degree=1)
    R, t, s = r.pose()
    want = transform_gaussians(tensors, [R], [t], [s])
    got = r.apply(tensors)
    for key in ("means", "quats", "scales", "opacities", "colors"):
        assert torch.equal(got[key], want[key]), key
    moved = got["means"].cpu().numpy().astype(np.float64)
    assert np.abs(moved - RR.apply((s, R, t), P)).max() <= 1e-5
    flat = r.apply(tensors, rotate_sh=False)
    assert torch.equal(flat["colors"], tensors["colors"]) and torch.equal(flat["means"], want["means"])
