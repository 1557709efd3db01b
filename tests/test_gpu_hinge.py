"""The hinge fit on the GPU (include/mgs_hinge.h, csrc/hinge.hip, robosimgs_amd/articulation.py) against the fp64 reference of
tests/hinge_ref.py.

Masks are compared EXACTLY.  What makes that fair is a condition on the input that every case asserts first: `gap`, the
smallest distance of any point's nearest-neighbour distance from the contact limit, is above 1e-5 in fp64, while the
kernel's fp32 difference form and sqrtf are off by under 1e-6 at these coordinate magnitudes (|x| <= 4: a coordinate
difference is rounded to 2^-24 of itself, the three-term sum and the root add as much again).  The record is held to
1e-9 (the fixture's bound, which follows from fp64 accumulation about a pivot: both sides read the same fp32 inputs, so
only summation order and the eigen solver differ, ~1e-12 here); the axis only where the top eigenvalue is separated by
more than 1e-4, because an eigenvector moves by (error of the covariance, ~2e-16 |x - pivot|^2) / (that separation).

Synthetic sets (`two_parts`): the bulk of each part keeps at least 0.2 from the other; h "hinge" points per part sit in
pairs along a line, each within 0.0045 + planted gap of its partner, so they are contact and nothing else is; the closest
pair is planted at the LAST index of both sets (the last partial LDS tile of B, the last partial workgroup of A).
"""
import os
import re

import numpy as np
import pytest
import torch

import hinge_ref as HR

pytestmark = pytest.mark.gpu
DEV = "cuda"
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = open(os.path.join(ROOT, "robosimgs_amd", "csrc", "hinge.hip")).read()
_const = lambda name: int(re.search(r"constexpr\s+\w+\s+%s\s*=\s*(\d+)\s*;" % name, SRC).group(1))
G, T, Q = _const("kHingeGroup"), _const("kHingeTile"), _const("kHingeQueries")
TARGET = _const("kHingeTargetBlocks")
THR = 0.01


@pytest.fixture(scope="module")
def art():
    from robosimgs_amd import articulation
    return articulation


def two_parts(n_a, n_b, seed, gap=0.0, offset=(0.0, 0.0, 0.0)):
    rng = np.random.default_rng(seed)
    h = max(1, min(n_a, n_b, 400) // 2)

    def part(n, sign):
        p = np.empty((n, 3))
        p[:, 0] = sign * rng.uniform(0.1, 1.0, n)
        p[:, 1] = rng.uniform(-0.5, 1.5, n)
        p[:, 2] = rng.uniform(-0.5, 0.5, n)
        rows = np.concatenate([rng.permutation(n - 1)[:h - 1], [n - 1]]).astype(np.int64)     # the planted pair comes last
        s = rng.uniform(0.0002, 0.002, h)
        s[-1] = 0.0
        p[rows, 0] = sign * (gap / 2 + s)
        p[rows, 1] = 0.003 * np.arange(h) + np.where(s > 0, rng.uniform(-0.0005, 0.0005, h), 0.0)
        p[rows, 2] = np.where(s > 0, rng.uniform(-0.0005, 0.0005, h), 0.0)
        return p, rows
    a, rows_a = part(n_a, +1.0)
    b, rows_b = part(n_b, -1.0)
    b[rows_b[:-1], 1] = a[rows_a[:-1], 1] + rng.uniform(-0.0003, 0.0003, h - 1)               # partners share their y
    b[rows_b[-1], 1] = a[rows_a[-1], 1]
    off = np.asarray(offset)
    return (a + off).astype(np.float32), (b + off).astype(np.float32)


def run(art, a, b, thr=THR):
    """One fit with masks; everything read back."""
    ta, tb = torch.from_numpy(np.ascontiguousarray(a)).to(DEV), torch.from_numpy(np.ascontiguousarray(b)).to(DEV)
    h = art.fit_hinge_points(ta, tb, thr, return_contacts=True)
    return h, h.contact_a.cpu().numpy(), h.contact_b.cpu().numpy()


def check(ref, h, ca, cb, what, tol=1e-9):
    assert ref.gap > 1e-5, f"{what}: the input's gap {ref.gap:.2e} does not separate fp32 from fp64"
    wrong = int((ca != ref.contact_a).sum() + (cb != ref.contact_b).sum())
    err = dict(position=float(np.abs(h.position - ref.position).max()), confidence=abs(h.axis_confidence - ref.axis_confidence),
               eigenvalues=float(np.abs(h.eigenvalues - ref.eigenvalues).max()), axis=float(np.abs(h.axis - ref.axis).max()))
    print(f"\n{what}: n_contact {h.n_contact}, min_distance {h.min_distance:.9g}, gap {ref.gap:.2e}, wrong mask bytes {wrong}, "
          + ", ".join(f"{k} {v:.2e}" for k, v in err.items()))
    assert wrong == 0
    assert h.n_contact == ref.n_contact == (int(ca.sum()), int(cb.sum()))
    assert h.fallback == ref.fallback and h.nonfinite == ref.nonfinite
    assert err["position"] <= tol and err["confidence"] <= tol and err["eigenvalues"] <= tol
    if ref.fallback:
        assert h.axis.tolist() == [1.0, 0.0, 0.0]
    elif ref.eigenvalues[2] - ref.eigenvalues[1] > 1e-4:
        assert err["axis"] <= tol                       # the sign too: both follow the rule
    assert abs(np.linalg.norm(h.axis) - 1.0) <= 1e-12
    assert np.array_equal(h._host()[14:], [0.0, 0.0])


# ---- 1. the reference project's open box ---------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def box():
    g = np.load(os.path.join(ROOT, "tests", "golden", "hinge_openbox.npz"))
    return g, HR.fit(g["lid"], g["body"], THR)


def test_open_box_fixture(art, box):
    g, ref = box
    h, ca, cb = run(art, g["lid"], g["body"])
    check(ref, h, ca, cb, "open box")
    assert h.min_distance == 0.0 and h.n_contact == (212, 208) and ref.gap > 1e-4
    assert np.abs(h.position - g["position"]).max() <= 1e-9
    assert abs(h.axis_confidence - float(g["axis_confidence"])) <= 1e-9
    assert abs(1.0 - abs(h.axis @ g["axis"])) <= 1e-9 and np.abs(h.axis + g["axis"]).max() <= 1e-9      # the file has the other sign
    assert h.axis[2] > 0.99 and np.abs(h.to_origin() - g["translation_applied"]).max() <= 1e-9


# ---- 2. every tiling edge ---------------------------------------------------------------------------------------------------
SHAPES = [(1, 1), (1, T + 1), (G - 1, G + 1), (G + 1, 2 * T - 1), (1000, 4099), (G * Q + 1, T + 1)]


@pytest.mark.parametrize("n_a,n_b", SHAPES)
@pytest.mark.parametrize("gap", [0.0, 0.003])
def test_shapes_across_the_tiling_edges(art, n_a, n_b, gap):
    a, b = two_parts(n_a, n_b, seed=n_a + n_b, gap=gap)
    ref = HR.fit(a, b, THR)
    assert ref.contact_a[-1] and ref.contact_b[-1]                       # the planted pair, last in both sets
    h, ca, cb = run(art, a, b)
    check(ref, h, ca, cb, f"{n_a} x {n_b}, planted gap {gap}")
    # parts a known gap apart: the planted coordinates are +-gap/2, whose difference is exact, so the fp32 square and root
    # are within 2 ulp of the fp32 root of the fp64 minimum (0 stays 0)
    want = np.sqrt(np.float32(ref.min2))
    assert abs(np.float32(h.min_distance) - want) <= 2 * np.spacing(want), (h.min_distance, want)
    assert abs(ref.min_distance - gap) < 1e-7


def test_a_split_that_walks_more_than_one_tile(art):
    """Few queries against more tiles than the launch has splits: a workgroup reuses its LDS tile (n_b past TARGET * T)."""
    n_b = TARGET * T + T + 1
    a, b = two_parts(3, n_b, seed=11)
    ref = HR.fit(a, b, THR)
    h, ca, cb = run(art, a, b)
    check(ref, h, ca, cb, f"3 x {n_b}")


# ---- 3. symmetry, order, determinism ----------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def mid():
    a, b = two_parts(1500, 2300, seed=44, gap=0.003, offset=(2.0, -1.0, 3.0))
    return a, b, HR.fit(a, b, THR)


def test_swapping_the_parts_swaps_the_masks(art, mid):
    a, b, ref = mid
    h, ca, cb = run(art, a, b)
    check(ref, h, ca, cb, "a, b")
    s, sa, sb = run(art, b, a)
    assert np.array_equal(sa, cb) and np.array_equal(sb, ca) and s.n_contact == h.n_contact[::-1]
    assert s.min_distance == h.min_distance
    assert np.abs(s.position - h.position).max() <= 1e-12 and np.abs(s.axis - h.axis).max() <= 1e-12
    assert abs(s.axis_confidence - h.axis_confidence) <= 1e-12


def test_two_runs_are_the_same_bytes_and_a_permutation_permutes(art, mid):
    a, b, ref = mid
    h1, ca1, cb1 = run(art, a, b)
    h2, ca2, cb2 = run(art, a, b)
    assert h1._host().tobytes() == h2._host().tobytes() and ca1.tobytes() == ca2.tobytes() and cb1.tobytes() == cb2.tobytes()
    rng = np.random.default_rng(0)
    pa, pb = rng.permutation(len(a)), rng.permutation(len(b))
    hp, cap, cbp = run(art, a[pa], b[pb])
    assert np.array_equal(cap, ca1[pa]) and np.array_equal(cbp, cb1[pb])
    assert hp.min_distance == h1.min_distance and hp.n_contact == h1.n_contact
    assert np.abs(hp._host()[:7] - h1._host()[:7]).max() <= 1e-12 and np.abs(hp.eigenvalues - h1.eigenvalues).max() <= 1e-12


def test_non_finite_rows_take_no_part(art, mid):
    a, b, ref = mid
    clean, ca, cb = run(art, a, b)
    free_a, free_b = np.flatnonzero(~ref.contact_a), np.flatnonzero(~ref.contact_b)          # bulk rows only
    k = int(np.searchsorted(free_b, T)) - 1                                                   # either side of a tile edge
    bad_a, bad_b = free_a[[0, 7, len(free_a) // 2, -1]], free_b[[1, k, k + 1, -1]]
    assert bad_a[0] == 0                           # A's first row: the pivot of the clean run's moments
    a2, b2 = a.copy(), b.copy()
    for k, r in enumerate(bad_a):
        a2[r, k % 3] = (np.nan, np.inf, -np.inf)[k % 3]
    for k, r in enumerate(bad_b):
        b2[r, (k + 1) % 3] = (np.inf, np.nan, -np.inf)[k % 3]
    assert not ca[bad_a].any() and not cb[bad_b].any()
    dirty, da, db = run(art, a2, b2)
    assert not da[bad_a].any() and not db[bad_b].any()
    assert dirty.nonfinite and not clean.nonfinite and int(dirty._host()[13]) & 2
    assert np.array_equal(da, ca) and np.array_equal(db, cb)
    want, got = clean._host().copy(), dirty._host().copy()
    # row 0 of A was the pivot of the clean run's moments: the sums are taken about another point, to 1e-12
    assert np.array_equal(got[7:10], want[7:10]) and np.abs(got[:7] - want[:7]).max() <= 1e-12
    assert np.abs(got[10:13] - want[10:13]).max() <= 1e-12 and int(got[13]) == int(want[13]) | 2
    check(HR.fit(a2, b2, THR), dirty, da, db, "non-finite rows planted")


def test_isotropic_contact_set_falls_back_to_x(art):
    rng = np.random.default_rng(9)
    blob = (rng.normal(size=(600, 3)) * 0.01 + [0.3, -0.2, 1.0]).astype(np.float32)
    a, b = blob[:250], blob[250:]
    ref = HR.fit(a, b, 1.0)                        # every point is contact
    assert ref.fallback and ref.n_contact == (250, 350)
    h, ca, cb = run(art, a, b, 1.0)
    check(ref, h, ca, cb, "isotropic blob")
    assert h.fallback and h.axis.tolist() == [1.0, 0.0, 0.0] and h.axis_confidence < 0.5 and int(h._host()[13]) & 1


# ---- 4. graph capture --------------------------------------------------------------------------------------------------------
def test_hinge_fit_raw_replays_in_a_graph(art):
    n_a, n_b = 700, 1300
    sets = [two_parts(n_a, n_b, seed=s, gap=g) for s, g in ((1, 0.0), (2, 0.003), (3, 0.001))]
    eager = []
    for a, b in sets:
        h, ca, cb = run(art, a, b)
        eager.append((h._host().copy(), ca, cb))
    assert eager[0][0].tobytes() != eager[1][0].tobytes() != eager[2][0].tobytes()
    pa, pb = torch.from_numpy(sets[0][0]).to(DEV), torch.from_numpy(sets[0][1]).to(DEV)
    ca = torch.empty(n_a, dtype=torch.uint8, device=DEV)
    cb = torch.empty(n_b, dtype=torch.uint8, device=DEV)
    joint = torch.empty(art.JOINT_DOUBLES, dtype=torch.float64, device=DEV)
    ws = art.hinge_workspace(n_a, n_b, DEV)
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        art.hinge_fit_raw(pa, pb, THR, ca, cb, joint, workspace=ws)
        torch.cuda.synchronize()
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph, stream=s):
            art.hinge_fit_raw(pa, pb, THR, ca, cb, joint, workspace=ws)
        for k in (1, 2):
            pa.copy_(torch.from_numpy(sets[k][0]).to(DEV))
            pb.copy_(torch.from_numpy(sets[k][1]).to(DEV))
            ws.fill_(0x5A)                          # nothing in the workspace outlives a call
            graph.replay()
            torch.cuda.synchronize()
            assert joint.cpu().numpy().tobytes() == eager[k][0].tobytes(), k
            assert np.array_equal(ca.cpu().numpy().astype(bool), eager[k][1]) and np.array_equal(cb.cpu().numpy().astype(bool), eager[k][2])
    torch.cuda.synchronize()


# ---- 5. on a scene of Gaussians ----------------------------------------------------------------------------------------------
def test_fit_hinge_on_two_slabs_of_gaussians(art):
    from robosimgs_amd import transform_gaussians
    rng = np.random.default_rng(21)
    m, s = 45, 1.0 / 44
    i, j = [x.reshape(-1).astype(np.float64) for x in np.meshgrid(np.arange(m), np.arange(m), indexing="ij")]
    lid = np.stack([i * s, j * s, 0 * i], 1)                     # in z = 0, hinged on the edge x = 0
    body = np.stack([0 * i, j * s, -i * s], 1)                   # in x = 0, below it: the shared edge is the line (0, y, 0)
    extra = rng.uniform(1.5, 2.5, (300, 3))                      # a third class the fit must not see
    means = np.concatenate([lid, body, extra]) + rng.uniform(-0.001, 0.001, (2 * m * m + 300, 3))
    ids = np.concatenate([np.full(m * m, 2), np.full(m * m, 0), np.full(300, 1)]).astype(np.int32)
    order = rng.permutation(len(means))
    means, ids = means[order].astype(np.float32), ids[order]
    t_means, t_ids = torch.from_numpy(means).to(DEV), torch.from_numpy(ids).to(DEV)
    a, b = means[ids == 2], means[ids == 0]
    ref = HR.fit(a, b, THR)
    h = art.fit_hinge(t_means, t_ids, part=2, base=0, threshold=THR, return_contacts=True)
    check(ref, h, h.contact_a.cpu().numpy(), h.contact_b.cpu().numpy(), "two slabs")
    p = art.fit_hinge_points(t_means[t_ids == 2], t_means[t_ids == 0], THR)
    assert p._host().tobytes() == h._host().tobytes()
    assert h.n_contact == (m, m)                                 # the two edge rows
    angle = np.degrees(np.arccos(min(1.0, abs(h.axis @ [0.0, 1.0, 0.0]))))
    print(f"axis {h.axis}, {angle:.3f} degrees from the edge, position {h.position}")
    assert angle < 2.0 and h.axis[1] > 0 and np.abs(h.position[[0, 2]]).max() < 0.002
    with pytest.raises(ValueError, match="class 7"):
        art.fit_hinge(t_means, t_ids, part=7, base=0)
    with pytest.raises(ValueError, match=r"class 5 \(base\)"):
        art.fit_hinge(t_means, t_ids, part=2, base=5)
    # pose the lid: its contact Gaussians stay within threshold + their extent across the axis of where they were
    n = len(means)
    tensors = dict(means=t_means, quats=torch.tensor([[1.0, 0, 0, 0]], device=DEV).repeat(n, 1),
                   scales=torch.full((n, 3), 0.01, device=DEV), opacities=torch.full((n,), 0.5, device=DEV),
                   colors=torch.rand(n, 1, 3, device=DEV), sh_degree=0)
    R, t = h.pose(0.5)
    group = torch.where(t_ids == 2, 0, -1).to(torch.int32)
    moved = transform_gaussians(tensors, rotations=[R], translations=[t], group_ids=group)["means"].cpu().numpy()
    lid_rows = np.flatnonzero(ids == 2)
    contact_rows = lid_rows[h.contact_a.cpu().numpy()]
    rel = means[contact_rows].astype(np.float64) - h.position
    across = np.linalg.norm(rel - np.outer(rel @ h.axis, h.axis), axis=1).max()
    shift = np.linalg.norm(moved[contact_rows] - means[contact_rows], axis=1).max()
    print(f"contact extent across the axis {across:.4f}, largest shift of a contact Gaussian {shift:.4f}")
    assert shift <= THR + across
    assert np.array_equal(moved[ids != 2], means[ids != 2])                      # nobody else moved
    far = lid_rows[np.argmax(means[lid_rows, 0])]
    assert np.linalg.norm(moved[far] - means[far]) > 0.4                         # the free edge swung: 2 sin(0.25) of ~1
