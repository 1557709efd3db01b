"""The statement of register_points (include/mgs_register.h) in fp64 NumPy: matching, the Kabsch / Umeyama update, the loop
and its stop rule, plus the cell arithmetic of robosimgs_amd/csrc/register_grid.h restated for the host harness, and the
separation condition the GPU tests assert before they compare anything exactly.

Matching is by definition the brute-force answer.  `match` finds it through scipy's cKDTree (candidates within a slightly
wider radius in fp64, then the fp32 difference form on those), `match_dense` by evaluating every pair; the host tests hold
one to the other.  The pair form fma(dz, dz, fma(dy, dy, dx * dx)) is emulated as fp32 differences, an fp32 square, and
each fma as an exact fp64 product plus the fp32 addend rounded once to fp32 (the fp64 sum is rounded too, which can differ
from a true fma in the last bit of rare cases: no test compares distances closer than the counted bound).

The update is Horn's closed form (the largest eigenvector of a 4x4 matrix is the quaternion): it never returns a
reflection and shares nothing with the SVD the host test compares it with.
"""
from dataclasses import dataclass, field

import numpy as np
from scipy.spatial import cKDTree

FLAG_UNDETERMINED, FLAG_NONFINITE = 1, 2
COLLINEAR = 1e-12
SEPARATION = 1e-5
IDENTITY = (1.0, np.eye(3), np.zeros(3))


def finite_rows(x):
    return np.isfinite(np.asarray(x)).all(axis=1)


def apply(T, P):
    """s R p + t in fp64."""
    s, R, t = T
    return s * (np.asarray(P, np.float64) @ np.asarray(R, np.float64).T) + np.asarray(t, np.float64)


def pair_d2(pf, q):
    """The fp32 difference form of one point pf [3] against q [m,3], both float32 -> float32 [m]."""
    with np.errstate(over="ignore", invalid="ignore"):
        d = pf[None, :].astype(np.float32) - q.astype(np.float32)
        xx = (d[:, 0] * d[:, 0]).astype(np.float32)
        yy = (d[:, 1].astype(np.float64) ** 2 + xx.astype(np.float64)).astype(np.float32)
        return (d[:, 2].astype(np.float64) ** 2 + yy.astype(np.float64)).astype(np.float32)


def limit2_of(max_distance):
    with np.errstate(over="ignore"):
        return np.float32(max_distance) * np.float32(max_distance)


def _pick(d2, idx, limit2):
    """argmin over (d2, idx) of the candidates; (-1, inf) where there is none at or below the limit."""
    if len(idx) == 0:
        return -1, np.float32(np.inf)
    order = np.lexsort((idx, d2))
    k = order[0]
    return (int(idx[k]), np.float32(d2[k])) if d2[k] <= limit2 else (-1, np.float32(np.inf))


def match_dense(T, P, Q, max_distance):
    """(correspondence int32 [n_s], distance2 float32 [n_s]) by evaluating every pair."""
    P, Q = np.asarray(P, np.float32), np.asarray(Q, np.float32)
    limit2, okq = limit2_of(max_distance), np.flatnonzero(finite_rows(Q))
    with np.errstate(over="ignore", invalid="ignore"):
        moved = apply(T, P).astype(np.float32)
    c, d = np.full(len(P), -1, np.int32), np.full(len(P), np.inf, np.float32)
    for i in np.flatnonzero(finite_rows(P)):
        c[i], d[i] = _pick(pair_d2(moved[i], Q[okq]), okq, limit2)
    return c, d


def match(T, P, Q, max_distance, tree=None):
    """The same answer through a k-d tree over the finite targets (tree: a cKDTree of Q[finite_rows(Q)] to reuse)."""
    P, Q = np.asarray(P, np.float32), np.asarray(Q, np.float32)
    limit2, okq = limit2_of(max_distance), np.flatnonzero(finite_rows(Q))
    with np.errstate(over="ignore", invalid="ignore"):
        moved = apply(T, P).astype(np.float32)
    c, d = np.full(len(P), -1, np.int32), np.full(len(P), np.inf, np.float32)
    rows = np.flatnonzero(finite_rows(P) & finite_rows(moved))
    if len(okq) == 0 or len(rows) == 0:
        return c, d
    tree = tree if tree is not None else cKDTree(Q[okq].astype(np.float64))
    near = tree.query_ball_point(moved[rows].astype(np.float64), float(max_distance) * (1 + 1e-5) + 1e-30)
    for i, cand in zip(rows, near):
        cand = np.asarray(cand, np.int64)
        c[i], d[i] = _pick(pair_d2(moved[i], Q[okq[cand]]), okq[cand], limit2)
    return c, d


def stats(T, P, Q, c):
    """(n_in, rmse, fitness) of a matching: the residual in fp64, rmse 0 where there is no inlier."""
    P, Q = np.asarray(P, np.float32), np.asarray(Q, np.float32)
    rows = np.flatnonzero(c >= 0)
    n_fin = int(finite_rows(P).sum())
    if len(rows) == 0:
        return 0, 0.0, 0.0
    r = apply(T, P[rows]) - Q[c[rows]].astype(np.float64)
    return len(rows), float(np.sqrt((r * r).sum() / len(rows))), len(rows) / n_fin


def _collinear(x):
    w = np.linalg.eigvalsh((x - x.mean(0)).T @ (x - x.mean(0)))[::-1]
    return not (w[1] > COLLINEAR * w[0])


def update(p, q, with_scale):
    """(s, R, t) from matched rows p, q (fp32 values, taken in fp64), or None where the rotation is undetermined."""
    p, q = np.asarray(p, np.float64), np.asarray(q, np.float64)
    if len(p) < 3 or _collinear(p) or _collinear(q):
        return None
    pm, qm = p.mean(0), q.mean(0)
    M = (p - pm).T @ (q - qm)                     # M[a, b] = sum p_a q_b: the transpose of the statement's S
    (xx, xy, xz), (yx, yy, yz), (zx, zy, zz) = M
    N = np.array([[xx + yy + zz, yz - zy, zx - xz, xy - yx],
                  [yz - zy, xx - yy - zz, xy + yx, zx + xz],
                  [zx - xz, xy + yx, -xx + yy - zz, yz + zy],
                  [xy - yx, zx + xz, yz + zy, -xx - yy + zz]])
    w, x, y, z = np.linalg.eigh(N)[1][:, -1]
    R = np.array([[1 - 2 * (y * y + z * z), 2 * (x * y - w * z), 2 * (x * z + w * y)],
                  [2 * (x * y + w * z), 1 - 2 * (x * x + z * z), 2 * (y * z - w * x)],
                  [2 * (x * z - w * y), 2 * (y * z + w * x), 1 - 2 * (x * x + y * y)]])
    s = float(np.trace(R.T @ M.T) / ((p - pm) ** 2).sum()) if with_scale else 1.0
    return s, R, qm - s * R @ pm


@dataclass
class Reference:
    scale: float
    rotation: np.ndarray
    translation: np.ndarray
    correspondence: np.ndarray
    distance2: np.ndarray
    rmse: float
    fitness: float
    n_inliers: int
    iterations: int
    converged: bool
    flags: int
    history: np.ndarray
    transforms: list = field(default_factory=list)        # T_k of every executed iteration, then the final T
    matchings: list = field(default_factory=list)         # c under each of those

    @property
    def T(self):
        return self.scale, self.rotation, self.translation


def icp(P, Q, max_distance, iterations=30, with_scale=False, tol=1e-6, init=None, history=None):
    """The loop of include/mgs_register.h.  history: the caller's [iterations,4] array (rows past the last executed iteration
    keep their value); a zero one otherwise."""
    P, Q = np.asarray(P, np.float32), np.asarray(Q, np.float32)
    T = IDENTITY if init is None else (float(init[0]), np.asarray(init[1], np.float64), np.asarray(init[2], np.float64))
    hist = np.zeros((iterations, 4)) if history is None else np.array(history, np.float64)
    okq = finite_rows(Q)
    tree = cKDTree(Q[okq].astype(np.float64)) if okq.any() else None
    flags = 0 if (okq.all() and finite_rows(P).all()) else FLAG_NONFINITE
    executed, converged, prev = 0, False, None
    transforms, matchings = [], []
    for k in range(iterations):
        c, _ = match(T, P, Q, max_distance, tree)
        n_in, rmse, _ = stats(T, P, Q, c)
        transforms.append(T)
        matchings.append(c)
        hist[k] = [n_in, rmse, T[0], 0.0]
        executed = k + 1
        new = update(P[c >= 0], Q[c[c >= 0]], with_scale)
        if new is None:
            flags |= FLAG_UNDETERMINED
            break
        T = new
        stop = k > 0 and abs(rmse - prev) <= tol * prev
        prev = rmse
        if stop:
            converged = True
            break
    c, d2 = match(T, P, Q, max_distance, tree)
    n_in, rmse, fitness = stats(T, P, Q, c)
    transforms.append(T)
    matchings.append(c)
    return Reference(T[0], T[1], T[2], c, d2, rmse, fitness, n_in, executed, converged, flags, hist, transforms, matchings)


def separation(T, P, Q, max_distance):
    """Per source point, in fp64: `undecided` (bool [n_s]) where the best and the second-best DISTINCT distance, or the best
    distance and max_distance, are within SEPARATION of each other (two near-tied targets that are both farther than
    max_distance + SEPARATION do not count: the point has no inlier either way); `candidates` (dict: row -> set) the answers such a point
    may receive (-1 stands for "no inlier").  A non-finite source point is decided."""
    P, Q = np.asarray(P, np.float32), np.asarray(Q, np.float32)
    okq = np.flatnonzero(finite_rows(Q))
    undecided, candidates = np.zeros(len(P), bool), {}
    if len(okq) == 0:
        return undecided, candidates
    Qd, md = Q[okq].astype(np.float64), float(max_distance)
    rows = np.flatnonzero(finite_rows(P))
    moved = apply(T, P[rows])
    k = min(len(Qd), 4)
    near = cKDTree(Qd).query(moved, k=k)[0].reshape(len(rows), k)          # the k smallest distances, ascending
    best = near[:, 0]
    distinct = near > best[:, None]
    other = np.where(distinct.any(1), np.where(distinct, near, np.inf).min(1), np.inf)
    for r in np.flatnonzero(~distinct.any(1) & (k < len(Qd))):                 # k copies of one point: look at every target
        dist = np.sqrt(((moved[r] - Qd) ** 2).sum(1))
        other[r] = np.where(dist > best[r], dist, np.inf).min()
    # a tie among targets that are all out of reach decides nothing: the answer is "no inlier" whichever is nearer
    near_tie, near_limit = (other - best <= SEPARATION) & (best <= md + SEPARATION), np.abs(best - md) <= SEPARATION
    for r in np.flatnonzero(near_tie | near_limit):
        dist = np.sqrt(((moved[r] - Qd) ** 2).sum(1))
        cand = set(okq[dist <= best[r] + SEPARATION].tolist()) if best[r] <= md + SEPARATION else set()
        if near_limit[r] or best[r] > md:
            cand.add(-1)
        undecided[rows[r]] = True
        candidates[int(rows[r])] = cand
    return undecided, candidates


# ---- the cell arithmetic of robosimgs_amd/csrc/register_grid.h ---------------------------------------------------------------
EDGE_MARGIN, EDGE_GROWTH = 1.0 + 1.0 / 1024.0, 1.25


@dataclass
class Grid:
    origin: np.ndarray
    h: float
    dims: tuple


def grid_make(Q, max_distance, max_cells):
    Q = np.asarray(Q, np.float32)
    Q = Q[finite_rows(Q)]
    lo, hi = (Q.min(0), Q.max(0)) if len(Q) else (np.zeros(3, np.float32), np.zeros(3, np.float32))
    lo, ext = lo.astype(np.float64), hi.astype(np.float64) - lo.astype(np.float64)
    h = float(np.float32(max_distance)) * EDGE_MARGIN
    while True:
        dims = np.floor(ext * (1.0 / h)) + 1.0
        if dims.prod() <= max_cells:
            break
        h *= EDGE_GROWTH
    return Grid(lo, h, tuple(int(d) for d in dims))


def cell_coord(grid, axis, x):
    """floor((x - origin) / h) clamped to -2..n+1."""
    t = np.floor((np.float64(np.float32(x)) - grid.origin[axis]) * (1.0 / grid.h))
    return int(min(max(t, -2.0), float(grid.dims[axis]) + 1.0))


def query_ranges(grid, p):
    """[(lo, hi)] per axis of the cells about p, cut to the grid (lo > hi: none)."""
    out = []
    for a in range(3):
        c = cell_coord(grid, a, p[a])
        out.append((max(c - 1, 0), min(c + 1, grid.dims[a] - 1)))
    return out


def target_cell(grid, q):
    return tuple(min(max(cell_coord(grid, a, q[a]), 0), grid.dims[a] - 1) for a in range(3))
