"""Fusing depth frames into a truncated signed distance volume and extracting its isosurface, in fp64 (NumPy), with the bounds
an fp32 evaluation can be held to.  Every bound is a count of roundings, none is tuned to an output.  A helper module, not a
test file (the kernels are robosimgs_amd/csrc/tsdf.hip and csrc/tsdf_tets.h).

The volume.  nx x ny x nz samples, x fastest; sample (i, j, k) sits at origin + (i + 0.5, j + 0.5, k + 0.5) voxel.  Arrays are
[nz, ny, nx]; the colour is planar, [3, nz, ny, nx].

Integration, per sample p and camera c in call order:
    q = R p + t, skipped if q.z <= near;  u = fx q.x / q.z + cx, v alike, pixel (floor u, floor v), skipped outside the frame;
    d the depth there, skipped if not finite, <= 0 or alpha < alpha_min;  s = d - q.z, skipped if s < -trunc;
    t = min(1, s / trunc);  tsdf <- (tsdf w + t) / (w + 1), each colour plane alike;  w <- min(w + 1, max_weight).

integration_bound.  p_k = (i + 0.5) voxel + origin_k is two roundings, q_k = R_k0 p_0 + R_k1 p_1 + R_k2 p_2 + t_k six more:
|dq_k| <= e_q := gamma(8) (sum_j |R_kj| |p_j| + |t_k|).  s = d - q.z: |ds| <= e_s := e_q.z + U |s|.  s / trunc is one more
rounding: |dt| <= e_t := e_s / trunc + gamma(2) |t|.  The running mean is a product, a sum and a quotient of values of
magnitude <= 1 (tsdf stays in [-1, 1]): with e the error of the stored value, e' <= (w e + e_t) / (w + 1) + gamma(3) <=
e + e_t + gamma(3).  So integration_bound is the sum of e_t + gamma(3) over the updates a sample received; a colour plane's is
gamma(3) max(1, |c|) per update (the pixel's colour is exact).  Weights are small integers: exact.

The thresholds.  A decision is open where its margin is inside the error of what it compares: |q.z - near| <= e_q.z;
|s + trunc| <= e_s; and u within e_u of an integer (a pixel boundary; the frame's edges are two of them), where
e_u := |fx| (e_q.x / |q.z| + |q.x| e_q.z / q.z^2) + gamma(3) (|fx q.x / q.z| + |cx|).  `flip` re-states the update with one
such decision of one camera taken the other way.

Extraction: marching tetrahedra on the Kuhn split.  Tetrahedron n belongs to the n-th permutation pi of the axes in
lexicographic order: corners v0 = (0,0,0), v1 = v0 + e_pi0, v2 = v1 + e_pi1, v3 = (1,1,1).  A corner is inside iff tsdf <
level (fp32 compare); a cell is emitted iff its eight weights are >= min_weight.  Every tetrahedron edge runs from a grid
point to that point plus one of EDGE_OFFSETS (type 0..6) and is owned by that lower point.  Vertices: one per crossed edge
of an emitted cell, ordered by (owner, x fastest; type); position p_a + s (p_b - p_a), s = (level - f_a) / (f_b - f_a), a the
owner; colour with the same s, clamped to [0, 1].  Faces: by cell, x fastest, then tetrahedron 0..5; one inside or one
outside corner l gives the triangle of the edges (l, m), m ascending; two inside corners a < b with outside corners
c0 < c1 give the quad (a,c0), (a,c1), (b,c1), (b,c0) as the triangles (q0, q1, q2) and (q0, q2, q3).  WINDING[n][case] says
whether each triangle (A, B, C) of that (tetrahedron, case) is emitted as (A, C, B) instead, so that (B - A) x (C - A) points
towards increasing tsdf; it is derived below, at import, from generic values.

Vertex bound.  s is two differences and a quotient: relative gamma(3), and s <= 1.  A coordinate is fma(s, delta, p_a) with
delta = voxel or 0 (exact) and p_a one fma: gamma(3) voxel + U |p_a| + U (|p_a| + voxel) <= gamma(5) (|p_a| + voxel), one
division and one fma at the magnitude of the coordinate.  A colour is fma(s, c_b - c_a, c_a): gamma(5) (|c_a| + |c_b|).
"""
import itertools

import numpy as np

U = 2.0 ** -24


def gamma(k):
    return k * U / (1 - k * U)


# ---- the split --------------------------------------------------------------------------------------------------------
PERMS = list(itertools.permutations(range(3)))                      # lexicographic
EDGE_OFFSETS = [(1, 0, 0), (0, 1, 0), (0, 0, 1), (1, 1, 0), (1, 0, 1), (0, 1, 1), (1, 1, 1)]     # (dx, dy, dz) of type 0..6
EDGE_TYPE = {o: t for t, o in enumerate(EDGE_OFFSETS)}


def tet_corners(n):
    """[4,3] integer offsets (dx, dy, dz) of tetrahedron n's corners."""
    p, v = PERMS[n], np.zeros((4, 3), np.int64)
    v[1, p[0]] = 1
    v[2] = v[1]
    v[2, p[1]] = 1
    v[3] = 1
    return v


TET_CORNERS = np.stack([tet_corners(n) for n in range(6)])


def case_triangles(case):
    """The triangles of a case (bit l set: local corner l inside) before winding: lists of three local corner pairs (lo, hi)."""
    ins = [l for l in range(4) if case >> l & 1]
    out = [l for l in range(4) if not case >> l & 1]
    pair = lambda a, b: (min(a, b), max(a, b))
    if len(ins) in (0, 4):
        return []
    if len(ins) == 1:
        return [[pair(ins[0], m) for m in out]]
    if len(ins) == 3:
        return [[pair(out[0], m) for m in ins]]
    (a, b), (c0, c1) = ins, out
    q = [pair(a, c0), pair(a, c1), pair(b, c1), pair(b, c0)]
    return [[q[0], q[1], q[2]], [q[0], q[2], q[3]]]


def _derive_winding():
    rng = np.random.default_rng(5)
    table = np.zeros((6, 16), bool)
    for n in range(6):
        v = TET_CORNERS[n].astype(np.float64)
        for case in range(1, 15):
            votes = []
            for _ in range(4):                                     # four sets of generic values must agree
                f = rng.uniform(0.2, 1.0, 4) * np.where([(case >> l) & 1 for l in range(4)], -1.0, 1.0)
                grad = np.linalg.solve(v[1:] - v[0], f[1:] - f[0])    # the linear interpolant's gradient on the tetrahedron
                for tri in case_triangles(case):
                    P = [v[a] + (0.0 - f[a]) / (f[b] - f[a]) * (v[b] - v[a]) for a, b in tri]
                    votes.append(float(np.dot(np.cross(P[1] - P[0], P[2] - P[0]), grad)))
            votes = np.array(votes)
            assert (np.abs(votes) > 1e-9).all() and (np.sign(votes) == np.sign(votes[0])).all(), (n, case, votes)
            table[n, case] = votes[0] < 0
    return table


WINDING = _derive_winding()


def tet_triangles(n, case):
    """The triangles of (tetrahedron, case) as emitted: local corner pairs, winding applied."""
    return [[t[0], t[2], t[1]] if WINDING[n, case] else t for t in case_triangles(case)]


# ---- integration ------------------------------------------------------------------------------------------------------
FLIPS = ("near", "trunc", "px-", "px+", "py-", "py+")


def integrate(dtype, ijk, tsdf, weight, color, origin, voxel, trunc, max_weight, depth, rgb, alphas, alpha_min, near,
              viewmats, Ks, flip=None):
    """The statement above on the samples ijk [M,3] (i, j, k), every operation in `dtype` (np.float64: the reference;
    np.float32: the plain fp32 restatement).  tsdf, weight [M] and color [3,M] | None are the state before; depth [C,H,W],
    rgb [C,H,W,3] | None, alphas [C,H,W] | None.  flip = (camera, one of FLIPS): that decision of that camera is taken the
    other way for every sample.  Returns dict(tsdf, weight, color, n_updates, bound, color_bound, open): bound is
    integration_bound, open[kind] a bool [C,M] of the decisions whose margin is inside their error."""
    T = dtype
    ijk = np.asarray(ijk)
    M = len(ijk)
    f, w = np.array(tsdf, T), np.array(weight, T)
    col = None if color is None or rgb is None else np.array(color, T)
    origin, voxel, trunc = np.asarray(origin, np.float32).astype(T), T(np.float32(voxel)), T(np.float32(trunc))
    near, alpha_min, max_weight = T(np.float32(near)), T(np.float32(alpha_min)), T(np.float32(max_weight))
    depth = np.asarray(depth, np.float32)
    C, H, W = depth.shape
    p = (ijk.astype(T) + T(0.5)) * voxel + origin                                  # [M,3]
    n_upd, bound, cbound = np.zeros(M, np.int64), np.zeros(M), np.zeros(M)
    opened = {k: np.zeros((C, M), bool) for k in FLIPS}
    for c in range(C):
        V, K = np.asarray(viewmats[c], np.float32).astype(T), np.asarray(Ks[c], np.float32).astype(T)
        R, t = V[:3, :3], V[:3, 3]
        q = (R[None, :, 0] * p[:, None, 0] + R[None, :, 1] * p[:, None, 1]) + R[None, :, 2] * p[:, None, 2] + t[None]
        e_q = gamma(8) * (np.abs(R).astype(np.float64) @ np.abs(p).astype(np.float64).T + np.abs(t)[:, None].astype(np.float64)).T
        qz = q[:, 2]
        fl = flip[1] if flip is not None and flip[0] == c else None
        front = qz > near
        opened["near"][c] = np.abs(qz.astype(np.float64) - float(near)) <= e_q[:, 2]
        if fl == "near":
            front = ~front
        with np.errstate(all="ignore"):
            qzs = np.where(qz != 0, qz, T(1))
            uv = [K[a, a] * (q[:, a] / qzs) + K[a, 2] for a in (0, 1)]
            pix, inside = [], front.copy()
            for a, (x, size, minus, plus) in enumerate(((uv[0], W, "px-", "px+"), (uv[1], H, "py-", "py+"))):
                e_u = (abs(float(K[a, a])) * (e_q[:, a] / np.abs(qzs) + np.abs(q[:, a]) * e_q[:, 2] / (qzs.astype(np.float64) ** 2))
                       + gamma(3) * (np.abs(float(K[a, a]) * q[:, a] / qzs) + abs(float(K[a, 2]))))
                lo = np.floor(x)
                opened[minus][c] = front & (x - lo <= e_u)
                opened[plus][c] = front & (lo + 1 - x <= e_u)
                cell = lo + (fl == plus) - (fl == minus)
                inside &= (cell >= 0) & (cell < size)                                # NaN compares false
                pix.append(np.where(inside, cell, 0).astype(np.int64))
        d = depth[c, pix[1], pix[0]]
        ok = inside & np.isfinite(d) & (d > 0)
        if alphas is not None:
            with np.errstate(invalid="ignore"):
                ok &= np.asarray(alphas, np.float32)[c, pix[1], pix[0]] >= np.float32(alpha_min)
        d = np.where(ok, d, np.float32(1)).astype(T)                                 # a select: what a skipped pixel holds is not used
        s = d - qz
        e_s = e_q[:, 2] + U * np.abs(s)
        seen = s >= -trunc
        opened["trunc"][c] = ok & (np.abs(s.astype(np.float64) + float(trunc)) <= e_s)
        if fl == "trunc":
            seen = ~seen
        ok &= seen
        tt = np.minimum(T(1), s / trunc)
        e_t = e_s / float(trunc) + gamma(2) * np.abs(tt)
        f = np.where(ok, (f * w + tt) / (w + T(1)), f)
        if col is not None:
            px = np.asarray(rgb, np.float32)[c, pix[1], pix[0]].astype(T)             # [M,3]
            px = np.where(ok[:, None], px, T(0))
            col = np.where(ok[None], (col * w[None] + px.T) / (w[None] + T(1)), col)
            cbound += np.where(ok, gamma(3) * np.maximum(1.0, np.abs(px).max(1)), 0.0)
        w = np.where(ok, np.minimum(w + T(1), max_weight), w)
        n_upd += ok
        bound += np.where(ok, e_t + gamma(3), 0.0)
    return dict(tsdf=f, weight=w, color=col, n_updates=n_upd, bound=bound, color_bound=cbound, open=opened)


def grid_ijk(dims):
    """[M,3] (i, j, k) of every sample of an nx x ny x nz volume, x fastest."""
    nx, ny, nz = dims
    k, j, i = np.meshgrid(np.arange(nz), np.arange(ny), np.arange(nx), indexing="ij")
    return np.stack([i.ravel(), j.ravel(), k.ravel()], 1)


# ---- extraction -------------------------------------------------------------------------------------------------------
def extract(tsdf, weight, color, origin, voxel, level=0.0, min_weight=1.0):
    """The surface of the fp32 arrays given: dict(vertices fp64 [V,3], vertex_bound [V,3], faces int32 [F,3], colors fp64 [V,3]
    | None, color_bound [V,3], pairs: the set of (tetrahedron, case) the volume exercised)."""
    f = np.asarray(tsdf, np.float32)
    nz, ny, nx = f.shape
    inside = f < np.float32(level)
    wok = np.asarray(weight, np.float32) >= np.float32(min_weight)
    cell = np.ones((max(nz - 1, 0), max(ny - 1, 0), max(nx - 1, 0)), bool)
    for dz, dy, dx in itertools.product((0, 1), repeat=3):
        cell &= wok[dz:nz - 1 + dz, dy:ny - 1 + dy, dx:nx - 1 + dx]
    lin = lambda i, j, k: (k * ny + j) * nx + i
    tris, pairs = [], set()                                     # a triangle: three (owner linear index, type)
    for k, j, i in zip(*np.nonzero(cell)):
        for n in range(6):
            cn = TET_CORNERS[n]
            case = sum(int(inside[k + cn[l, 2], j + cn[l, 1], i + cn[l, 0]]) << l for l in range(4))
            pairs.add((n, case))
            for tri in tet_triangles(n, case):
                tris.append([(lin(i + cn[a, 0], j + cn[a, 1], k + cn[a, 2]), EDGE_TYPE[tuple(cn[b] - cn[a])]) for a, b in tri])
    keys = sorted({e for tri in tris for e in tri})
    index = {e: n for n, e in enumerate(keys)}
    faces = np.array([[index[e] for e in tri] for tri in tris], np.int32).reshape(-1, 3)
    V = len(keys)
    own = np.array([e[0] for e in keys], np.int64).reshape(V)
    off = np.array([EDGE_OFFSETS[e[1]] for e in keys], np.int64).reshape(V, 3)
    a = np.stack([own % nx, own // nx % ny, own // (nx * ny)], 1)
    b = a + off
    f64 = f.astype(np.float64)
    fa, fb = f64[a[:, 2], a[:, 1], a[:, 0]], f64[b[:, 2], b[:, 1], b[:, 0]]
    s = (float(np.float32(level)) - fa) / (fb - fa)
    vox, org = float(np.float32(voxel)), np.asarray(origin, np.float32).astype(np.float64)
    pa = (a + 0.5) * vox + org
    out = dict(vertices=pa + s[:, None] * (off * vox), vertex_bound=gamma(5) * (np.abs(pa) + vox), faces=faces, colors=None,
               color_bound=None, pairs=pairs)
    if color is not None:
        c = np.asarray(color, np.float32).astype(np.float64)
        ca, cb = c[:, a[:, 2], a[:, 1], a[:, 0]].T, c[:, b[:, 2], b[:, 1], b[:, 0]].T
        out["colors"] = np.clip(ca + s[:, None] * (cb - ca), 0.0, 1.0)
        out["color_bound"] = gamma(5) * (np.abs(ca) + np.abs(cb))
    return out


def mesh_topology(faces, n_vertices):
    """dict(closed: every directed edge has exactly one opposite and occurs once; euler: V - E + F; unreferenced: vertices no
    face names; boundary: directed edges without an opposite)."""
    faces = np.asarray(faces, np.int64)
    d = np.concatenate([faces[:, [0, 1]], faces[:, [1, 2]], faces[:, [2, 0]]])
    key = d[:, 0] * (n_vertices + 1) + d[:, 1]
    rev = d[:, 1] * (n_vertices + 1) + d[:, 0]
    uniq, counts = np.unique(key, return_counts=True)
    has_opposite = np.isin(rev, uniq)
    und = np.unique(np.sort(d, 1), axis=0)
    return dict(closed=bool((counts == 1).all() and has_opposite.all()), euler=int(n_vertices - len(und) + len(faces)),
                unreferenced=int(n_vertices - len(np.unique(faces))), boundary=int((~has_opposite).sum()),
                open_edge=~has_opposite, directed=d)


# ---- scenes -----------------------------------------------------------------------------------------------------------
def sphere_volume(dims=(19, 18, 17), radius=6.3, center=(9.2, 8.9, 8.4)):
    """tsdf [nz,ny,nx] fp32 of the analytic sphere |x - center| - radius (voxel units, origin 0, voxel 1), weights all 1."""
    g = grid_ijk(dims) + 0.5
    f = (np.linalg.norm(g - np.asarray(center), axis=1) - radius).astype(np.float32).reshape(dims[2], dims[1], dims[0])
    return f, np.ones_like(f)


def random_volume(dims=(9, 8, 7), seed=3, holes=0.0):
    rng = np.random.default_rng(seed)
    shape = (dims[2], dims[1], dims[0])
    f = rng.uniform(-1, 1, shape).astype(np.float32)
    w = (rng.uniform(0, 1, shape) >= holes).astype(np.float32) * 2
    c = rng.uniform(0, 1, (3,) + shape).astype(np.float32)
    return f, w, c


def look_at(eye, target, up=(0.0, 0.0, 1.0)):
    """World-to-camera [4,4] fp32, OpenCV axes (x right, y down, z forward)."""
    eye, target = np.asarray(eye, np.float64), np.asarray(target, np.float64)
    z = target - eye
    z /= np.linalg.norm(z)
    x = np.cross(z, np.asarray(up, np.float64))
    x /= np.linalg.norm(x)
    y = np.cross(z, x)
    V = np.eye(4)
    V[:3, :3] = np.stack([x, y, z])
    V[:3, 3] = -V[:3, :3] @ eye
    return V.astype(np.float32)


def analytic_views(eyes, target, width=40, height=30, focal=38.0, sphere=((0.6, 0.5, 0.45), 0.25), plane_z=0.2):
    """Views of a sphere over the plane z = plane_z: dict(viewmats [C,4,4], Ks [C,3,3], depth [C,H,W] z-depth fp32 (0 where a ray
    meets nothing), rgb [C,H,W,3], alphas [C,H,W])."""
    C = len(eyes)
    viewmats = np.stack([look_at(e, target) for e in eyes])
    K = np.array([[focal, 0, width / 2], [0, focal, height / 2], [0, 0, 1]], np.float32)
    Ks = np.repeat(K[None], C, 0)
    depth = np.zeros((C, height, width), np.float32)
    ys, xs = np.meshgrid(np.arange(height) + 0.5, np.arange(width) + 0.5, indexing="ij")
    rays = np.stack([(xs - K[0, 2]) / focal, (ys - K[1, 2]) / focal, np.ones_like(xs)], -1)       # camera space, z = 1
    sc, sr = np.asarray(sphere[0], np.float64), sphere[1]
    for c in range(C):
        R, t = viewmats[c, :3, :3].astype(np.float64), viewmats[c, :3, 3].astype(np.float64)
        o, dirs = -R.T @ t, rays @ R                                                # world origin and directions
        with np.errstate(all="ignore"):
            lam_p = (plane_z - o[2]) / dirs[..., 2]
            lam_p = np.where(lam_p > 0, lam_p, np.inf)
            oc = o - sc
            A, B, Cq = (dirs * dirs).sum(-1), 2 * (dirs @ oc), oc @ oc - sr * sr
            disc = B * B - 4 * A * Cq
            lam_s = np.where(disc > 0, (-B - np.sqrt(np.abs(disc))) / (2 * A), np.inf)
            lam_s = np.where(lam_s > 0, lam_s, np.inf)
        lam = np.minimum(lam_p, lam_s)
        depth[c] = np.where(np.isfinite(lam), lam, 0.0)                              # rays have z = 1: lambda is the z-depth
    rng = np.random.default_rng(11)
    rgb = rng.uniform(0, 1, (C, height, width, 3)).astype(np.float32)
    alphas = np.ones((C, height, width), np.float32)
    return dict(viewmats=viewmats, Ks=Ks, depth=depth, rgb=rgb, alphas=alphas)


def fusion_case(dims, n_views, seed=0):
    """The integration tests' inputs: a volume of voxel 0.05 around a sphere over a plane and n_views views of 40 x 30: a ring of
    views of the scene, then one that has the volume behind it and, from five views on, one that sees none of it (every sample
    in front of it and outside its frame); with alpha holes, NaN, infinite and zero depth pixels."""
    voxel = 0.05
    origin = np.array([0.0, 0.0, 0.0], np.float32)
    hi = np.asarray(dims) * voxel
    target = hi / 2
    n_ring = n_views - (2 if n_views >= 5 else 1)
    radius = 1.2 + 0.3 * hi[0]
    eyes = [(target[0] + radius * np.cos(a), target[1] + radius * np.sin(a), 1.1) for a in np.linspace(0.3, 2.9, n_ring)]
    eyes += [(target[0], target[1] - 3.0, 1.0), (target[0] + 40.0, target[1] - 1.0, 1.0)][:n_views - n_ring]
    views = analytic_views(eyes, target, sphere=((target[0], target[1], 0.45), 0.25))
    views["viewmats"][n_ring] = look_at(eyes[n_ring], (target[0], target[1] - 9.0, 1.0))
    if n_views - n_ring > 1:
        views["viewmats"][n_ring + 1] = look_at(eyes[n_ring + 1], (target[0] + 40.3, target[1] + 5.0, 1.2))
    rng = np.random.default_rng(seed)
    d, a = views["depth"], views["alphas"]
    a[rng.uniform(size=a.shape) < 0.08] = 0.2                    # alpha holes
    a[rng.uniform(size=a.shape) < 0.01] = np.nan
    d[rng.uniform(size=d.shape) < 0.03] = np.nan
    d[rng.uniform(size=d.shape) < 0.03] = 0.0
    d[rng.uniform(size=d.shape) < 0.01] = np.inf
    hidden = ~(a >= 0.5)
    views["rgb"][hidden & (rng.uniform(size=a.shape) < 0.5)] = np.nan         # what a skipped pixel holds changes nothing
    return dict(dims=tuple(dims), origin=origin, voxel=voxel, trunc=np.float32(3 * voxel), **views)


def check_integration(got_tsdf, got_weight, got_color, ref, rerun):
    """Holds an fp32 result [M] (and colour [3,M] | None) to the reference `ref` (integrate(np.float64, ...) on all M samples):
    every sample within integration_bound with the reference's weight, or, with exactly one open decision flipped
    (rerun(sample indices, flip) -> integrate(np.float64, ...) on those samples), within that bound.  Returns dict(excused:
    the number of samples that needed a flip, observed: samples with an update, worst: the largest tsdf error of the rest, in
    units of its bound); raises AssertionError where a sample meets neither."""
    def misses(r, tsdf, weight, color):
        bad = (weight != r["weight"]) | ~(np.abs(tsdf - r["tsdf"]) <= r["bound"] + 0.0)
        if color is not None:
            bad |= ~(np.abs(color - r["color"]) <= r["color_bound"][None] + 0.0).all(0)
        return bad
    bad = misses(ref, got_tsdf, got_weight, got_color)
    ok = ~bad & (ref["bound"] > 0)
    worst = float((np.abs(got_tsdf - ref["tsdf"])[ok] / ref["bound"][ok]).max()) if ok.any() else 0.0
    excused = 0
    for m in np.nonzero(bad)[0]:
        cands = [(c, kind) for kind in FLIPS for c in np.nonzero(ref["open"][kind][:, m])[0]]
        sub = lambda x: None if x is None else x[..., m:m + 1]
        assert any(not misses(rerun(np.array([m]), fl), got_tsdf[m:m + 1], got_weight[m:m + 1], sub(got_color))[0]
                   for fl in cands), \
            (f"sample {m}: tsdf {got_tsdf[m]!r} vs {ref['tsdf'][m]!r} (bound {ref['bound'][m]:.3g}), weight {got_weight[m]} vs "
             f"{ref['weight'][m]}, open decisions {cands}")
        excused += 1
    return dict(excused=excused, observed=int((ref["n_updates"] > 0).sum()), worst=worst)


# ---- what the host and the GPU tests share --------------------------------------------------------------------------------
FUSION_CASES = (((24, 20, 17), 3), ((70, 5, 3), 5))          # neither nx is a multiple of the wave
MAX_WEIGHT = 2.0                                             # the first view is fused three times: the cap binds
_cache = {}


def fusion_views(case):
    """The case's arrays in the order the tests fuse them: every view once, then view 0 twice more."""
    order = list(range(len(case["viewmats"]))) + [0, 0]
    return {k: np.ascontiguousarray(case[k][order]) for k in ("depth", "rgb", "alphas", "viewmats", "Ks")}


def fuse(dtype, case, color=True, ijk=None, flip=None):
    """integrate(dtype, ...) of an empty volume with fusion_views(case), on the samples ijk (None: all); the camera of `flip`
    counts through that order."""
    v = fusion_views(case)
    ijk = grid_ijk(case["dims"]) if ijk is None else ijk
    M = len(ijk)
    return integrate(dtype, ijk, np.zeros(M), np.zeros(M), np.zeros((3, M)) if color else None, case["origin"], case["voxel"],
                     case["trunc"], MAX_WEIGHT, v["depth"], v["rgb"] if color else None, v["alphas"], 0.5, 0.01, v["viewmats"],
                     v["Ks"], flip=flip)


def fusion_reference(dims, n_views):
    """(case, fp64 reference of fuse) of one of FUSION_CASES, computed once and shared: treat both as read-only."""
    key = (tuple(dims), n_views)
    if key not in _cache:
        case = fusion_case(dims, n_views)
        _cache[key] = (case, fuse(np.float64, case))
    return _cache[key]


def level_volume(dims=(8, 7, 6), seed=9):
    """A volume with many values exactly on the level 0 (and on both sides of it), weights 1, random colours."""
    rng = np.random.default_rng(seed)
    shape = (dims[2], dims[1], dims[0])
    f = rng.choice(np.array([-0.5, 0.0, 0.0, 0.25, 1.0], np.float32), shape)
    return f, np.ones(shape, np.float32), rng.uniform(0, 1, (3,) + shape).astype(np.float32)
