"""Registration without a GPU: include/mgs_register.h <-> libmgs.so / libmgs_debug.so <-> the ctypes table
(_lib.REGISTER_EXPORTS), the argument checks of mgs_register_icp, the workspace size, the cell arithmetic of
csrc/register_grid.h compiled with g++ (tests/host_harness/register_grid_harness.cpp) against tests/register_ref.py and
against brute force, the statement's own properties, Mesh.sample_points and Registration's host math.
"""
import ctypes
import os
import re
import subprocess

import numpy as np
import pytest

import register_ref as RR

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "mgs_register.h")
HARNESS = os.path.join(ROOT, "tests", "host_harness", "register_grid_harness.cpp")
SRC = open(os.path.join(ROOT, "robosimgs_amd", "csrc", "register.hip")).read()
_shift = re.search(r"constexpr\s+int\s+kRegisterMaxCells\s*=\s*1\s*<<\s*(\d+)\s*;", SRC)
MAX_CELLS = 1 << int(_shift.group(1))


def _code(path=HEADER):
    return re.sub(r"/\*.*?\*/", "", open(path).read(), flags=re.S)


def _declared(path=HEADER):
    decls = re.findall(r"\b(?:int|void|size_t|const char \*)\s*\*?\s*(mgs_\w+)\s*\(([^;]*?)\)\s*;", _code(path), flags=re.S)
    return {name: 0 if args.strip() == "void" else len([a for a in args.split(",") if a.strip()]) for name, args in decls}


# ---- header, library, binding -------------------------------------------------------------------------------------------------
def test_register_header_symbols_are_exported_and_bound_in_both_libraries():
    from robosimgs_amd import _lib
    from robosimgs_amd.csrc import build
    decl = _declared()
    assert sorted(decl) == sorted(_lib.REGISTER_EXPORTS) == ["mgs_register_icp", "mgs_register_workspace_bytes"]
    others = [getattr(_lib, n) for n in dir(_lib) if n.endswith("EXPORTS") and n != "REGISTER_EXPORTS"]
    assert not set(_lib.REGISTER_EXPORTS) & set().union(*map(set, others))
    assert len(_lib.EXPORTS) == 29                                        # include/mgs.h's table is untouched
    assert decl == {"mgs_register_workspace_bytes": 3, "mgs_register_icp": 16}
    c = ctypes
    want = [c.c_int, c.c_void_p, c.c_int, c.c_void_p, c.c_float, c.c_int, c.c_int, c.c_double, c.c_void_p, c.c_void_p,
            c.c_size_t, c.c_void_p, c.c_void_p, c.c_void_p, c.c_void_p, c.c_void_p]
    for L in (_lib.lib(), _lib.debug_lib()):
        for name, nargs in decl.items():
            assert len(getattr(L, name).argtypes) == nargs, name
        assert list(L.mgs_register_icp.argtypes) == want and L.mgs_register_icp.restype is c.c_int
        assert list(L.mgs_register_workspace_bytes.argtypes) == [c.c_int] * 3
        assert L.mgs_register_workspace_bytes.restype is c.c_size_t
    nm = lambda path: subprocess.run(["nm", "-D", "--defined-only", path], capture_output=True, text=True).stdout
    for path in (_lib.LIB_PATH, _lib.DEBUG_LIB_PATH):
        assert all(name in nm(path) for name in decl), path
    code = _code()
    assert "MGS_VERSION" not in code and "#define" not in code.replace("#define MGS_REGISTER_H_", "")
    assert '#include "mgs.h"' in code and "register.hip" in build.SOURCES


@pytest.mark.parametrize("kw,word", [
    (dict(n_s=0), b"a point set is empty"),
    (dict(n_t=0), b"a point set is empty"),
    (dict(n_s=-3), b"a point set is empty"),
    (dict(source=None), b"source or target is null"),
    (dict(target=None), b"source or target is null"),
    (dict(result=None), b"result is null"),
    (dict(workspace=None), b"workspace is null"),
    (dict(workspace=0x10010), b"not 256-byte aligned"),
    (dict(workspace_bytes=0), b"workspace of 0 bytes"),
    (dict(workspace_bytes=-1), b"needed"),              # one byte short of what the size function reports
    (dict(max_distance=0.0), b"max_distance"),
    (dict(max_distance=-0.01), b"max_distance"),
    (dict(max_distance=float("nan")), b"max_distance"),
    (dict(max_distance=float("inf")), b"max_distance"),
    (dict(tol=-1e-9), b"tol"),
    (dict(tol=float("nan")), b"tol"),
    (dict(tol=float("inf")), b"tol"),
    (dict(iterations=-1), b"iterations -1 outside"),
    (dict(iterations=257), b"iterations 257 outside"),
])
def test_register_icp_argument_errors_are_reported_without_a_gpu(kw, word):
    """mgs_register_icp on made-up addresses: every case must be refused before anything is launched."""
    from robosimgs_amd import _lib
    L = _lib.lib()
    a = dict(n_s=100, source=0x1000, n_t=200, target=0x2000, max_distance=0.05, iterations=5, tol=1e-6, workspace=0x10000,
             workspace_bytes=None, result=0x3000)
    a.update(kw)
    need = L.mgs_register_workspace_bytes(100, 200, 5)
    if a["workspace_bytes"] is None:
        a["workspace_bytes"] = need
    elif a["workspace_bytes"] == -1:
        a["workspace_bytes"] = need - 1
    rc = L.mgs_register_icp(a["n_s"], a["source"], a["n_t"], a["target"], a["max_distance"], a["iterations"], 1, a["tol"],
                            None, a["workspace"], a["workspace_bytes"], None, None, None, a["result"], None)
    msg = L.mgs_last_error_string()
    assert rc == -1 and word in msg and msg.startswith(b"register_icp:"), (rc, msg)


def test_workspace_bytes_is_monotone_and_depends_on_the_three_counts_only():
    from robosimgs_amd import _lib, registration
    size = _lib.lib().mgs_register_workspace_bytes
    assert size(0, 5, 1) == size(5, 0, 1) == size(-1, -1, 0) == size(5, 5, -1) == size(5, 5, 257) == 0
    ns = [1, 2, 63, 64, 65, 255, 256, 257, 1000, 4099, 100_000, 800_000, 2**31 - 1]
    for fixed in (1, 4099):
        a = [size(n, fixed, 30) for n in ns]
        b = [size(fixed, n, 30) for n in ns]
        assert a == sorted(a) and b == sorted(b) and a[0] > 0
        assert b[-1] > 16 * (2**31 - 1)                                      # no 32-bit wrap in the layout
    its = [size(1000, 4099, k) for k in (0, 1, 2, 30, 256)]
    assert its == sorted(its) and its[0] > 0
    assert all(size(n, m, 7) % 256 == 0 and size(n, m, 7) >= 16 * m + 4 * MAX_CELLS for n in ns[:-1] for m in (1, 777))
    # the entry point takes counts, never a point: the same counts give the same size, which is what the wrapper allocates
    assert registration.workspace_bytes(1000, 4099, 30) == size(1000, 4099, 30)
    assert registration.register_workspace(10, 20, 3, "cpu").numel() == size(10, 20, 3) + 256


# ---- the cell arithmetic, through g++ -----------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def harness(tmp_path_factory):
    so = tmp_path_factory.mktemp("register_grid") / "libregister_grid_harness.so"
    subprocess.run(["g++", "-O2", "-std=c++17", "-shared", "-fPIC", HARNESS, "-o", str(so)], check=True)
    lib = ctypes.CDLL(str(so))
    p, i, f = ctypes.c_void_p, ctypes.c_int, ctypes.c_float
    lib.rg_make.argtypes = [p, p, f, i, p, p]
    lib.rg_query_ranges.argtypes = [p, p, i, p, p]
    lib.rg_target_cells.argtypes = [p, p, i, p, p, p]
    return lib


def _ptr(a):
    return a.ctypes.data_as(ctypes.c_void_p)


def _grid_case(name):
    """(targets float32 [m,3], max_distance, max_cells) of one named case."""
    rng = np.random.default_rng(sum(map(ord, name)))
    if name == "regular":                   # a few cells per axis, different per axis, origin off zero
        q = rng.uniform([-1.0, 0.5, 2.0], [1.5, 1.2, 2.3], (300, 3))
        return q.astype(np.float32), 0.25, MAX_CELLS
    if name == "one_cell":                  # every target inside one cell
        q = rng.uniform(-0.01, 0.01, (40, 3)) + [3.0, -2.0, 0.5]
        return q.astype(np.float32), 0.5, MAX_CELLS
    if name == "single_target":
        return np.array([[0.3, -3.9, 4.0]], np.float32), 0.1, MAX_CELLS
    if name == "small_cap":                 # the cap forces h > max_distance
        q = rng.uniform(-4.0, 4.0, (400, 3))
        return q.astype(np.float32), 0.05, 4096
    if name == "library_cap":               # ... and so does the library's own cap at this radius
        q = rng.uniform(-4.0, 4.0, (400, 3))
        return q.astype(np.float32), 0.01, MAX_CELLS
    if name == "flat":                      # no extent along z
        q = rng.uniform(-1.0, 1.0, (200, 3))
        q[:, 2] = 0.75
        return q.astype(np.float32), 0.125, MAX_CELLS
    raise KeyError(name)


def _queries(q, md, grid, rng):
    """Random queries about the grid, queries next to targets, and planted ones: on every cell face of each axis (and one
    float to either side), on the outer faces, and outside the grid by less and by more than h on each of the six sides."""
    lo, hi = grid.origin, grid.origin + np.array(grid.dims) * grid.h
    qlo, qhi = q.min(0).astype(np.float64), q.max(0).astype(np.float64)
    out = [rng.uniform(qlo - 2.5 * grid.h, qhi + 2.5 * grid.h, (1500, 3)),
           q[rng.integers(0, len(q), 1500)] + rng.uniform(-1.2 * md, 1.2 * md, (1500, 3))]
    planted = []
    for a in range(3):
        faces = grid.origin[a] + np.arange(0, min(grid.dims[a], 40) + 1) * grid.h
        faces = np.concatenate([faces, [qlo[a], qhi[a]]])                           # the outer faces as the targets see them
        for off in (-1.7 * grid.h, -1.0001 * grid.h, -0.6 * grid.h, -0.5 * md, 0.0, 0.5 * md, 0.6 * grid.h):
            faces = np.concatenate([faces, [qlo[a] + off, qhi[a] - off]])
        for x in faces:
            base = q[rng.integers(0, len(q))].astype(np.float64)
            for y in (np.nextafter(np.float32(x), np.float32(-np.inf)), np.float32(x), np.nextafter(np.float32(x), np.float32(np.inf))):
                p = base.copy()
                p[a] = y
                planted.append(p)
    out.append(np.array(planted))
    return np.concatenate(out).astype(np.float32)


@pytest.mark.parametrize("name", ["regular", "one_cell", "single_target", "small_cap", "library_cap", "flat"])
def test_grid_header_matches_the_statement_and_its_27_cells_hold_every_target_in_reach(harness, name):
    q, md, cap = _grid_case(name)
    ref = RR.grid_make(q, md, cap)
    lo, hi = np.ascontiguousarray(q.min(0)), np.ascontiguousarray(q.max(0))
    g, dims = np.zeros(5), np.zeros(3, np.int32)
    harness.rg_make(_ptr(lo), _ptr(hi), md, cap, _ptr(g), _ptr(dims))
    assert tuple(dims) == ref.dims and g[3] == ref.h and np.array_equal(g[:3], ref.origin) and g[4] == 1.0 / ref.h
    assert int(np.prod(dims)) <= cap and g[3] >= np.float32(md)
    if name in ("small_cap", "library_cap"):
        assert g[3] > 1.2 * md                                      # the cap, not the radius, set the edge
        assert int(np.prod(dims)) * RR.EDGE_GROWTH**3 * 1.5 > cap   # ... and no further than it had to
    if name in ("one_cell", "single_target"):
        assert tuple(dims) == (1, 1, 1)
    if name == "flat":
        assert dims[2] == 1

    cells, linear = np.zeros((len(q), 3), np.int32), np.zeros(len(q), np.int32)
    harness.rg_target_cells(_ptr(g), _ptr(dims), len(q), _ptr(q), _ptr(cells), _ptr(linear))
    assert np.array_equal(cells, np.array([RR.target_cell(ref, x) for x in q]))
    assert (cells >= 0).all() and (cells < dims).all()
    assert np.array_equal(linear, (cells[:, 2] * dims[1] + cells[:, 1]) * dims[0] + cells[:, 0])     # x fastest
    assert cells.max(0).tolist() == (dims - 1).tolist() and cells.min(0).tolist() == [0, 0, 0]       # both bounds are inside

    pts = _queries(q, md, ref, np.random.default_rng(5))
    ranges = np.zeros((len(pts), 6), np.int32)
    harness.rg_query_ranges(_ptr(g), _ptr(dims), len(pts), _ptr(pts), _ptr(ranges))
    step = max(1, len(pts) // 400)
    for i in range(0, len(pts), step):                                # the statement, on a sample (pure Python)
        assert ranges[i].tolist() == [v for lo_hi in RR.query_ranges(ref, pts[i]) for v in lo_hi], (i, pts[i])
    assert (ranges[:, 0::2] >= 0).all() and (ranges[:, 1::2] < dims).all()
    assert ((ranges[:, 1::2] - ranges[:, 0::2]) <= 2).all()
    # brute force: every target the inlier rule can accept (fp32 form, <= limit2) or that lies within max_distance in fp64
    limit2 = RR.limit2_of(md)
    qd, reached, missed, empty = q.astype(np.float64), 0, 0, 0
    for i in range(len(pts)):
        d2f = RR.pair_d2(pts[i], q)
        dist = np.sqrt(((pts[i].astype(np.float64) - qd) ** 2).sum(1))
        near = np.flatnonzero((d2f <= limit2) | (dist <= md))
        r = ranges[i]
        empty += int(r[0] > r[1] or r[2] > r[3] or r[4] > r[5])
        inside = ((cells[near, 0] >= r[0]) & (cells[near, 0] <= r[1]) & (cells[near, 1] >= r[2]) & (cells[near, 1] <= r[3])
                  & (cells[near, 2] >= r[4]) & (cells[near, 2] <= r[5]))
        reached += len(near)
        missed += int((~inside).sum())
    print(f"\n{name}: dims {tuple(dims)}, h {g[3]:.6g}, {len(pts)} queries, {reached} pairs in reach, {missed} outside the 27 "
          f"cells, {empty} queries with an empty range")
    assert missed == 0 and reached > 0 and empty > 0


# ---- the statement's own properties -------------------------------------------------------------------------------------------
def _planted(seed, n=300, m=500):
    rng = np.random.default_rng(seed)
    P = rng.uniform(-1.0, 1.0, (n, 3))
    Q = np.concatenate([P[: n // 2] + rng.normal(0, 0.01, (n // 2, 3)), rng.uniform(-1.0, 1.0, (m - n // 2, 3))])
    Q[7] = Q[3]                                                     # a duplicated target: the lower index must win
    Q[400] = Q[3]
    P[11] = np.nan
    Q[5, 1] = np.inf
    return P.astype(np.float32), Q.astype(np.float32)


def test_statement_matching_equals_the_dense_argmin():
    P, Q = _planted(1)
    Rz = np.array([[np.cos(0.02), -np.sin(0.02), 0], [np.sin(0.02), np.cos(0.02), 0], [0, 0, 1.0]])
    for T, md in ((RR.IDENTITY, 0.05), ((1.01, Rz, np.array([0.004, -0.003, 0.002])), 0.08), (RR.IDENTITY, 3.9)):
        c, d = RR.match(T, P, Q, md)
        cd, dd = RR.match_dense(T, P, Q, md)
        assert np.array_equal(c, cd) and np.array_equal(d, dd)
        assert c[11] == -1 and np.isinf(d[11]) and not (c == 5).any() and not (c == 7).any() and not (c == 400).any()
        assert (c >= 0).sum() > 100 and (d[c >= 0] <= RR.limit2_of(md)).all() and np.isinf(d[c < 0]).all()
    # every pair by hand on a corner of it
    c, d = RR.match(RR.IDENTITY, P[:40], Q[:60], 0.3)
    for i in range(40):
        best = (np.inf, -1)
        for j in range(60):
            if np.isfinite(P[i]).all() and np.isfinite(Q[j]).all():
                v = float(RR.pair_d2(P[i], Q[j:j + 1])[0])
                best = min(best, (v, j))
        want = best[1] if best[0] <= RR.limit2_of(0.3) else -1
        assert c[i] == want


def _svd_umeyama(p, q, with_scale):
    pm, qm = p.mean(0), q.mean(0)
    S = (q - qm).T @ (p - pm)
    U, sig, Vt = np.linalg.svd(S)
    D = np.diag([1.0, 1.0, np.sign(np.linalg.det(U @ Vt))])
    R = U @ D @ Vt
    s = float((sig * np.diag(D)).sum() / ((p - pm) ** 2).sum()) if with_scale else 1.0
    return s, R, qm - s * R @ pm


def test_statement_update_equals_svd_umeyama_and_never_reflects():
    rng = np.random.default_rng(2)
    cases = []
    p = rng.normal(size=(50, 3))
    A = np.linalg.qr(rng.normal(size=(3, 3)))[0]
    A *= np.sign(np.linalg.det(A))
    cases.append((p, 1.3 * p @ A.T + [0.2, -1.0, 3.0] + rng.normal(0, 0.01, p.shape)))
    flat = np.concatenate([rng.normal(size=(30, 2)), np.zeros((30, 1))], 1)          # coplanar; the mirrored target's
    cases.append((flat, flat * [1.0, -1.0, 1.0] + rng.normal(0, 1e-3, flat.shape) * [1, 1, 0]))   # free solution reflects
    cases.append((p, rng.normal(size=p.shape)))                                        # unrelated sets
    for k, (a, b) in enumerate(cases):
        a, b = a.astype(np.float32).astype(np.float64), b.astype(np.float32).astype(np.float64)
        for with_scale in (False, True):
            s, R, t = RR.update(a, b, with_scale)
            s2, R2, t2 = _svd_umeyama(a, b, with_scale)
            assert abs(np.linalg.det(R) - 1.0) <= 1e-12 and np.abs(R @ R.T - np.eye(3)).max() <= 1e-12
            assert np.abs(R - R2).max() <= 1e-12 and abs(s - s2) <= 1e-12 and np.abs(t - t2).max() <= 1e-12, k
    U, _, Vt = np.linalg.svd((cases[1][1] - cases[1][1].mean(0)).T @ (cases[1][0] - cases[1][0].mean(0)))
    assert np.linalg.det(U @ Vt) < 0                                  # the case is what it claims to be
    line = np.outer(np.linspace(0, 1, 20), [1.0, 2.0, -0.5])
    assert RR.update(line, p[:20], False) is None and RR.update(p[:20], line, True) is None
    assert RR.update(p[:2], p[:2], False) is None and RR.update(p[:3], p[:3], False) is not None


def test_statement_recovers_a_planted_similarity():
    """Noise-free, full overlap: Q = T(P) rounded to fp32, the start 4 degrees, 0.02 and 2 % away.  The recovery error is
    the fp32 rounding of Q (6e-8 of a coordinate) averaged over 1500 points by the fit.  Measured here (this test prints it):
    rotation 9.3e-10, translation 7.2e-10, scale 1.5e-9; asserted at 4 x the largest of those, 6e-9."""
    rng = np.random.default_rng(3)
    P = rng.uniform(-1.0, 1.0, (1500, 3)).astype(np.float32)
    ang = np.radians(25.0)
    R = np.array([[np.cos(ang), -np.sin(ang), 0], [np.sin(ang), np.cos(ang), 0], [0, 0, 1.0]])
    axis = np.array([0.3, -0.5, 0.8]) / np.linalg.norm([0.3, -0.5, 0.8])
    K = np.array([[0, -axis[2], axis[1]], [axis[2], 0, -axis[0]], [-axis[1], axis[0], 0]])
    R = R @ (np.eye(3) + np.sin(0.4) * K + (1 - np.cos(0.4)) * K @ K)
    s, t = 1.7, np.array([0.5, -1.2, 0.3])
    Q = RR.apply((s, R, t), P).astype(np.float32)[rng.permutation(len(P))]
    d = np.radians(4.0)
    Rd = np.array([[1, 0, 0], [0, np.cos(d), -np.sin(d)], [0, np.sin(d), np.cos(d)]])
    ref = RR.icp(P, Q, 0.2, iterations=40, with_scale=True, tol=0.0, init=(s * 1.02, Rd @ R, t + [0.02, -0.01, 0.015]))
    err = (np.abs(ref.rotation - R).max(), np.abs(ref.translation - t).max(), abs(ref.scale - s))
    print(f"\nrecovery error: rotation {err[0]:.2e}, translation {err[1]:.2e}, scale {err[2]:.2e}; rmse {ref.rmse:.2e}, "
          f"fitness {ref.fitness}, {ref.iterations} iterations")
    assert ref.fitness == 1.0 and ref.n_inliers == len(P) and ref.flags == 0
    assert max(err) <= 6e-9
    # the rigid loop on a rigid plant, stopping on its own
    Q1 = RR.apply((1.0, R, t), P).astype(np.float32)
    hist = np.full((40, 4), -7.0)
    rigid = RR.icp(P, Q1, 0.2, iterations=40, tol=1e-3, init=(1.0, Rd @ R, t + [0.02, -0.01, 0.015]), history=hist)
    assert rigid.converged and 2 <= rigid.iterations < 40 and rigid.scale == 1.0
    assert (rigid.history[rigid.iterations:] == -7.0).all() and (rigid.history[:rigid.iterations, 3] == 0.0).all()
    assert np.abs(rigid.rotation - R).max() <= 1e-6
    m = rigid.iterations
    again = RR.icp(P, Q1, 0.2, iterations=m, tol=1e-3, init=(1.0, Rd @ R, t + [0.02, -0.01, 0.015]))
    assert again.iterations == m and np.array_equal(again.rotation, rigid.rotation) and again.converged


# ---- Mesh.sample_points ---------------------------------------------------------------------------------------------------------
def test_mesh_sample_points():
    from robosimgs_amd.mesh import Mesh
    rng = np.random.default_rng(4)
    v = rng.uniform(-2, 2, (30, 3)).astype(np.float32)
    f = np.array([rng.choice(30, 3, replace=False) for _ in range(40)])
    mesh = Mesh(v, f)
    a, b, c = mesh.sample_points(2000, seed=1), mesh.sample_points(2000, seed=1), mesh.sample_points(2000, seed=2)
    assert a.dtype == np.float32 and a.shape == (2000, 3) and np.array_equal(a, b) and not np.array_equal(a, c)
    assert mesh.sample_points(0).shape == (0, 3)
    # every sample is in the plane of, and inside, some face: barycentric coordinates against every face, in fp64
    v64 = v.astype(np.float64)
    A, B, C = v64[f[:, 0]], v64[f[:, 1]], v64[f[:, 2]]
    n = np.cross(B - A, C - A)
    n2 = (n * n).sum(1)
    worst = 0.0
    for p in a[:400].astype(np.float64):
        w = p - A
        gamma = (np.cross(B - A, w) * n).sum(1) / n2
        beta = (np.cross(w, C - A) * n).sum(1) / n2
        off = np.abs((w * n).sum(1)) / np.sqrt(n2)                                  # distance from each face's plane
        bad = np.maximum.reduce([off, np.maximum(0, -beta) * 4, np.maximum(0, -gamma) * 4, np.maximum(0, beta + gamma - 1) * 4])
        worst = max(worst, bad.min())
    assert worst <= 4 * 2.0**-23 * 4                                                # fp32 rounding of coordinates up to 2 (x4 slack)
    # two faces of area 3 : 1
    two = Mesh(np.array([[0, 0, 0], [3, 0, 0], [0, 2, 0], [5, 5, 5], [6, 5, 5], [5, 7, 5]], np.float32), np.array([[0, 1, 2], [3, 4, 5]]))
    N = 20000
    s = two.sample_points(N, seed=9)
    first = int((s[:, 2] < 1).sum())
    sigma = np.sqrt(N * 0.75 * 0.25)
    print(f"\nface counts {first} / {N - first}, expected {0.75 * N:.0f} +- {sigma:.1f}")
    assert abs(first - 0.75 * N) <= 5 * sigma
    # uniform inside a face: the mean of the samples is the centroid, to 5 sigma of a uniform triangle's spread
    big = s[s[:, 2] < 1].astype(np.float64)
    assert np.abs(big.mean(0) - [1.0, 2.0 / 3.0, 0.0]).max() <= 5 * 1.0 / np.sqrt(len(big))
    with pytest.raises(ValueError):
        Mesh(v, np.zeros((0, 3), np.int64)).sample_points(5)


# ---- Registration's host math ---------------------------------------------------------------------------------------------------
def test_registration_matrix_and_pose_and_pack_init():
    from robosimgs_amd.registration import Registration, pack_init, RESULT_DOUBLES
    rng = np.random.default_rng(6)
    R = np.linalg.qr(rng.normal(size=(3, 3)))[0]
    R *= np.sign(np.linalg.det(R))
    t, s = rng.normal(size=3), 1.37
    rec = np.zeros(RESULT_DOUBLES)
    rec[:9], rec[9:12], rec[12] = R.reshape(9), t, s
    rec[13:19] = [0.01, 0.75, 1500, 12, 1, 2]
    rec[19:23] = [0.0512, 10, 11, 12]
    hist = np.arange(80, dtype=np.float64).reshape(20, 4)
    reg = Registration(rec, hist)
    assert np.array_equal(reg.rotation, R) and np.array_equal(reg.translation, t) and reg.scale == s
    assert (reg.rmse, reg.fitness, reg.n_inliers, reg.iterations, reg.converged, reg.flags) == (0.01, 0.75, 1500, 12, True, 2)
    assert reg.cell_edge == 0.0512 and reg.grid_dims == (10, 11, 12)
    assert reg.history.shape == (12, 4) and np.array_equal(reg.history, hist[:12])
    M = reg.matrix()
    x = rng.normal(size=(5, 3))
    assert M.shape == (4, 4) and np.array_equal(M[3], [0, 0, 0, 1])
    assert np.abs((np.c_[x, np.ones(5)] @ M.T)[:, :3] - (s * x @ R.T + t)).max() <= 1e-14
    Rp, tp, sp = reg.pose()
    assert np.array_equal(Rp, R) and np.array_equal(tp, t) and sp == s
    Rp[0, 0] = 99.0                                                    # a copy: the record is not the caller's to edit
    assert reg.rotation[0, 0] == R[0, 0]
    # init in its three forms gives the same 13 doubles
    a, b, c = pack_init((R, t, s)), pack_init(M), pack_init((R, t))
    assert a.shape == (13,) and np.abs(a - b).max() <= 1e-14 and np.array_equal(a[:12], c[:12]) and c[12] == 1.0
    for bad in ((2 * R, t), (R * [1, 1, -1], t), np.eye(3), (R, t, -1.0), (R, t * np.nan)):
        with pytest.raises(ValueError):
            pack_init(bad)
