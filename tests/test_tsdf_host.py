"""TSDF fusion and surface extraction without a GPU: the fp64 statement's own properties (tests/tsdf_ref.py), the shipped tables
and per-point logic (robosimgs_amd/csrc/tsdf_tets.h, compiled with g++: tests/host_harness/tsdf_harness.cpp) against that
statement, a plain fp32 restatement of the integration against its counted bound, include/mgs_tsdf.h <-> libmgs.so <-> the
ctypes table, the three entry points' refusals (no launch: CPU-only) and Mesh.to_obj."""
import ctypes
import os
import re
import subprocess

import numpy as np
import pytest

import tsdf_ref as R

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
HEADER = os.path.join(ROOT, "include", "mgs_tsdf.h")
SRC = os.path.join(HERE, "host_harness", "tsdf_harness.cpp")


# ---- the reference's own properties -----------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def sphere():
    center, radius = np.array([9.2, 8.9, 8.4]), 6.3
    f, w = R.sphere_volume((19, 18, 17), radius, center)
    return R.extract(f, w, None, (0, 0, 0), 1.0), center, radius


def test_sphere_is_a_closed_outward_manifold(sphere):
    out, center, radius = sphere
    v, faces = out["vertices"], out["faces"]
    top = R.mesh_topology(faces, len(v))
    assert len(faces) > 1000 and top["closed"] and top["euler"] == 2 and top["unreferenced"] == 0
    normals = np.cross(v[faces[:, 1]] - v[faces[:, 0]], v[faces[:, 2]] - v[faces[:, 0]])
    assert ((normals * (v[faces].mean(1) - center)).sum(1) > 0).all()        # towards increasing tsdf: outward


def test_sphere_radial_error_meets_the_interpolation_bound(sphere):
    """A vertex is the root of the linear interpolant L of f = |x - c| - r along an edge of length h <= sqrt(3) voxels.  f's
    second derivative along any line is at most 1 / |x - c|, and every point of a crossed edge is within h of the surface, so
    |L - f| <= h^2 / (8 (r - h)) on the edge; f is the signed radial distance itself, so the radial error is |f(x*)| =
    |f(x*) - L(x*)|.  The fp32 rounding of the two samples moves L by at most U max|f| <= U h."""
    out, center, radius = sphere
    h = np.sqrt(3.0)
    bound = h * h / (8 * (radius - h)) + R.U * h
    err = np.abs(np.linalg.norm(out["vertices"] - center, axis=1) - radius).max()
    print(f"radial error {err:.4f} voxel, bound {bound:.4f}")
    assert 0 < err <= bound < 0.1


def test_random_volume_covers_every_tetrahedron_case():
    f, w, c = R.random_volume((9, 8, 7))
    out = R.extract(f, w, c, (0, 0, 0), 1.0)
    assert out["pairs"] == {(n, case) for n in range(6) for case in range(16)}
    assert R.mesh_topology(out["faces"], len(out["vertices"]))["unreferenced"] == 0
    assert sorted(len(R.case_triangles(case)) for case in range(16)) == [0, 0] + [1] * 8 + [2] * 6


def test_winding_of_one_inside_corner_is_the_permutation_parity_rule():
    """csrc/tsdf_tets.h's closed form for the one-corner cases: flipped iff parity(pi) (-1)^l is negative."""
    for n, perm in enumerate(R.PERMS):
        parity = round(np.linalg.det(np.eye(3)[list(perm)]))
        for l in range(4):
            assert R.WINDING[n, 1 << l] == (parity * (-1) ** l < 0), (n, l)
            assert R.WINDING[n, 15 ^ (1 << l)] != R.WINDING[n, 1 << l]


# ---- the shipped header, through g++ ----------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def harness(tmp_path_factory):
    so = tmp_path_factory.mktemp("tsdf_harness") / "libtsdf_harness.so"
    subprocess.run(["g++", "-O2", "-std=c++17", "-shared", "-fPIC", SRC, "-o", str(so)], check=True)
    lib = ctypes.CDLL(str(so))
    p, i, f, ll = ctypes.c_void_p, ctypes.c_int, ctypes.c_float, ctypes.c_longlong
    lib.th_tet_triangles.argtypes = [i, i, p]
    lib.th_tables.argtypes = [p, p]
    lib.th_extract.argtypes = [i, i, i, p, p, p, p, f, f, f, ll, ll, p, p, p, p]
    return lib


def _ptr(a):
    return None if a is None else a.ctypes.data_as(ctypes.c_void_p)


def harness_extract(lib, f, w, c, origin, voxel, level=0.0, min_weight=1.0, capacities=None, guard=0):
    """(vertices, faces, colors, counts, overflow) of th_extract; capacities None: the counts of a first call."""
    nz, ny, nx = f.shape
    f, w = np.ascontiguousarray(f, np.float32), np.ascontiguousarray(w, np.float32)
    c = None if c is None else np.ascontiguousarray(c, np.float32)
    origin = np.asarray(origin, np.float32)
    counts = np.zeros(2, np.int64)
    head = (nx, ny, nz, _ptr(f), _ptr(w), _ptr(c), _ptr(origin), voxel, level, min_weight)
    lib.th_extract(*head, 0, 0, None, None, None, _ptr(counts))
    cv, cf = (int(counts[0]), int(counts[1])) if capacities is None else capacities
    v = np.full((cv + guard, 3), -7, np.float32)
    col = None if c is None else np.full((cv + guard, 3), -7, np.float32)
    faces = np.full((cf + guard, 3), -7, np.int32)
    over = lib.th_extract(*head, cv, cf, _ptr(v), _ptr(col), _ptr(faces), _ptr(counts))
    return v, faces, col, counts, over


def test_harness_tables_match_the_reference(harness):
    corners, offsets = np.zeros((6, 4), np.int32), np.zeros(7, np.int32)
    harness.th_tables(_ptr(corners), _ptr(offsets))
    bits = lambda o: int(o[0]) | int(o[1]) << 1 | int(o[2]) << 2
    assert [[bits(R.TET_CORNERS[n][l]) for l in range(4)] for n in range(6)] == corners.tolist()
    assert [bits(o) for o in R.EDGE_OFFSETS] == offsets.tolist()
    for n in range(6):
        for case in range(16):
            pairs = np.zeros(6, np.int32)
            k = harness.th_tet_triangles(n, case, _ptr(pairs))
            got = [[(int(e) & 3, int(e) >> 2) for e in pairs[3 * t:3 * t + 3]] for t in range(k)]
            assert got == [[tuple(e) for e in tri] for tri in R.tet_triangles(n, case)], (n, case)      # count, pairs, winding


def _volumes():
    f, w = R.sphere_volume()
    yield "sphere", f, w, None, (0.0, 0.0, 0.0), 1.0
    f, w, c = R.random_volume((9, 8, 7), holes=0.15)
    yield "random with weight holes", f, w, c, (-0.3, 0.1, 2.0), 0.05
    yield ("values on the level",) + R.level_volume() + ((1.0, -2.0, 0.5), 0.02)
    f, w, c = R.random_volume((2, 2, 2), seed=4)
    yield "one cell", f, w, c, (0.0, 0.0, 0.0), 0.1
    yield "no crossing", np.ones((4, 3, 5), np.float32), np.ones((4, 3, 5), np.float32), None, (0.0, 0.0, 0.0), 0.1


def test_harness_extracts_whole_volumes_as_the_reference_does(harness):
    for name, f, w, c, origin, voxel in _volumes():
        ref = R.extract(f, w, c, origin, voxel)
        v, faces, col, counts, over = harness_extract(harness, f, w, c, origin, voxel)
        assert not over and counts.tolist() == [len(ref["vertices"]), len(ref["faces"])], name
        assert np.array_equal(faces, ref["faces"]), name
        assert (np.abs(v - ref["vertices"]) <= ref["vertex_bound"]).all(), name
        if c is not None:
            assert (np.abs(col - ref["colors"]) <= ref["color_bound"]).all(), name
        if name == "no crossing":
            assert len(v) == 0 and len(faces) == 0
        if name == "values on the level":                    # zero-area triangles are kept: the count is the reference's
            assert (np.linalg.norm(np.cross(v[faces[:, 1]] - v[faces[:, 0]], v[faces[:, 2]] - v[faces[:, 0]]), axis=1) == 0).any()


def test_harness_never_writes_past_a_capacity(harness):
    f, w, c = R.random_volume((9, 8, 7))
    full_v, full_f, full_c, counts, _ = harness_extract(harness, f, w, c, (0, 0, 0), 1.0)
    cv, cf = int(counts[0]) // 2, int(counts[1]) // 3
    v, faces, col, _, over = harness_extract(harness, f, w, c, (0, 0, 0), 1.0, capacities=(cv, cf), guard=8)
    assert over == 1
    assert (v[cv:] == -7).all() and (col[cv:] == -7).all() and (faces[cf:] == -7).all()
    assert np.array_equal(v[:cv], full_v[:cv]) and np.array_equal(faces[:cf], full_f[:cf])


def test_harness_main_runs_clean_under_the_sanitizers(tmp_path):
    """The stand-alone program: the whole extraction on volumes with weight holes and exact-level values, and exactly sized heap
    blocks of short capacities, built with -fsanitize=address,undefined and run as it is: any report aborts it."""
    exe = tmp_path / "tsdf_harness_main"
    subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-DTSDF_HARNESS_MAIN", "-fsanitize=address,undefined",
                    "-fno-sanitize-recover=all", SRC, "-o", str(exe)], check=True)
    r = subprocess.run([str(exe)], capture_output=True, text=True)
    assert r.returncode == 0 and r.stdout.strip().endswith("OK"), r.stdout + r.stderr


# ---- the integration's precision ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dims,n_views", R.FUSION_CASES)
def test_fp32_restatement_meets_integration_bound_with_nothing_excused(dims, n_views):
    case, ref = R.fusion_reference(dims, n_views)
    got = R.fuse(np.float32, case)
    rerun = lambda idx, flip: R.fuse(np.float64, case, ijk=R.grid_ijk(dims)[idx], flip=flip)
    res = R.check_integration(got["tsdf"].astype(np.float64), got["weight"].astype(np.float64), got["color"].astype(np.float64),
                              ref, rerun)
    print(dims, res, "largest bound", ref["bound"].max())
    assert res["excused"] == 0 and res["observed"] > 100 and res["worst"] <= 1.0
    # the inputs do what they are there for: the cap binds, some samples are seen once, some never, and the view that has
    # the volume behind it and the one that sees none of it update nothing
    assert ref["n_updates"].max() > R.MAX_WEIGHT and (ref["weight"] == 1).any() and (ref["n_updates"] == 0).any()
    assert ref["bound"].max() < 1e-4
    M = len(ref["tsdf"])
    for cam in range(n_views - (2 if n_views >= 5 else 1), n_views):
        alone = R.integrate(np.float64, R.grid_ijk(dims), np.zeros(M), np.zeros(M), None, case["origin"], case["voxel"],
                            case["trunc"], 2.0, case["depth"][cam:cam + 1], None, None, 0.5, 0.01, case["viewmats"][cam:cam + 1],
                            case["Ks"][cam:cam + 1])
        assert alone["n_updates"].sum() == 0


def test_a_flipped_decision_is_what_excuses_a_sample():
    """check_integration on a result that took one pixel decision the other way: excused where that decision is open, refused
    where it is not."""
    dims, n_views = R.FUSION_CASES[0]
    case, ref = R.fusion_reference(dims, n_views)
    ijk = R.grid_ijk(dims)
    rerun = lambda idx, flip: R.fuse(np.float64, case, ijk=ijk[idx], flip=flip)
    open_px = ref["open"]["px-"][0] | ref["open"]["px+"][0]
    flipped = R.fuse(np.float64, case, flip=(0, "px-"))
    changed = np.nonzero(np.abs(flipped["tsdf"] - ref["tsdf"]) > ref["bound"] + 1e-3)[0]
    closed = [m for m in changed if not open_px[m] and not ref["open"]["py-"][0][m] and not ref["open"]["py+"][0][m]]
    assert len(closed) > 0
    got = {k: ref[k].copy() for k in ("tsdf", "weight", "color")}
    m = closed[0]
    for k in got:
        got[k][..., m] = flipped[k][..., m]
    with pytest.raises(AssertionError, match=f"sample {m}"):
        R.check_integration(got["tsdf"], got["weight"], got["color"], ref, rerun)
    if open_px.any():
        m = np.nonzero(open_px)[0][0]
        kind = "px-" if ref["open"]["px-"][0][m] else "px+"
        flipped = R.fuse(np.float64, case, ijk=ijk[[m]], flip=(0, kind))
        got = {k: ref[k].copy() for k in ("tsdf", "weight", "color")}
        for k in got:
            got[k][..., m] = flipped[k][..., 0]
        assert R.check_integration(got["tsdf"], got["weight"], got["color"], ref, rerun)["excused"] <= 1


# ---- the ABI ------------------------------------------------------------------------------------------------------------------
def _declared():
    src = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    decls = re.findall(r"\b(?:int|void|size_t)\s+(mgs_\w+)\s*\(([^;]*?)\)\s*;", src, flags=re.S)
    return {name: len([a for a in args.split(",") if a.strip()]) for name, args in decls}


def test_tsdf_header_symbols_are_exported_and_bound_in_both_libraries():
    from robosimgs_amd import _lib
    from robosimgs_amd.csrc import build
    decl = _declared()
    assert sorted(decl) == sorted(_lib.TSDF_EXPORTS) == ["mgs_tsdf_extract_count", "mgs_tsdf_extract_emit", "mgs_tsdf_integrate"]
    assert not set(_lib.TSDF_EXPORTS) & set(_lib.EXPORTS) and len(_lib.EXPORTS) == 29
    for L in (_lib.lib(), _lib.debug_lib()):
        for name, nargs in decl.items():
            assert len(getattr(L, name).argtypes) == nargs, name
    nm = lambda path: subprocess.run(["nm", "-D", "--defined-only", path], capture_output=True, text=True).stdout
    for path in (_lib.LIB_PATH, _lib.DEBUG_LIB_PATH):
        assert all(name in nm(path) for name in decl), path
    header = open(HEADER).read()
    assert "MGS_VERSION" not in re.sub(r"/\*.*?\*/", "", header, flags=re.S)      # the version is mgs.h's alone
    assert int(re.search(r"#define\s+MGS_TSDF_STATUS_OVERFLOW\s+(\d+)u", header).group(1)) == _lib.TSDF_STATUS_OVERFLOW
    assert "tsdf.hip" in build.SOURCES


def test_volume_struct_matches_the_header():
    from robosimgs_amd import _lib
    src = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    body = re.search(r"typedef struct mgs_tsdf_volume \{(.*?)\} mgs_tsdf_volume;", src, flags=re.S).group(1)
    names = []
    for d in body.split(";"):
        if d.strip():
            names += [re.sub(r"[\s*]|\[\d+\]", "", n) for n in re.sub(r"^\s*(?:int|float)\s", "", d.strip()).split(",")]
    V = _lib.TsdfVolume
    assert names == [f[0] for f in V._fields_]
    assert [getattr(V, n).offset for n in names] == [0, 4, 8, 12, 24, 28, 32, 40, 48, 56] and ctypes.sizeof(V) == 64


def _volume(**kw):
    from robosimgs_amd import _lib
    f = dict(nx=4, ny=3, nz=2, origin=(ctypes.c_float * 3)(0, 0, 0), voxel_size=0.1, trunc=0.3, max_weight=64.0, tsdf=0x1000,
             weight=0x2000, color=0x3000)
    f.update(kw)
    return _lib.TsdfVolume(**f)


def _integrate(vol=None, n_cams=2, height=4, width=5, frames=0x4000, channels=4, alphas=None, alpha_min=0.5, near=0.01,
               viewmats=0x5000, Ks=0x6000, camera_model=0):
    from robosimgs_amd import _lib
    L = _lib.lib()
    rc = L.mgs_tsdf_integrate(None if vol is False else ctypes.byref(vol or _volume()), n_cams, height, width, frames, channels,
                              alphas, alpha_min, near, viewmats, Ks, camera_model, None)
    return rc, L.mgs_last_error_string()


@pytest.mark.parametrize("kw,word", [
    (dict(vol=False), b"vol is null"),
    (dict(vol=lambda: _volume(tsdf=None)), b"vol->tsdf"),
    (dict(vol=lambda: _volume(weight=None)), b"vol->weight"),
    (dict(vol=lambda: _volume(nx=0)), b"dimension"),
    (dict(vol=lambda: _volume(nx=2048, ny=2048, nz=512)), b"2^31 - 1"),
    (dict(vol=lambda: _volume(voxel_size=0.0)), b"voxel_size"),
    (dict(vol=lambda: _volume(voxel_size=float("nan"))), b"voxel_size"),
    (dict(vol=lambda: _volume(trunc=-0.1)), b"trunc"),
    (dict(vol=lambda: _volume(max_weight=0.5)), b"max_weight"),
    (dict(vol=lambda: _volume(max_weight=float("nan"))), b"max_weight"),
    (dict(n_cams=0), b"n_cams"),
    (dict(height=0), b"frame of"),
    (dict(frames=None), b"frames is null"),
    (dict(viewmats=None), b"viewmats"),
    (dict(Ks=None), b"Ks"),
    (dict(channels=3), b"frame_channels"),
    (dict(camera_model=1), b"MGS_CAMERA_PINHOLE"),
    (dict(camera_model=4), b"MGS_CAMERA_PINHOLE"),
])
def test_integrate_refuses_before_any_launch(kw, word):
    kw = {k: (v() if callable(v) else v) for k, v in kw.items()}
    rc, msg = _integrate(**kw)
    assert rc == -1 and word in msg, (rc, msg)


def test_extract_entry_points_refuse_before_any_launch():
    from robosimgs_amd import _lib
    L = _lib.lib()
    size = ctypes.c_size_t(0)
    assert L.mgs_tsdf_extract_count(ctypes.byref(_volume()), 0.0, 1.0, None, None, ctypes.byref(size), None) == 0    # the size query
    need = size.value
    assert need >= 4 * 3 * 2 * 6

    def count(vol=None, level=0.0, min_weight=1.0, counts=0x7000, workspace=0x8000, nbytes=need, size_ptr=True):
        n = ctypes.c_size_t(nbytes)
        rc = L.mgs_tsdf_extract_count(ctypes.byref(vol or _volume()), level, min_weight, counts, workspace,
                                      ctypes.byref(n) if size_ptr else None, None)
        return rc, L.mgs_last_error_string()

    for kw, rc_want, word in ((dict(vol=_volume(ny=-1)), -1, b"dimension"), (dict(vol=_volume(voxel_size=-1.0)), -1, b"voxel_size"),
                              (dict(vol=_volume(tsdf=None)), -1, b"vol->tsdf"), (dict(level=float("nan")), -1, b"level"),
                              (dict(min_weight=float("inf")), -1, b"min_weight"), (dict(counts=None), -1, b"counts"),
                              (dict(size_ptr=False), -1, b"workspace_bytes"), (dict(nbytes=need - 1), -2, b"workspace of")):
        rc, msg = count(**kw)
        assert rc == rc_want and word in msg, (kw, rc, msg)
    # trunc and max_weight are integration's: the extraction does not read them (the size query of such a volume succeeds)
    assert L.mgs_tsdf_extract_count(ctypes.byref(_volume(trunc=0.0, max_weight=0.0)), 0.0, 1.0, None, None, ctypes.byref(size), None) == 0

    def emit(vol=None, level=0.0, counts=0x7000, workspace=0x8000, nbytes=need, vertices=0x9000, colors=None, cap_v=10,
             faces=0xa000, cap_f=10, status=0xb000):
        rc = L.mgs_tsdf_extract_emit(ctypes.byref(vol or _volume()), level, 1.0, counts, workspace, nbytes, vertices, colors,
                                     cap_v, faces, cap_f, status, None)
        return rc, L.mgs_last_error_string()

    for kw, rc_want, word in ((dict(vol=_volume(nz=0)), -1, b"dimension"), (dict(level=float("inf")), -1, b"level"),
                              (dict(counts=None), -1, b"counts"), (dict(workspace=None), -1, b"workspace"),
                              (dict(vertices=None), -1, b"vertices"), (dict(faces=None), -1, b"faces"),
                              (dict(status=None), -1, b"status"), (dict(vol=_volume(color=None), colors=0xc000), -1, b"colour"),
                              (dict(cap_v=-1), -1, b"capacities"), (dict(cap_f=1 << 31), -1, b"capacities"),
                              (dict(nbytes=need - 1), -2, b"workspace of")):
        rc, msg = emit(**kw)
        assert rc == rc_want and word in msg, (kw, rc, msg)


def test_python_layer_refuses_lenses_and_cpu_volumes():
    import torch
    import robosimgs_amd
    from robosimgs_amd import TSDFVolume
    from robosimgs_amd._lib import MgsError
    assert TSDFVolume is robosimgs_amd.tsdf.TSDFVolume
    with pytest.raises(MgsError, match="GPU"):
        TSDFVolume((0, 0, 0), 0.1, (4, 4, 4), device="cpu")
    for kw in (dict(dims=(4, 4)), dict(dims=(0, 4, 4)), dict(dims=(2048, 2048, 512)), dict(voxel_size=0.0), dict(trunc=-1.0),
               dict(max_weight=0.0)):
        args = dict(origin=(0, 0, 0), voxel_size=0.1, dims=(4, 4, 4), device="cpu")
        args.update(kw)
        with pytest.raises(ValueError):
            TSDFVolume(**args)
    with pytest.raises(ValueError, match="lo < hi"):
        TSDFVolume.from_bounds((0, 0, 0), (1, 0, 1), 0.1)
    vol = TSDFVolume.__new__(TSDFVolume)                       # integrate's camera checks come before anything touches a buffer
    for kw in (dict(camera_model="fisheye"), dict(camera_model="ortho"), dict(distortion=torch.zeros(1, 4)),
               dict(pinhole_distortion=torch.zeros(1, 5))):
        with pytest.raises(NotImplementedError, match="pinhole"):
            vol.integrate(torch.zeros(1, 4, 4, 4), torch.eye(4)[None], torch.eye(3)[None], **kw)


# ---- Mesh.to_obj --------------------------------------------------------------------------------------------------------------
def test_to_obj_round_trips_through_from_obj(tmp_path):
    from robosimgs_amd import Mesh
    rng = np.random.default_rng(2)
    v = (rng.normal(size=(40, 3)) * [1e-3, 1.0, 1e3]).astype(np.float32)
    faces = rng.integers(0, 40, (60, 3)).astype(np.int32)
    colors = rng.uniform(0, 1, (40, 3)).astype(np.float32)
    for name, mesh in (("plain", Mesh(v, faces)), ("coloured", Mesh(v, faces, vertex_colors=colors))):
        path = str(tmp_path / f"{name}.obj")
        mesh.to_obj(path)
        back = Mesh.from_obj(path)
        assert np.array_equal(back.vertices.numpy(), v) and np.array_equal(back.faces.numpy(), faces), name
        rows = [l.split() for l in open(path) if l.startswith("v ")]
        assert len(rows) == 40 and all(len(r) == (7 if name == "coloured" else 4) for r in rows)
        if name == "coloured":
            assert np.array_equal(np.array([r[4:] for r in rows], np.float32), colors)
        assert min(int(t) for l in open(path) if l.startswith("f ") for t in l.split()[1:]) >= 1           # 1-based
