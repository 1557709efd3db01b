"""The mesh rasteriser under a lens without a GPU: robosimgs_amd/csrc/mesh_lens_raster.h -- the text csrc/mesh_lens.hip's
kernels are made of -- compiled with g++ (tests/host_harness/mesh_lens_harness.cpp walks the launches serially on heap buffers
of the ABI's sizes) and held to the fp64 statement of tests/mesh_lens_ref.py: the ray map's closed forms, its bound and its
valid set on the four test lenses; every raster case under each lens through check_raster and the resolve bounds; the box's
conservativeness against a walk of every block; the large-face threshold.  Then the C ABI (include/mgs_mesh_lens.h), the
Python layer's errors, and the stand-alone program under the address and undefined-behaviour sanitizers."""
import ctypes
import os
import re
import subprocess

import numpy as np
import pytest

import lens_ref as LR
import mesh_lens_ref as ML
import mesh_lens_scenes as LS
import mesh_ref as MR
import mesh_scenes as MS
import pinhole_lens_ref as PR

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LENS_NAMES = list(ML.LENSES)


@pytest.fixture(scope="module")
def harness(tmp_path_factory):
    """The harness built with plain g++ -O2 -ffp-contract=off: the fmas are the ones the headers write out."""
    return LS.build_harness(tmp_path_factory.mktemp("mesh_lens_harness"))


def _colors(n, seed):
    return np.random.default_rng(seed).uniform(0.0, 1.0, (n, 3)).astype(np.float32)


def _d32(K, W, H):
    """d as the kernel forms it, float32 [H,W,2]."""
    K = np.asarray(K, np.float32)
    x, y = np.meshgrid(np.arange(W, dtype=np.float32) + np.float32(0.5), np.arange(H, dtype=np.float32) + np.float32(0.5))
    return np.stack([(x - K[0, 2]) / K[0, 0], (y - K[1, 2]) / K[1, 1]], -1)


# ---- the ray map ------------------------------------------------------------------------------------------------------------------
def test_zero_coefficients_give_the_pixel_itself_to_one_ulp(harness):
    W, H = 37, 29
    K = ML.intrinsics("bc_mild", W, H)
    row = PR.lens_row(K, (0.0, 0.0, 0.0, 0.0, 0.0)).astype(np.float32)
    assert row[14] == np.finfo(np.float32).max                                     # no fold
    rays, _, _ = LS.harness_rays(harness, ML.BC, row, W, H)
    d = _d32(K, W, H)
    assert not np.isnan(rays).any()
    assert (np.abs(rays[0] - d) <= np.spacing(np.abs(d))).all()
    # the ideal fisheye is MGS_CAMERA_FISHEYE_KB with every k zero: q = d tan|d| / |d|, nothing beyond 90 degrees
    K = np.array([[9.0, 0, 18.5], [0, 9.0, 14.5], [0, 0, 1]], np.float32)        # |d| up to 2.6: past pi / 2
    rays, _, _ = LS.harness_rays(harness, ML.KB, LR.lens_row(K, (0.0, 0.0, 0.0, 0.0)).astype(np.float32), W, H)
    d = ML.pixel_d(K, W, H)
    rd = np.hypot(d[..., 0], d[..., 1])
    has = ~np.isnan(rays[0]).any(-1)
    assert np.array_equal(has, rd < 0.5 * np.pi) and has.any() and not has.all()
    want = d * (np.tan(rd) / np.where(rd > 0, rd, 1.0))[..., None]
    ref = ML.RayRef(ML.KB, K, (0.0, 0.0, 0.0, 0.0), W, H)
    near = ref.near_fold
    assert (np.abs(rays[0] - want)[has & ~near] <= ref.bound[has & ~near]).all()


def test_pure_k1_lens_is_its_cubics_root_and_the_round_trip_closes(harness):
    W, H = 112, 80
    k1 = -0.2
    k = (k1, 0.0, 0.0, 0.0, 0.0)
    K = PR.intrinsics("mild", W, H).astype(np.float32)
    rays, _, _ = LS.harness_rays(harness, ML.BC, PR.lens_row(K, k).astype(np.float32), W, H)
    d = ML.pixel_d(K, W, H)
    rd = np.hypot(d[..., 0], d[..., 1])
    q = rays[0].astype(np.float64)
    r = np.hypot(q[..., 0], q[..., 1])
    assert not np.isnan(rays).any()                                                # the fold (u = 1 / 0.6) is outside this frame
    for y, x in [(0, 0), (79, 111), (40, 57), (10, 100), (70, 3), (39, 56)]:
        roots = np.roots([k1, 0.0, 1.0, -rd[y, x]])
        root = min(v.real for v in roots if abs(v.imag) < 1e-12 and v.real > 0)   # the branch through the origin
        slope = 1.0 + 3.0 * k1 * root * root                                       # d r_d / d r
        assert abs(r[y, x] - root) <= (3 * MR.gamma(11) * (root + abs(k1) * root ** 3) + MR.gamma(2) * rd[y, x]) / slope * 1.01
    # D(q) = d, to the residual the statement allows
    xd, yd, _, _ = PR.distort(q[..., 0], q[..., 1], k)
    res = 3 * MR.gamma(11) * ML._bc_abs(q[..., 0], q[..., 1], k) + MR.gamma(2) * np.abs(d).max(-1)
    assert (np.maximum(np.abs(xd - d[..., 0]), np.abs(yd - d[..., 1])) <= res).all()


def test_the_kernels_evaluation_of_D_stays_inside_its_counted_bound(harness):
    """The residual threshold is twice the bound of one fp32 evaluation: that bound has to hold."""
    rng = np.random.default_rng(2)
    out = (ctypes.c_float * 3)()
    for k in (PR.MILD, PR.FOLDING):
        kk = np.asarray(PR.full(k), np.float32)
        for a, b in rng.uniform(-1.2, 1.2, (200, 2)).astype(np.float32):
            harness.mlh_distort(ML.BC, kk.ctypes.data_as(ctypes.c_void_p), float(a), float(b), out)
            xd, yd, _, _ = PR.distort(float(a), float(b), kk.astype(np.float64))
            assert max(abs(out[0] - xd), abs(out[1] - yd)) <= out[2]
    for k in (LR.MILD, LR.FOLDING):
        kk = np.asarray(k, np.float32)
        for t in rng.uniform(0.0, 1.57, 200).astype(np.float32):
            harness.mlh_distort(ML.KB, kk.ctypes.data_as(ctypes.c_void_p), float(t), 0.0, out)
            assert abs(out[0] - float(t) * ML._kb_P(kk.astype(np.float64), float(t) ** 2)) <= out[2]


@pytest.mark.parametrize("lens", LENS_NAMES)
@pytest.mark.parametrize("size", LS.SIZES)
def test_rays_stay_inside_their_bound_and_the_valid_set_is_the_references(harness, lens, size):
    W, H = size
    model, k, K, row = LS.camera(lens, W, H)
    rays, blocks, supers = LS.harness_rays(harness, model, row, W, H)
    ref = ML.RayRef(model, K, k, W, H)
    got = ref.check_rays(rays[0])
    has = ~np.isnan(rays[0]).any(-1)
    # on these lenses the fold's neighbourhood hides nothing: the valid sets are equal pixel for pixel
    assert np.array_equal(has, ref.valid), int((has != ref.valid).sum())
    if (lens, size) == ("bc_folding", (112, 80)):
        assert got["valid"] == 3326                                                # of 8960: the fold is inside the frame
    if "folding" in lens:
        assert 0 < got["valid"] < W * H
    else:
        assert got["valid"] == W * H
    # the block tables: every valid ray inside its block's and its superblock's rectangle; empty exactly where no pixel is valid
    (BY, BX), (SY, SX) = LS.table_shapes(W, H)
    for by in range(BY):
        for bx in range(BX):
            own = rays[0, 8 * by:8 * by + 8, 8 * bx:8 * bx + 8].reshape(-1, 2)
            own = own[~np.isnan(own).any(1)]
            ring = rays[0, max(8 * by - 1, 0):8 * by + 9, max(8 * bx - 1, 0):8 * bx + 9].reshape(-1, 2)
            ring = ring[~np.isnan(ring).any(1)]
            b, s = blocks[0, by, bx], supers[0, by // 8, bx // 8]
            if len(own) == 0:
                assert np.array_equal(b, np.array([np.inf, np.inf, -np.inf, -np.inf], np.float32))
                continue
            assert np.array_equal(b, np.concatenate([ring.min(0), ring.max(0)]))
            assert (s[:2] <= b[:2]).all() and (s[2:] >= b[2:]).all()


# ---- raster and resolve -------------------------------------------------------------------------------------------------------------
def _render_and_check(harness, lens, W, H, c, name, **shade):
    model, k, K, row = LS.camera(lens, W, H)
    kw = dict(near=c["near"], far=c["far"], cull=c["cull"], **shade)
    o = LS.harness_render(harness, c["verts"], c["faces"], MS.IDENTITY_VIEW, model, row, W, H, **kw)
    assert np.array_equal(o["verts_cam"][0], c["verts"]), name
    R = ML.LensRasterRef(o["verts_cam"][0], c["faces"], o["rays"][0], W, H, c["near"], c["far"], c["cull"])
    assert R.tolerance_share() <= 0.02, (name, R.tolerance_share())
    ids, depth = o["face_ids"][0], o["depth"][0]
    r = R.check_raster(ids, depth)
    MS.check_shading(R, r, c["faces"], o["rgb"][0], o["normals"][0], **shade)
    assert (depth[ids < 0] == 0).all() and (depth[ids >= 0] > 0).all()
    assert (ids[np.isnan(o["rays"][0]).any(-1)] == -1).all(), name                # a pixel without a ray is uncovered
    # the box is conservative: a walk of every block of the image for every face leaves the same visibility buffer
    b = LS.harness_render(harness, c["verts"], c["faces"], MS.IDENTITY_VIEW, model, row, W, H, every_block=True, **kw)
    assert np.array_equal(ids, b["face_ids"][0]) and np.array_equal(depth.view(np.uint32), b["depth"][0].view(np.uint32)), name
    assert o["keys"][0] <= b["keys"][0]
    return o, R


@pytest.mark.parametrize("lens", LENS_NAMES)
@pytest.mark.parametrize("size", LS.SIZES)
def test_every_raster_case_passes_the_statement_and_the_box_is_conservative(harness, lens, size):
    W, H = size
    cases = dict(MR.raster_cases(W, H))
    cases.update(LS.spanning_cases(lens, W, H))
    covered = 0
    for name, c in cases.items():
        o, R = _render_and_check(harness, lens, W, H, c, name, vertex_colors=_colors(len(c["verts"]), 5), headlight=True, ambient=0.25)
        ids = o["face_ids"][0]
        covered += int((ids >= 0).sum())
        if c.get("identical"):
            assert (ids[ids >= 0] % 2 == 0).all(), name
        if "only_face" in c:
            assert set(np.unique(ids)) <= {-1, c["only_face"]}, name
        if c.get("bad_index"):
            assert not np.isin(ids, np.arange(0, len(c["faces"]), 3)).any(), name
        if name in ("full_image_plus_64", "near_crossing_spans_frame"):
            has = ~np.isnan(o["rays"][0]).any(-1)
            assert np.array_equal(ids >= 0, has), name                             # covers every pixel that has a ray, and no other
    assert covered > 0


def test_faces_on_both_sides_of_the_large_face_threshold(harness):
    """Faces the harness itself reports at 14, 15 and 16 blocks: only the 16-block one goes to the list.  (128 x 128: under the
    folding lenses the rays of a 64 x 64 frame span six blocks, and 14 is 2 x 7.)"""
    W = H = 128
    for lens in LENS_NAMES:
        model, k, K, row = LS.camera(lens, W, H)
        v, f = LS.threshold_candidates(lens, W, H)
        nb = LS.harness_render(harness, v, f, MS.IDENTITY_VIEW, model, row, W, H)["face_blocks"][0]
        pick = [int(np.flatnonzero(nb == n)[0]) for n in (14, 15, 16)]             # IndexError: the candidates miss a count
        verts = np.concatenate([v[3 * p:3 * p + 3] for p in pick])
        c = dict(verts=verts, faces=np.arange(9, dtype=np.int32).reshape(3, 3), near=0.01, far=1e10, cull=False)
        o, R = _render_and_check(harness, lens, W, H, c, lens, face_colors=_colors(3, 1))
        assert o["face_blocks"][0].tolist() == [14, 15, 16] and o["listed"][0] == 1
        assert set(np.unique(o["face_ids"])) == {-1, 0, 1, 2}


# ---- the C ABI ------------------------------------------------------------------------------------------------------------------
def _declared():
    src = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "mgs_mesh_lens.h")).read(), flags=re.S)
    decls = re.findall(r"\bint\s+(mgs_\w+)\s*\(([^;]*?)\)\s*;", src, flags=re.S)
    return {name: len([a for a in args.split(",") if a.strip()]) for name, args in decls}


def test_abi_header_library_and_binding_agree():
    from robosimgs_amd import _lib
    from robosimgs_amd.csrc import build
    assert "mesh_lens.hip" in build.SOURCES
    decl = _declared()
    assert sorted(decl) == sorted(_lib.MESH_LENS_EXPORTS) and len(decl) == 5
    for L in (_lib.lib(), _lib.debug_lib()):
        for name, nargs in decl.items():
            assert len(getattr(L, name).argtypes) == nargs, name
    header = open(os.path.join(ROOT, "include", "mgs_mesh_lens.h")).read()
    defs = {m.group(1): int(m.group(2)) for m in re.finditer(r"^#define\s+MGS_MESH_LENS_(\w+)\s+(\d+)\b", header, flags=re.M)}
    assert defs == {"NEWTON_STEPS": _lib.MESH_LENS_NEWTON_STEPS, "SUPERBLOCK": _lib.MESH_LENS_SUPERBLOCK}
    assert "MGS_VERSION" not in re.sub(r"/\*.*?\*/", "", header, flags=re.S)        # the version is mgs.h's
    # mgs.h and mgs_mesh.h are as they were: 29 and 5 declarations
    for name, n in (("mgs.h", 29), ("mgs_mesh.h", 5)):
        src = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", name)).read(), flags=re.S)
        assert len(re.findall(r"\b(?:int|size_t|const char \*)\s*\*?(mgs_\w+)\s*\(", src)) == n, name


def test_abi_workspace_bytes_is_the_documented_layout(harness):
    from robosimgs_amd import _lib
    L = _lib.lib()
    up = lambda v: (v + 255) // 256 * 256
    for C, W, H in ((1, 1, 1), (2, 37, 29), (1, 1920, 1080), (1, 3840, 2160), (3, 16368, 16368)):
        n = ctypes.c_size_t(0)
        assert L.mgs_mesh_lens_workspace_bytes(C, W, H, ctypes.byref(n)) == 0
        (BY, BX), (SY, SX) = LS.table_shapes(W, H)
        want = [0, up(8 * C * H * W), up(8 * C * H * W) + up(16 * C * BY * BX)]
        assert n.value == want[2] + up(16 * C * SY * SX)
        lay = (ctypes.c_size_t * 4)()
        harness.mlh_workspace_layout(C, W, H, lay)
        assert list(lay) == want + [n.value]
    assert LS.table_shapes(1920, 1080)[1] == (17, 30) and LS.table_shapes(3840, 2160)[1] == (34, 60)     # 510 and 2040 superblocks


def test_abi_refuses_bad_arguments_with_a_message():
    from robosimgs_amd import _lib
    L = _lib.lib()
    msg = lambda: L.mgs_last_error_string()
    n = ctypes.c_size_t(0)
    big = 1 << 40                                    # never dereferenced: every call below is refused before a launch
    rays = lambda **kw: L.mgs_mesh_lens_rays(*[{**dict(C=1, model=4, rows=0x300, W=64, H=64, lws=0x2000, lbytes=big, stream=None),
                                                  **kw}[k] for k in ("C", "model", "rows", "W", "H", "lws", "lbytes", "stream")])
    assert rays(model=1) == -3 and b"ORTHO" in msg()
    assert rays(model=0) == -3 and b"no lens row" in msg()
    assert rays(model=2) == -3 and b"no lens row" in msg()
    assert rays(model=7) == -1 and b"not a camera model" in msg()
    assert rays(rows=None) == -1 and b"lens_rows is null" in msg()
    assert rays(lws=None) == -1 and b"lens_workspace is null" in msg()
    assert rays(lws=0x2001) == -1 and b"aligned" in msg()
    assert rays(lbytes=100) == -1 and b"needed" in msg()
    assert rays(W=16369) == -1 and b"16368" in msg()
    assert rays(C=0) == -1 and b"n_cams" in msg()
    assert L.mgs_mesh_lens_workspace_bytes(1, 0, 8, ctypes.byref(n)) == -1 and b"16368" in msg()
    assert L.mgs_mesh_lens_workspace_bytes(1, 8, 8, None) == -1 and b"null" in msg()
    names = ("C", "V", "vc", "F", "faces", "model", "rows", "W", "H", "near", "far", "cull", "ws", "nbytes", "lws", "lbytes", "stream")
    raster = lambda **kw: L.mgs_mesh_raster_lens(*[{**dict(C=1, V=3, vc=0x100, F=1, faces=0x200, model=3, rows=0x300, W=64, H=64,
                                                             near=0.01, far=1e10, cull=0, ws=0x1000, nbytes=big, lws=0x2000,
                                                             lbytes=big, stream=None), **kw}[k] for k in names])
    assert raster(vc=None) == -1 and b"null" in msg()
    assert raster(rows=None) == -1 and b"lens_rows is null" in msg()
    assert raster(model=1) == -3 and b"ORTHO" in msg()
    assert raster(ws=None) == -1 and b"workspace is null" in msg()
    assert raster(lws=None) == -1 and b"lens_workspace is null" in msg()
    assert raster(lbytes=100) == -1 and b"lens_workspace of 100 bytes" in msg()
    assert raster(nbytes=100) == -1 and b"workspace of 100 bytes" in msg()
    assert raster(near=0.0) == -1 and b"near_plane" in msg()
    assert raster(far=0.001) == -1 and b"far_plane" in msg()
    assert raster(F=0) == -1 and b"F 0" in msg()
    names = ("C", "V", "vc", "F", "faces", "vcol", "fcol", "model", "rows", "W", "H", "light", "ambient", "ws", "nbytes", "lws",
             "lbytes", "rgb", "depth", "ids", "normals", "stream")
    resolve = lambda **kw: L.mgs_mesh_resolve_lens(*[{**dict(C=1, V=3, vc=0x100, F=1, faces=0x200, vcol=None, fcol=None, model=4,
                                                               rows=0x300, W=64, H=64, light=0, ambient=0.3, ws=0x1000, nbytes=big,
                                                               lws=0x2000, lbytes=big, rgb=0x400, depth=0x500, ids=0x600,
                                                               normals=None, stream=None), **kw}[k] for k in names])
    assert resolve(rgb=None) == -1 and b"output" in msg()
    assert resolve(ambient=1.5) == -1 and b"ambient" in msg()
    assert resolve(model=9) == -1 and b"not a camera model" in msg()
    assert resolve(lws=0x2010) == -1 and b"aligned" in msg()
    # the fused call checks everything before its first launch
    fused = lambda **kw: L.mgs_rasterize_mesh_lens(*[{**dict(
        C=1, V=3, v=0x100, link=None, L=0, R=None, t=None, s=None, vm=0x200, model=4, rows=0x300, F=1, faces=0x400, vcol=None,
        fcol=None, W=64, H=64, near=0.01, far=1e10, cull=0, light=0, ambient=0.3, ws=0x1000, nbytes=big, lws=0x2000, lbytes=big,
        vc=0x500, rgb=0x600, depth=0x700, ids=0x800, normals=None, stream=None), **kw}[k] for k in (
        "C", "V", "v", "link", "L", "R", "t", "s", "vm", "model", "rows", "F", "faces", "vcol", "fcol", "W", "H", "near", "far",
        "cull", "light", "ambient", "ws", "nbytes", "lws", "lbytes", "vc", "rgb", "depth", "ids", "normals", "stream")])
    assert fused(ambient=2.0) == -1 and b"ambient" in msg()
    assert fused(model=1) == -3 and b"ORTHO" in msg()
    assert fused(rows=None) == -1 and b"lens_rows is null" in msg()
    assert fused(lbytes=8) == -1 and b"lens_workspace of 8 bytes" in msg()
    assert fused(L=2) == -1 and b"links" in msg()
    assert fused(ids=None) == -1 and b"output" in msg()


# ---- the Python layer's errors --------------------------------------------------------------------------------------------------------
def test_python_layer_raises_before_any_launch():
    import torch
    import robosimgs_amd
    from robosimgs_amd import mesh_render as M
    from robosimgs_amd.mesh import Mesh, Texture
    assert robosimgs_amd.mesh_lens_rays is M.mesh_lens_rays and robosimgs_amd.MeshLensMap is M.MeshLensMap
    mesh = Mesh(np.zeros((3, 3), np.float32), np.array([[0, 1, 2]]))
    vm, K = np.eye(4, dtype=np.float32), MR.pinhole(32, 32)
    with pytest.raises(NotImplementedError, match="ortho"):
        M.rasterize_mesh(mesh, vm, K, 32, 32, camera_model="ortho")
    with pytest.raises(NotImplementedError, match="ortho"):
        M.MeshRenderer(mesh, 32, 32, camera_model="ortho")
    with pytest.raises(ValueError, match="camera_model"):
        M.rasterize_mesh(mesh, vm, K, 32, 32, camera_model="panorama")
    with pytest.raises(ValueError, match="needs camera_model='pinhole'"):
        M.rasterize_mesh(mesh, vm, K, 32, 32, camera_model="fisheye", pinhole_distortion=PR.MILD)
    with pytest.raises(ValueError, match="needs camera_model='fisheye'"):
        M.rasterize_mesh(mesh, vm, K, 32, 32, distortion=LR.MILD)
    with pytest.raises(ValueError, match="give one of them"):
        M.rasterize_mesh(mesh, vm, K, 32, 32, distortion=LR.MILD, pinhole_distortion=PR.MILD)
    with pytest.raises(ValueError, match="pinhole_distortion must be"):
        M.rasterize_mesh(mesh, vm, K, 32, 32, pinhole_distortion=[0.1, 0.2])
    with pytest.raises(ValueError, match="finite"):
        M.rasterize_mesh(mesh, vm, K, 32, 32, pinhole_distortion=[float("nan"), 0, 0, 0, 0])
    # a lens is accepted up to the check that the mesh is on the GPU; all-zero coefficients select the plain path
    with pytest.raises(ValueError, match="CPU"):
        M.rasterize_mesh(mesh, vm, K, 32, 32, pinhole_distortion=PR.MILD)
    with pytest.raises(ValueError, match="CPU"):
        M.MeshRenderer(mesh, 32, 32, camera_model="fisheye", distortion=LR.FOLDING)
    assert M._lens_model("pinhole", None, (0.0,) * 5) is None and M._lens_model("pinhole", None, None) is None
    assert M._lens_model("pinhole", None, PR.MILD) == ML.BC and M._lens_model("fisheye", LR.MILD, None) == ML.KB
    assert M._lens_model("fisheye", None, None) == ML.KB and M._lens_model("fisheye", (0.0,) * 4, None) == ML.KB
    # a textured mesh under a lens is not built
    tex = Texture(np.full((2, 2, 4), 255, np.uint8))
    textured = Mesh(np.zeros((3, 3), np.float32), np.array([[0, 1, 2]]), face_uvs=np.zeros((1, 3, 2), np.float32),
                    face_textures=np.zeros(1, np.int32), textures=[tex])
    assert textured.has_textures
    with pytest.raises(NotImplementedError, match="textured mesh under a lens"):
        M.MeshRenderer(textured, 32, 32, pinhole_distortion=PR.MILD)
    # the stage operators
    with pytest.raises(ValueError, match="needs a lens"):
        M.mesh_lens_rays(torch.eye(3)[None], 32, 32)
    with pytest.raises(NotImplementedError, match="ortho"):
        M.mesh_lens_rays(torch.eye(3)[None], 32, 32, camera_model="ortho")
    with pytest.raises(ValueError, match="CPU tensor"):
        M.mesh_lens_rays(torch.eye(3)[None], 32, 32, pinhole_distortion=PR.MILD)
    assert M.mesh_lens_workspace_bytes(1, 32, 32) == 8 * 32 * 32 + 256 + 256
    with pytest.raises(ValueError, match="each side"):
        M.mesh_lens_workspace_bytes(1, 0, 32)


# ---- the sanitizers -----------------------------------------------------------------------------------------------------------------
def test_stand_alone_program_is_clean_under_address_and_undefined_sanitizers(tmp_path):
    """tests/host_harness/mesh_lens_harness_main.cpp (its own main; host code only) with the harness, built with
    -fsanitize=address,undefined and run as it is on its hostile inputs: any report aborts it."""
    exe = tmp_path / "mesh_lens_sanitized"
    subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-ffp-contract=off", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                    LS.HARNESS, os.path.join(LS.HERE, "host_harness", "mesh_lens_harness_main.cpp"), "-o", str(exe)], check=True)
    r = subprocess.run([str(exe)], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    assert re.search(r"mesh lens harness: 20 scenes, \d+ covered, 0 bad", r.stdout), r.stdout
