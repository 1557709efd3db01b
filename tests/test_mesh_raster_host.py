"""The mesh rasteriser without a GPU: robosimgs_amd/csrc/mesh_raster.h -- the text csrc/mesh.hip's kernels are made of --
compiled with g++ (tests/host_harness/mesh_harness.cpp walks the five launches serially on heap buffers of the ABI's sizes)
and held to the fp64 statement of tests/mesh_ref.py: every raster case at both sizes, the wide image, the threshold boxes
and the six views of the pin through check_raster and shade_ref.  Then the C ABI (include/mgs_mesh.h) -- the workspace
layout, the refusals with their messages -- and the Python layer's ValueErrors, none of which needs a GPU."""
import ctypes
import os
import re

import numpy as np
import pytest

import mesh_ref as MR
import mesh_scenes as MS

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def harness(tmp_path_factory):
    """The harness built with plain g++ -O2 -ffp-contract=off: the fmas are the ones the header writes out."""
    return MS.build_harness(tmp_path_factory.mktemp("mesh_harness"))


@pytest.fixture(scope="module")
def openbox():
    return MS.openbox()


def _colors(n, seed):
    return np.random.default_rng(seed).uniform(0.0, 1.0, (n, 3)).astype(np.float32)


@pytest.mark.parametrize("size", [(37, 29), (64, 64)])
def test_harness_passes_check_raster_and_shade_ref_on_every_raster_case(harness, size):
    W, H = size
    for name, c in MR.raster_cases(W, H).items():
        vcol = _colors(len(c["verts"]), 5)
        o = MS.harness_render(harness, c["verts"], c["faces"], MS.IDENTITY_VIEW, c["K"][None], W, H, near=c["near"], far=c["far"],
                              cull=c["cull"], vertex_colors=vcol)
        assert np.array_equal(o["verts_cam"][0], c["verts"]), name                 # static under the identity: copied
        R = MR.RasterRef(o["verts_cam"][0], c["faces"], c["K"], W, H, c["near"], c["far"], c["cull"])
        assert R.tolerance_share() <= 0.02, (name, R.tolerance_share())
        ids, depth = o["face_ids"][0], o["depth"][0]
        r = R.check_raster(ids, depth)
        MS.check_shading(R, r, c["faces"], o["rgb"][0], o["normals"][0], vertex_colors=vcol)
        assert (depth[ids < 0] == 0).all() and (depth[ids >= 0] > 0).all()
        if c.get("identical"):
            assert (ids[ids >= 0] % 2 == 0).all() and (ids >= 0).any(), name        # the lower index of every pair
        if "only_face" in c:
            assert set(np.unique(ids)) == {-1, c["only_face"]}, name
        if c.get("bad_index"):
            assert not np.isin(ids, np.arange(0, len(c["faces"]), 3)).any(), name   # faces naming vertex V never win
        if name == "full_image_plus_64":
            assert (ids >= 0).all() and o["listed"][0] == 1
        if name == "threshold_blocks":
            assert c["blocks"] == [14, 15, 16] and o["listed"][0] == 1              # only the 16-block box is past the threshold of 15
    assert ("threshold_blocks" in MR.raster_cases(W, H)) == (size == (64, 64))


def test_harness_threshold_boxes_wide_image_and_every_colour_mode(harness):
    # boxes just under, at and just over the kernel's own large-face threshold
    c = MS.own_threshold_case()
    o = MS.harness_render(harness, c["verts"], c["faces"], MS.IDENTITY_VIEW, c["K"][None], 64, 64)
    R = MR.RasterRef(o["verts_cam"][0], c["faces"], c["K"], 64, 64)
    R.check_raster(o["face_ids"][0], o["depth"][0])
    assert o["listed"][0] == 1 and set(np.unique(o["face_ids"])) == {-1, 0, 1, 2}
    # 258 blocks across: past any 8-bit block coordinate
    c = MS.wide_case()
    o = MS.harness_render(harness, c["verts"], c["faces"], MS.IDENTITY_VIEW, c["K"][None], c["width"], c["height"])
    R = MR.RasterRef(o["verts_cam"][0], c["faces"], c["K"], c["width"], c["height"])
    assert R.tolerance_share() <= 0.02
    R.check_raster(o["face_ids"][0], o["depth"][0])
    assert (o["face_ids"] >= 0).all() and o["listed"][0] >= 1
    # vertex colours, face colours and none, the headlight off and on
    c = MR.raster_cases(64, 64)["random129"]
    R = MR.RasterRef(c["verts"], c["faces"], c["K"], 64, 64)
    for kw in (dict(vertex_colors=_colors(len(c["verts"]), 1)), dict(face_colors=_colors(len(c["faces"]), 2)), dict()):
        for light in (dict(), dict(headlight=True, ambient=0.25)):
            o = MS.harness_render(harness, c["verts"], c["faces"], MS.IDENTITY_VIEW, c["K"][None], 64, 64, **kw, **light)
            r = R.check_raster(o["face_ids"][0], o["depth"][0])
            MS.check_shading(R, r, c["faces"], o["rgb"][0], o["normals"][0], **kw, **light)


def test_harness_vertex_stage_stays_inside_the_counted_bound(harness):
    rng = np.random.default_rng(3)
    verts = rng.normal(size=(50, 3)).astype(np.float32)
    link = rng.integers(-1, 2, 50).astype(np.int32)
    link[:4] = [2, 7, -2, -5]                                                       # outside 0 .. L-1: static
    Rm = np.stack([MS.rotation_about([0.2, -0.5, 0.8], 0.7), MS.rotation_about([1.0, 0.3, 0.1], -1.1)]).astype(np.float32)
    t, s = rng.normal(size=(2, 3)).astype(np.float32), np.array([1.7, 0.6], np.float32)
    vm = np.stack([np.eye(4), np.eye(4)]).astype(np.float32)
    vm[1, :3, :3] = MS.rotation_about([0.1, 0.9, 0.2], 0.4)
    vm[1, :3, 3] = [0.5, -0.5, 4.0]
    K = np.stack([MR.pinhole(8, 8)] * 2)
    o = MS.harness_render(harness, verts, np.array([[0, 1, 2]], np.int32), vm, K, 8, 8, link_ids=link, rotations=Rm,
                          translations=t, scales=s)
    cam, bound = MR.vertex_ref(verts, link, Rm, t, s, vm)
    assert (np.abs(o["verts_cam"] - cam) <= bound).all()
    static = (link < 0) | (link >= 2)
    assert static[:4].all() and np.array_equal(o["verts_cam"][0][static], verts[static])    # identity view: bit for bit


def test_harness_matches_the_pin_on_all_six_views(harness, openbox):
    """On the reference's own renders of the open box the xor is <= PIN[name] + d, d the pixels whose coverage differs
    from the fp64 statement's (check_raster has confined those to pixels without a certain face)."""
    seen = {}
    for name, v in openbox["views"].items():
        o = MS.harness_render(harness, openbox["verts"], openbox["faces"], v["viewmat"][None], v["K"][None], 800, 800,
                              headlight=True)
        R = MR.RasterRef(o["verts_cam"][0], openbox["faces"], v["K"], 800, 800)
        assert R.tolerance_share() <= 0.02, (name, R.tolerance_share())
        r = R.check_raster(o["face_ids"][0], o["depth"][0])
        MS.check_shading(R, r, openbox["faces"], o["rgb"][0], o["normals"][0], headlight=True)
        seen[name] = MS.check_pin(R, o["face_ids"][0], v["silhouette"], name)
    print("\n(xor, d) per view:", seen)


# ---- the C ABI ------------------------------------------------------------------------------------------------------------------
def _declared():
    src = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "mgs_mesh.h")).read(), flags=re.S)
    decls = re.findall(r"\bint\s+(mgs_\w+)\s*\(([^;]*?)\)\s*;", src, flags=re.S)
    return {name: len([a for a in args.split(",") if a.strip()]) for name, args in decls}


def test_abi_header_library_and_binding_agree(harness):
    from robosimgs_amd import _lib
    from robosimgs_amd.csrc import build
    assert "mesh.hip" in build.SOURCES
    decl = _declared()
    assert sorted(decl) == sorted(_lib.MESH_EXPORTS) and len(decl) == 5
    for L in (_lib.lib(), _lib.debug_lib()):
        for name, nargs in decl.items():
            assert len(getattr(L, name).argtypes) == nargs, name
    header = open(os.path.join(ROOT, "include", "mgs_mesh.h")).read()
    defs = {m.group(1): int(m.group(2)) for m in re.finditer(r"^#define\s+MGS_MESH_(\w+)\s+(\d+)\b", header, flags=re.M)}
    assert defs == {"MAX_SIDE": _lib.MESH_MAX_SIDE, "LARGE_BLOCKS": _lib.MESH_LARGE_BLOCKS} and MS.LARGE_BLOCKS == defs["LARGE_BLOCKS"]
    assert "MGS_VERSION" not in re.sub(r"/\*.*?\*/", "", header, flags=re.S)        # the version is mgs.h's


def test_abi_workspace_bytes_is_the_documented_layout(harness):
    from robosimgs_amd import _lib
    L = _lib.lib()
    up = lambda v: (v + 255) // 256 * 256
    for C, V, F, W, H in ((1, 3, 1, 1, 1), (2, 50, 129, 37, 29), (1, 12826, 25000, 1920, 1080), (3, 7, 1000, 16368, 16368)):
        n = ctypes.c_size_t(0)
        assert L.mgs_mesh_workspace_bytes(C, V, F, W, H, ctypes.byref(n)) == 0
        want = [0, up(8 * C * H * W), up(8 * C * H * W) + up(4 * C)]
        assert n.value == want[2] + up(64 * C * F)
        lay = (ctypes.c_size_t * 4)()
        harness.mh_workspace_layout(C, F, W, H, lay)
        assert list(lay) == want + [n.value]
    assert 8 * 3 * 16368 * 16368 > 2 ** 32                                          # (the last case needs the 64-bit products)


def test_abi_refuses_bad_arguments_with_a_message():
    from robosimgs_amd import _lib
    L = _lib.lib()
    msg = lambda: L.mgs_last_error_string()
    n = ctypes.c_size_t(0)
    ws = 0x1000                                     # never dereferenced: every call below is refused before a launch
    raster = lambda **kw: L.mgs_mesh_raster(*[{**dict(C=1, V=3, vc=0x100, F=1, faces=0x200, Ks=0x300, W=64, H=64, near=0.01,
                                                        far=1e10, cull=0, ws=ws, nbytes=1 << 30, stream=None), **kw}[k]
                                               for k in ("C", "V", "vc", "F", "faces", "Ks", "W", "H", "near", "far", "cull", "ws",
                                                         "nbytes", "stream")])
    assert raster(vc=None) == -1 and b"null" in msg()
    assert raster(ws=None) == -1 and b"workspace is null" in msg()
    assert raster(V=0) == -1 and b"V 0" in msg()
    assert raster(F=0) == -1 and b"F 0" in msg()
    assert raster(near=0.0) == -1 and b"near_plane" in msg()
    assert raster(near=-1.0) == -1 and b"near_plane" in msg()
    assert raster(near=float("nan")) == -1 and b"near_plane" in msg()
    assert raster(far=0.001) == -1 and b"far_plane" in msg()
    assert raster(W=16369) == -1 and b"16368" in msg()
    assert raster(H=0) == -1 and b"16368" in msg()
    assert raster(nbytes=100) == -1 and b"needed" in msg()
    assert raster(ws=0x1001) == -1 and b"aligned" in msg()
    assert raster(C=0) == -1 and b"n_cams" in msg()
    assert L.mgs_mesh_workspace_bytes(1, 3, 1, 16369, 8, ctypes.byref(n)) == -1 and b"16368" in msg()
    assert L.mgs_mesh_workspace_bytes(1, 3, 1, 8, 8, None) == -1 and b"null" in msg()
    assert L.mgs_mesh_vertices(1, 0, 0x100, None, 0, None, None, None, 0x200, 0x300, None) == -1 and b"V 0" in msg()
    assert L.mgs_mesh_vertices(1, 3, None, None, 0, None, None, None, 0x200, 0x300, None) == -1 and b"null" in msg()
    assert L.mgs_mesh_vertices(1, 3, 0x100, None, 2, None, None, None, 0x200, 0x300, None) == -1 and b"links" in msg()
    assert L.mgs_mesh_vertices(1, 3, 0x100, None, -1, None, None, None, 0x200, 0x300, None) == -1 and b"negative" in msg()
    resolve = lambda **kw: L.mgs_mesh_resolve(*[{**dict(C=1, V=3, vc=0x100, F=1, faces=0x200, vcol=None, fcol=None, Ks=0x300,
                                                          W=64, H=64, light=0, ambient=0.3, ws=ws, nbytes=1 << 30, rgb=0x400,
                                                          depth=0x500, ids=0x600, normals=None, stream=None), **kw}[k]
                                                 for k in ("C", "V", "vc", "F", "faces", "vcol", "fcol", "Ks", "W", "H", "light",
                                                           "ambient", "ws", "nbytes", "rgb", "depth", "ids", "normals", "stream")])
    assert resolve(rgb=None) == -1 and b"output" in msg()
    assert resolve(ambient=1.5) == -1 and b"ambient" in msg()
    assert resolve(F=0) == -1 and b"F 0" in msg()
    # the fused call checks everything before its first launch: a bad resolve argument, with valid vertex arguments
    rc = L.mgs_rasterize_mesh(1, 3, 0x100, None, 0, None, None, None, 0x200, 0x300, 1, 0x400, None, None, 64, 64, 0.01, 1e10, 0, 0,
                              2.0, ws, 1 << 30, 0x500, 0x600, 0x700, 0x800, None, None)
    assert rc == -1 and b"ambient" in msg()
    rc = L.mgs_rasterize_mesh(1, 3, 0x100, None, 0, None, None, None, 0x200, 0x300, 1, 0x400, None, None, 64, 64, 0.0, 1e10, 0, 0,
                              0.3, ws, 1 << 30, 0x500, 0x600, 0x700, 0x800, None, None)
    assert rc == -1 and b"near_plane" in msg()


# ---- the Python layer's argument errors --------------------------------------------------------------------------------------
def test_python_layer_raises_value_errors_before_any_launch():
    import torch
    import robosimgs_amd
    from robosimgs_amd import mesh_render as M
    from robosimgs_amd.mesh import Mesh
    assert robosimgs_amd.rasterize_mesh is M.rasterize_mesh and robosimgs_amd.MeshRenderer is M.MeshRenderer
    assert robosimgs_amd.mesh_vertices is M.mesh_vertices and robosimgs_amd.mesh_raster is M.mesh_raster
    assert robosimgs_amd.mesh_resolve is M.mesh_resolve
    mesh = Mesh(np.zeros((3, 3), np.float32), np.array([[0, 1, 2]]))
    vm, K = np.eye(4, dtype=np.float32), MR.pinhole(32, 32)
    with pytest.raises(ValueError, match="CPU"):
        M.rasterize_mesh(mesh, vm, K, 32, 32)                                      # a mesh on the CPU
    with pytest.raises(ValueError, match="CPU"):
        M.MeshRenderer(mesh, 32, 32)
    for kw, word in ((dict(width=0), "each side"), (dict(width=16369), "each side"), (dict(height=20000), "each side"),
                     (dict(near_plane=0.0), "near_plane"), (dict(near_plane=-1.0), "near_plane"),
                     (dict(near_plane=float("nan")), "near_plane"), (dict(far_plane=0.001), "far_plane"),
                     (dict(ambient=1.5), "ambient")):
        args = dict(width=32, height=32)
        args.update(kw)
        with pytest.raises(ValueError, match=word):
            M.rasterize_mesh(mesh, vm, K, args.pop("width"), args.pop("height"), **args)
    with pytest.raises(ValueError, match="viewmats must be"):
        M.rasterize_mesh(mesh, np.eye(3), K, 32, 32)
    with pytest.raises(ValueError, match="Ks must be"):
        M.rasterize_mesh(mesh, vm, np.eye(4), 32, 32)
    with pytest.raises(ValueError, match="floating-point"):
        M.rasterize_mesh(mesh, np.eye(4, dtype=np.int32), K, 32, 32)
    with pytest.raises(ValueError, match="rotations must be"):
        M.rasterize_mesh(mesh, vm, K, 32, 32, rotations=np.eye(3)[None], translations=np.zeros((2, 3)))
    with pytest.raises(ValueError, match="scales must be"):
        M.rasterize_mesh(mesh, vm, K, 32, 32, rotations=np.eye(3)[None], translations=np.zeros((1, 3)), scales=np.ones(2))
    with pytest.raises(ValueError, match="must be a Mesh"):
        M.rasterize_mesh(dict(vertices=0), vm, K, 32, 32)
    with pytest.raises(ValueError, match="at least one"):
        M.MeshRenderer(Mesh(np.zeros((3, 3), np.float32), np.zeros((0, 3), np.int32)), 32, 32)
    # the stage operators take launch-ready tensors only
    v, f = torch.zeros(3, 3), torch.tensor([[0, 1, 2]], dtype=torch.int32)
    with pytest.raises(ValueError, match="CPU tensor"):
        M.mesh_vertices(v, torch.eye(4)[None])
    with pytest.raises(ValueError, match="vertices must be"):
        M.mesh_vertices(torch.zeros(3, 2), torch.eye(4)[None])
    with pytest.raises(ValueError, match="float32"):
        M.mesh_vertices(v.double(), torch.eye(4)[None])
    with pytest.raises(ValueError, match="CPU tensor"):
        M.mesh_raster(v[None], f, torch.eye(3)[None], 32, 32)
    with pytest.raises(ValueError, match="verts_cam must be"):
        M.mesh_raster(v, f, torch.eye(3)[None], 32, 32)
    with pytest.raises(ValueError, match="CPU tensor"):
        M.mesh_resolve(v[None], f, torch.eye(3)[None], 32, 32, torch.zeros(1 << 16, dtype=torch.uint8))
    with pytest.raises(ValueError, match="go together"):
        M._links(torch.eye(3)[None], None, None, None)
    assert M.mesh_workspace_bytes(1, 3, 1, 32, 32) == 8 * 32 * 32 + 256 + 256
