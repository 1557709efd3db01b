"""Triangle meshes without a GPU: the fp64 statement of how a mesh is rasterised as the opaque foreground of a frame
(tests/mesh_ref.py) against closed forms and against the reference project's own renders of the open box (the pin), the
tolerance cap of its acceptance rule on the synthetic raster cases, and the Mesh class with its readers.
"""
import json
import os
import struct

import numpy as np
import pytest

import mesh_ref as MR

HERE = os.path.dirname(os.path.abspath(__file__))
PIN = {"top": 5, "bottom": 0, "front": 3, "back": 1, "left": 4, "right": 2}      # xor pixels against the reference's renders


# ---- the fp64 reference against closed forms -------------------------------------------------------------------------------
def _square(x0, y0, x1, y1, z, K):
    """Camera-space corners whose projections are the pixel-space corners given, at depth z."""
    uv = np.array([[x0, y0], [x1, y0], [x1, y1], [x0, y1]], np.float64)
    return np.stack([(uv[:, 0] - K[0, 2]) / K[0, 0] * z, (uv[:, 1] - K[1, 2]) / K[1, 1] * z, np.full(4, z)], 1)


def test_reference_square_at_constant_depth_has_the_exact_pixel_count_and_depth():
    W, H = 40, 30
    K = np.array([[32.0, 0, 20.0], [0, 32.0, 15.0], [0, 0, 1]])          # dyadic: the corners below are exact in fp32
    v = _square(5.25, 4.25, 21.25, 17.75, 4.0, K).astype(np.float32)
    for faces in ([[0, 1, 2], [0, 2, 3]], [[0, 2, 1], [0, 3, 2]], [[1, 2, 3], [1, 3, 0]]):
        R = MR.RasterRef(v, np.array(faces), K.astype(np.float32), W, H)
        m = R.mask()
        # pixel centres x + 0.5 in [5.25, 21.25]: x = 5 .. 20; y + 0.5 in [4.25, 17.75]: y = 4 .. 17
        want = np.zeros((H, W), bool)
        want[4:18, 5:21] = True
        assert np.array_equal(m, want) and int(m.sum()) == 16 * 14                   # no crack along the diagonal, no gap
        assert np.abs(R.zwin[R.covered] - 4.0).max() <= 1e-14
        assert set(np.unique(R.winner[R.covered])) == {0, 1}
        assert R.tolerance_share() <= 0.02 or faces == [[0, 1, 2], [0, 2, 3]]


def test_reference_shared_diagonal_through_pixel_centres_goes_to_the_lower_face_and_leaves_no_crack():
    W, H = 24, 24
    K = np.array([[16.0, 0, 12.0], [0, 16.0, 12.0], [0, 0, 1]])
    v = _square(4.5, 4.5, 20.5, 20.5, 2.0, K).astype(np.float32)                 # the diagonal runs through pixel centres
    R = MR.RasterRef(v, np.array([[0, 1, 2], [0, 2, 3]]), K.astype(np.float32), W, H)
    m = R.mask()
    assert int(m.sum()) == 17 * 17 and m[4:21, 4:21].all()                         # edges inclusive on all four sides
    win = R.winner.reshape(H, W)
    assert all(win[4 + i, 4 + i] == 0 for i in range(17))                          # equal depth: the lower index
    assert (win[4:21, 4:21] == 0).sum() == 17 * 18 // 2 and (win[4:21, 4:21] == 1).sum() == 17 * 16 // 2
    assert R.by_tolerance.reshape(H, W)[10, 10]                                    # and the reference knows it is a tie


def test_reference_resolve_gives_barycentric_colours_and_normals_toward_the_camera():
    W, H = 40, 30
    K = np.array([[32.0, 0, 20.0], [0, 32.0, 15.0], [0, 0, 1]])
    v = _square(5.25, 4.25, 21.25, 17.75, 4.0, K).astype(np.float32)
    faces = np.array([[0, 1, 2], [0, 2, 3]])
    R = MR.RasterRef(v, faces, K.astype(np.float32), W, H)
    r = R.check_raster(R.winner.reshape(H, W), R.zwin.reshape(H, W))
    col = np.array([[0.0, 0, 0], [1, 0, 0], [1, 1, 0], [0, 1, 0]], np.float32)        # red grows with x, green with y
    ref = R.shade_ref(r["pairs"], r["pixels"], faces, vertex_colors=col)
    x, y = r["pixels"] % W + 0.5, r["pixels"] // W + 0.5
    assert np.abs(ref["rgb"][:, 0] - (x - 5.25) / 16.0).max() <= 1e-12 and np.abs(ref["rgb"][:, 1] - (y - 4.25) / 13.5).max() <= 1e-12
    assert np.abs(ref["normal"] - [0, 0, -1]).max() <= 1e-12 and not ref["flip_open"].any() and (ref["tol_rgb"] < 1e-5).all()
    lit = R.shade_ref(r["pairs"], r["pixels"], faces, face_colors=np.ones((2, 3), np.float32), headlight=True, ambient=0.25)
    centre = np.argmin((x - 20.0) ** 2 + (y - 15.0) ** 2)
    assert abs(lit["rgb"][centre, 0] - 1.0) <= 1e-3 and (lit["rgb"] <= 1.0).all() and (lit["rgb"] >= 0.25).all()


def _in_polygon(poly, W, H):
    """Pixel centres inside a convex polygon (either winding)."""
    y, x = np.mgrid[0:H, 0:W]
    px, py = x + 0.5, y + 0.5
    s = []
    for i in range(len(poly)):
        (x0, y0), (x1, y1) = poly[i], poly[(i + 1) % len(poly)]
        s.append((x1 - x0) * (py - y0) - (y1 - y0) * (px - x0))
    s = np.stack(s)
    return (s >= 0).all(0) | (s <= 0).all(0)


def test_reference_triangle_crossing_the_near_plane_covers_the_clipped_outline():
    W, H, near = 64, 48, 0.5
    K = np.array([[40.0, 0, 32.0], [0, 40.0, 24.0], [0, 0, 1]])
    a, b, c = np.array([-0.53, -0.31, 2.0]), np.array([0.61, -0.22, 2.5]), np.array([0.11, 0.17, -1.0])
    R = MR.RasterRef(np.stack([a, b, c]).astype(np.float32), np.array([[0, 1, 2]]), K.astype(np.float32), W, H, near_plane=near)
    a, b, c = (np.float32(v).astype(np.float64) for v in (a, b, c))
    cut = lambda p, q: p + (near - p[2]) / (q[2] - p[2]) * (q - p)
    proj = lambda p: (K[0, 0] * p[0] / p[2] + K[0, 2], K[1, 1] * p[1] / p[2] + K[1, 2])
    want = _in_polygon([proj(a), proj(b), proj(cut(b, c)), proj(cut(c, a))], W, H)
    assert np.array_equal(R.mask(), want) and 40 < want.sum() < W * H
    assert R.zwin[R.covered].min() >= near and R.zwin[R.covered].max() <= 2.5
    # far_plane cuts the other end the same way
    R2 = MR.RasterRef(np.stack([a, b, c]).astype(np.float32), np.array([[0, 1, 2]]), K.astype(np.float32), W, H, near, far_plane=2.0)
    assert R2.covered.sum() < R.covered.sum() and R2.zwin[R2.covered].max() <= 2.0
    # wholly behind: nothing; cull: this face's normal (b - a) x (c - a) points away from the camera or toward it
    front = float(np.dot(a, np.cross(b, c))) < 0
    R3 = MR.RasterRef(np.stack([a, b, c]).astype(np.float32), np.array([[0, 1, 2], [0, 2, 1]]), K.astype(np.float32), W, H, near,
                      cull_backfaces=True)
    assert np.array_equal(R3.mask(), want) and set(np.unique(R3.winner[R3.covered])) == {0 if front else 1}


# ---- the pin: the reference project's own renders of the open box -----------------------------------------------------------
@pytest.fixture(scope="module")
def openbox():
    g = np.load(os.path.join(HERE, "golden", "mesh_openbox.npz"))
    cam = np.load(os.path.join(HERE, "golden", "camera_reference.npz"))
    verts = np.concatenate([g["lid_vertices"], g["body_vertices"]])
    faces = np.concatenate([g["lid_faces"].astype(np.int32), g["body_faces"].astype(np.int32) + len(g["lid_vertices"])])
    assert faces.shape == (8393 + 16607, 3) and verts.dtype == np.float32
    hinge = np.load(os.path.join(HERE, "golden", "hinge_openbox.npz"))
    assert np.array_equal(hinge["lid"], g["lid_vertices"]) and np.array_equal(hinge["body"], g["body_vertices"])
    names = [str(n) for n in cam["cam_names"]]
    views = {}
    for k, name in enumerate(str(n) for n in g["sil_names"]):
        i = names.index(name)
        viewmat = (np.diag([1.0, -1.0, -1.0, 1.0]) @ np.linalg.inv(cam["cam_c2w"][i])).astype(np.float32)
        h, w = (int(v) for v in g["sil_shape"])
        sil = np.unpackbits(g["sil_bits"][k])[:h * w].reshape(h, w).astype(bool)
        views[name] = dict(viewmat=viewmat, K=cam["cam_K"][i].astype(np.float32), silhouette=sil)
    return dict(verts=verts, faces=faces, views=views, n_lid=len(g["lid_vertices"]))



def test_the_pin_reference_silhouettes_of_the_open_box(openbox):
    """The reference ships six GL renders of the open box beside their cameras: mesh_ref's silhouettes of the same meshes
    under viewmat = diag(1, -1, -1, 1) inv(c2w) and the recorded K differ from them in at most these pixels."""
    assert list(openbox["views"]) == list(PIN)
    seen = {}
    for name, v in openbox["views"].items():
        cam, _ = MR.vertex_ref(openbox["verts"], None, None, None, None, v["viewmat"][None])
        R = MR.RasterRef(cam[0].astype(np.float32), openbox["faces"], v["K"], 800, 800)
        seen[name] = int((R.mask() ^ v["silhouette"]).sum())
        assert 15_000 < R.covered.sum() < 58_000
        assert R.tolerance_share() <= 0.02, (name, R.tolerance_share())
    print("\nxor against the reference's renders:", seen)
    assert all(seen[k] <= PIN[k] for k in PIN), seen


def test_vertex_reference_is_the_pose_then_the_view():
    rng = np.random.default_rng(3)
    verts = rng.normal(size=(50, 3)).astype(np.float32)
    link = rng.integers(-1, 2, 50).astype(np.int32)
    a = 0.3
    Rm = np.array([[[np.cos(a), -np.sin(a), 0], [np.sin(a), np.cos(a), 0], [0, 0, 1]], np.eye(3)], np.float32)
    t, s = np.array([[0.1, 0.2, 0.3], [0, 0, 0]], np.float32), np.array([2.0, 1.0], np.float32)
    vm = np.eye(4, dtype=np.float32)[None].copy()
    vm[0, :3, 3] = [0.5, -0.5, 4.0]
    cam, bound = MR.vertex_ref(verts, link, Rm, t, s, vm)
    want = verts.astype(np.float64).copy()
    on0 = link == 0
    want[on0] = 2.0 * want[on0] @ Rm[0].astype(np.float64).T + t[0]
    assert np.abs(cam[0] - (want + vm[0, :3, 3])).max() <= 1e-14 and (bound > 0).all() and bound.max() < 1e-5
    assert np.array_equal(cam[0][link != 0], verts[link != 0].astype(np.float64) + vm[0, :3, 3].astype(np.float64))


@pytest.mark.parametrize("size", [(37, 29), (64, 64)])
def test_raster_cases_stay_inside_the_tolerance_cap_and_the_rule_accepts_the_reference_itself(size):
    """The synthetic cases a rasteriser is to be held to: at most 2 % of covered pixels are decided by tolerance (none, in
    fact), and the reference's own winners and depths pass its acceptance rule."""
    W, H = size
    cases = MR.raster_cases(W, H)
    assert ("threshold_blocks" in cases) == (size == (64, 64))                     # 2 x 7 blocks do not fit 37 x 29
    for name, c in cases.items():
        R = MR.RasterRef(c["verts"], c["faces"], c["K"], W, H, c["near"], c["far"], c["cull"])
        assert R.tolerance_share() <= 0.02, (name, R.tolerance_share())
        r = R.check_raster(R.winner.reshape(H, W), R.zwin.reshape(H, W))
        assert r["differs"] == 0 and r["depth_ratio"] == 0.0
        if c.get("identical"):
            assert (R.winner[R.covered] % 2 == 0).all() and R.covered.any()         # the lower index of every pair
        if "only_face" in c:
            assert set(np.unique(R.winner)) == {-1, c["only_face"]}
        if c.get("bad_index"):
            assert R.setup.bad_index[::3].all() and not np.isin(R.winner, np.arange(0, len(c["faces"]), 3)).any()
        if name == "full_image_plus_64":
            assert R.covered.all()
        wrong = np.where(R.covered, -1, 0).reshape(H, W)                            # and it refuses a wrong answer
        if R.has_certain.any():
            with pytest.raises(AssertionError):
                R.check_raster(wrong, np.zeros((H, W)))
    assert cases["cull_on"]["cull"] and not cases["cull_off"]["cull"]


# ---- mesh files -------------------------------------------------------------------------------------------------------------
def _write_glb(path, pos, idx=None, idx_type="<u2", colors=None, mode=4, node=None, material=None, stride=0):
    blob, views, accessors, attrs = b"", [], [], {}

    def add(arr, comp, typ, normalized=False):
        nonlocal blob
        blob += b"\0" * (-len(blob) % 4)
        views.append({"buffer": 0, "byteOffset": len(blob), "byteLength": arr.nbytes})
        acc = {"bufferView": len(views) - 1, "componentType": comp, "type": typ, "count": len(arr)}
        if normalized:
            acc["normalized"] = True
        accessors.append(acc)
        blob += arr.tobytes()
        return len(accessors) - 1
    attrs["POSITION"] = add(np.asarray(pos, "<f4"), 5126, "VEC3")
    prim = {"attributes": attrs, "mode": mode}
    if idx is not None:
        comp = {"u1": 5121, "<u2": 5123, "<u4": 5125}[idx_type]
        prim["indices"] = add(np.asarray(idx).reshape(-1).astype(idx_type), comp, "SCALAR")
    if colors is not None:
        colors = np.asarray(colors)
        attrs["COLOR_0"] = add(colors, 5126 if colors.dtype.kind == "f" else 5121, "VEC4" if colors.shape[1] == 4 else "VEC3",
                               normalized=colors.dtype.kind != "f")
    if material is not None:
        prim["material"] = 0
    doc = {"asset": {"version": "2.0"}, "scene": 0, "scenes": [{"nodes": [0]}], "nodes": [dict({"mesh": 0}, **(node or {}))],
           "meshes": [{"primitives": [prim]}], "buffers": [{"byteLength": len(blob)}], "bufferViews": views, "accessors": accessors}
    if material is not None:
        doc["materials"] = [material]
    js = json.dumps(doc).encode()
    js += b" " * (-len(js) % 4)
    blob += b"\0" * (-len(blob) % 4)
    body = struct.pack("<II", len(js), 0x4E4F534A) + js + struct.pack("<II", len(blob), 0x004E4942) + blob
    open(path, "wb").write(b"glTF" + struct.pack("<II", 2, 12 + len(body)) + body)


def test_mesh_from_glb_reads_what_it_claims_and_refuses_the_rest(tmp_path):
    from robosimgs_amd.mesh import Mesh
    rng = np.random.default_rng(0)
    pos = rng.normal(size=(7, 3)).astype(np.float32)
    idx = np.array([[0, 1, 2], [2, 3, 4], [4, 5, 6]])
    for t in ("u1", "<u2", "<u4"):
        _write_glb(tmp_path / "a.glb", pos, idx, t)
        m = Mesh.from_glb(str(tmp_path / "a.glb"))
        assert np.array_equal(m.vertices.numpy(), pos) and np.array_equal(m.faces.numpy(), idx) and m.vertex_colors is None
        assert m.faces.dtype.is_floating_point is False and m.link_ids is None and m.n_links() == 0
    _write_glb(tmp_path / "b.glb", pos[:6], None)                                  # no indices: consecutive triples
    assert Mesh.from_glb(str(tmp_path / "b.glb")).faces.tolist() == [[0, 1, 2], [3, 4, 5]]
    col = rng.uniform(size=(7, 3)).astype(np.float32)
    _write_glb(tmp_path / "c.glb", pos, idx, colors=col)
    assert np.array_equal(Mesh.from_glb(str(tmp_path / "c.glb")).vertex_colors.numpy(), col)
    col8 = rng.integers(0, 256, (7, 4)).astype(np.uint8)
    _write_glb(tmp_path / "d.glb", pos, idx, colors=col8)
    assert np.allclose(Mesh.from_glb(str(tmp_path / "d.glb")).vertex_colors.numpy(), col8[:, :3] / 255.0, atol=1e-7)
    for kw, word in ((dict(mode=1), "mode 1"), (dict(mode=5), "mode 5"), (dict(node={"translation": [1, 0, 0]}), "transform"),
                     (dict(node={"matrix": list(np.eye(4).reshape(-1))}), "transform"),
                     (dict(material={"pbrMetallicRoughness": {"baseColorTexture": {"index": 0}}}), "texture")):
        _write_glb(tmp_path / "bad.glb", pos, idx, **kw)
        with pytest.raises(ValueError, match=word):
            Mesh.from_glb(str(tmp_path / "bad.glb"))
    _write_glb(tmp_path / "e.glb", pos, np.arange(7))
    with pytest.raises(ValueError, match="whole number of triangles"):
        Mesh.from_glb(str(tmp_path / "e.glb"))
    open(tmp_path / "f.glb", "wb").write(b"not a glb file at all, but long enough")
    with pytest.raises(ValueError, match="not a binary glTF"):
        Mesh.from_glb(str(tmp_path / "f.glb"))


def test_mesh_from_obj_merge_and_the_dataclass_checks(tmp_path):
    import torch
    from robosimgs_amd.mesh import Mesh
    import robosimgs_amd
    assert robosimgs_amd.Mesh is Mesh
    (tmp_path / "a.obj").write_text("# a comment\nv 0 0 0\nv 1 0 0\nv 0 1 0\nvn 0 0 1\nv 0 0 1\nf 1 2 3\nf 1/1/1 3/2/1 4/3/1\nf -1 -2 -3\n")
    m = Mesh.from_obj(str(tmp_path / "a.obj"))
    assert m.vertices.tolist() == [[0, 0, 0], [1, 0, 0], [0, 1, 0], [0, 0, 1]] and m.faces.tolist() == [[0, 1, 2], [0, 2, 3], [3, 2, 1]]
    (tmp_path / "q.obj").write_text("v 0 0 0\nv 1 0 0\nv 0 1 0\nv 1 1 0\nf 1 2 3 4\n")
    with pytest.raises(ValueError, match="only triangles"):
        Mesh.from_obj(str(tmp_path / "q.obj"))
    both = Mesh.merge([m, m], link_ids=[-1, 0])
    assert both.n_vertices == 8 and both.faces[3:].tolist() == [[4, 5, 6], [4, 6, 7], [7, 6, 5]]
    assert both.link_ids.tolist() == [-1] * 4 + [0] * 4 and both.n_links() == 1 and both.link_ids.dtype == torch.int32
    red = Mesh(m.vertices, m.faces, vertex_colors=torch.tensor([[1.0, 0, 0]] * 4))
    mixed = Mesh.merge([m, red])
    assert mixed.vertex_colors[:4].tolist() == [[pytest.approx(0.7)] * 3] * 4 and mixed.vertex_colors[4:].tolist() == [[1, 0, 0]] * 4
    assert mixed.link_ids is None and mixed.to("cpu").faces.tolist() == mixed.faces.tolist()
    with pytest.raises(ValueError, match="vertices must be"):
        Mesh(np.zeros((3, 2)), np.zeros((1, 3), np.int32))
    with pytest.raises(ValueError, match="faces must be"):
        Mesh(np.zeros((3, 3)), np.zeros((1, 4), np.int32))
    with pytest.raises(ValueError, match="integer"):
        Mesh(np.zeros((3, 3)), np.zeros((1, 3), np.float32))
    with pytest.raises(ValueError, match="not both"):
        Mesh(np.zeros((3, 3)), np.zeros((1, 3), np.int32), vertex_colors=np.zeros((3, 3)), face_colors=np.zeros((1, 3)))
    with pytest.raises(ValueError, match="link_ids"):
        Mesh(np.zeros((3, 3)), np.zeros((1, 3), np.int32), link_ids=np.zeros(2, np.int32))
    with pytest.raises(ValueError, match="names 1 parts"):
        Mesh.merge([m, m], link_ids=[0])
    with pytest.raises(ValueError, match="vertex colours and one with face colours"):
        Mesh.merge([red, Mesh(m.vertices, m.faces, face_colors=torch.zeros(3, 3))])


