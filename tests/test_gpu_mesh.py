"""The mesh rasteriser on the GPU (include/mgs_mesh.h, csrc/mesh.hip, robosimgs_amd/mesh_render.py) against the fp64
statement of tests/mesh_ref.py, stage by stage: the vertex stage to vertex_ref's bound; the raster stage, on the kernel's
own verts_cam, through check_raster (each case first asserts that at most 2 % of its covered pixels are decided by
tolerance, so the strict face-id comparison covers the rest); the resolve stage, on the raster stage's own winners, to
shade_ref's bounds.  Then the pin (the reference's own renders of the open box), the posed box, two cameras in one call,
repeatability, a captured graph of MeshRenderer.render alone, and composite_over fed with the result."""
import numpy as np
import pytest
import torch

import mesh_ref as MR
import mesh_scenes as MS

pytestmark = pytest.mark.gpu
DEV = "cuda"


def _dev(x, dtype=None):
    return None if x is None else torch.from_numpy(np.ascontiguousarray(x, dtype)).to(DEV)


def _decode(vis):
    """(face_ids int32, depth float32) of a visibility buffer: the key's low word is the face (all ones: -1), its high word
    the bits of z."""
    v = vis.cpu().numpy().view(np.uint64)
    ids = (v & np.uint64(0xFFFFFFFF)).astype(np.uint32).view(np.int32)
    depth = (v >> np.uint64(32)).astype(np.uint32).view(np.float32).copy()
    depth[ids < 0] = 0.0
    return ids, depth


def _bits(x):
    return np.ascontiguousarray(x, np.float32).view(np.uint32)


def _colors(n, seed):
    return np.random.default_rng(seed).uniform(0.0, 1.0, (n, 3)).astype(np.float32)


def _stages(c, W, H, **shade):
    """One camera-space case through mesh_raster and mesh_resolve: (RasterRef of the kernel's input, check_raster's result,
    ids, depth of the raster stage, the resolve stage's dict as numpy)."""
    from robosimgs_amd import mesh_raster, mesh_resolve
    vc, faces, K = _dev(c["verts"], np.float32)[None].contiguous(), _dev(c["faces"], np.int32), _dev(c["K"], np.float32)[None].contiguous()
    vis, ws = mesh_raster(vc, faces, K, W, H, near_plane=c.get("near", 0.01), far_plane=c.get("far", 1e10),
                          cull_backfaces=c.get("cull", False))
    ids, depth = _decode(vis[0])
    R = MR.RasterRef(c["verts"], c["faces"], c["K"], W, H, c.get("near", 0.01), c.get("far", 1e10), c.get("cull", False))
    assert R.tolerance_share() <= 0.02, R.tolerance_share()
    r = R.check_raster(ids, depth)
    res = mesh_resolve(vc, faces, K, W, H, ws, vertex_colors=_dev(shade.get("vertex_colors")), face_colors=_dev(shade.get("face_colors")),
                       headlight=shade.get("headlight", False), ambient=shade.get("ambient", 0.3), return_normals=True)
    res = {k: v[0].cpu().numpy() for k, v in res.items()}
    # the resolve stage on the raster stage's own winners: ids and depth bit for bit, uncovered exactly (0, 0, 0), 0, -1
    assert np.array_equal(res["face_ids"], ids) and np.array_equal(_bits(res["depth"]), _bits(depth))
    assert (res["depth"][ids < 0] == 0).all() and (res["rgb"][ids < 0] == 0).all() and (res["depth"][ids >= 0] > 0).all()
    return R, r, ids, depth, res


def test_vertex_stage_stays_inside_the_counted_bound_and_copies_static_vertices():
    from robosimgs_amd import mesh_vertices
    rng = np.random.default_rng(3)
    verts = rng.normal(size=(50, 3)).astype(np.float32)
    link = rng.integers(-1, 2, 50).astype(np.int32)
    link[:4] = [2, 7, -2, -5]                                                       # >= L and < -1: static
    Rm = np.stack([MS.rotation_about([0.2, -0.5, 0.8], 0.7), MS.rotation_about([1.0, 0.3, 0.1], -1.1)]).astype(np.float32)
    t, s = rng.normal(size=(2, 3)).astype(np.float32), np.array([1.7, 0.6], np.float32)
    vm = np.stack([np.eye(4), np.eye(4)]).astype(np.float32)
    vm[1, :3, :3] = MS.rotation_about([0.1, 0.9, 0.2], 0.4)
    vm[1, :3, 3] = [0.5, -0.5, 4.0]
    got = mesh_vertices(_dev(verts), _dev(vm), _dev(link), _dev(Rm), _dev(t), _dev(s)).cpu().numpy()
    cam, bound = MR.vertex_ref(verts, link, Rm, t, s, vm)
    ratio = np.abs(got - cam) / bound
    print(f"\nvertex stage: worst error / bound {ratio.max():.3f}")
    assert got.shape == (2, 50, 3) and ratio.max() <= 1
    static = (link < 0) | (link >= 2)
    assert static[:4].all() and (~static).sum() > 10
    assert np.array_equal(_bits(got[0][static]), _bits(verts[static]))              # identity view: bit for bit
    # without scales s = 1, and without link ids everything is static
    got1 = mesh_vertices(_dev(verts), _dev(vm), _dev(link), _dev(Rm), _dev(t)).cpu().numpy()
    cam1, bound1 = MR.vertex_ref(verts, link, Rm, t, None, vm)
    assert (np.abs(got1 - cam1) <= bound1).all()
    got2 = mesh_vertices(_dev(verts), _dev(vm), None, _dev(Rm), _dev(t)).cpu().numpy()
    assert np.array_equal(_bits(got2[0]), _bits(verts))


@pytest.mark.parametrize("size", [(37, 29), (64, 64)])
def test_raster_cases_pass_check_raster_and_the_resolve_stage_its_bounds(size):
    W, H = size
    for name, c in MR.raster_cases(W, H).items():
        vcol = _colors(len(c["verts"]), 5)
        R, r, ids, depth, res = _stages(c, W, H, vertex_colors=vcol)
        worst = MS.check_shading(R, r, c["faces"], res["rgb"], res["normals"], vertex_colors=vcol)
        print(f"\n{name} {W}x{H}: covered {r['covered']}, by tolerance {r['by_tolerance']}, depth ratio {r['depth_ratio']:.3f}, "
              f"rgb ratio {worst['rgb']:.3f}, normal ratio {worst['normal']:.3f}")
        if c.get("identical"):
            assert (ids[ids >= 0] % 2 == 0).all() and (ids >= 0).any()               # the lower index of every pair wins
        if "only_face" in c:
            assert set(np.unique(ids)) == {-1, c["only_face"]}
        if c.get("bad_index"):
            assert not np.isin(ids, np.arange(0, len(c["faces"]), 3)).any()          # faces naming vertex V never win
        if name == "full_image_plus_64":
            assert (ids >= 0).all()
    cases = MR.raster_cases(W, H)
    assert ("threshold_blocks" in cases) == (size == (64, 64))
    if "threshold_blocks" in cases:
        assert cases["threshold_blocks"]["blocks"] == [14, 15, 16] and MS.LARGE_BLOCKS == 15
    on, off = _stages(cases["cull_on"], W, H)[2], _stages(cases["cull_off"], W, H)[2]
    assert 0 < (on >= 0).sum() < (off >= 0).sum()


def test_boxes_around_the_large_face_threshold_and_the_wide_image():
    c = MS.own_threshold_case()
    ids = _stages(c, 64, 64)[2]
    assert set(np.unique(ids)) == {-1, 0, 1, 2}
    c = MS.wide_case()                                                              # 258 blocks across
    R, r, ids, depth, res = _stages(c, c["width"], c["height"], face_colors=_colors(len(c["faces"]), 2))
    MS.check_shading(R, r, c["faces"], res["rgb"], res["normals"], face_colors=_colors(len(c["faces"]), 2))
    assert (ids >= 0).all() and ids.shape == (16, 2064)


def test_resolve_colour_modes_and_the_headlight_on_random129():
    c = MR.raster_cases(64, 64)["random129"]
    for kw in (dict(vertex_colors=_colors(len(c["verts"]), 1)), dict(face_colors=_colors(len(c["faces"]), 2)), dict()):
        for light in (dict(), dict(headlight=True, ambient=0.25)):
            R, r, ids, depth, res = _stages(c, 64, 64, **kw, **light)
            worst = MS.check_shading(R, r, c["faces"], res["rgb"], res["normals"], **kw, **light)
            print(f"\n{sorted(kw)} {light}: rgb ratio {worst['rgb']:.3f}, normal ratio {worst['normal']:.3f}")
            if not kw and not light:
                assert (_bits(res["rgb"][ids >= 0]) == _bits(np.float32(0.7))).all()


def _mesh(verts, faces, **kw):
    from robosimgs_amd import Mesh
    return Mesh(verts, faces, **kw).to(DEV)


def test_two_cameras_in_one_call_equal_two_calls_and_a_repeated_call_is_bit_identical():
    from robosimgs_amd import rasterize_mesh
    c = MR.raster_cases(64, 64)["full_image_plus_64"]
    mesh = _mesh(c["verts"], c["faces"], vertex_colors=_colors(len(c["verts"]), 9))
    vm = np.stack([np.eye(4), np.eye(4)]).astype(np.float32)
    vm[1, :3, :3] = MS.rotation_about([0.3, 1.0, -0.2], 0.15)
    vm[1, :3, 3] = [0.1, -0.2, 0.5]
    Ks = np.stack([c["K"], MR.pinhole(64, 64, f=75.0)])
    kw = dict(headlight=True, return_normals=True)
    both = rasterize_mesh(mesh, vm, Ks, 64, 64, **kw)
    flat = lambda o: [o[0], o[1], o[2]["face_ids"], o[2]["verts_cam"], o[2]["normals"]]
    for k in range(2):
        one = rasterize_mesh(mesh, vm[k], Ks[k], 64, 64, **kw)
        for a, b in zip(flat(both), flat(one)):
            assert torch.equal(a[k], b[0]), k
    assert not torch.equal(both[2]["face_ids"][0], both[2]["face_ids"][1])
    again = rasterize_mesh(mesh, vm, Ks, 64, 64, **kw)
    for a, b in zip(flat(both), flat(again)):
        assert torch.equal(a.view(torch.int32), b.view(torch.int32))                # ids, depth and rgb: the same bits
    assert (both[2]["face_ids"][0] >= 0).all()


@pytest.fixture(scope="module")
def openbox():
    return MS.openbox()


@pytest.mark.parametrize("name", list(MS.PIN))
def test_the_pin_views_of_the_open_box(openbox, name):
    """xor against the reference's own silhouettes <= PIN[name] + d, d the pixels whose coverage differs from the fp64
    statement's (check_raster has confined them to pixels without a certain face)."""
    from robosimgs_amd import rasterize_mesh
    v = openbox["views"][name]
    mesh = _mesh(openbox["verts"], openbox["faces"])
    rgb, depth, meta = rasterize_mesh(mesh, v["viewmat"], v["K"], 800, 800, headlight=True, return_normals=True)
    vc = meta["verts_cam"][0].cpu().numpy()
    cam, bound = MR.vertex_ref(openbox["verts"], None, None, None, None, v["viewmat"][None])
    assert (np.abs(vc - cam[0]) <= bound[0]).all()
    R = MR.RasterRef(vc, openbox["faces"], v["K"], 800, 800)
    assert R.tolerance_share() <= 0.02, R.tolerance_share()
    ids = meta["face_ids"][0].cpu().numpy()
    r = R.check_raster(ids, depth[0].cpu().numpy())
    MS.check_shading(R, r, openbox["faces"], rgb[0].cpu().numpy(), meta["normals"][0].cpu().numpy(), headlight=True)
    xor, d = MS.check_pin(R, ids, v["silhouette"], name)
    print(f"\npin {name}: (xor, d) = ({xor}, {d}), covered {r['covered']}, by tolerance {r['by_tolerance']}")


def test_the_posed_box_moves_its_lid(openbox):
    from robosimgs_amd import rasterize_mesh
    v = openbox["views"]["top"]
    K = MS.scaled_K(v["K"], 0.25)
    Rm, t = MS.lid_pose(0.6)
    mesh = _mesh(openbox["verts"], openbox["faces"], link_ids=openbox["link_ids"])
    rgb, depth, meta = rasterize_mesh(mesh, v["viewmat"], K, 200, 200, rotations=Rm, translations=t)
    vc = meta["verts_cam"][0].cpu().numpy()
    cam, bound = MR.vertex_ref(openbox["verts"], openbox["link_ids"], Rm, t, None, v["viewmat"][None])
    assert (np.abs(vc - cam[0]) <= bound[0]).all()
    R = MR.RasterRef(vc, openbox["faces"], K, 200, 200)
    assert R.tolerance_share() <= 0.02, R.tolerance_share()
    ids = meta["face_ids"][0].cpu().numpy()
    R.check_raster(ids, depth[0].cpu().numpy())
    rest = rasterize_mesh(mesh, v["viewmat"], K, 200, 200)[2]["face_ids"][0].cpu().numpy()
    lid = lambda i: (i >= 0) & (i < 8393)                                           # the lid's faces come first
    assert lid(ids).sum() > 100 and lid(rest).sum() > 100 and (lid(ids) != lid(rest)).sum() > 100
    body_only = ~lid(ids) & ~lid(rest)
    assert np.array_equal(ids[body_only], rest[body_only])                          # where no lid is, nothing moved
    # Hinge.pose's convention: one link given as R [3,3], t [3]
    one = rasterize_mesh(mesh, v["viewmat"], K, 200, 200, rotations=Rm[0].astype(np.float64), translations=t[0].astype(np.float64))
    assert np.array_equal(one[2]["face_ids"][0].cpu().numpy(), ids)


def test_mesh_renderer_alone_in_one_captured_graph_replays_bit_identically():
    from robosimgs_amd import MeshRenderer
    c = MR.raster_cases(64, 64)["full_image_plus_64"]
    link = np.full(len(c["verts"]), 0, np.int32)
    link[:3] = -1                                                                   # the big triangle stays, the 64 small ones turn
    mesh = _mesh(c["verts"], c["faces"], vertex_colors=_colors(len(c["verts"]), 4), link_ids=link)
    r = MeshRenderer(mesh, 64, 64, headlight=True, return_normals=True)
    vm, K = _dev(np.eye(4, dtype=np.float32)[None]), _dev(c["K"][None])
    rots = [torch.from_numpy(MS.rotation_about([0, 0, 1], a).astype(np.float32))[None] for a in (0.0, 0.2, -0.35)]
    Rd, td = rots[0].to(DEV).contiguous(), torch.zeros(1, 3, device=DEV)
    eager = []
    for Rh in rots:
        Rd.copy_(Rh)
        rgb, depth, meta = r.render(vm, K, rotations=Rd, translations=td)
        eager.append([x.clone() for x in (rgb, depth, meta["face_ids"], meta["normals"], meta["verts_cam"])])
    assert not torch.equal(eager[0][2], eager[1][2])
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):                                                       # one linear graph on one stream
        rgb, depth, meta = r.render(vm, K, rotations=Rd, translations=td)
    outs = (rgb, depth, meta["face_ids"], meta["normals"], meta["verts_cam"])
    for k in (1, 2, 0):
        Rd.copy_(rots[k])
        g.replay()
        torch.cuda.synchronize()
        for a, b in zip(outs, eager[k]):
            assert torch.equal(a.view(torch.int32), b.view(torch.int32)), k


def test_composite_over_takes_the_mesh_depth_as_it_stands():
    from robosimgs_amd import composite_over, rasterize_mesh
    W = H = 48
    K = MR.pinhole(W, H)
    near_face = MR.box_in_blocks(0, 0, 3, 3, K, z=2.0)                              # in front of the background at z = 4
    far_face = MR.box_in_blocks(2, 2, 4, 4, K, z=6.0)                               # behind it
    mesh = _mesh(np.concatenate([near_face, far_face]), np.array([[0, 1, 2], [3, 4, 5]]),
                 face_colors=np.array([[1.0, 0.25, 0.0], [0.0, 0.5, 1.0]], np.float32))
    rgb, depth, meta = rasterize_mesh(mesh, np.eye(4), K, W, H)
    bg_rgb = torch.rand(H, W, 3, device=DEV, generator=torch.Generator(DEV).manual_seed(2))
    bg_alpha, bg_depth = torch.ones(H, W, device=DEV), torch.full((H, W), 4.0, device=DEV)
    out_rgb, out_depth = composite_over(bg_rgb, bg_alpha, bg_depth, rgb[0], depth[0])
    alone_rgb, alone_depth = composite_over(bg_rgb, bg_alpha, bg_depth, torch.zeros_like(rgb[0]), torch.zeros_like(depth[0]))
    d, ids = depth[0], meta["face_ids"][0]
    front = (d > 0) & (d < 4.0)
    assert torch.equal(front, ids == 0) and (ids == 1).sum() > 50 and front.sum() > 50 and (ids == -1).sum() > 50
    assert torch.equal(out_rgb[front], rgb[0][front]) and torch.equal(out_depth[front], d[front])
    assert torch.equal(out_rgb[~front], alone_rgb[~front]) and torch.equal(out_depth[~front], alone_depth[~front])
    assert (d[ids == -1] == 0).all() and (out_depth[d == 0] == 4.0).all()
