"""The mesh rasteriser under a lens on the GPU (include/mgs_mesh_lens.h, csrc/mesh_lens.hip, robosimgs_amd/mesh_render.py)
against the fp64 statement of tests/mesh_lens_ref.py, stage by stage: the ray map to its bound and its valid set; the raster
stage, ON THE GPU'S OWN RAY MAP, through check_raster; the resolve stage, on the raster stage's own winners, to shade_ref's
bounds.  Then what holds the lens path to the rest of the project: zero coefficients against the pinhole path, registration
with fully_fused_projection under the same lens (row layout, coefficient order, half-pixel convention), two cameras in one
call, repeatability, and rasterization(foreground=) fed with a mesh layer rendered under the frame's lens."""
import numpy as np
import pytest
import torch

import lens_ref as LR
import mesh_lens_ref as ML
import mesh_lens_scenes as LS
import mesh_ref as MR
import mesh_scenes as MS
import pinhole_lens_ref as PR

pytestmark = pytest.mark.gpu
DEV = "cuda"
LENS_NAMES = list(ML.LENSES)
CASES = ("random1", "random63", "random64", "random65", "random129", "full_image_plus_64", "crosses_near", "cull_on", "cull_off",
         "index_equal_V")


def _dev(x, dtype=None):
    return None if x is None else torch.from_numpy(np.ascontiguousarray(x, dtype)).to(DEV)


def _decode(vis):
    v = vis.cpu().numpy().view(np.uint64)
    ids = (v & np.uint64(0xFFFFFFFF)).astype(np.uint32).view(np.int32)
    depth = (v >> np.uint64(32)).astype(np.uint32).view(np.float32).copy()
    depth[ids < 0] = 0.0
    return ids, depth


def _bits(x):
    return np.ascontiguousarray(x, np.float32).view(np.uint32)


def _colors(n, seed):
    return np.random.default_rng(seed).uniform(0.0, 1.0, (n, 3)).astype(np.float32)


def _lens_kw(lens):
    model, k, _ = ML.LENSES[lens]
    return dict(pinhole_distortion=k) if model == ML.BC else dict(camera_model="fisheye", distortion=k)


def _ray_map(lens, W, H):
    from robosimgs_amd import mesh_lens_rays
    K = ML.intrinsics(lens, W, H)
    return mesh_lens_rays(_dev(K[None]), W, H, **_lens_kw(lens)), K


def _stages(c, lens_map, W, H, **shade):
    """One camera-space case through mesh_raster and mesh_resolve on a ray map: (LensRasterRef on the map, check_raster's
    result, ids, the resolve stage's dict as numpy)."""
    from robosimgs_amd import mesh_raster, mesh_resolve
    vc, faces, K = _dev(c["verts"], np.float32)[None].contiguous(), _dev(c["faces"], np.int32), torch.eye(3, device=DEV)[None]
    near, far, cull = c.get("near", 0.01), c.get("far", 1e10), c.get("cull", False)
    vis, ws = mesh_raster(vc, faces, K, W, H, near_plane=near, far_plane=far, cull_backfaces=cull, rays=lens_map)
    ids, depth = _decode(vis[0])
    rays = lens_map.rays[0].cpu().numpy()
    R = ML.LensRasterRef(c["verts"], c["faces"], rays, W, H, near, far, cull)
    assert R.tolerance_share() <= 0.02, R.tolerance_share()
    r = R.check_raster(ids, depth)
    res = mesh_resolve(vc, faces, K, W, H, ws, vertex_colors=_dev(shade.get("vertex_colors")), face_colors=_dev(shade.get("face_colors")),
                       headlight=shade.get("headlight", False), ambient=shade.get("ambient", 0.3), return_normals=True, rays=lens_map)
    res = {k: v[0].cpu().numpy() for k, v in res.items()}
    assert np.array_equal(res["face_ids"], ids) and np.array_equal(_bits(res["depth"]), _bits(depth))
    assert (res["depth"][ids < 0] == 0).all() and (res["rgb"][ids < 0] == 0).all() and (res["depth"][ids >= 0] > 0).all()
    assert (ids[np.isnan(rays).any(-1)] == -1).all()                               # a pixel without a ray is uncovered
    MS.check_shading(R, r, c["faces"], res["rgb"], res["normals"], **shade)
    return R, r, ids, res


@pytest.mark.parametrize("lens", LENS_NAMES)
@pytest.mark.parametrize("size", [(37, 29), (64, 64), (112, 80)])
def test_rays_stay_inside_their_bound_and_the_valid_set_is_the_references(lens, size):
    W, H = size
    lens_map, K = _ray_map(lens, W, H)
    model, k, _ = ML.LENSES[lens]
    got = ML.RayRef(model, K, k, W, H).check_rays(lens_map.rays[0].cpu().numpy())
    print(f"\n{lens} {W}x{H}: rays worst error / bound {got['worst']:.3f}, {got['valid']} valid, {got['near_fold']} next to a fold")
    assert (got["valid"] < W * H) == ("folding" in lens)
    assert lens_map.rays.shape == (1, H, W, 2) and lens_map.rows.shape == (1, 16)


@pytest.mark.parametrize("lens", LENS_NAMES)
@pytest.mark.parametrize("size", [(37, 29), (64, 64), (112, 80)])
def test_raster_and_resolve_on_the_gpus_rays_pass_the_statement(lens, size):
    W, H = size
    lens_map, _ = _ray_map(lens, W, H)
    cases = MR.raster_cases(W, H)
    has = ~np.isnan(lens_map.rays[0].cpu().numpy()).any(-1)
    covered = 0
    for name in CASES:
        c = cases[name]
        R, r, ids, res = _stages(c, lens_map, W, H, vertex_colors=_colors(len(c["verts"]), 5), headlight=True, ambient=0.25)
        covered += r["covered"]
        if c.get("bad_index"):
            assert not np.isin(ids, np.arange(0, len(c["faces"]), 3)).any(), name   # faces naming vertex V never win
        if name == "full_image_plus_64":                                            # the large path: every pixel that has a ray
            assert np.array_equal(ids >= 0, has), name
    assert covered > 0


def test_tall_frame_mostly_without_rays_and_face_colours():
    """16 x 2064: 258 rows of blocks, 33 of superblocks; under the mild pinhole lens the fold crosses the frame."""
    W, H = 16, 2064
    lens_map, K = _ray_map("bc_mild", W, H)
    rays = lens_map.rays[0].cpu().numpy()
    has = ~np.isnan(rays).any(-1)
    assert 0 < has.sum() < W * H
    ML.RayRef(ML.BC, K, PR.MILD, W, H).check_rays(rays)
    v, f = MR.random_faces(64, W, H, seed=21, K=MR.pinhole(W, H))
    big = np.array([[-400, -300, 4.0], [400, -300, 4.0], [0, 500, 4.0]], np.float32)
    c = dict(verts=np.concatenate([big, v]), faces=np.concatenate([[[0, 1, 2]], f + 3]).astype(np.int32))
    R, r, ids, res = _stages(c, lens_map, W, H, face_colors=_colors(65, 2))
    assert np.array_equal(ids >= 0, has)


def test_zero_coefficients_through_the_lens_entry_points_give_the_pinhole_paths_faces():
    """All-zero pinhole coefficients select the plain path in the Python layer; handed to the lens entry points as a row they
    give the pinhole path's face ids wherever neither statement calls the pixel decided by tolerance."""
    from robosimgs_amd import _lib, mesh_raster
    from robosimgs_amd import mesh_render as M
    W, H = 64, 64
    c = MR.raster_cases(W, H)["random129"]
    K = c["K"]
    rows = _dev(PR.lens_row(K, (0.0,) * 5)[None], np.float32)
    ws, pad = M._workspace(None, M.mesh_lens_workspace_bytes(1, W, H), torch.device(DEV, torch.cuda.current_device()))
    _lib.check(_lib.lib().mgs_mesh_lens_rays(1, ML.BC, _lib.ptr(rows), W, H, ws.data_ptr() + pad, ws.numel() - pad,
                                              _lib.stream_handle()), "mgs_mesh_lens_rays")
    lens_map = M.MeshLensMap(ML.BC, rows, ws, pad, 1, W, H)
    rays = lens_map.rays[0].cpu().numpy()
    d = ML.pixel_d(K, W, H)
    assert not np.isnan(rays).any() and (np.abs(rays - d) <= 2 * np.spacing(np.abs(d).astype(np.float32))).all()
    vc, faces, Kd = _dev(c["verts"], np.float32)[None].contiguous(), _dev(c["faces"], np.int32), _dev(K[None], np.float32)
    ids_lens, depth_lens = _decode(mesh_raster(vc, faces, Kd, W, H, rays=lens_map)[0][0])
    ids_pin, depth_pin = _decode(mesh_raster(vc, faces, Kd, W, H)[0][0])
    Rl = ML.LensRasterRef(c["verts"], c["faces"], rays, W, H)
    Rp = MR.RasterRef(c["verts"], c["faces"], K, W, H)
    Rl.check_raster(ids_lens, depth_lens)
    strict = ~(Rl.by_tolerance | Rp.by_tolerance).reshape(H, W)
    assert np.array_equal(ids_lens[strict], ids_pin[strict]) and strict.mean() > 0.98 and (ids_pin >= 0).sum() > 100


@pytest.mark.parametrize("lens", LENS_NAMES)
def test_mesh_registers_with_the_gaussian_projection_under_the_same_lens(lens):
    """Marker triangles about 6 px across, fronto-parallel at depth z: fully_fused_projection under the lens maps a marker's
    centroid to means2d; the mesh frame's face id at that pixel is the marker's and its depth is z within tol_z."""
    from robosimgs_amd import Mesh, fully_fused_projection, rasterize_mesh
    W, H, z = 112, 80, 2.5
    model, k, _ = ML.LENSES[lens]
    K = ML.intrinsics(lens, W, H)
    ref = ML.RayRef(model, K, k, W, H)
    # marker pixels: a grid over the frame, kept where the 9 x 9 pixels around them all have rays
    ok = ref.valid.copy()
    for dy in range(-4, 5):
        for dx in range(-4, 5):
            ok &= np.roll(np.roll(ref.valid, dy, 0), dx, 1)
    ok[:4], ok[-4:], ok[:, :4], ok[:, -4:] = False, False, False, False
    ys, xs = np.meshgrid(np.arange(6, H, 11), np.arange(7, W, 11), indexing="ij")
    keep = ok[ys, xs]
    rng = np.random.default_rng(4)
    pix = np.stack([xs[keep], ys[keep]], 1) + 0.5 + rng.uniform(-0.3, 0.3, (int(keep.sum()), 2))
    assert len(pix) >= 8
    verts, faces = ML.markers(model, k, K, pix, z)
    kw = _lens_kw(lens)
    rgb, depth, meta = rasterize_mesh(Mesh(verts, faces).to(DEV), np.eye(4, dtype=np.float32), K, W, H, **kw)
    ids, depth, rays = meta["face_ids"][0].cpu().numpy(), depth[0].cpu().numpy(), meta["rays"][0].cpu().numpy()
    centroids = verts.reshape(-1, 3, 3).astype(np.float64).mean(1).astype(np.float32)
    n = len(centroids)
    quats = np.tile(np.array([1.0, 0, 0, 0], np.float32), (n, 1))
    radii, means2d, depths, _, _ = fully_fused_projection(_dev(centroids), None, _dev(quats), _dev(np.full((n, 3), 0.01, np.float32)),
                                                          torch.eye(4, device=DEV)[None], _dev(K[None], np.float32), W, H, **kw)
    m2 = means2d[0].cpu().numpy()
    assert (radii[0].cpu().numpy().reshape(n, -1) > 0).all()
    assert np.abs(m2 - pix).max() < 0.02                                           # the projection lands where the markers were aimed
    px, py = np.floor(m2[:, 0]).astype(int), np.floor(m2[:, 1]).astype(int)
    assert np.array_equal(ids[py, px], np.arange(n))
    R = ML.LensRasterRef(verts, faces, rays, W, H)
    pr = R.pair_of(py * W + px, np.arange(n))
    assert (pr >= 0).all() and (np.abs(depth[py, px] - float(np.float32(z))) <= R.tolz[pr]).all()
    R.check_raster(ids, depth)


def test_two_cameras_with_different_lenses_equal_two_calls_and_a_repeat_is_bit_identical():
    from robosimgs_amd import Mesh, rasterize_mesh
    W, H = 64, 64
    c = MR.raster_cases(W, H)["full_image_plus_64"]
    mesh = Mesh(c["verts"], c["faces"], vertex_colors=_colors(len(c["verts"]), 3)).to(DEV)
    Ks = np.stack([ML.intrinsics("bc_mild", W, H), ML.intrinsics("bc_folding", W, H)])
    ks = np.array([PR.MILD, PR.FOLDING])
    vm = np.stack([np.eye(4), np.eye(4)]).astype(np.float32)
    vm[1, :3, 3] = [0.1, -0.05, 0.3]
    kw = dict(headlight=True, return_normals=True)
    both = rasterize_mesh(mesh, vm, Ks, W, H, pinhole_distortion=ks, **kw)
    again = rasterize_mesh(mesh, vm, Ks, W, H, pinhole_distortion=ks, **kw)
    flat = lambda o: [o[0], o[1], o[2]["face_ids"], o[2]["normals"], o[2]["rays"], o[2]["verts_cam"]]
    for a, b in zip(flat(both), flat(again)):
        assert torch.equal(a.view(torch.int32) if a.dtype == torch.float32 else a, b.view(torch.int32) if b.dtype == torch.float32 else b)
    for i in range(2):
        one = rasterize_mesh(mesh, vm[i], Ks[i], W, H, pinhole_distortion=ks[i], **kw)
        for a, b in zip(flat(both), flat(one)):
            a, b = a[i].contiguous(), b[0].contiguous()
            assert torch.equal(a.view(torch.int32) if a.dtype == torch.float32 else a, b.view(torch.int32) if b.dtype == torch.float32 else b)
    has = ~torch.isnan(both[2]["rays"]).any(-1)
    assert has[0].all() and not has[1].all() and torch.equal(both[2]["face_ids"] >= 0, has)
    # the fisheye, ideal and distorted, through the same call
    Kf = ML.intrinsics("kb_folding", W, H)
    ideal = rasterize_mesh(mesh, vm[0], Kf, W, H, camera_model="fisheye")
    bent = rasterize_mesh(mesh, vm[0], Kf, W, H, camera_model="fisheye", distortion=LR.FOLDING)
    assert (ideal[2]["face_ids"] >= 0).sum() > (bent[2]["face_ids"] >= 0).sum() > 0
    # all-zero coefficients select the plain path: no ray map, the pinhole path's bytes
    plain, zero = rasterize_mesh(mesh, vm[0], Ks[0], W, H), rasterize_mesh(mesh, vm[0], Ks[0], W, H, pinhole_distortion=(0.0,) * 5)
    assert "rays" not in zero[2] and torch.equal(plain[0], zero[0]) and torch.equal(plain[2]["face_ids"], zero[2]["face_ids"])


def test_rasterization_takes_a_mesh_layer_rendered_under_its_lens_as_foreground():
    from robosimgs_amd import Mesh, camera_ring, rasterization, rasterize_mesh, synthetic_scene
    import math
    W, H = 112, 80
    K = ML.intrinsics("bc_mild", W, H)
    g = synthetic_scene(400, math.log(0.07), 0, 0)
    vm = camera_ring(1, W, H, thetas=[0.7], radius=3.0)[0].viewmat().astype(np.float32)
    # a quad in front of the scene's middle, in camera space, carried to the world
    quad = np.array([[-0.4, -0.3, 2.0], [0.5, -0.3, 2.2], [0.5, 0.35, 2.2], [-0.4, 0.35, 2.0]], np.float64)
    world = (quad - vm[:3, 3]) @ vm[:3, :3]
    mesh = Mesh(world.astype(np.float32), np.array([[0, 1, 2], [0, 2, 3]], np.int32)).to(DEV)
    fg_rgb, fg_depth, meta = rasterize_mesh(mesh, vm, K, W, H, pinhole_distortion=PR.MILD)
    assert 200 < int((fg_depth > 0).sum()) < W * H
    t = lambda a: torch.as_tensor(np.asarray(a, np.float32), device=DEV)
    colors = torch.rand(len(g.means), 3, device=DEV)
    out, alphas, m = rasterization(t(g.means), t(g.quats), t(g.scales), t(g.opacities), colors, t(vm)[None], t(K)[None], W, H,
                                   render_mode="RGB+ED", pinhole_distortion=PR.MILD, foreground=(fg_rgb, fg_depth))
    vis = m["fg_visibility"]
    assert vis.shape == (1, H, W) and torch.isfinite(m["hybrid_rgb"]).all()
    assert (vis[fg_depth <= 0] == 0).all() and (vis[fg_depth > 0] > 0).any()
