"""TSDFVolume on the GPU (csrc/tsdf.hip): the integration against the fp64 statement and its counted bound (tests/tsdf_ref.py),
its invariance under chunking and under the frame layout, the extraction on the GPU's own volumes against the statement
index for index, the emit pass's capacity guards, and a Gaussian scene rendered, fused, extracted and rasterised again."""
import numpy as np
import pytest
import torch

import tsdf_ref as R
from robosimgs_amd import Mesh, TSDFVolume, rasterization, rasterize_mesh
from robosimgs_amd._lib import MgsError
from robosimgs_amd.tsdf import check_extract_status, tsdf_extract_raw

DEV = "cuda"
pytestmark = pytest.mark.gpu


def _dev(a):
    return torch.as_tensor(np.ascontiguousarray(a), device=DEV)


def _frames(views, sl=slice(None)):
    """(RGB+ED frames [C,H,W,4], alphas [C,H,W,1], viewmats, Ks) of a view dict, on the device."""
    frames = np.concatenate([views["rgb"][sl], views["depth"][sl][..., None]], -1)
    return _dev(frames), _dev(views["alphas"][sl][..., None]), _dev(views["viewmats"][sl]), _dev(views["Ks"][sl])


def _volume(case, color=True, max_weight=R.MAX_WEIGHT):
    return TSDFVolume(case["origin"], case["voxel"], case["dims"], color=color, max_weight=max_weight, device=DEV)


def _flat(vol):
    f = vol.tsdf.cpu().numpy().astype(np.float64).ravel()
    w = vol.weight.cpu().numpy().astype(np.float64).ravel()
    c = None if vol.color is None else vol.color.cpu().numpy().astype(np.float64).reshape(3, -1)
    return f, w, c


_fused = {}


def fused_volume(dims, n_views):
    """The GPU's volume of one of R.FUSION_CASES, fused once and shared (read-only)."""
    key = (tuple(dims), n_views)
    if key not in _fused:
        case, _ = R.fusion_reference(dims, n_views)
        vol = _volume(case)
        frames, alphas, vm, Ks = _frames(R.fusion_views(case))
        assert vol.integrate(frames, vm, Ks, alphas=alphas) is vol
        _fused[key] = vol
    return _fused[key]


@pytest.mark.parametrize("dims,n_views", R.FUSION_CASES)
def test_integrate_meets_integration_bound(dims, n_views):
    """Every sample within integration_bound of the fp64 statement with its weight, or on one of the statement's own thresholds
    and equal to it with that decision flipped; at most 0.5 % of the observed samples may need that (the fp32 restatement
    needs none: tests/test_tsdf_host.py).  Three and five views of 40 x 30 analytic depth with alpha holes, NaN, infinite and zero
    depth pixels, among them a view that has the volume behind it and (of the five) one that sees none of it; the first view
    is then fused twice more in the same call, so that max_weight = 2 binds.  Measured on an MI355X: nothing excused, the
    largest error 0.17 and 0.18 of the bound."""
    case, ref = R.fusion_reference(dims, n_views)
    f, w, c = _flat(fused_volume(dims, n_views))
    assert np.isfinite(f).all() and np.isfinite(c).all()
    ijk = R.grid_ijk(dims)
    res = R.check_integration(f, w, c, ref, lambda idx, flip: R.fuse(np.float64, case, ijk=ijk[idx], flip=flip))
    print(dims, res, "largest bound", ref["bound"].max())
    assert res["observed"] > 100 and res["excused"] <= 0.005 * res["observed"]
    untouched = ref["n_updates"] == 0
    assert (f[untouched] == 0).all() and (w[untouched] == 0).all() and (c[:, untouched] == 0).all()


def test_chunking_gives_identical_bytes():
    dims, n_views = R.FUSION_CASES[1]
    case, _ = R.fusion_reference(dims, n_views)
    assert n_views == 5
    vols = []
    for chunks in ([slice(0, 5)], [slice(0, 2), slice(2, 5)], [slice(i, i + 1) for i in range(5)]):
        vol = _volume(case, max_weight=64.0)
        for sl in chunks:
            frames, alphas, vm, Ks = _frames(case, sl)
            vol.integrate(frames, vm, Ks, alphas=alphas)
        vols.append(vol)
    assert vols[0].weight.max() >= 2
    for other in vols[1:]:
        for name in ("tsdf", "weight", "color"):
            assert torch.equal(getattr(vols[0], name).view(torch.int32), getattr(other, name).view(torch.int32)), name
    again = vols[0].reset()
    assert not again.tsdf.any() and not again.weight.any() and not again.color.any()


@pytest.mark.parametrize("dims,n_views", R.FUSION_CASES)
def test_depth_only_path_gives_the_rgbd_path_bytes(dims, n_views):
    """A [C,H,W] depth tensor into a volume without colour: the tsdf and weight bytes of the RGB+ED path on the same depth (the
    alpha test folded into the depth image, which is what a sensor delivers: 0 where it saw nothing)."""
    case, _ = R.fusion_reference(dims, n_views)
    views = R.fusion_views(case)
    frames, alphas, vm, Ks = _frames(views)
    with_color = fused_volume(dims, n_views)
    plain = _volume(case, color=False)
    plain.integrate(frames, vm, Ks, alphas=alphas)                      # the RGB+ED frame into a volume without colour
    with np.errstate(invalid="ignore"):
        depth = _dev(np.where(views["alphas"] >= 0.5, views["depth"], 0.0).astype(np.float32))
    sensor = _volume(case, color=False)
    sensor.integrate(depth, vm, Ks)
    for vol in (plain, sensor):
        assert vol.color is None
        assert torch.equal(vol.tsdf.view(torch.int32), with_color.tsdf.view(torch.int32))
        assert torch.equal(vol.weight.view(torch.int32), with_color.weight.view(torch.int32))
    with pytest.raises(ValueError, match="color=False"):
        _volume(case).integrate(depth, vm, Ks)
    with pytest.raises(ValueError, match="frames"):
        plain.integrate(frames[..., :3].contiguous(), vm, Ks)
    with pytest.raises(ValueError, match="viewmats"):
        plain.integrate(frames, vm[:1], Ks)
    with pytest.raises(NotImplementedError):
        plain.integrate(frames, vm, Ks, camera_model="fisheye")


def _set(vol, f, w, c):
    vol.tsdf.copy_(_dev(f))
    vol.weight.copy_(_dev(w))
    if c is not None:
        vol.color.copy_(_dev(c))
    return vol


def _extract_volumes():
    dims, n_views = R.FUSION_CASES[0]
    case, _ = R.fusion_reference(dims, n_views)
    yield "fused", fused_volume(dims, n_views)
    f, w, c = R.random_volume((9, 8, 7), holes=0.15)
    yield "random with weight holes", _set(TSDFVolume((-0.3, 0.1, 2.0), 0.05, (9, 8, 7), device=DEV), f, w, c)
    f, w, c = R.level_volume()
    yield "values on the level", _set(TSDFVolume((1.0, -2.0, 0.5), 0.02, (8, 7, 6), device=DEV), f, w, c)
    f, w, c = R.random_volume((2, 2, 2), seed=4)
    yield "one cell", _set(TSDFVolume((0, 0, 0), 0.1, (2, 2, 2), device=DEV), f, w, c)
    f, w = R.sphere_volume()                                             # six workgroups of the count pass
    yield "sphere", _set(TSDFVolume((0, 0, 0), 1.0, (19, 18, 17), color=False, device=DEV), f, w, None)


def test_extract_matches_the_statement_on_the_gpus_own_volumes():
    """faces equal as integers; vertices and colours within the bound tsdf_ref counts (one division and one fma per coordinate at
    the coordinate's magnitude) -- the statement reads the bytes the GPU holds."""
    for name, vol in _extract_volumes():
        c = None if vol.color is None else vol.color.cpu().numpy()
        ref = R.extract(vol.tsdf.cpu().numpy(), vol.weight.cpu().numpy(), c, np.float32(vol.origin), vol.voxel_size)
        v, faces, col = vol.extract_arrays()
        assert v.dtype == torch.float32 and faces.dtype == torch.int32
        assert tuple(v.shape) == (len(ref["vertices"]), 3) and tuple(faces.shape) == (len(ref["faces"]), 3), name
        assert len(ref["faces"]) > 0, name
        assert np.array_equal(faces.cpu().numpy(), ref["faces"]), name
        assert (np.abs(v.cpu().numpy() - ref["vertices"]) <= ref["vertex_bound"]).all(), name
        if c is not None:
            assert (np.abs(col.cpu().numpy() - ref["colors"]) <= ref["color_bound"]).all(), name
        mesh = vol.extract_mesh()
        assert isinstance(mesh, Mesh) and mesh.n_faces == len(ref["faces"]) and (mesh.vertex_colors is None) == (c is None)


def test_a_volume_of_more_than_one_scan_round_comes_out_closed():
    """72 x 64 x 64 samples are 288 workgroups of the count pass, more than the 256 block sums the scan takes per round: the
    carry between rounds is in every offset behind it, and a sphere comes out closed, outward and of Euler characteristic 2
    only if every one of them is right."""
    center, radius = (35.2, 31.9, 32.4), 20.3
    f, w = R.sphere_volume((72, 64, 64), radius, center)
    vol = _set(TSDFVolume((0, 0, 0), 1.0, (72, 64, 64), color=False, device=DEV), f, w, None)
    v, faces, col = vol.extract_arrays()
    assert col is None and vol.tsdf.numel() > 256 * 1024
    v, faces = v.cpu().numpy().astype(np.float64), faces.cpu().numpy()
    top = R.mesh_topology(faces, len(v))
    assert len(faces) > 20000 and top["closed"] and top["euler"] == 2 and top["unreferenced"] == 0
    normals = np.cross(v[faces[:, 1]] - v[faces[:, 0]], v[faces[:, 2]] - v[faces[:, 0]])
    assert ((normals * (v[faces].mean(1) - np.array(center))).sum(1) > 0).all()
    h = np.sqrt(3.0)
    assert np.abs(np.linalg.norm(v - np.array(center), axis=1) - radius).max() <= h * h / (8 * (radius - h)) + 1e-4


def test_no_crossing_gives_empty_arrays_and_a_named_error():
    vol = TSDFVolume((0, 0, 0), 0.1, (5, 4, 3), device=DEV)
    for fill, weight in ((1.0, 1.0), (0.0, 0.0)):                   # all outside; and the empty volume, which nobody observed
        vol.tsdf.fill_(fill)
        vol.weight.fill_(weight)
        v, faces, col = vol.extract_arrays()
        assert tuple(v.shape) == (0, 3) and tuple(faces.shape) == (0, 3) and tuple(col.shape) == (0, 3)
        with pytest.raises(ValueError, match="surface is empty"):
            vol.extract_mesh()
    vol.tsdf.copy_(_dev(R.random_volume((5, 4, 3))[0]))
    vol.weight.fill_(1.0)
    assert vol.extract_arrays()[1].shape[0] > 0 and vol.extract_arrays(min_weight=2.0)[1].shape[0] == 0


def test_short_capacities_are_refused_and_nothing_is_written_past_them():
    f, w, c = R.random_volume((9, 8, 7))
    vol = _set(TSDFVolume((0, 0, 0), 1.0, (9, 8, 7), device=DEV), f, w, c)
    full_v, full_f, full_c, (n_v, n_f), status = tsdf_extract_raw(vol, 0.0, 1.0)
    check_extract_status(status)
    assert n_v == full_v.shape[0] > 100 and n_f == full_f.shape[0] > 100
    guard = 16
    for cap_v, cap_f in ((n_v // 2, n_f), (n_v, n_f // 3), (0, 0), (n_v - 1, n_f - 1)):
        v, faces, col, counts, status = tsdf_extract_raw(vol, 0.0, 1.0, vertex_capacity=cap_v, face_capacity=cap_f,
                                                         guard_rows=guard)
        assert counts == (n_v, n_f)
        with pytest.raises(MgsError, match="OVERFLOW"):
            check_extract_status(status)
        assert (v[cap_v:] == -7).all() and (col[cap_v:] == -7).all() and (faces[cap_f:] == -7).all()
        assert torch.equal(v[:cap_v], full_v[:cap_v]) and torch.equal(col[:cap_v], full_c[:cap_v])
        assert torch.equal(faces[:cap_f], full_f[:cap_f])
    v, faces, col, _, status = tsdf_extract_raw(vol, 0.0, 1.0, vertex_capacity=n_v + 5, face_capacity=n_f + 5, guard_rows=guard)
    check_extract_status(status)                                        # room to spare: no overflow, the spare rows untouched
    assert (v[n_v:] == -7).all() and (faces[n_f:] == -7).all() and torch.equal(faces[:n_f], full_f)


# ---- end to end -----------------------------------------------------------------------------------------------------------
def _surfel_scene():
    """About 3,000 flat opaque Gaussians: a plane z = 0.3 and a sphere shell of radius 0.22 about (0.6, 0.6, 0.62)."""
    g = np.arange(-0.5, 1.7001, 0.05)
    px, py = np.meshgrid(g, g)
    plane = np.stack([px.ravel(), py.ravel(), np.full(px.size, 0.3)], 1)
    n_s = 1000
    k = np.arange(n_s) + 0.5
    phi, z = np.pi * (1 + 5 ** 0.5) * k, 1 - 2 * k / n_s
    normals_s = np.stack([np.cos(phi) * np.sqrt(1 - z * z), np.sin(phi) * np.sqrt(1 - z * z), z], 1)
    shell = np.array([0.6, 0.6, 0.62]) + 0.22 * normals_s
    normals = np.concatenate([np.tile([0.0, 0.0, 1.0], (len(plane), 1)), normals_s])
    quats = np.stack([1 + normals[:, 2], -normals[:, 1], normals[:, 0], np.zeros(len(normals))], 1)      # z axis -> normal, wxyz
    quats[quats[:, 0] < 1e-6] = [0.0, 1.0, 0.0, 0.0]
    quats /= np.linalg.norm(quats, axis=1, keepdims=True)
    means = np.concatenate([plane, shell])
    scales = np.concatenate([np.tile([0.035, 0.035, 0.002], (len(plane), 1)), np.tile([0.02, 0.02, 0.002], (n_s, 1))])
    colors = np.concatenate([np.tile([0.2, 0.6, 0.3], (len(plane), 1)), np.tile([0.8, 0.3, 0.2], (n_s, 1))])
    f32 = lambda a: _dev(a.astype(np.float32))
    return f32(means), f32(quats), f32(scales), torch.full((len(means),), 0.99, device=DEV), f32(colors)


def test_gaussian_scene_to_mesh_end_to_end():
    W, H, voxel = 96, 72, 0.025
    scene = _surfel_scene()
    assert 2500 <= scene[0].shape[0] <= 3500
    target = (0.6, 0.6, 0.5)
    eye = lambda a, h=1.4: (0.6 + 1.5 * np.cos(a), 0.6 + 1.5 * np.sin(a), h)
    vm = _dev(np.stack([R.look_at(eye(a), target) for a in np.linspace(0, 2 * np.pi, 6, endpoint=False)]))
    K = np.array([[85.0, 0, W / 2], [0, 85.0, H / 2], [0, 0, 1]], np.float32)
    Ks = _dev(np.repeat(K[None], 6, 0))
    frames, alphas, _ = rasterization(*scene, vm, Ks, W, H, render_mode="RGB+ED")
    assert tuple(frames.shape) == (6, H, W, 4) and tuple(alphas.shape) == (6, H, W, 1)
    vol = TSDFVolume.from_bounds((0, 0, 0), (1.2, 1.2, 1.2), voxel, device=DEV)
    assert vol.dims == (48, 48, 48) and vol.trunc == 3 * voxel
    vol.integrate(frames, vm, Ks, alphas=alphas)
    mesh = vol.extract_mesh()
    v, faces = mesh.vertices.cpu().numpy().astype(np.float64), mesh.faces.cpu().numpy()
    assert len(faces) > 5000 and mesh.vertex_colors is not None
    top = R.mesh_topology(faces, len(v))
    assert top["unreferenced"] == 0
    # closed where fully observed: every open edge lies within two samples of one that was not observed, or of the grid's border
    seen = torch.nn.functional.pad((vol.weight >= 1).float()[1:-1, 1:-1, 1:-1], (1,) * 6)[None, None]
    near_unseen = (-torch.nn.functional.max_pool3d(-seen, 5, 1, 2))[0, 0].cpu().numpy() == 0
    ends = np.unique(top["directed"][top["open_edge"]])
    idx = np.clip(np.floor(v[ends] / voxel - 0.5).astype(int), 0, 47)
    assert near_unseen[idx[:, 2], idx[:, 1], idx[:, 0]].all()
    assert top["boundary"] < 0.05 * 3 * len(faces)
    # from a held-out camera the mesh's depth is the splat frame's, to the volume's sampling step
    vm_h, K_h = _dev(R.look_at(eye(0.55, 1.25), target)[None]), Ks[:1]
    held, held_alpha, _ = rasterization(*scene, vm_h, K_h, W, H, render_mode="RGB+ED")
    _, depth, meta = rasterize_mesh(mesh, vm_h, K_h, W, H)
    both = (meta["face_ids"][0] >= 0) & (held_alpha[0, ..., 0] > 0.5)
    assert int(both.sum()) > 0.3 * W * H
    median = float((depth[0] - held[0, ..., 3]).abs()[both].median())
    print(f"held-out camera: median |mesh depth - expected depth| = {median:.5f} = {median / voxel:.3f} voxel over "
          f"{int(both.sum())} pixels; {len(v)} vertices, {len(faces)} faces, {top['boundary']} open edges")
    assert median <= voxel
