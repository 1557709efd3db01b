"""Device-side similarity transforms of Gaussian groups against the host-side
NumPy `Gaussians.transformed()` and against the renderer itself (equivariance)."""
import math

import numpy as np
import pytest
import torch

import frame_helper_ref as F
from robosimgs_amd import camera_ring, synthetic_scene

pytestmark = pytest.mark.gpu
DEV = "cuda"


def _rot(rng):
    q, _ = np.linalg.qr(rng.normal(size=(3, 3)))
    if np.linalg.det(q) < 0:
        q[:, 0] = -q[:, 0]
    return q


def _t(a):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32)).to(DEV)


@pytest.mark.parametrize("deg,scale", [(3, 1.0), (2, 1.7), (0, 0.5)])
def test_single_transform_matches_host(deg, scale):
    from robosimgs_amd import transform_gaussians
    rng = np.random.default_rng(deg)
    g = synthetic_scene(5000, math.log(0.05), deg, 2)
    R, t = _rot(rng), rng.normal(size=3)
    ref = g.transformed(R, t, scale).to_torch(DEV, deg)
    got = transform_gaussians(g.to_torch(DEV, deg), [R], [t], [scale])
    for k in ("means", "scales", "opacities"):
        torch.testing.assert_close(got[k], ref[k], rtol=2e-5, atol=2e-5)
    # quaternions up to sign / norm conventions: compare the rotation they encode
    a = got["quats"] / got["quats"].norm(dim=1, keepdim=True)
    b = ref["quats"] / ref["quats"].norm(dim=1, keepdim=True)
    assert float((1 - (a * b).sum(1).abs()).max()) < 1e-5
    kc = (deg + 1) ** 2
    torch.testing.assert_close(got["colors"][:, :kc], ref["colors"][:, :kc], rtol=1e-4, atol=2e-5)


def test_groups_static_rows_and_in_place():
    from robosimgs_amd import transform_gaussians
    rng = np.random.default_rng(7)
    n = 7001
    g = synthetic_scene(n, math.log(0.05), 3, 5)
    t0 = g.to_torch(DEV, 3)
    gid = torch.from_numpy(rng.integers(-1, 3, size=n).astype(np.int32)).to(DEV)     # -1 static, 3 groups
    Rs = [_rot(rng) for _ in range(3)]
    ts = [rng.normal(size=3) for _ in range(3)]
    ss = [1.0, 1.3, 0.8]
    got = transform_gaussians(t0, Rs, ts, ss, group_ids=gid)
    for k in range(-1, 3):
        sel = (gid == k)
        if k < 0:
            for name in ("means", "quats", "scales", "colors"):
                assert torch.equal(got[name][sel], t0[name][sel]), name        # untouched bit for bit
            continue
        ref = g.transformed(Rs[k], ts[k], ss[k]).to_torch(DEV, 3)
        torch.testing.assert_close(got["means"][sel], ref["means"][sel], rtol=2e-5, atol=2e-5)
        torch.testing.assert_close(got["scales"][sel], ref["scales"][sel], rtol=2e-5, atol=1e-6)
        torch.testing.assert_close(got["colors"][sel], ref["colors"][sel], rtol=1e-4, atol=2e-5)
    # in place: same result, the static rows are not even written
    t1 = {k: (v.clone() if torch.is_tensor(v) else v) for k, v in t0.items()}
    same = transform_gaussians(t1, Rs, ts, ss, group_ids=gid, out=t1)
    for name in ("means", "quats", "scales", "colors"):
        assert same[name].data_ptr() == t1[name].data_ptr()
        assert torch.equal(same[name], got[name]), name
    # pre-packed device transforms (no host work per call) give the same bits
    from robosimgs_amd.transform import pack_transforms
    xp, rp = pack_transforms(Rs, ts, ss, 3)
    pk = transform_gaussians(t0, group_ids=gid, packed=(_t(xp), _t(rp)))
    for name in ("means", "quats", "scales", "colors"):
        assert torch.equal(pk[name], got[name]), name
    # without SH rotation the coefficient tensor is passed through
    plain = transform_gaussians(t0, Rs, ts, ss, group_ids=gid, rotate_sh=False)
    assert plain["colors"] is t0["colors"] and torch.equal(plain["means"], got["means"])


def test_render_is_equivariant_under_a_moved_scene_and_camera():
    """Moving the whole scene AND the camera by the same rigid motion must not change the image
    (this is what rotating the SH colour field with the Gaussians buys)."""
    from robosimgs_amd import rasterization, transform_gaussians
    rng = np.random.default_rng(3)
    g = synthetic_scene(20_000, math.log(0.04), 3, 1)
    cam = camera_ring(1, 320, 200, thetas=[0.9])[0]
    t0 = g.to_torch(DEV, 3)
    R, t = _rot(rng), rng.normal(size=3)
    moved = transform_gaussians(t0, [R], [t])
    T = np.eye(4)
    T[:3, :3], T[:3, 3] = R, t
    vm0 = cam.viewmat()
    vm1 = vm0 @ np.linalg.inv(T)                      # world-to-camera of the moved camera
    args = dict(sh_degree=3, render_mode="RGB+ED")
    a, aa, _ = rasterization(t0["means"], t0["quats"], t0["scales"], t0["opacities"], t0["colors"],
                             _t(vm0)[None], _t(cam.K)[None], 320, 200, **args)
    b, ba, _ = rasterization(moved["means"], moved["quats"], moved["scales"], moved["opacities"],
                             moved["colors"], _t(vm1)[None], _t(cam.K)[None], 320, 200, **args)
    bad = ((a - b).abs().amax(-1) > 2e-3) | ((aa - ba).abs()[..., 0] > 2e-3)
    assert float(bad.float().mean()) < 2e-3, float(bad.float().mean())


def test_frame_renderer_poses_groups_per_frame():
    """Dynamic scene through FrameRenderer: every submit poses the groups (in-graph
    mgs_transform_gaussians on the slot's own copy); frames equal transform + rasterization done
    by hand, with three frames in flight and a different pose per frame."""
    from robosimgs_amd import FrameRenderer, rasterization, transform_gaussians
    rng = np.random.default_rng(11)
    n = 30_000
    g = synthetic_scene(n, math.log(0.05), 3, 6)
    t0 = g.to_torch(DEV, 3)
    gid = torch.from_numpy(rng.integers(-1, 2, size=n).astype(np.int32)).to(DEV)
    cams = camera_ring(5, 256, 160)
    r = FrameRenderer(t0, 256, 160, render_mode="RGB+ED", frames_in_flight=3, isect_capacity=600_000,
                      group_ids=gid, n_groups=2)
    poses = [([_rot(rng), _rot(rng)], [0.3 * rng.normal(size=3), 0.3 * rng.normal(size=3)]) for _ in cams]
    tickets, got = [], []
    for cam, (Rs, ts) in zip(cams, poses):
        if len(tickets) == 3:
            tk = tickets.pop(0)
            f = r.fetch(tk)
            got.append((f["colors"].clone(), f["alphas"].clone()))
            r.release(tk)
        tickets.append(r.submit(cam.viewmat(), cam.K, rotations=Rs, translations=ts))
    for tk in tickets:
        f = r.fetch(tk)
        got.append((f["colors"].clone(), f["alphas"].clone()))
        r.release(tk)
    for (c, a), cam, (Rs, ts) in zip(got, cams, poses):
        # (the renderer keeps its own Morton-ordered copy of the scene, group ids permuted with it: r.t, r.group_ids)
        posed = transform_gaussians(r.t, Rs, ts, group_ids=r.group_ids)
        rc, ra, _ = rasterization(posed["means"], posed["quats"], posed["scales"], posed["opacities"],
                                  posed["colors"], _t(cam.viewmat())[None], _t(cam.K)[None], 256, 160,
                                  sh_degree=3, render_mode="RGB+ED")
        assert torch.equal(c, rc[0]) and torch.equal(a, ra[0])
    # a static renderer refuses poses
    static = FrameRenderer(t0, 256, 160, frames_in_flight=1, isect_capacity=600_000)
    with pytest.raises(ValueError):
        static.submit(cams[0].viewmat(), cams[0].K, rotations=[np.eye(3)], translations=[[0, 0, 0]])


# ---- against tests/frame_helper_ref.py::transform_ref: every SH write path, out-of-range ids, in place ----------------
NAMES = ("means", "quats", "scales", "colors")


def _bits(x):
    return x.contiguous().view(torch.int32) if torch.is_tensor(x) else np.ascontiguousarray(x).view(np.int32)


def _tensors(t, deg):
    d = {k: _t(t[k]) for k in NAMES + ("opacities",)}
    d["sh_degree"] = deg
    return d


def _against_ref(t, deg, in_place, what):
    """transform_gaussians on the arrays of `t` (n_groups = 3) against transform_ref.  Rows that do not move are
    compared bit for bit; in place they are filled with a signalling-NaN pattern first, which any write that went
    through arithmetic would change.  Returns the worst ratio to each bound."""
    from robosimgs_amd import transform_gaussians
    K = t["colors"].shape[1]
    kc = (deg + 1) ** 2
    gid = t["gids"]
    moving = np.isin(gid, (0, 1, 2))
    src = {k: t[k].copy() for k in NAMES}
    if in_place:
        for k in NAMES:
            src[k][~moving] = np.array([F.SENTINEL], np.uint32).view(np.float32)[0]
    dev = _tensors({**src, "opacities": t["opacities"]}, deg)
    before = {k: dev[k].clone() for k in NAMES}
    got = transform_gaussians(dev, t["rotations"], t["translations"], t["group_scales"], group_ids=_t_i32(gid),
                              out=dev if in_place else None)
    for k in NAMES:
        assert (got[k].data_ptr() == dev[k].data_ptr()) == in_place, k
        if not in_place:
            assert torch.equal(_bits(dev[k]), _bits(before[k])), f"{what}: input {k} changed"
    g = {k: got[k].cpu().numpy() for k in NAMES}
    for k in NAMES:                               # static and out-of-range rows, coefficients above the degree, DC
        assert np.array_equal(_bits(g[k][~moving]), _bits(src[k][~moving])), f"{what}: {k} of a row that does not move"
    assert np.array_equal(_bits(g["colors"][:, kc:]), _bits(src["colors"][:, kc:])), f"{what}: above the degree"
    assert np.array_equal(_bits(g["colors"][:, 0]), _bits(src["colors"][:, 0])), f"{what}: DC"
    ref = F.transform_ref(t["means"], t["quats"], t["scales"], t["colors"], deg, gid, 3, t["rotations"],
                          t["translations"], t["group_scales"])
    m = moving
    ratios = {k: F.worst_ratio(g[k][m], ref[k][0][m], ref[k][1][m]) for k in ("means", "scales", "colors")}
    q64 = g["quats"][m].astype(np.float64)
    ratios["norm"] = F.worst_ratio(np.linalg.norm(q64, axis=1), ref["norm"][0][m], ref["norm"][1][m])
    ratios["rot"] = F.worst_ratio(F.quat_to_rotmat(q64), ref["rot"][0][m], ref["rot"][1][m])
    print(f"transform {what} K={K} degree {deg} in place {in_place}: " + ", ".join(f"{k} {v:.3f}" for k, v in ratios.items()))
    assert max(ratios.values()) <= 1.0, (what, ratios)
    return ratios


def _t_i32(a):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.int32)).to(DEV)


@pytest.mark.parametrize("in_place", [False, True])
@pytest.mark.parametrize("K,deg", F.TRANSFORM_CASES)
def test_every_sh_write_path_against_fp64(K, deg, in_place):
    """200 Gaussians, ids from {-1, 0, 1, 2, 3, 7} with three groups (3 and 7 are out of range and pass through bit
    for bit): rows of 16 coefficients (staged through LDS) at degrees 1, 2, 3, shorter and longer-than-needed rows
    (read and written per lane, the copy-through above the active degree included), each to a fresh buffer and in
    place."""
    t = F.transform_inputs(200, K)
    assert set(t["gids"].tolist()) == set(F.TRANSFORM_GIDS)
    _against_ref(t, deg, in_place, "n=200")


@pytest.mark.parametrize("K,deg", [(16, 3), (9, 1)])
def test_a_wave_of_static_gaussians_in_place_next_to_a_moving_one(K, deg):
    """128 Gaussians in place: the first wave's 64 are all static (the kernel returns before touching SH rows), the
    second wave's all move."""
    t = dict(F.transform_inputs(128, K))
    t["gids"] = np.concatenate([np.full(64, -1), np.resize(np.array([0, 1, 2]), 64)]).astype(np.int32)
    _against_ref(t, deg, True, "static wave | moving wave")
    t["gids"] = t["gids"][::-1].copy()
    _against_ref(t, deg, True, "moving wave | static wave")


@pytest.mark.parametrize("n", [1, 63, 64, 65])
@pytest.mark.parametrize("K,deg", [(16, 3), (9, 2)])
def test_counts_around_one_wave(n, K, deg):
    t = F.transform_inputs(n, K, gids=(0, -1, 1, 2, 5))
    for in_place in (False, True):
        _against_ref(t, deg, in_place, f"n={n}")
