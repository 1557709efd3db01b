"""robosimgs_amd.points (HIP) against oracle/points_np.py."""
import numpy as np
import pytest
import torch

import frame_helper_ref as F
from oracle import points_np as P

pytestmark = pytest.mark.gpu


def _camera(rng):
    q, _ = np.linalg.qr(rng.normal(size=(3, 3)))
    if np.linalg.det(q) < 0:
        q[:, 0] = -q[:, 0]
    c2w = np.eye(4)
    c2w[:3, :3], c2w[:3, 3] = q, rng.normal(size=3)
    return c2w


def test_project_and_unproject_match_oracle():
    from robosimgs_amd import points
    rng = np.random.default_rng(1)
    K = np.array([[400.0, 0, 160], [0, 410.0, 120], [0, 0, 1]])
    c2w = _camera(rng)
    cam_pts = np.column_stack([rng.uniform(-1, 1, 5000), rng.uniform(-1, 1, 5000), rng.uniform(0.5, 6, 5000)])
    pts = P.unproject_pcd(cam_pts, c2w)
    uv, cam, depth = points.project_pcd(pts.astype(np.float32), K, c2w)
    ruv, rcam, rdepth = P.project_pcd(pts, K, c2w)
    assert uv.dtype == np.float32 and uv.shape == (5000, 3) and depth.shape == (5000, 1)
    np.testing.assert_allclose(cam, rcam, atol=2e-5)
    np.testing.assert_allclose(depth, rdepth, atol=2e-5)
    # each row within the forward error of its own fp64 magnitudes (no flat tolerance in pixels), against the oracle
    # on the fp32 points, K and c2w the kernel reads
    _project_against_bound(pts.astype(np.float32), K, c2w, "5000 points, z in [0.5, 6]")
    np.testing.assert_allclose(points.unproject_pcd(cam, c2w), pts, atol=2e-5)
    # torch in -> torch out, on the device
    tuv, _, _ = points.project_pcd(torch.from_numpy(pts).float().cuda(), K, c2w)
    assert torch.is_tensor(tuv) and tuv.is_cuda and torch.equal(tuv.cpu(), torch.from_numpy(uv))


def _project_against_bound(pts32, K, c2w, what):
    from robosimgs_amd import points
    K32, c32 = np.asarray(K, np.float32).astype(np.float64), np.asarray(c2w, np.float32).astype(np.float64)
    uv, cam, depth = points.project_pcd(pts32, K, c2w)
    with np.errstate(divide="ignore", invalid="ignore"):
        ruv, rcam, _ = P.project_pcd(pts32.astype(np.float64), K32, c32)
    ecam, euv = F.project_bound(pts32, K32, c32)
    assert np.array_equal(depth[:, 0], cam[:, 2])
    fin = np.isfinite(ruv).all(1)
    assert np.array_equal(np.isnan(uv), np.isnan(ruv)), what                 # z == 0: NaN, as the reference
    r_cam = F.worst_ratio(cam, rcam, ecam)
    r_uv = F.worst_ratio(uv[fin], ruv[fin], euv[fin])
    print(f"project_pcd, {what}: worst cam error / bound {r_cam:.3f}, uv {r_uv:.3f}")
    assert r_cam <= 1.0 and r_uv <= 1.0, (what, r_cam, r_uv)
    return uv, cam


@pytest.mark.parametrize("n", [1, 255, 256, 257])
def test_project_counts_around_one_workgroup_and_edge_depths(n):
    """Counts around the 256-thread workgroup, under a random camera; the first rows (where there is room) sit at
    z = 1e-6, z < 0 and far off axis."""
    rng = np.random.default_rng(n)
    K = np.array([[400.0, 0, 160], [0, 410.0, 120], [0, 0, 1]])
    c2w = _camera(rng)
    cam_pts = np.column_stack([rng.uniform(-1, 1, n), rng.uniform(-1, 1, n), rng.uniform(0.5, 6, n)])
    edge = np.array([[0.3, -0.2, 1e-6], [0.3, -0.2, -2.0], [50.0, -80.0, 0.01]])[: max(n - 1, 0)]
    cam_pts[: len(edge)] = edge
    _project_against_bound(P.unproject_pcd(cam_pts, c2w).astype(np.float32), K, c2w, f"{n} points")


def test_project_at_zero_depth_is_nan_like_the_reference():
    """An axis-aligned camera so that z is exactly 0, -2, 1e-6: the reference divides z by z too."""
    K = np.array([[400.0, 0, 160], [0, 410.0, 120], [0, 0, 1]])
    pts = np.array([[1.0, 2.0, 0.0], [0.0, 0.0, 0.0], [1.0, 1.0, -2.0], [1.0, 1.0, 1e-6], [1.0, 1.0, 1.0]], np.float32)
    uv, cam = _project_against_bound(pts, K, np.eye(4), "z in {0, 0, -2, 1e-6, 1}")
    assert np.isnan(uv[:2]).all() and np.isfinite(uv[2:]).all() and np.array_equal(cam, pts)
    assert uv[2].tolist() == [-40.0, -85.0, 1.0]


def _depth_map_equals_oracle(uv, depth, h, w, **kw):
    from robosimgs_amd import points
    dm, idx = points.get_depth_map(uv, depth, h, w, **kw)
    rdm, ridx = P.get_depth_map(uv, depth, h, w, **kw)
    np.testing.assert_array_equal(idx, ridx)
    np.testing.assert_array_equal(dm, rdm)
    return dm, idx


@pytest.mark.parametrize("depths,bg,winner", [([0.0, -0.0], 1e10, 0), ([-0.0, 0.0], 1e10, 0), ([-0.0], 0.0, 1),
                                              ([0.0], -0.0, 1), ([1.0, -0.0, 0.0, -0.0], 1e10, 1)])
def test_depth_map_signed_zeros_are_one_depth(depths, bg, winner):
    """-0.0 is not below +0.0 (the reference's '<'): the first zero of a cell wins it, whichever sign, and no zero
    undercuts a zero bg_depth (index N)."""
    n = len(depths)
    for stride in (2, 3):
        uv = np.full((n, stride), 1.0, np.float32)
        _, idx = _depth_map_equals_oracle(uv, np.array(depths, np.float32), 4, 4, bg_depth=bg, scale=2)
        assert idx.reshape(2, 2)[0, 0] == winner and (idx.reshape(-1)[1:] == n).all()


def test_depth_map_out_of_range_and_non_finite_coordinates():
    """+-inf, NaN, +-3e9 and +-2^31 as u and as v: a rounded quotient that is not a finite int32 goes to cell 0 on that
    axis (include/mgs.h; oracle/points_np.py states the reference's cast), 2^31 - 128 to the last cell."""
    uv, depth = F.depth_map_far_inputs()
    _, idx = _depth_map_equals_oracle(uv, depth, 4, 4, scale=1)
    assert idx.reshape(4, 4)[0, 2] == 0 and idx.reshape(4, 4)[2, 0] == 7 and idx.reshape(4, 4)[3, 2] == 14
    _depth_map_equals_oracle(uv, depth, 8, 8, scale=2)                     # the quotient decides: 3e9 / 2 is in range
    _depth_map_equals_oracle(uv, -depth, 8, 12, scale=1.5)                 # the last point wins now


@pytest.mark.parametrize("h,w,scale,n,stride", [(5, 5, 5, 300, 2), (30, 45, 1.5, 5000, 2), (30, 45, 1.5, 5000, 3),
                                                (7, 9, 2, 1000, 2)])
def test_depth_map_one_cell_float_scale_and_uv_stride_2(h, w, scale, n, stride):
    """A 1 x 1 cell grid (h = w = scale = 5), a float scale (1.5: 20 x 30 cells) and [N,2] uv rows, on coordinates that
    are not within 0.05 cells of a rounding tie (an fp32 and an fp64 quotient round alike)."""
    rng = np.random.default_rng(n + stride)
    cw, ch = int(w / scale), int(h / scale)
    uv = F.cells_off_ties(rng, n, cw, ch, scale, stride)
    depth = np.round(rng.uniform(0.3, 20.0, n), 1).astype(np.float32)       # many equal depths: first index wins
    dm, idx = _depth_map_equals_oracle(uv, depth, h, w, scale=scale)
    assert idx.shape == (cw * ch,) and (idx < n).mean() > 0.9


def test_depth_map_50000_points_contend_for_one_cell():
    """Equal depths in one cell of a 3 x 3 grid: the lowest index among the minima wins, however the atomics land."""
    n = 50_000
    uv = np.full((n, 2), 2.0, np.float32)
    depth = np.full(n, 1.0, np.float32)
    depth[:10] = 2.0
    _, idx = _depth_map_equals_oracle(uv, depth, 6, 6, scale=2)
    assert idx.reshape(3, 3)[1, 1] == 10 and (idx < n).sum() == 1


@pytest.mark.parametrize("h,w,scale,n", [(64, 96, 2, 20000), (48, 50, 3, 4000), (30, 40, 1, 3000), (16, 16, 2, 0)])
def test_depth_map_matches_oracle_bit_for_bit(h, w, scale, n):
    from robosimgs_amd import points
    rng = np.random.default_rng(h * w + n)
    uv = np.column_stack([rng.uniform(-10, w + 10, n), rng.uniform(-10, h + 10, n), np.ones(n)]).astype(np.float32)
    uv[: n // 10] = np.floor(uv[: n // 10]) + 0.5 * (scale == 1)           # exact .5 ties where they survive fp32
    depth = rng.uniform(0.3, 20.0, n).astype(np.float32)
    depth[n // 2:] = np.round(depth[n // 2:], 1)                           # many equal depths: first index wins
    if n:
        depth[:5] = [-1.0, np.nan, 1e10, 2e10, 0.0]
    dm, idx = points.get_depth_map(uv, depth, h, w, bg_depth=1e10, scale=scale)
    rdm, ridx = P.get_depth_map(uv, depth, h, w, bg_depth=1e10, scale=scale)
    assert dm.shape == (h, w) and dm.dtype == np.float32 and idx.dtype == np.int64
    np.testing.assert_array_equal(idx, ridx)
    np.testing.assert_array_equal(dm, rdm)


def test_mask_lookup_matches_oracle():
    from robosimgs_amd import points
    rng = np.random.default_rng(5)
    h, w, n = 60, 80, 30000
    mask = (rng.uniform(size=(h, w)) > 0.5).astype(np.float32)
    depth = rng.uniform(1, 3, size=(h, w)).astype(np.float32)
    uv = np.column_stack([rng.uniform(-5, w + 5, n), rng.uniform(-5, h + 5, n)]).astype(np.float32)
    pd = rng.uniform(1, 3, size=(n, 1)).astype(np.float32)
    for args in ((), (depth, pd, 0.4)):
        got = points.mask_pcd_2d(uv, mask, 0.5, *args)
        ref = P.mask_pcd_2d(uv, mask, 0.5, *args)
        assert got.dtype == bool and got.shape == (n,)
        # the sampled value sits exactly on a threshold only by rounding: allow a handful of flips
        assert (got != ref).sum() <= n * 1e-3, (got != ref).sum()
        # ... and each of them within the bilinear bound of its threshold in fp64
        keep, near = F.mask_rule(uv, mask, 0.5, *args)
        assert not ((got != keep) & ~near).any()


@pytest.mark.parametrize("h,w,n,uv_stride", F.MASK_CASES)
def test_mask_lookup_against_fp64_bilinear(h, w, n, uv_stride):
    """mask_pcd_2d against grid_sample in fp64: a decision differs only where the fp64 sample is within its derived
    bound of the threshold (mask branch) or |sample - pnt_depth| within it of depth_thresh (depth branch) -- zero
    unexplained, at most 1e-3 explained.  h == 1, w == 1, uv rows of 2 and 3 floats, the corners / edge midpoints /
    centre, points far outside and NaN rows (kept by nobody)."""
    from robosimgs_amd import points
    mask, depth, uv, pd = F.mask_inputs(h, w, n, uv_stride)
    for args in ((), (depth, pd, 0.4)):
        got = points.mask_pcd_2d(uv, mask, 0.5, *args)
        keep, near = F.mask_rule(uv, mask, 0.5, *args)
        differ = got != keep
        print(f"mask_pcd_2d {h}x{w}, depth branch {bool(args)}: {differ.sum()} of {n} differ, near {near.sum()}")
        assert not (differ & ~near).any(), np.flatnonzero(differ & ~near)[:8]
        assert differ.sum() <= n * 1e-3
        assert not got[np.isnan(uv[:, :2]).any(1)].any()


def test_zbuffer_visibility_round_trip():
    """The use the reference's helpers are written for: project a cloud, z-buffer it, and keep
    the points that are the visible surface -- a wall in front of another wall hides it."""
    from robosimgs_amd import points
    h, w = 96, 128
    K = np.array([[100.0, 0, 64], [0, 100.0, 48], [0, 0, 1]])
    c2w = np.eye(4)
    gx, gy = np.meshgrid(np.linspace(-0.6, 0.6, 200), np.linspace(-0.45, 0.45, 150))
    near = np.column_stack([gx.ravel(), gy.ravel(), np.full(gx.size, 1.0)])
    far = np.column_stack([gx.ravel() * 2, gy.ravel() * 2, np.full(gx.size, 2.0)])
    pts = np.concatenate([near, far]).astype(np.float32)
    uv, cam, depth = points.project_pcd(pts, K, c2w)
    dm, idx = points.get_depth_map(uv, depth, h, w, scale=2)
    vis = points.mask_pcd_2d(uv, np.ones((h, w), np.float32), 0.5, dm, depth, depth_thresh=0.1)
    # (the near wall's rim blends with empty background cells in the bilinear lookup and drops out)
    assert vis[: near.shape[0]].mean() > 0.95 and vis[near.shape[0]:].mean() < 0.01
    winners = idx[idx < len(pts)]
    assert (winners < near.shape[0]).all() and len(winners) > 0.85 * idx.size
