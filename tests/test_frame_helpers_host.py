"""tests/frame_helper_ref.py on closed-form cases, and -- computed from the references alone -- the conditions that keep
the GPU tests of the frame-edge helper kernels from excusing a failure: how much of each randomised input sits where a
test may look away.  Runs without a GPU; the GPU modules import the same builders."""
import numpy as np
import pytest

import frame_helper_ref as F
from oracle import gs_oracle_np as O
from oracle import points_np as P


# ---- the references on closed-form cases ---------------------------------------------------------------
def test_composite_rule_rows_by_hand():
    one = lambda v: np.array([v], np.float32)
    bg, fg = np.array([[0.1, 0.2, 0.3]]), np.array([[0.5, 0.6, 0.7]])
    cases = [  # a, zb, zf, mask -> rgb, depth
        (0.5, 2.0, 1.0, None, fg, 1.0),                                   # nearer: the foreground
        (0.5, 2.0, 2.0, None, fg, 2.0),                                   # equal depths: the foreground
        (0.5, 2.0, 3.0, None, bg + 0.5 * fg, 2.0),                        # behind
        (0.0, 2.0, 3.0, None, fg, 3.0),                                   # no splats: in front wherever it is
        (np.nan, 2.0, 3.0, None, fg, 3.0),                                # NaN alpha is no splats
        (0.5, 2.0, np.nan, None, bg + 0.5 * np.array([[1.0, 1.0, 1.0]]), 2.0),    # NaN depth, no mask: absent
        (0.5, 2.0, np.nan, 1, bg + 0.5 * fg, 2.0),                        # NaN depth under a mask: behind
        (0.5, np.nan, 1.0, 1, bg + 0.5 * fg, np.nan),                     # NaN splat depth: behind, and it shows
        (0.5, 2.0, -1.0, 0.5, fg, -1.0),                                  # a float mask of 0.5 is present
        (0.0, 2.0, 1.0, 0, bg + np.array([[1.0, 1.0, 1.0]]), np.inf),     # nothing at all
    ]
    for a, zb, zf, m, rgb, depth in cases:
        mask = None if m is None else np.array([m])
        r, d, _ = F.composite_rule(bg, one(a), one(zb), fg, one(zf), mask, (1.0, 1.0, 1.0))
        np.testing.assert_allclose(r, rgb, rtol=0, atol=1e-15, err_msg=str((a, zb, zf, m)))
        np.testing.assert_array_equal(d, [depth])
    # a front pixel hides whatever the splats hold
    r, _, front = F.composite_rule(np.full((1, 3), np.nan), one(0.5), one(2.0), fg, one(1.0), None, (0, 0, 0))
    assert front.all() and np.array_equal(r, fg)


@pytest.mark.parametrize("kind", F.MASK_KINDS)
def test_truth_table_holds_every_row_and_value(kind):
    t = F.composite_truth_table(kind)
    rows = F.composite_rows(t["a"], t["zb"], t["zf"], t["mask"])
    assert set(rows.tolist()) == set(range(len(F.COMPOSITE_ROWS)))
    _, _, front = F.composite_rule(t["bg"], t["a"], t["zb"], t["fg"], t["zf"], t["mask"], (0, 0, 0))
    assert (front & ~np.isfinite(t["bg"]).all(1)).sum() >= 10            # non-finite splats behind a front pixel
    assert 100 < len(rows) < 1000
    if kind == "float":                                                   # the values a cast to uint8 loses
        assert {0.5, 256.0} <= set(t["mask"].tolist())


@pytest.mark.parametrize("masked", [False, True])
def test_grid_stride_frame_has_both_occlusion_orders(masked):
    t = F.composite_random_frame(513, 1024, masked)
    rows = F.composite_rows(t["a"], t["zb"], t["zf"], t["mask"])
    share = np.bincount(rows.ravel(), minlength=5) / rows.size
    assert (share > 0.05).all(), share                                    # every row, each on > 5 % of the pixels
    assert (t["zf"] == t["zb"]).mean() > 0.05
    assert rows.size > 2048 * 256                                         # the second trip of the stride loop


def test_u8_rule_by_hand():
    b, near = F.u8_rule(np.array([[0.5, 1.0 / 255, 2.5 / 255], [-1.0, 2.0, np.nan], [np.inf, -np.inf, 0.0]]),
                        np.array([1.0, 1.0, 1.0]), (0.2, 0.4, 0.9))
    assert b.tolist() == [[128, 1, 2], [0, 255, 0], [255, 0, 0]]          # 127.5 -> 128 and 2.5 -> 2: half to even
    assert near.tolist() == [[True, False, True], [False] * 3, [False] * 3]
    b, _ = F.u8_rule(np.array([[0.25, 0.25, 0.25]]), np.array([0.5]), (0.5, 1.0, 0.0))
    assert b.tolist() == [[128, 191, 64]]                                 # 127.5 -> 128, 191.25, 63.75


def test_all_255_exact_ties_exist():
    ties, want = F.u8_tie_colors()
    assert all(t is not None for t in ties)
    for k, t in enumerate(ties):
        assert t.dtype == np.float32 and np.float32(255.0) * t == np.float32(k + 0.5)
    assert want[:4].tolist() == [0, 2, 2, 4] and want[254] == 254
    c, a, exp = F.u8_tie_frame(3)
    assert c.shape == (255, 3) and sorted(c[:, 1].tolist()) == sorted(t.item() for t in ties)


def test_u8_clamp_inputs_pin_the_non_finite_bytes():
    c, a = F.u8_clamp_inputs()
    for bg in (None, F.U8_BACKGROUND):
        ref, near = F.u8_rule(c, a, bg)
        odd = ~np.isfinite(c) | ~np.isfinite(a)[:, None]
        assert set(ref[odd].tolist()) == {0, 255} and not near[odd].any()
        assert near.sum() <= 2
    ref, _ = F.u8_rule(c, a, F.U8_BACKGROUND)
    assert (ref[np.isnan(c)] == 0).all() and (ref[np.isnan(a)] == 0).all()


@pytest.mark.parametrize("n_px,stride", F.U8_CASES)
def test_u8_near_tie_share(n_px, stride):
    """What u8_check may excuse: at most 5e-4 of the bytes (2 * U8_DELTA of a uniform fraction is 4e-4, less the bytes
    the clamp pins)."""
    c, a = F.u8_random_inputs(n_px, stride)
    _, near = F.u8_rule(c, a, F.U8_BACKGROUND)
    assert c.dtype == np.float32 and c.min() < 0 and c.max() > 1
    assert near.mean() <= 5e-4, near.mean()
    # and a plain fp32 restatement differs from the fp64 bytes at near-ties only
    v = c[:, :3] + (np.float32(1) - a)[:, None] * np.array(F.U8_BACKGROUND, np.float32)
    f32 = np.rint(np.float32(255) * np.clip(v, np.float32(0), np.float32(1))).astype(np.uint8)
    differ, unexplained, worst = F.u8_check(f32, c, a, F.U8_BACKGROUND)
    assert unexplained == 0 and worst <= 1, (differ, unexplained, worst)


def test_bilinear_fp64_by_hand():
    img = np.array([[0.0, 1.0, 2.0], [10.0, 11.0, 12.0]])                 # h = 2, w = 3: x = u * 2 / 3, y = v / 2
    uv = np.array([[0, 0], [3, 2], [1.5, 1], [0.75, 0], [-7, -7], [9, 9], [np.nan, 0]], np.float32)
    s, b = F.bilinear_fp64(img, uv)
    np.testing.assert_allclose(s[:6], [0, 12, 6, 0.5, 0, 12], atol=1e-12)
    assert np.isnan(s[6]) and np.isnan(b[6])
    assert b[4] == b[5] == pytest.approx(1.01 * 7 * F.U * 12)             # far outside: the interpolation's share only
    assert 1e-6 < b[2] < 1e-5
    one = np.full((1, 1), 3.0)                                            # a 1 x 1 image is its value everywhere
    assert F.bilinear_fp64(one, uv[:6])[0].tolist() == [3.0] * 6
    # against the oracle's fp32 restatement on a random case: within the bound
    mask, depth, uv, _ = F.mask_inputs(37, 53, 2000, 3)
    s, b = F.bilinear_fp64(depth, uv)
    ok = ~np.isnan(s)
    with np.errstate(invalid="ignore"):
        s32 = P._grid_sample_bilinear(depth, uv[ok])
    assert (np.abs(s32 - s[ok]) <= b[ok]).all()


@pytest.mark.parametrize("h,w,n,uv_stride", F.MASK_CASES)
def test_mask_inputs_near_threshold_share(h, w, n, uv_stride):
    mask, depth, uv, pd = F.mask_inputs(h, w, n, uv_stride)
    for args in ((), (depth, pd, 0.4)):
        keep, near = F.mask_rule(uv, mask, 0.5, *args)
        assert near.mean() <= 1e-3, near.mean()
        assert 0.1 < keep.mean() < 0.9 or (args and keep.mean() > 0.02)
    assert np.isnan(uv[:, :2]).any(1).sum() == 2 and uv.shape[1] == uv_stride


def test_cells_off_ties():
    for scale in (1.5, 2, 5):
        uv = F.cells_off_ties(np.random.default_rng(0), 5000, 30, 20, scale)
        q = uv[:, :2].astype(np.float64) / scale
        assert (np.abs(q - np.rint(q)) < 0.46).all() and uv.dtype == np.float32
        q32 = uv[:, :2] / np.float32(scale)
        assert np.array_equal(np.rint(q32), np.rint(q))


def test_depth_map_oracle_states_the_cast():
    """oracle/points_np.py: a rounded quotient that is NaN, infinite or outside int32 goes to cell 0 on that axis; -0.0
    is not below +0.0."""
    uv, depth = F.depth_map_far_inputs()
    n = len(uv)
    _, idx = P.get_depth_map(uv, depth, 4, 4, scale=1)
    cells = idx.reshape(4, 4)                                             # [u, v]
    assert cells[0, 2] == 0 and cells[2, 0] == 7                          # the first of each group of seven wins
    assert cells[3, 2] == 14                                              # the largest fp32 below 2^31 is still clipped
    assert (idx < n).sum() == 3
    _, idx = P.get_depth_map(uv, depth, 8, 8, scale=2)                    # the QUOTIENT decides: 3e9 / 2 < 2^31
    assert idx.reshape(4, 4)[3, 1] == 3 and idx.reshape(4, 4)[0, 1] == 0
    for d, bg, want in (([0.0, -0.0], 1e10, 0), ([-0.0, 0.0], 1e10, 0), ([-0.0], 0.0, 1)):
        _, idx = P.get_depth_map(np.zeros((len(d), 2), np.float32), np.array(d, np.float32), 2, 2, bg_depth=bg, scale=2)
        assert idx.tolist() == [want]


def test_project_bound_by_hand():
    K = np.array([[400.0, 0, 160], [0, 410.0, 120], [0, 0, 1]])
    ecam, euv = F.project_bound(np.array([[1.0, 2.0, 4.0]]), K, np.eye(4))
    assert ecam[0] == pytest.approx(4 * F.GAMMA * np.array([1, 2, 4]))
    ex = (4 * F.GAMMA * 1 + 0.25 * 4 * F.GAMMA * 4) / 4 + F.GAMMA * 0.25
    assert euv[0, 0] == pytest.approx(400 * ex + 3 * F.GAMMA * (400 * 0.25 + 160))
    assert euv[0, 2] == pytest.approx(3 * F.GAMMA)


@pytest.mark.parametrize("deg", [1, 2, 3])
def test_sh_rotation_matrices_rotate_the_colour_field(deg):
    """Independent of the fit that makes them: the SH colour of the rotated row at direction d is the original row's
    colour at R^T d (the oracle's basis, fp64)."""
    t = F.transform_inputs(200, 16, gids=(0, 1, 2))
    ref = F.transform_ref(t["means"], t["quats"], t["scales"], t["colors"], deg, t["gids"], 3, t["rotations"],
                          t["translations"], t["group_scales"])
    rng = np.random.default_rng(9)
    d = rng.normal(size=(200, 3))
    d /= np.linalg.norm(d, axis=1, keepdims=True)
    kc = (deg + 1) ** 2
    rotated, c = ref["colors"][0], t["colors"].astype(np.float64)
    for g in range(3):
        sel = t["gids"] == g
        new = np.einsum("nk,nkc->nc", O.sh_basis(deg, d[sel]), rotated[sel, :kc])
        old = np.einsum("nk,nkc->nc", O.sh_basis(deg, d[sel] @ t["rotations"][g]), c[sel, :kc])
        np.testing.assert_allclose(new, old, rtol=0, atol=1e-12)
    assert np.array_equal(rotated[:, kc:], c[:, kc:]) and np.array_equal(rotated[:, 0], c[:, 0])


def test_transform_ref_by_hand():
    """A quarter turn about z, scale 2, shift (1, 0, 0) on one Gaussian."""
    R = np.array([[0.0, -1, 0], [1, 0, 0], [0, 0, 1]])
    q = np.array([[2.0, 0, 0, 0]], np.float32)                            # identity, norm 2
    ref = F.transform_ref(np.array([[1.0, 2, 3]], np.float32), q, np.array([[0.1, 0.2, 0.3]], np.float32),
                          np.zeros((1, 4, 3), np.float32), 1, np.array([0]), 1, [R], [np.array([1.0, 0, 0])], [2.0])
    np.testing.assert_allclose(ref["means"][0], [[-3, 2, 6]], atol=1e-15)
    np.testing.assert_allclose(ref["scales"][0], 2 * np.array([[0.1, 0.2, 0.3]], np.float32).astype(np.float64))
    np.testing.assert_allclose(ref["rot"][0][0], R, atol=1e-15)
    assert ref["norm"][0][0] == 2.0 and 0 < ref["norm"][1][0] < 1e-6
    assert ref["means"][1][0, 0] == pytest.approx(5 * F.GAMMA * (4 + 1))
    # ids outside [0, n_groups) do not move
    t = F.transform_inputs(200, 9)
    assert set(t["gids"].tolist()) == set(F.TRANSFORM_GIDS)
    ref = F.transform_ref(t["means"], t["quats"], t["scales"], t["colors"], 2, t["gids"], 3, t["rotations"],
                          t["translations"], t["group_scales"])
    still = ~np.isin(t["gids"], (0, 1, 2))
    assert np.array_equal(ref["means"][0][still], t["means"][still]) and not ref["means"][1][still].any()
    assert (ref["means"][1][~still] > 0).all()
