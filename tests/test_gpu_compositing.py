"""Row (f2): depth-tested compositing of the splat background with an opaque foreground layer."""
import math

import numpy as np
import pytest
import torch

import frame_helper_ref as F
from robosimgs_amd import camera_ring, synthetic_scene

pytestmark = pytest.mark.gpu
DEV = "cuda"
BACKDROP = (0.2, 0.3, 0.4)


def _rule(bg, a, zb, fg, zf, mask, backdrop):
    """The rule in include/mgs.h (tests/frame_helper_ref.py states it)."""
    return F.composite_rule(bg, a, zb, fg, zf, mask, backdrop)[:2]


def _dev(x):
    return None if x is None else torch.from_numpy(np.ascontiguousarray(x)).to(DEV)


def _bits(x):
    return np.ascontiguousarray(x, dtype=np.float32).view(np.uint32)


def _composite_against_rule(t, what):
    """composite_over on the arrays of `t` against composite_rule: depth bit for bit, RGB bit for bit where the rule
    selects the foreground and within composite_blend_bound where it blends (non-finite values: the same ones).
    Returns the blend's worst ratio to its bound."""
    from robosimgs_amd import composite_over
    rgb, depth = composite_over(_dev(t["bg"]), _dev(t["a"]), _dev(t["zb"]), _dev(t["fg"]), _dev(t["zf"]), _dev(t["mask"]),
                                backdrop=BACKDROP)
    rgb, depth = rgb.cpu().numpy(), depth.cpu().numpy()
    r_rgb, r_depth, front = F.composite_rule(t["bg"], t["a"], t["zb"], t["fg"], t["zf"], t["mask"], BACKDROP)
    assert np.array_equal(_bits(depth), _bits(r_depth)), f"{what}: depth at {np.flatnonzero(_bits(depth) != _bits(r_depth))[:8]}"
    assert np.array_equal(_bits(rgb[front]), _bits(t["fg"][front])), f"{what}: a front pixel is not the foreground's bits"
    got, ref = rgb[~front].astype(np.float64), r_rgb[~front]
    fin = np.isfinite(ref)
    assert np.array_equal(got[~fin], ref[~fin], equal_nan=True), f"{what}: non-finite blends"
    with np.errstate(invalid="ignore"):
        has = (t["mask"] != 0) if t["mask"] is not None else ((t["zf"] > 0) & (t["zf"] < np.inf))
    src = np.where(has[..., None], t["fg"], np.array(BACKDROP, np.float32))[~front]
    bound = F.composite_blend_bound(t["bg"][~front], t["a"][~front], src)
    ratio = np.abs(got[fin] - ref[fin]) / bound[fin]
    print(f"{what}: {front.sum()} front, {(~front).sum()} blended pixels, worst blend error / bound {ratio.max():.3f}")
    assert ratio.max() <= 1.0, f"{what}: blend {ratio.max()} of its bound"
    return float(ratio.max())


@pytest.mark.parametrize("kind", F.MASK_KINDS)
def test_composite_truth_table(kind):
    """Every alpha in {0, -0.0, smallest subnormal, 0.5, 1, NaN} x splat depth in {0, 1, inf, NaN} x foreground depth in
    {-1, 0, 1, zb, nextafter(zb, -+), inf, NaN} under no mask, uint8 {0, 1, 2, 255}, bool and float {0, 0.5, 256, -0.0}
    masks, with non-finite splat colours behind a third of the pixels: the C reading of the rule in include/mgs.h."""
    _composite_against_rule(F.composite_truth_table(kind), f"truth table, mask {kind}")


@pytest.mark.parametrize("masked", [False, True])
def test_composite_second_trip_of_the_stride_loop(masked):
    """1024 x 513: the grid is capped at 2048 workgroups of 256, so the last row is a second trip."""
    t = F.composite_random_frame(513, 1024, masked)
    _composite_against_rule(t, f"1024x513, masked {masked}")


@pytest.mark.parametrize("use_mask", [False, True])
def test_composite_matches_rule_on_a_real_render(use_mask):
    from robosimgs_amd import composite_over, rasterization
    g = synthetic_scene(8000, math.log(0.08), 1, 2)
    cam = camera_ring(1, 200, 120, thetas=[0.5])[0]
    t = g.to_torch(DEV, 1)
    f = lambda x: torch.from_numpy(np.ascontiguousarray(x, dtype=np.float32)).to(DEV)
    c, a, _ = rasterization(t["means"], t["quats"], t["scales"], t["opacities"], t["colors"],
                            f(cam.viewmat())[None], f(cam.K)[None], 200, 120, sh_degree=1, render_mode="RGB+ED")
    rng = np.random.default_rng(0)
    fg = rng.random((120, 200, 3)).astype(np.float32)
    zf = rng.uniform(3.0, 11.0, size=(120, 200)).astype(np.float32)
    present = rng.random((120, 200)) < 0.6
    mask = present.astype(np.uint8) if use_mask else None
    if not use_mask:
        zf = np.where(present, zf, np.inf).astype(np.float32)
    rgb, depth = composite_over(c[0, ..., :3], a[0], c[0, ..., 3:], f(fg), f(zf),
                                torch.from_numpy(mask).to(DEV) if use_mask else None, backdrop=BACKDROP)
    r_rgb, r_depth = _rule(c[0, ..., :3].cpu().numpy().astype(np.float64), a[0, ..., 0].cpu().numpy().astype(np.float64),
                           c[0, ..., 3].cpu().numpy().astype(np.float64), fg.astype(np.float64),
                           zf.astype(np.float64), mask, BACKDROP)
    np.testing.assert_allclose(rgb.cpu().numpy(), r_rgb, atol=1e-6)
    np.testing.assert_array_equal(depth.cpu().numpy(), r_depth.astype(np.float32))
    # both occlusion orders actually occur in this scene
    av, zb = a[0, ..., 0].cpu().numpy(), c[0, ..., 3].cpu().numpy()
    assert (present & (av > 0) & (zf <= zb)).any() and (present & (av > 0) & (zf > zb)).any()


@pytest.mark.parametrize("mode,bg", [("RGB", None), ("RGB+ED", (0.2, 0.4, 0.9))])
def test_frame_to_u8_is_splatfacto_postprocessing_quantised(mode, bg):
    from robosimgs_amd import frame_to_u8, rasterization
    g = synthetic_scene(8000, math.log(0.08), 1, 2)
    cam = camera_ring(1, 203, 117, thetas=[0.5])[0]
    t = g.to_torch(DEV, 1)
    f = lambda x: torch.from_numpy(np.ascontiguousarray(x, dtype=np.float32)).to(DEV)
    c, a, _ = rasterization(t["means"], t["quats"], t["scales"], t["opacities"], t["colors"],
                            f(cam.viewmat())[None], f(cam.K)[None], 203, 117, sh_degree=1, render_mode=mode)
    u8 = frame_to_u8(c[0], a[0], bg)
    assert u8.dtype == torch.uint8 and u8.shape == (117, 203, 3)
    back = torch.tensor(bg if bg is not None else (0.0, 0.0, 0.0), device=DEV)
    ref = (c[0, ..., :3] + (1 - a[0]) * back).clamp(0, 1)
    diff = (u8.float() - ref * 255).abs()
    assert float(diff.max()) <= 0.5 + 1e-3                     # round to nearest
    assert int(u8.max()) > 100
    # and the exact byte of the fp64 rule wherever it is not within U8_DELTA of a tie
    differ, unexplained, worst = F.u8_check(u8.cpu().numpy().reshape(-1, 3), c[0].cpu().numpy().reshape(117 * 203, -1),
                                            a[0].cpu().numpy().reshape(-1), bg)
    assert unexplained == 0 and worst <= 1, (differ, unexplained, worst)


def _u8(colors, alpha, bg, **kw):
    from robosimgs_amd import frame_to_u8
    return frame_to_u8(_dev(colors), _dev(alpha), bg, **kw).cpu().numpy()


@pytest.mark.parametrize("stride", [3, 4])
def test_frame_to_u8_exact_ties_round_half_to_even(stride):
    """255 fp32 colours with fl(255 c) == k + 0.5 exactly, alpha 1 (the value is c, fused or not): the byte is k for
    even k, k + 1 for odd k, with no excuse.  Stride 3: 63 quads and a tail of 3; stride 4: the generic loop."""
    c, a, want = F.u8_tie_frame(stride)
    for bg in (None, F.U8_BACKGROUND):
        got = _u8(c, a, bg)
        assert np.array_equal(got, want), np.argwhere(got != want)[:8]


@pytest.mark.parametrize("stride", [3, 5])
@pytest.mark.parametrize("bg", [None, F.U8_BACKGROUND])
def test_frame_to_u8_clamp_and_non_finite(stride, bg):
    """Negative, > 1, +-inf and NaN in colour and in alpha: rint(255 fmin(fmax(v, 0), 1)), NaN -> 0 (include/mgs.h)."""
    c3, a = F.u8_clamp_inputs()
    c = np.zeros((len(c3), stride), np.float32)
    c[:, :3] = c3
    ref, near = F.u8_rule(c, a, bg)
    got = _u8(c, a, bg)
    assert np.array_equal(got[~near], ref[~near]), np.argwhere((got != ref) & ~near)[:8]
    assert (np.abs(got.astype(int) - ref) <= 1).all()


@pytest.mark.parametrize("n_px,stride", F.U8_CASES)
def test_frame_to_u8_random_with_background(n_px, stride):
    """Colours in [-0.1, 1.1], alpha in [0, 1], background (0.2, 0.4, 0.9) against the fp64 byte: within 1 everywhere,
    different only within U8_DELTA of a tie (tests/test_frame_helpers_host.py caps those at 5e-4 of these very
    arrays).  1,027 packed pixels are 256 quads and a tail of 3; 4,195,507 packed and 1,049,093 strided pixels reach
    the second trip of the quad loop and of the generic loop (4096 workgroups of 256)."""
    c, a = F.u8_random_inputs(n_px, stride)
    got = _u8(c, a, F.U8_BACKGROUND)
    differ, unexplained, worst = F.u8_check(got, c, a, F.U8_BACKGROUND)
    print(f"{n_px} px, stride {stride}: {differ} bytes differ from fp64, all near-ties: {unexplained == 0}")
    assert unexplained == 0 and worst <= 1, (differ, unexplained, worst)


def test_frame_to_u8_misaligned_pointers_take_the_generic_path():
    """rgb or alpha one element past a 16-byte boundary, or out= one byte past a 4-byte boundary: the host code must
    fall back to the pixel-by-pixel loop, with the same bytes."""
    from robosimgs_amd import frame_to_u8
    n = 1027
    c, a = F.u8_random_inputs(n, 3)
    want = _u8(c, a, F.U8_BACKGROUND)
    assert F.u8_check(want, c, a, F.U8_BACKGROUND)[1] == 0
    cd = torch.zeros(3 * n + 1, device=DEV)
    cd[1:] = _dev(c).reshape(-1)
    ad = torch.zeros(n + 1, device=DEV)
    ad[1:] = _dev(a)
    c_off, a_off = cd[1:].view(n, 3), ad[1:]
    assert c_off.data_ptr() % 16 == 4 and a_off.data_ptr() % 16 == 4 and c_off.is_contiguous()
    for cc, aa in ((c_off, _dev(a)), (_dev(c), a_off), (c_off, a_off)):
        assert np.array_equal(frame_to_u8(cc, aa, F.U8_BACKGROUND).cpu().numpy(), want)
    buf = torch.full((3 * n + 2,), 7, dtype=torch.uint8, device=DEV)
    out = buf[1:-1]
    assert out.data_ptr() % 4 == 1
    res = frame_to_u8(_dev(c), _dev(a), F.U8_BACKGROUND, out=out)
    assert res.data_ptr() == out.data_ptr() and res.shape == (n, 3)
    assert np.array_equal(out.cpu().numpy().reshape(n, 3), want) and int(buf[0]) == 7 and int(buf[-1]) == 7


def test_frame_to_u8_out_argument():
    """The frame lands in the caller's tensor; a tensor the kernel could not safely write 3 bytes per pixel into is
    refused before the launch."""
    from robosimgs_amd import frame_to_u8
    n = 1027
    c, a = F.u8_random_inputs(n, 4)
    cd, ad = _dev(c), _dev(a)
    want = frame_to_u8(cd, ad, F.U8_BACKGROUND)
    out = torch.zeros(n, 3, dtype=torch.uint8, device=DEV)
    res = frame_to_u8(cd, ad, F.U8_BACKGROUND, out=out)
    assert res.data_ptr() == out.data_ptr() and torch.equal(out, want)
    flat = torch.zeros(3 * n, dtype=torch.uint8, device=DEV)               # any shape of 3 n bytes, as bench.py's staging
    assert torch.equal(frame_to_u8(cd, ad, F.U8_BACKGROUND, out=flat), want) and torch.equal(flat.view(n, 3), want)
    for bad in (torch.zeros(n, 3, dtype=torch.int8, device=DEV), torch.zeros(n, 3, dtype=torch.float32, device=DEV),
                torch.zeros(n - 1, 3, dtype=torch.uint8, device=DEV), torch.zeros(n, 4, dtype=torch.uint8, device=DEV),
                torch.zeros(n, 6, dtype=torch.uint8, device=DEV)[:, ::2], torch.zeros(n, 3, dtype=torch.uint8),
                np.zeros((n, 3), np.uint8)):
        with pytest.raises(ValueError):
            frame_to_u8(cd, ad, F.U8_BACKGROUND, out=bad)
