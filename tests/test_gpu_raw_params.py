"""The raw parameter form on the GPU (include/mgs.h MGS_PARAMS_RAW; rasterization(raw_params=True)): `scales` hold
log-scales and `opacities` logits, the projection kernels activate them in registers and their backward returns the
gradients of the raw tensors.

Raw inputs are the fp32 `log_scales` / `opacity_logits` of synthetic_scene; the oracles get exp / sigmoid of exactly those
fp32 values, evaluated in fp64 (NOT Gaussians.scales / .opacities, which round the activations to fp32 first).
Tolerances and gates are the ones of the activated form's tests, named next to each use."""
import math

import numpy as np
import pytest
import torch

from oracle import gs_oracle_np as O
from oracle import gs_oracle_torch as OT
from robosimgs_amd import camera_ring, synthetic_scene

from grad_gate import compare as _compare      # tests/grad_gate.py: the gradient gate and its rules

pytestmark = pytest.mark.gpu
DEV = "cuda"
NAMES = ("means", "quats", "scales", "opacities", "colors")


def _t(a):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32)).to(DEV)


def _d(a, grad=False):
    return torch.tensor(np.asarray(a, dtype=np.float64), requires_grad=grad)


def _f32(a):
    """What the GPU is given: the matrix rounded to fp32 (the oracle then computes in fp64 from it)."""
    return np.asarray(a, dtype=np.float32).astype(np.float64)


def _scene(n, mu, deg, w, h, theta=0.3, seed=0):
    g = synthetic_scene(n, math.log(mu), deg, seed)
    cam = camera_ring(1, w, h, thetas=[theta])[0]
    return g, cam


def _activated64(g):
    """exp / sigmoid, in fp64, of the fp32 raw values the GPU is handed."""
    ls = np.asarray(g.log_scales, np.float32).astype(np.float64)
    x = np.asarray(g.opacity_logits, np.float32).astype(np.float64)
    return np.exp(ls), 1.0 / (1.0 + np.exp(-x))


def _raw_leaves(g, deg, grad=True):
    t = g.to_torch(DEV, deg, raw=True)
    return {k: t[k].detach().clone().requires_grad_(grad) for k in NAMES}


def _render(p, vm, K, w, h, **kw):
    from robosimgs_amd import rasterization
    return rasterization(p["means"], p["quats"], p["scales"], p["opacities"], p["colors"], vm, K, w, h, **kw)


# ---- 1. the projection stage -----------------------------------------------------------------------------------------
@pytest.mark.parametrize("rule", ["classic", "opacity_aware"])
@pytest.mark.parametrize("aa", [False, True])
@pytest.mark.parametrize("n,mu,w,h,theta", [(10_000, 0.05, 256, 256, 0.3), (3_000, 0.2, 200, 120, 2.1), (500, 0.6, 64, 48, 4.0)])
def test_raw_projection_matches_oracle(n, mu, w, h, theta, aa, rule):
    """project_color_fwd_raw(raw=True) against the fp64 oracle on fp64 activations, with the tolerances of
    tests/test_gpu_forward.py::test_projection_matches_oracle (written next to each assertion), plus opac_out against
    sigmoid x compensation at the compensation's tolerance.  SH colours: test_spherical_harmonics_matches_oracle's."""
    from robosimgs_amd import ops
    g, cam = _scene(n, mu, 0, w, h, theta)
    s64, o64 = _activated64(g)
    per_axis = rule == "opacity_aware"
    ref = O.project(g.means, g.quats, s64, cam.viewmat(), cam.K, w, h, radius_rule=rule, opacities=o64, antialiased=aa)
    t = g.to_torch(DEV, 0, raw=True)
    radii, means2d, depths, conics, opac, feats = ops.project_color_fwd_raw(
        t["means"], t["quats"], t["scales"], t["opacities"], 0, t["colors"], _t(cam.viewmat()), _t(cam.K), w, h, 0.3, 0.01,
        1e10, 0.0, aa, False, per_axis=per_axis, raw=True)
    assert opac is not None and opac.shape == (n,)          # raw form keeps the activated opacity, anti-aliased or not
    radii = ops.radii_meta(radii).cpu().numpy().reshape(n, -1)
    ref_radii = np.asarray(ref["radii"]).reshape(n, -1)
    vis_ref, vis = ref_radii[:, 0] > 0, radii[:, 0] > 0
    flips = int((vis_ref != vis).sum())
    print(f"\nraw projection n={n} aa={aa} {rule}: visibility flips {flips}")
    assert flips <= max(1, n // 5000), f"{flips} visibility flips of {n}"
    both = vis_ref & vis
    dr = np.abs(radii[both] - ref_radii[both]).max(axis=1)
    print(f"  radius mismatches {(dr > 0).sum()} rows (max {dr.max()})")
    assert dr.max() <= 1 and (dr > 0).sum() <= max(1, n // 2000), f"radius mismatches: {(dr > 0).sum()} (max {dr.max()})"
    np.testing.assert_allclose(means2d.cpu().numpy()[both], ref["means2d"][both], rtol=2e-5, atol=2e-3)
    np.testing.assert_allclose(depths.cpu().numpy()[both], ref["depths"][both], rtol=1e-5, atol=1e-5)
    np.testing.assert_allclose(conics.cpu().numpy()[both], ref["conics"][both], rtol=2e-4, atol=1e-6)
    want = o64 * ref["compensations"] if aa else o64
    np.testing.assert_allclose(opac.cpu().numpy()[both], want[both], rtol=2e-4, atol=1e-6)
    if not aa:                                              # (no compensation: every row holds the plain sigmoid)
        np.testing.assert_allclose(opac.cpu().numpy(), o64, rtol=2e-4, atol=1e-6)
    rgb = O.sh_colors(0, g.means, O.campos_from_viewmat(_f32(cam.viewmat())), g.sh_coeffs[:, :1])
    np.testing.assert_allclose(feats.cpu().numpy()[both], rgb[both], rtol=1e-4, atol=2e-5)
    assert np.all(means2d.cpu().numpy()[~vis] == 0) and np.all(conics.cpu().numpy()[~vis] == 0)


# ---- 2. the whole frame ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n,mu,w,h,deg,mode", [(10_000, 0.05, 256, 256, 0, "RGB+ED"), (6_000, 0.07, 112, 80, 2, "RGB")])
def test_raw_frame_passes_the_forward_gate(n, mu, w, h, deg, mode):
    """rasterization(raw_params=True) against the fp64 oracle fed fp64 activations, through the unchanged forward gate:
    zero unexplained pixels, zero could-flip pixels over their bound (O.check_frame, default max_explained)."""
    g, cam = _scene(n, mu, deg, w, h)
    s64, o64 = _activated64(g)
    p = _raw_leaves(g, deg, grad=False)
    vm, K = _t(cam.viewmat())[None], _t(cam.K)[None]
    colors, alphas, meta = _render(p, vm, K, w, h, sh_degree=deg, render_mode=mode, tile_bounds="classic", raw_params=True)
    ref, ref_alpha, rmeta = O.render(g.means, g.quats, s64, o64, g.sh_coeffs, _f32(cam.viewmat()), _f32(cam.K), w, h,
                                     sh_degree=deg, render_mode=mode, margins=True, flip_eps=O.EPS_PATH)
    assert colors.shape == (1,) + ref.shape
    if n == 10_000:                                         # configs[0]: the counts of test_rasterization_end_to_end
        assert int(meta["radii"].gt(0).sum()) == rmeta["n_vis"] == 9849
        assert int(meta["n_isects"][0]) == rmeta["n_isect"] == 37024
    st = O.check_frame(colors[0].cpu().numpy(), alphas[0].cpu().numpy(), ref, ref_alpha, rmeta["margins"], O.EPS_PATH,
                       rmeta["edge_mask"], expected_depth="E" in mode, what=f"raw n={n} {mode}",
                       flip_weight=rmeta["flip_weight"], feat_max=rmeta["feat_max"], require_flip_bound=True)
    print(f"\nraw frame n={n} {mode}: {st}")
    # gsplat reports post-activation opacities [C,N]
    assert meta["opacities"].shape == (1, n)
    np.testing.assert_allclose(meta["opacities"][0].cpu().numpy(), o64, rtol=2e-4, atol=1e-6)
    # default (tight) bounds: the same image bit for bit
    c2, a2, _ = _render(p, vm, K, w, h, sh_degree=deg, render_mode=mode, raw_params=True)
    assert torch.equal(c2, colors) and torch.equal(a2, alphas)


# ---- 3. gradients at the real leaves ---------------------------------------------------------------------------------
@pytest.mark.parametrize("deg,mode,aa,seg", [(0, "RGB", False, 256), (3, "RGB", False, 64), (2, "RGB+ED", False, 64),
                                             (1, "RGB", True, 64), (3, "RGB+D", True, 0), (2, "RGB+ED", False, 0)])
def test_raw_gradients_match_autograd_through_the_activations(deg, mode, aa, seg):
    """The six cases of test_rasterization_backward_end_to_end with raw leaves.  Reference: the fp64 torch oracle on
    leaves log_s, x with exp / sigmoid INSIDE its graph.  Gate: that test's (row_tol 5e-3, bad_frac 1e-2, cos_min 0.999),
    and without anti-aliasing every row within rounding + 1.5 x its flip budget -- the activated parameters' budgets
    times the absolute Jacobians of the activations, s and o (1 - o)."""
    w, h = 112, 80
    g, cam = _scene(6000, 0.07, deg, w, h)
    s64, o64 = _activated64(g)
    p = _raw_leaves(g, deg)
    rm = "antialiased" if aa else "classic"
    colors, alphas, meta = _render(p, _t(cam.viewmat()[None]), _t(cam.K[None]), w, h, sh_degree=deg, render_mode=mode,
                                   rasterize_mode=rm, backward_segment=seg, raw_params=True)
    rng = np.random.default_rng(2)
    wr, wa = rng.normal(size=tuple(colors.shape[1:])), rng.normal(size=(h, w))
    ((colors[0] * _t(wr)).sum() + (alphas[0, ..., 0] * _t(wa)).sum()).backward()
    r = {"means": _d(g.means, True), "quats": _d(g.quats, True),
         "scales": _d(np.asarray(g.log_scales, np.float32), True), "opacities": _d(np.asarray(g.opacity_logits, np.float32), True),
         "colors": _d(g.sh_coeffs[:, :(deg + 1) ** 2], True)}
    img, al, _ = OT.render(r["means"], r["quats"], torch.exp(r["scales"]), torch.sigmoid(r["opacities"]), r["colors"],
                           _d(cam.viewmat()), _d(cam.K), w, h, sh_degree=deg, render_mode=mode, rasterize_mode=rm)
    ((img * _d(wr)).sum() + (al[..., 0] * _d(wa)).sum()).backward()
    budgets = {k: None for k in NAMES}
    if not aa:
        from grad_gate import oracle_budgets, parameter_budgets
        f32 = lambda m: np.asarray(m, dtype=np.float32)
        info = oracle_budgets(g, f32(cam.viewmat()), f32(cam.K), w, h, deg, mode, wr, wa, O.EPS_PATH_GRAD)
        bud = info["budget"]
        budgets.update(parameter_budgets(g, f32(cam.viewmat()), f32(cam.K), w, h, deg, mode != "RGB", bud))
        budgets["scales"] = budgets["scales"] * s64                  # |d s / d log_s| = s
        budgets["opacities"] = bud[:, 3] * o64 * (1.0 - o64)          # |d o / d x| = o (1 - o)
    for k in NAMES:
        ref = r[k].grad.numpy()
        _compare("raw v_" + k, p[k].grad, ref if ref.ndim > 1 else ref.reshape(-1, 1), row_tol=5e-3, bad_frac=1e-2,
                 cos_min=0.999, budget=budgets[k])


# ---- 4. against today's route ----------------------------------------------------------------------------------------
@pytest.mark.parametrize("aa", [False, True])
def test_raw_route_equals_torch_activations_into_the_activated_path(aa):
    """One backward each on the same scene: raw leaves with raw_params=True, and the same leaves through torch.exp /
    torch.sigmoid into the activated path.  The two differ by the rounding of the activations and by the rare threshold
    that rounding flips: grad_gate.compare's fraction rule at test_rasterization_backward_end_to_end's settings."""
    w, h, deg = 112, 80, 2
    g, cam = _scene(6000, 0.07, deg, w, h)
    vm, K = _t(cam.viewmat()[None]), _t(cam.K[None])
    kw = dict(sh_degree=deg, render_mode="RGB+ED", rasterize_mode="antialiased" if aa else "classic", backward_segment=64)
    gen = torch.Generator(DEV).manual_seed(4)
    w_c = torch.randn(1, h, w, 4, device=DEV, generator=gen)
    w_a = torch.randn(1, h, w, 1, device=DEV, generator=gen)
    a, b = _raw_leaves(g, deg), _raw_leaves(g, deg)
    c0, a0, _ = _render(a, vm, K, w, h, raw_params=True, **kw)
    ((c0 * w_c).sum() + (a0 * w_a).sum()).backward()
    act = dict(b, scales=torch.exp(b["scales"]), opacities=torch.sigmoid(b["opacities"]))
    c1, a1, _ = _render(act, vm, K, w, h, **kw)
    ((c1 * w_c).sum() + (a1 * w_a).sum()).backward()
    for k in NAMES:
        _compare("raw vs torch-activated v_" + k, a[k].grad, b[k].grad.cpu().double().numpy().reshape(6000, -1),
                 row_tol=5e-3, bad_frac=1e-2, cos_min=0.999)


# ---- 5. bit identities inside raw form -------------------------------------------------------------------------------
@pytest.mark.parametrize("mode,aa,bg,seg", [("RGB+ED", False, True, 64), ("RGB", True, False, 256), ("RGB+D", False, False, 0)])
def test_raw_batched_training_cameras_equal_the_per_camera_loop(mode, aa, bg, seg):
    """As test_batched_training_cameras_through_one_call_equal_the_per_camera_loop, in raw form: frames, all five
    gradients and the screen-space gradients of mgs_render_frames_train / _backward are the per-camera entry points',
    bit for bit; a second run of the backward gives the same bits again."""
    g = synthetic_scene(9000, math.log(0.09), 2, 5)
    cams = camera_ring(3, 144, 96)
    vm0 = _t(np.stack([c.viewmat() for c in cams]))
    Ks = _t(np.stack([c.K for c in cams]))
    ch = 3 if mode == "RGB" else 4
    gen = torch.Generator(DEV).manual_seed(8)
    w_c = torch.randn(3, 96, 144, ch, device=DEV, generator=gen)
    w_a = torch.randn(3, 96, 144, 1, device=DEV, generator=gen)
    bgs = torch.rand(3, ch, device=DEV, generator=gen) if bg else None

    def run(cap):
        p = _raw_leaves(g, 2)
        vm = vm0.clone().requires_grad_(True)
        c, a, meta = _render(p, vm, Ks, 144, 96, sh_degree=2, render_mode=mode, rasterize_mode="antialiased" if aa else "classic",
                             backgrounds=bgs, absgrad=True, isect_capacity=cap, backward_segment=seg, raw_params=True)
        meta["means2d"].retain_grad()
        ((c * w_c).sum() + (a * w_a).sum()).backward()
        return c.detach(), a.detach(), [p[k].grad for k in NAMES], vm.grad, meta

    c0, a0, g0, v0, m0 = run(None)               # per-camera entry points
    c1, a1, g1, v1, m1 = run(600_000)            # the batch behind two C calls
    c2, a2, g2, v2, m2 = run(600_000)            # and once more: bit-reproducible
    assert torch.equal(c0, c1) and torch.equal(a0, a1) and torch.equal(c1, c2)
    for k, x, y, z in zip(NAMES, g0, g1, g2):
        assert torch.isfinite(x).all() and float(x.abs().sum()) > 0, k
        assert torch.equal(x, y) and torch.equal(y, z), k
    torch.testing.assert_close(v0, v1, rtol=1e-4, atol=1e-5)
    assert torch.equal(m0["means2d"].grad, m1["means2d"].grad) and torch.equal(m0["means2d"].absgrad, m1["means2d"].absgrad)
    for key in ("radii", "means2d", "depths", "conics", "opacities", "tiles_per_gauss", "n_isects", "isect_offsets"):
        assert torch.equal(m0[key], m1[key]), key
    assert m1["opacities"].shape == (3, 9000) and int(m1["isect_status"].max()) == 0


@pytest.mark.parametrize("rule,camera", [("classic", "pinhole"), ("opacity_aware", "pinhole"), ("classic", "fisheye"),
                                         ("opacity_aware", "ortho")])
def test_raw_lean_frames_keep_every_bit(rule, camera):
    """As test_lean_frames_drop_the_unread_arrays_and_keep_every_bit, in raw form: lean_meta=True (mgs_render_frames)
    against the full per-camera call, bit for bit, both rasterize modes, under each radius rule and camera model."""
    g = synthetic_scene(60_000, math.log(0.04), 3, 4)
    cam = camera_ring(3, 400, 304)[1]
    p = _raw_leaves(g, 3, grad=False)
    vm, K = _t(cam.viewmat())[None], _t(cam.K)[None]
    if camera == "ortho":
        K = K.clone()
        K[0, 0, 0] = K[0, 1, 1] = 40.0               # pixels per world unit
    for mode in ("RGB", "RGB+ED"):
        for aa in ("classic", "antialiased"):
            kw = dict(sh_degree=3, render_mode=mode, rasterize_mode=aa, isect_capacity=3_000_000, radius_rule=rule,
                      camera_model=camera)
            with torch.no_grad():
                c0, a0, m0 = _render(p, vm, K, 400, 304, raw_params=True, **kw)
                c1, a1, m1 = _render(p, vm, K, 400, 304, raw_params=True, lean_meta=True, **kw)
            assert torch.equal(c0, c1) and torch.equal(a0, a1), (mode, aa)
            assert int(m1["n_isects"][0]) == int(m0["n_isects"][0]) > 0 and int(m1["isect_status"][0]) == 0
            assert "radii" in m0 and "radii" not in m1 and float(a0.max()) > 0.5


def test_frame_renderer_renders_a_raw_scene_and_refuses_posed_groups():
    """FrameRenderer(to_torch(raw=True), raw_params=True): the frame of rasterization(raw_params=True), bit for bit (the
    caller's order kept, so that depth ties cannot differ); with group_ids it refuses."""
    from robosimgs_amd import FrameRenderer
    g = synthetic_scene(20_000, math.log(0.05), 2, 3)
    cam = camera_ring(1, 240, 160, thetas=[0.8])[0]
    t = g.to_torch(DEV, 2, raw=True)
    with torch.no_grad():
        c, a, _ = _render(t, _t(cam.viewmat())[None], _t(cam.K)[None], 240, 160, sh_degree=2, render_mode="RGB+ED",
                          isect_capacity=600_000, raw_params=True)
    fr = FrameRenderer(t, 240, 160, render_mode="RGB+ED", frames_in_flight=2, isect_capacity=600_000, reorder=None,
                       raw_params=True)
    out = fr.render(cam.viewmat(), cam.K)
    assert torch.equal(out["colors"], c[0]) and float(a.max()) > 0.5
    with pytest.raises(ValueError, match="raw_params"):
        FrameRenderer(t, 240, 160, isect_capacity=600_000, group_ids=torch.zeros(20_000, dtype=torch.int32, device=DEV),
                      n_groups=1, raw_params=True)


# ---- 6. the Trainer in raw form under a HIP graph --------------------------------------------------------------------
def test_raw_trainer_step_captures_in_a_hip_graph_and_descends():
    """render -> l1_loss -> step on raw leaves with torch.optim.Adam, captured once and replayed five times: nothing
    raises, every parameter stays finite, the loss ends lower than it started.  The leaves the optimiser owns are the
    tensors handed in: their .grad comes straight out of the library's backward."""
    from robosimgs_amd import Trainer, l1_loss
    g = synthetic_scene(8000, math.log(0.08), 2, 12)
    cam = camera_ring(1, 160, 112, thetas=[0.5])[0]
    vm, K = _t(cam.viewmat())[None], _t(cam.K)[None]
    target = torch.rand(1, 112, 160, 4, device=DEV, generator=torch.Generator(DEV).manual_seed(2))
    p = _raw_leaves(g, 2)
    assert torch.equal(p["scales"].detach().cpu(), torch.from_numpy(np.asarray(g.log_scales, np.float32)))
    opt = torch.optim.Adam(list(p.values()), lr=1e-3, capturable=True)
    tr = Trainer(p, opt, 160, 112, auto_reorder_every=500, sh_degree=2, render_mode="RGB+ED", isect_capacity=400_000,
                 raw_params=True)
    loss_buf = torch.zeros((), device=DEV)

    def step():
        c, a, meta = tr.render(vm, K)
        loss = l1_loss(c, target)
        loss_buf.copy_(loss.detach())
        tr.step(loss)

    side = torch.cuda.Stream(DEV)
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        for _ in range(3):                       # warm-up: the first render reorders (Morton), allocations settle
            step()
        torch.cuda.synchronize()
        assert tr.reorders == 1
        first = float(loss_buf)
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph, stream=side):
            step()
    torch.cuda.synchronize()
    losses = []
    for _ in range(5):
        graph.replay()
        torch.cuda.synchronize()
        losses.append(float(loss_buf))
    assert tr.reorders == 1
    for k in NAMES:
        assert torch.isfinite(p[k]).all(), k
        assert p[k].grad is None or torch.isfinite(p[k].grad).all()
    assert all(math.isfinite(x) for x in losses) and math.isfinite(first) and losses[-1] < losses[0], (first, losses)
    # the leaves moved, and they are still log-scales / logits: the frame of the final state passes as a raw frame
    assert not torch.equal(p["scales"].detach().cpu(), torch.from_numpy(np.asarray(g.log_scales, np.float32))[tr.last_order.cpu()])
    with torch.no_grad():
        c, a, _ = tr.render(vm, K)
    assert torch.isfinite(c).all() and float(a.max()) > 0.5
