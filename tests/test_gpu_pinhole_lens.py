"""Pinhole lens distortion on the GPU (include/mgs_lens_pinhole.h MGS_CAMERA_PINHOLE_BC; pinhole_distortion=(k1, k2, p1, p2,
k3) with camera_model="pinhole") through every entry point that projects, against the fp64 oracle under the lens
(tests/pinhole_lens_ref.py substitutes the lens's mean, Jacobian and culls into the unchanged oracle.project / render).
Section by section tests/test_gpu_lens.py, with its gates unchanged (O.check_frame, grad_gate.compare through
test_gpu_camera_models._gate, the projection operator's bounds).

Two lenses on a 112 x 80 frame (cx = 57.5, cy = 39): the mild (-0.12, 0.03, 0.002, -0.0015, -0.004) at f = 90, whose folds
lie far outside the clamp box, so the box cull is the live one; and the folding (-0.35, 0, 0.003, -0.002, 0) at f = 50,
whose radial fold u_max = 0.95238 lies 32 pixels from the centre, inside the frame, with the tangential fold just before
it on one side: the outer frame must come out empty.  The scenes (pinhole_lens_ref.scene) hold Gaussians planted just
inside and just outside every cull and no Gaussian within 1e-4 of flipping one (tests/test_pinhole_lens_host.py checks on
the CPU that this removes at most 2 % of a scene)."""
import math

import numpy as np
import pytest
import torch

import label_gates as LG
import lift_gates as LF
import pinhole_lens_ref as PR
from oracle import gs_oracle_np as O
from oracle import gs_oracle_torch as OT
from robosimgs_amd import camera_ring, synthetic_scene
from test_gpu_camera_models import _d, _f32, _gate, _t

pytestmark = pytest.mark.gpu

DEV = "cuda"
LENSES = PR.LENSES
NAMES = ("means", "quats", "scales", "opacities", "colors")
W, H, NEAR = PR.W, PR.H, PR.NEAR
KW = dict(camera_model="pinhole", near_plane=NEAR)


def _culled(lens, g, vm, K, w=W, h=H):
    """The reference's own verdict on every Gaussian's centre: culled by the near plane or by one of the lens's three."""
    pc = PR.camera_points(g.means, vm)
    front = pc[:, 2] > NEAR
    out = np.ones(len(g), bool)
    out[front], margin = PR.cull_margins(pc[front, 0], pc[front, 1], pc[front, 2], K[0, 0], K[1, 1], K[0, 2], K[1, 2],
                                         LENSES[lens], w, h)
    assert margin.min() >= PR.FLIP_MARGIN
    return out


# ---- 1. the projection operator --------------------------------------------------------------------------------------
@pytest.mark.parametrize("lens", list(LENSES))
@pytest.mark.parametrize("rule", ["classic", "opacity_aware"])
@pytest.mark.parametrize("aa", [False, True])
def test_projection_operator_matches_fp64(lens, rule, aa):
    from robosimgs_amd import ops
    k, n = LENSES[lens], 2000
    g, vm, K, info = PR.scene(lens, n, 0)
    n = len(g)
    op = np.asarray(g.opacities, dtype=np.float32)
    with PR.lens(k, W, H):
        ref = O.project(_f32(g.means), _f32(g.quats), _f32(g.scales), _f32(vm), _f32(K), W, H, near_plane=NEAR,
                        radius_rule=rule, opacities=op.astype(np.float64) if rule != "classic" else None, antialiased=aa,
                        camera_model="fisheye")
    rr = ref["radii"] if rule == "classic" else ref["radii"][:, 0]
    vis_ref = rr > 0
    culled = _culled(lens, g, vm, K)
    # (checked on the CPU before the GPU is asked anything)
    assert vis_ref.sum() > 400 and culled.sum() > n // 10
    assert not (vis_ref & culled).any()
    for cull, (inside, outside) in info["where"].items():
        assert vis_ref[inside].all() and culled[outside].all() and not culled[inside].any(), cull
    radii, means2d, depths, conics, comps = ops.fully_fused_projection(
        _t(g.means), None, _t(g.quats), _t(g.scales), _t(vm)[None], _t(K)[None], W, H, calc_compensations=aa,
        opacities=_t(op) if rule != "classic" else None, radius_rule=rule, pinhole_distortion=k, **KW)
    radii = radii[0].cpu().numpy()
    rx = radii if rule == "classic" else radii[:, 0]
    vis = rx > 0
    assert not (vis & culled).any(), "a Gaussian the lens culls has a radius"
    for cull, (inside, outside) in info["where"].items():
        assert vis[inside].all() and not vis[outside].any(), cull
    flips = int((vis_ref != vis).sum())
    print(f"\n{lens} {rule} aa={aa}: visible {int(vis_ref.sum())}, culled by the lens or the near plane {int(culled.sum())}, "
          f"flips {flips}")
    assert flips <= max(1, n // 5000), f"{flips} visibility flips of {n}"
    both = vis & vis_ref
    assert (np.abs(radii[both] - ref["radii"][both]) > 0).sum() <= max(2, n // 1000)
    np.testing.assert_allclose(means2d[0].cpu().numpy()[both], ref["means2d"][both], rtol=2e-5, atol=2e-3)
    np.testing.assert_allclose(depths[0].cpu().numpy()[both], ref["depths"][both], rtol=1e-5, atol=1e-5)
    np.testing.assert_allclose(conics[0].cpu().numpy()[both], ref["conics"][both], rtol=2e-4, atol=1e-6)
    if aa:
        np.testing.assert_allclose(comps[0].cpu().numpy()[both], ref["compensations"][both], rtol=2e-4, atol=1e-6)
    gone = ~vis
    assert np.all(means2d[0].cpu().numpy()[gone] == 0) and np.all(conics[0].cpu().numpy()[gone] == 0)
    assert np.all(depths[0].cpu().numpy()[gone] == 0)
    # the lens is not the plain pinhole: the same Gaussians land elsewhere
    plain = ops.fully_fused_projection(_t(g.means), None, _t(g.quats), _t(g.scales), _t(vm)[None], _t(K)[None], W, H, **KW)
    assert not torch.equal(plain[1], means2d)
    seen = (plain[0][0].cpu().numpy() > 0) & vis
    assert np.abs(plain[1][0].cpu().numpy()[seen] - means2d[0].cpu().numpy()[seen]).max() > 1.0


# ---- 2. the whole forward path -------------------------------------------------------------------------------------------
def _check_path(lens, g, vm, K, deg, mode, aa, what):
    from robosimgs_amd import rasterization
    k = LENSES[lens]
    t = g.to_torch(DEV, deg)
    rm = "antialiased" if aa else "classic"
    colors, alphas, meta = rasterization(t["means"], t["quats"], t["scales"], t["opacities"], t["colors"], _t(vm)[None],
                                         _t(K)[None], W, H, sh_degree=deg, render_mode=mode, rasterize_mode=rm,
                                         tile_bounds="classic", pinhole_distortion=k, **KW)
    with PR.lens(k, W, H):
        ref, ref_alpha, rmeta = O.render(g.means, g.quats, g.scales, g.opacities, g.sh_coeffs[:, :(deg + 1) ** 2],
                                         _f32(vm), _f32(K), W, H, sh_degree=deg, render_mode=mode, rasterize_mode=rm,
                                         margins=True, flip_eps=O.EPS_PATH, camera_model="fisheye", near_plane=NEAR)
    assert rmeta["n_vis"] > 400
    assert abs(int(meta["radii"][0].gt(0).sum()) - rmeta["n_vis"]) <= 1
    assert torch.isfinite(colors).all() and torch.isfinite(alphas).all()
    st = O.check_frame(colors[0].cpu().numpy(), alphas[0].cpu().numpy(), ref, ref_alpha, rmeta["margins"], O.EPS_PATH,
                       rmeta["edge_mask"], expected_depth="E" in mode, what=what, flip_weight=rmeta["flip_weight"],
                       feat_max=rmeta["feat_max"], require_flip_bound=True)
    print(f"\n{what}: {st}; n_vis {rmeta['n_vis']} n_isect {int(meta['n_isects'][0])}")
    return colors, alphas, meta, ref_alpha


def _outer_frame(K, k):
    """(mask, r_px): the pixels further from the principal point than 1.35 x r_px, the pixel radius of the radial fold's
    image.  A splat centred inside the fold is squashed radially towards it, so none reaches that far (the fp64 frame is
    held to the same statement)."""
    um = PR.u_max(k)
    r = math.sqrt(um)
    xd, _, _, _ = PR.distort(np.array([r]), np.array([0.0]), (k[0], k[1], 0.0, 0.0, k[4]))
    ys, xs = np.mgrid[0:H, 0:W]
    return np.hypot(xs + 0.5 - K[0, 2], ys + 0.5 - K[1, 2]) > 1.35 * K[0, 0] * xd[0], K[0, 0] * xd[0]


@pytest.mark.parametrize("lens", list(LENSES))
@pytest.mark.parametrize("mode,deg,aa", [("RGB", 0, False), ("RGB+ED", 3, False), ("RGB+D", 3, True), ("RGB+ED", 0, True)])
def test_rasterization_matches_fp64_render(lens, mode, deg, aa):
    """The whole forward path under the lens vs the fp64 render under the lens: zero unexplained pixels over 1e-4.  Under
    the folding lens nothing is drawn past the fold: the outer frame is empty in both."""
    g, vm, K, _ = PR.scene(lens, 2000, deg, mu=0.05)
    colors, alphas, meta, ref_alpha = _check_path(lens, g, vm, K, deg, mode, aa, f"{lens} pinhole lens {mode} deg {deg} aa {aa}")
    if lens == "folding":
        outer, r_px = _outer_frame(K, LENSES[lens])
        assert 31.0 < r_px < 34.0 and outer.sum() > 0.3 * W * H
        a = alphas[0, ..., 0].cpu().numpy()
        assert a[outer].max() == 0.0 and ref_alpha[..., 0][outer].max() == 0.0 and a[~outer].max() > 0.5
        # ... which the plain pinhole fills
        from robosimgs_amd import rasterization
        t = g.to_torch(DEV, deg)
        _, plain, _ = rasterization(t["means"], t["quats"], t["scales"], t["opacities"], t["colors"], _t(vm)[None], _t(K)[None],
                                    W, H, sh_degree=deg, render_mode=mode, **KW)
        assert plain[0, ..., 0].cpu().numpy()[outer].max() > 0.5


# ---- 3. the same pixels on every path --------------------------------------------------------------------------------------
def test_same_pixels_on_every_path():
    """Per-camera path (tight and classic tile bounds), the one-call inference path and the batched training path with
    three cameras whose [C,5] coefficients differ, Trainer, and FrameRenderer(pinhole_distortion=): the same frames bit for
    bit."""
    from robosimgs_amd import FrameRenderer, rasterization
    from robosimgs_amd.training import Trainer
    deg, mode = 3, "RGB+ED"
    g = synthetic_scene(2000, math.log(0.05), deg, 0)
    cams = [c.viewmat() for c in camera_ring(3, W, H, thetas=[0.3, 1.4, 2.9], radius=3.0)]
    K = PR.intrinsics("folding")
    lenses = np.array([PR.MILD, PR.FOLDING, (0.05, -0.01, -0.001, 0.002, 0.0)])
    t = g.to_torch(DEV, deg)
    vms, Ks = _t(np.stack(cams)), _t(np.stack([K] * 3))
    kw = dict(sh_degree=deg, render_mode=mode, **KW)
    args = (t["means"], t["quats"], t["scales"], t["opacities"], t["colors"])

    def one(c, lens):
        ct, at, _ = rasterization(*args, vms[c:c + 1], Ks[c:c + 1], W, H, pinhole_distortion=lens, **kw)
        cc, ac, _ = rasterization(*args, vms[c:c + 1], Ks[c:c + 1], W, H, pinhole_distortion=lens, tile_bounds="classic", **kw)
        assert torch.equal(ct, cc) and torch.equal(at, ac)
        return ct[0], at[0]
    per_cam = [one(c, lenses[c]) for c in range(3)]
    assert not torch.equal(per_cam[0][0], one(0, lenses[1])[0])
    c3, a3, m3 = rasterization(*args, vms, Ks, W, H, isect_capacity=200_000, lean_meta=True, pinhole_distortion=lenses, **kw)
    assert m3["n_isects"].shape == (3,) and int(m3["isect_status"].max()) == 0
    for c in range(3):
        assert torch.equal(c3[c], per_cam[c][0]) and torch.equal(a3[c], per_cam[c][1]), c
    # one lens for all three cameras, given as [5]; and as [4] when k3 = 0
    c1, a1, _ = rasterization(*args, vms, Ks, W, H, isect_capacity=200_000, lean_meta=True, pinhole_distortion=PR.FOLDING, **kw)
    assert torch.equal(c1[1], per_cam[1][0]) and torch.equal(a1[1], per_cam[1][1])
    c4, a4, _ = rasterization(*args, vms, Ks, W, H, isect_capacity=200_000, lean_meta=True, pinhole_distortion=PR.FOLDING[:4], **kw)
    assert torch.equal(c4, c1) and torch.equal(a4, a1)
    fr = FrameRenderer(t, W, H, render_mode=mode, isect_capacity=200_000, frames_in_flight=2, reorder=None,
                       pinhole_distortion=PR.FOLDING, **KW)
    for c in range(3):
        tk = fr.submit(cams[c], K)
        f = fr.fetch(tk)
        want = per_cam[1] if c == 1 else one(c, PR.FOLDING)
        assert torch.equal(f["colors"], want[0]) and torch.equal(f["alphas"], want[1]), c
        fr.release(tk)
    tg = {k: v.detach().clone().requires_grad_(True) if torch.is_tensor(v) and v.is_floating_point() else v
          for k, v in t.items()}
    ctr, atr, _ = rasterization(tg["means"], tg["quats"], tg["scales"], tg["opacities"], tg["colors"], vms, Ks, W, H,
                                isect_capacity=200_000, pinhole_distortion=lenses, **kw)
    for c in range(3):
        assert torch.equal(ctr[c].detach(), per_cam[c][0]) and torch.equal(atr[c].detach(), per_cam[c][1]), c
    params = {k: t[k].detach().clone().requires_grad_(True) for k in Trainer.KEYS}
    tr = Trainer(params, None, W, H, auto_reorder_every=0, isect_capacity=200_000, pinhole_distortion=lenses, **kw)
    cT, aT, _ = tr.render(vms, Ks)
    for c in range(3):
        assert torch.equal(cT[c].detach(), per_cam[c][0]) and torch.equal(aT[c].detach(), per_cam[c][1]), c


# ---- 4. backward -----------------------------------------------------------------------------------------------------------
def _ref_grads(lens, g, vm, K, deg, mode, aa, wr, wa, raw):
    r = {"means": _d(g.means, True), "quats": _d(g.quats, True), "colors": _d(g.sh_coeffs[:, :(deg + 1) ** 2], True)}
    if raw:          # leaves log_s, x with exp / sigmoid inside the graph, from the fp32 values the GPU is handed
        r["scales"] = _d(np.asarray(g.log_scales, np.float32).astype(np.float64), True)
        r["opacities"] = _d(np.asarray(g.opacity_logits, np.float32).astype(np.float64), True)
        scales, opac = torch.exp(r["scales"]), torch.sigmoid(r["opacities"])
    else:
        r["scales"], r["opacities"] = _d(g.scales, True), _d(g.opacities, True)
        scales, opac = r["scales"], r["opacities"]
    vmd = _d(_f32(vm), True)
    with PR.lens(LENSES[lens], W, H):
        img, al, p = OT.render(r["means"], r["quats"], scales, opac, r["colors"], vmd, _d(_f32(K)), W, H, sh_degree=deg,
                               render_mode=mode, rasterize_mode="antialiased" if aa else "classic", camera_model="fisheye",
                               near_plane=NEAR)
    ((img * _d(wr)).sum() + (al[..., 0] * _d(wa)).sum()).backward()
    return {k: v.grad.numpy() for k, v in r.items()}, vmd.grad.numpy(), p


def _inside_planted(info):
    return np.concatenate([np.arange(16)] + [inside for inside, _ in info["where"].values()])


@pytest.mark.parametrize("lens,raw,deg,mode,aa,cap", [("mild", False, 2, "RGB+ED", False, None), ("mild", True, 3, "RGB+D", False, 200_000),
                                                      ("folding", False, 3, "RGB+D", False, 200_000),
                                                      ("folding", True, 1, "RGB", True, None)])
def test_backward_matches_fp64_autograd(lens, raw, deg, mode, aa, cap):
    """Gradients of means, quats, scales, opacities, colours and the view matrix vs fp64 autograd of the torch oracle under
    the lens, activated and raw (gradients of log-scales and logits), with Gaussians planted on the axis and just inside
    every cull.  cap given: the batched training path (mgs_render_frames_train / _backward)."""
    from robosimgs_amd import rasterization
    g, vm, K, info = PR.scene(lens, 2000, deg)
    t = g.to_torch(DEV, deg, raw=raw)
    p = {k: t[k].detach().clone().requires_grad_(True) for k in NAMES}
    vmt = _t(vm)[None].requires_grad_(True)
    colors, alphas, meta = rasterization(p["means"], p["quats"], p["scales"], p["opacities"], p["colors"], vmt, _t(K)[None],
                                         W, H, sh_degree=deg, render_mode=mode,
                                         rasterize_mode="antialiased" if aa else "classic", isect_capacity=cap,
                                         pinhole_distortion=LENSES[lens], raw_params=raw, **KW)
    rng = np.random.default_rng(2)
    wr, wa = rng.normal(size=tuple(colors.shape[1:])), rng.normal(size=(H, W))
    ((colors[0] * _t(wr)).sum() + (alphas[0, ..., 0] * _t(wa)).sum()).backward()
    ref, ref_vm, pr = _ref_grads(lens, g, vm, K, deg, mode, aa, wr, wa, raw)
    vis_ref = pr["radii"].numpy() > 0
    planted = _inside_planted(info)
    assert vis_ref[planted].all() and vis_ref.sum() > 400
    assert np.abs(ref["means"][planted]).max(axis=1).min() > 0, "every planted Gaussian takes part in the loss"
    for _, outside in info["where"].values():
        assert not vis_ref[outside].any() and not p["means"].grad[_t(outside, torch.int64)].any()
    assert int(((meta["radii"][0].cpu().numpy() > 0) != vis_ref).sum()) <= 1
    for k in NAMES:
        _gate(f"{lens} pinhole lens raw={raw} v_{k}", p[k].grad, ref[k])
    _gate(f"{lens} pinhole lens raw={raw} v_viewmat", vmt.grad[0, :3], ref_vm[:3])


@pytest.mark.parametrize("lens", list(LENSES))
def test_projection_operator_backward_matches_fp64_autograd(lens):
    """mgs_projection_bwd under the lens (fully_fused_projection(...).backward(), the operator's own backward kernel):
    gradients of means, quats, scales and the view matrix for random cotangents of means2d, depths and conics vs fp64
    autograd of the torch oracle's projection under the lens, planted Gaussians included."""
    from robosimgs_amd import ops
    g, vm, K, info = PR.scene(lens, 2000, 0)
    n = len(g)
    leaves = {k: _t(v).requires_grad_(True) for k, v in (("means", g.means), ("quats", g.quats), ("scales", g.scales))}
    vmt = _t(vm)[None].requires_grad_(True)
    radii, m2d, dep, con, _ = ops.fully_fused_projection(leaves["means"], None, leaves["quats"], leaves["scales"], vmt,
                                                         _t(K)[None], W, H, pinhole_distortion=LENSES[lens], **KW)
    r = {k: _d(_f32(v), True) for k, v in (("means", g.means), ("quats", g.quats), ("scales", g.scales))}
    vmd = _d(_f32(vm), True)
    with PR.lens(LENSES[lens], W, H):
        p = OT.project(r["means"], r["quats"], r["scales"], vmd, _d(_f32(K)), W, H, near_plane=NEAR, camera_model="fisheye")
    vis_gpu, vis_ref = radii[0].cpu().numpy() > 0, p["radii"].numpy() > 0
    assert vis_ref[_inside_planted(info)].all() and vis_ref.sum() > 400 and int((vis_gpu != vis_ref).sum()) <= 1
    mask = (vis_gpu & vis_ref).astype(np.float64)          # both sides sum over the same Gaussians
    rng = np.random.default_rng(4)
    c2, c1, c3 = rng.normal(size=(n, 2)) * mask[:, None], rng.normal(size=n) * mask, rng.normal(size=(n, 3)) * mask[:, None]
    ((m2d[0] * _t(c2)).sum() + (dep[0] * _t(c1)).sum() + (con[0] * _t(c3)).sum()).backward()
    ((p["means2d"] * _d(c2)).sum() + (p["depths"] * _d(c1)).sum() + (p["conics"] * _d(c3)).sum()).backward()
    for k in leaves:
        _gate(f"{lens} pinhole lens operator v_{k}", leaves[k].grad, r[k].grad.numpy())
    _gate(f"{lens} pinhole lens operator v_viewmat", vmt.grad[0, :3], vmd.grad.numpy()[:3])


def test_trainer_backward_matches_fp64_autograd():
    """The same gradients through Trainer.render / step (pinhole_distortion= as a raster keyword, batched training path)."""
    from robosimgs_amd.training import Trainer
    deg, mode, lens = 2, "RGB+ED", "folding"
    g, vm, K, _ = PR.scene(lens, 2000, deg)
    t = g.to_torch(DEV, deg)
    params = {k: t[k].detach().clone().requires_grad_(True) for k in Trainer.KEYS}
    tr = Trainer(params, None, W, H, sh_degree=deg, render_mode=mode, isect_capacity=200_000, pinhole_distortion=LENSES[lens], **KW)
    colors, alphas, meta = tr.render(_t(vm)[None], _t(K)[None])
    rng = np.random.default_rng(3)
    wr, wa = rng.normal(size=tuple(colors.shape[1:])), rng.normal(size=(H, W))
    tr.step((colors[0] * _t(wr)).sum() + (alphas[0, ..., 0] * _t(wa)).sum())
    ref, _, _ = _ref_grads(lens, g, vm, K, deg, mode, False, wr, wa, False)
    for k in Trainer.KEYS:
        _gate(f"trainer pinhole lens v_{k}", tr.in_original_order(tr.params[k].grad), ref[k])


# ---- 5. nothing existing moved ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("cap", [None, 200_000])
def test_no_lens_is_the_pinhole_bit_for_bit(cap):
    from robosimgs_amd import rasterization
    w, h, deg = 96, 64, 3
    g = synthetic_scene(1500, math.log(0.06), deg, 0)
    cams = [c.viewmat() for c in camera_ring(2, w, h, thetas=[0.3, 2.0], radius=3.0)]
    vms, Ks = _t(np.stack(cams)), _t(np.stack([PR.intrinsics("folding", w, h)] * 2))
    outs = []
    for extra in ({}, {"pinhole_distortion": None}, {"pinhole_distortion": (0.0,) * 5}, {"pinhole_distortion": (0.0,) * 4},
                  {"pinhole_distortion": np.zeros((2, 5))}, {"pinhole_distortion": PR.MILD}):
        t = g.to_torch(DEV, deg)
        for k in NAMES:
            t[k].requires_grad_(True)
        c, a, _ = rasterization(t["means"], t["quats"], t["scales"], t["opacities"], t["colors"], vms, Ks, w, h,
                                sh_degree=deg, render_mode="RGB+ED", isect_capacity=cap, **KW, **extra)
        (c.square().sum() + a.sum()).backward()
        outs.append([c.detach(), a.detach()] + [t[k].grad for k in NAMES])
    for other in outs[1:5]:
        for x, y in zip(outs[0], other):
            assert torch.equal(x, y)
    assert not torch.equal(outs[0][0], outs[5][0]) and not torch.equal(outs[0][2], outs[5][2])
    with torch.no_grad():          # and the inference path
        t = g.to_torch(DEV, deg)
        a0 = rasterization(t["means"], t["quats"], t["scales"], t["opacities"], t["colors"], vms, Ks, w, h, sh_degree=deg,
                           isect_capacity=200_000, lean_meta=True, **KW)
        a1 = rasterization(t["means"], t["quats"], t["scales"], t["opacities"], t["colors"], vms, Ks, w, h, sh_degree=deg,
                           isect_capacity=200_000, lean_meta=True, pinhole_distortion=np.zeros(5), **KW)
    assert torch.equal(a0[0], a1[0]) and torch.equal(a0[1], a1[1])


# ---- 6. refusals; labels, groups and lifting under the lens ------------------------------------------------------------------
def test_refusals(monkeypatch):
    from robosimgs_amd import FrameRenderer, _lib, lift_labels, ops, rasterization
    w, h = 64, 48
    g = synthetic_scene(500, math.log(0.1), 0, 0)
    vm = camera_ring(1, w, h, thetas=[0.3], radius=3.0)[0].viewmat()
    t = g.to_torch(DEV, 0)
    K = PR.intrinsics("mild", w, h)
    args = (t["means"], t["quats"], t["scales"], t["opacities"], t["colors"], _t(vm)[None], _t(K)[None], w, h)
    rows = ops.lens_rows(args[6], None, PR.MILD)
    assert rows.shape == (1, 16) and torch.equal(rows[0, :9], args[6].reshape(9))
    np.testing.assert_allclose(rows[0, 9:].cpu().numpy(), np.float32(PR.lens_row(K, PR.MILD)[9:]), rtol=1e-7)
    no_fold = ops.lens_rows(args[6], None, (0.1, 0.02, 0.001, 0.0, 0.0))
    assert float(no_fold[0, 14]) == float(np.finfo(np.float32).max) and float(no_fold[0, 15]) == 0.0
    rgba = torch.empty(1, h, w, 4, dtype=torch.uint8, device=DEV)
    dist = torch.empty(1, h, w, 1, dtype=torch.float32, device=DEV)
    for model in ("ortho", "fisheye"):
        with pytest.raises(ValueError, match="pinhole"):
            rasterization(*args, sh_degree=0, camera_model=model, pinhole_distortion=PR.MILD)
        with pytest.raises(ValueError, match="pinhole"):
            ops.fully_fused_projection(t["means"], None, t["quats"], t["scales"], args[5], args[6], w, h, camera_model=model,
                                       pinhole_distortion=PR.MILD)
        with pytest.raises(ValueError, match="pinhole"):
            lift_labels(t["means"], t["quats"], t["scales"], t["opacities"], args[5], args[6], w, h,
                        torch.zeros(1, h, w, dtype=torch.uint8, device=DEV), 2, camera_model=model, pinhole_distortion=PR.MILD)
        with pytest.raises(ValueError, match="pinhole"):
            FrameRenderer(t, w, h, isect_capacity=100_000, camera_model=model, pinhole_distortion=PR.MILD)
    with pytest.raises(ValueError, match="one of them"):
        rasterization(*args, sh_degree=0, distortion=(0.01, 0, 0, 0), pinhole_distortion=PR.MILD)
    with pytest.raises(ValueError, match="fisheye"):          # distortion= keeps its meaning and its error
        rasterization(*args, sh_degree=0, distortion=(0.01, 0, 0, 0))
    with pytest.raises(ValueError, match="dataset"):
        rasterization(*args, sh_degree=0, render_mode="RGB+ED", isect_capacity=100_000, lean_meta=True,
                      dataset_out=(rgba, dist, K, False), pinhole_distortion=PR.MILD)
    with pytest.raises(ValueError, match="dataset"):
        FrameRenderer(t, w, h, render_mode="RGB+ED", isect_capacity=100_000, dataset_output=torch.float32, dataset_K=K,
                      pinhole_distortion=PR.MILD)
    with pytest.raises(ValueError, match="finite"):
        rasterization(*args, sh_degree=0, pinhole_distortion=(0.1, float("nan"), 0, 0, 0))
    with pytest.raises(ValueError, match="device"):
        rasterization(*args, sh_degree=0, pinhole_distortion=torch.zeros(5, device=DEV))
    # a lens the process has not seen cannot be uploaded under graph capture; one it has seen only concatenates
    side = torch.cuda.Stream(DEV)
    with torch.cuda.stream(side):
        torch.cuda.synchronize()
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph, stream=side):
            with pytest.raises(ValueError, match="graph capture"):
                ops.lens_rows(args[6], None, (0.0123, -0.0045, 0.0, 0.00067, 0.0))
            captured = ops.lens_rows(args[6], None, PR.MILD)
        graph.replay()
    torch.cuda.synchronize()
    assert torch.equal(captured, rows)
    # rows a caller keeps itself (FrameRenderer's camera slots): the same frame as the coefficients
    c0, a0, _ = rasterization(*args, sh_degree=0, pinhole_distortion=PR.MILD)
    c1, a1, _ = rasterization(*args, sh_degree=0, pinhole_distortion=ops.LensRows(rows))
    assert torch.equal(c0, c1) and torch.equal(a0, a1)
    with pytest.raises(ValueError, match="LensRows"):
        rasterization(*args, sh_degree=0, pinhole_distortion=ops.LensRows(rows[:, :9].contiguous()))
    # the C ABI: dataset output under the lens -> MGS_ERR_UNSUPPORTED (-3); two camera bits -> MGS_ERR_INVALID_ARGUMENT (-1)
    raw = (t["means"], t["quats"], t["scales"], t["opacities"], 0, t["colors"])
    with pytest.raises(_lib.MgsError, match=r"status -3: .*pinhole lens"):
        ops.render_frames_raw(*raw, args[5], rows, w, h, 0.3, 0.01, 1e10, 0.0, False, True, 100_000, expected_last=True,
                              dataset=(rgba, dist, K), camera=ops.CAMERA_PINHOLE_BC)
    for other in (ops.FRAMES_CAMERA_ORTHO, ops.FRAMES_CAMERA_FISHEYE, ops.FRAMES_CAMERA_FISHEYE_KB):
        monkeypatch.setitem(ops.CAMERA_FRAME_FLAGS, 6, ops.FRAMES_CAMERA_PINHOLE_BC | other)
        with pytest.raises(_lib.MgsError, match=r"status -1: .*more than one MGS_FRAMES_CAMERA_"):
            ops.render_frames_raw(*raw, args[5], rows, w, h, 0.3, 0.01, 1e10, 0.0, False, True, 100_000, camera=6)
    for other in (ops.BIN_CAMERA_ORTHO, ops.BIN_CAMERA_FISHEYE, ops.BIN_CAMERA_FISHEYE_KB):
        monkeypatch.setitem(ops.CAMERA_BIN_FLAGS, 6, ops.BIN_CAMERA_PINHOLE_BC | other)
        with pytest.raises(_lib.MgsError, match=r"status -1: .*more than one MGS_BIN_CAMERA_"):
            ops.project_color_fwd_raw(*raw, args[5][0], rows[0], w, h, 0.3, 0.01, 1e10, 0.0, False, True, camera=6)
    with pytest.raises(_lib.MgsError, match=r"status -1: .*camera_model 7"):
        ops.projection_fwd_raw(t["means"], t["quats"], t["scales"], args[5][0], rows[0], w, h, 0.3, 0.01, 1e10, 0.0, False, camera=7)
    torch.cuda.synchronize()


def test_frame_renderer_with_groups_and_labels_under_the_lens():
    """FrameRenderer(pinhole_distortion=, group_ids=, labels=True): a posed frame under the lens is the eager frame of the
    posed scene bit for bit, colours and labels, and the labels pass the fp64 label gate on that frame's own projection."""
    from robosimgs_amd import FrameRenderer, rasterization, transform_gaussians
    lens = PR.FOLDING
    g = synthetic_scene(2000, math.log(0.08), 0, 7)
    t = g.to_torch(DEV, 0)
    z = g.means[:, 2]
    gid = np.where(z < np.quantile(z, 0.3), 0, np.where(z > np.quantile(z, 0.7), 1, -1)).astype(np.int32)
    cam = camera_ring(1, W, H, thetas=[0.4], radius=3.0)[0]
    K = PR.intrinsics("folding")
    fr = FrameRenderer(t, W, H, render_mode="RGB+ED", frames_in_flight=2, isect_capacity=200_000, group_ids=_t(gid).to(torch.int32),
                       n_groups=2, labels=True, pinhole_distortion=lens, **KW)
    c, s = math.cos(0.5), math.sin(0.5)
    Rs, ts = [np.array([[c, -s, 0.0], [s, c, 0.0], [0.0, 0.0, 1.0]]), np.eye(3)], [np.zeros(3), np.array([0.0, 0.0, 0.2])]
    tk = fr.submit(cam.viewmat(), K, rotations=Rs, translations=ts)
    f = fr.fetch(tk)
    got = {k: f[k].clone() for k in ("colors", "alphas", "labels", "label_weights")}
    fr.release(tk)
    posed = transform_gaussians(fr.t, Rs, ts, group_ids=fr.group_ids)
    colors, alphas, meta = rasterization(posed["means"], posed["quats"], posed["scales"], posed["opacities"], posed["colors"],
                                         _t(cam.viewmat())[None], _t(K)[None], W, H, sh_degree=fr.t["sh_degree"],
                                         render_mode="RGB+ED", class_ids=fr.class_ids, n_classes=3, pinhole_distortion=lens, **KW)
    assert torch.equal(got["colors"], colors[0]) and torch.equal(got["alphas"], alphas[0])
    assert torch.equal(got["labels"], meta["labels"][0]) and torch.equal(got["label_weights"], meta["label_weights"][0])
    plain, _, _ = rasterization(posed["means"], posed["quats"], posed["scales"], posed["opacities"], posed["colors"],
                                _t(cam.viewmat())[None], _t(K)[None], W, H, sh_degree=fr.t["sh_degree"], render_mode="RGB+ED", **KW)
    assert not torch.equal(plain[0], got["colors"])
    n = int(meta["n_isects"][0])
    tl = meta["tile_lists"][0]
    npy = lambda x: x.detach().cpu().numpy()
    ref = LG.LabelReference(npy(meta["means2d"][0]), npy(meta["conics"][0]), npy(meta["opacities"][0]), npy(tl.flatten_ids[:n]),
                            npy(tl.tile_offsets[:-1]), W, H, npy(fr.class_ids))
    LG.check_labels(ref.blend.img[..., :3], ref.flip_weight, npy(got["labels"]), npy(got["label_weights"]),
                    what="FrameRenderer labels under the pinhole lens")
    assert {0, 1, 2} <= set(np.unique(npy(got["labels"])).tolist())


def test_lift_labels_under_the_lens():
    """lift_labels(pinhole_distortion=): the votes are cast on the lens's projection (the operator's own, bit for bit) and
    pass the fp64 vote gate on it; [C,5] lenses differ per camera; the plain pinhole votes differently."""
    from robosimgs_amd import lift_labels, ops
    n_classes = 5
    g, vm, K, _ = PR.scene("folding", 2000, 0)
    vm2 = camera_ring(1, W, H, thetas=[1.9], radius=3.0)[0].viewmat()
    t = g.to_torch(DEV, 0)
    vms, Ks = _t(np.stack([vm, vm2])), _t(np.stack([K, K]))
    lenses = np.array([PR.FOLDING, PR.MILD])
    ys, xs = np.mgrid[0:H, 0:W]
    masks_np = np.stack([(xs // 12 + ys // 16) % n_classes, np.where((xs + ys) % 7 == 0, 255, (xs // 9) % n_classes)]).astype(np.uint8)
    masks = torch.from_numpy(masks_np).to(DEV)
    args = (t["means"], t["quats"], t["scales"], t["opacities"])
    debug = []
    res = lift_labels(*args, vms, Ks, W, H, masks, n_classes, pinhole_distortion=lenses, _debug=debug, **KW)
    assert len(debug) == 2
    npy = lambda x: x.detach().cpu().numpy()
    V = B = 0
    for c, (d, mask) in enumerate(zip(debug, masks_np)):
        _, m2d, _, con, _ = ops.fully_fused_projection(*args[:1], None, *args[1:3], vms[c:c + 1], Ks[c:c + 1], W, H,
                                                       pinhole_distortion=lenses[c], **KW)
        assert torch.equal(d["means2d"], m2d[0]) and torch.equal(d["conics"], con[0])
        n = int(d["lists"].n_isect.item())
        assert int(d["lists"].status.item()) == 0 and n > 0
        ref = LF.VoteReference(npy(d["means2d"]), npy(d["conics"]), npy(d["opacities"]), npy(d["lists"].flatten_ids[:n]),
                               npy(d["lists"].tile_offsets[:-1]), W, H, {"m": (mask, n_classes)})
        V, B = V + ref.V("m"), B + ref.bound("m")
    st = LF.check_votes(V, B, npy(res.votes), npy(res.class_ids), npy(res.confidence), capped=True,
                        what="lift_labels under the pinhole lens")
    assert st["voted"] > 0.3 * len(g)
    plain = lift_labels(*args, vms, Ks, W, H, masks, n_classes, **KW)
    assert not torch.equal(plain.votes, res.votes)
