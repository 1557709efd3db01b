"""Fisheye lens distortion on the GPU (include/mgs.h MGS_CAMERA_FISHEYE_KB; distortion=(k1, k2, k3, k4) with
camera_model="fisheye") through every entry point that projects, against the fp64 oracle under the lens
(tests/lens_ref.py substitutes the lens's mean and Jacobian into the unchanged oracle.project / render).

Scenes, sizes and gates are tests/test_gpu_camera_models.py's.  Two lenses: the mild (-0.04, 0.012, -0.006, 0.0015), which
stays monotonic up to pi/2, on that file's ring camera, and the folding (-0.2, 0, 0, 0), theta_max = 1.2909944, on a
180-degree f = w / pi camera standing inside the scene, where over a thousand Gaussians in front of the near plane lie
past theta_max and must be culled."""
import math

import numpy as np
import pytest
import torch

import label_gates as LG
import lens_ref as LR
from oracle import gs_oracle_np as O
from oracle import gs_oracle_torch as OT
from robosimgs_amd import Camera, camera_ring, synthetic_scene
from test_gpu_camera_models import _K, _d, _f32, _gate, _scene, _t

pytestmark = pytest.mark.gpu

DEV = "cuda"
LENSES = {"mild": LR.MILD, "folding": LR.FOLDING}
NAMES = ("means", "quats", "scales", "opacities", "colors")
NEAR = {"mild": 0.01, "folding": 0.05}


def _inside(n, deg, w, h, mu=0.05):
    """The 180-degree camera inside the scene's cube (Gaussians all around it, behind it too)."""
    g = synthetic_scene(n, math.log(mu), deg, 0)
    c2w = np.eye(4)
    c2w[:3, 3] = (0.2, -0.1, 0.3)
    return g, Camera(c2w, 1, 1, 0, 0, w, h).viewmat()


def _lens_scene(lens, n, deg, w, h, mu=0.05):
    """(Gaussians, viewmat, K, near plane) of a lens's scene: both cameras are f = w / pi fisheyes."""
    g, vm = _scene(n, mu, deg, w, h) if lens == "mild" else _inside(n, deg, w, h, mu)
    return g, vm, _K("fisheye", w, h), NEAR[lens]


def _camera_points(g, vm):
    pc = _f32(g.means) @ _f32(vm)[:3, :3].T + _f32(vm)[:3, 3]
    return pc


def _u(pc, near):
    """The reference's own u = theta^2 of every Gaussian in front of the near plane (inf behind it)."""
    front = pc[:, 2] > near
    return np.where(front, LR.u_of(pc[:, 0], pc[:, 1], np.where(front, pc[:, 2], 1.0)), np.inf)


# ---- 1. the projection operator --------------------------------------------------------------------------------------
@pytest.mark.parametrize("lens", list(LENSES))
@pytest.mark.parametrize("rule", ["classic", "opacity_aware"])
@pytest.mark.parametrize("aa", [False, True])
def test_projection_operator_matches_fp64(lens, rule, aa):
    from robosimgs_amd import ops
    k, n, w, h = LENSES[lens], 10_000, 256, 192
    g, vm, K, near = _lens_scene(lens, n, 0, w, h)
    op = np.asarray(g.opacities, dtype=np.float32)
    with LR.lens(k) as u_max:
        ref = O.project(_f32(g.means), _f32(g.quats), _f32(g.scales), _f32(vm), _f32(K), w, h, near_plane=near,
                        radius_rule=rule, opacities=op.astype(np.float64) if rule != "classic" else None, antialiased=aa,
                        camera_model="fisheye")
    rr = ref["radii"] if rule == "classic" else ref["radii"][:, 0]
    vis_ref = rr > 0
    u = _u(_camera_points(g, vm), near)
    past = np.isfinite(u) & (u > u_max)
    band = np.isfinite(u) & (np.abs(u - u_max) <= 1e-5 * u_max)
    # (checked on the CPU before the GPU is asked anything)
    assert vis_ref.sum() > 2000
    assert band.sum() <= n / 1000, "the exemption below covers too much of this scene"
    if lens == "folding":
        assert past.sum() > 1000
    assert not (vis_ref & past).any()
    radii, means2d, depths, conics, comps = ops.fully_fused_projection(
        _t(g.means), None, _t(g.quats), _t(g.scales), _t(vm)[None], _t(K)[None], w, h, near_plane=near,
        calc_compensations=aa, opacities=_t(op) if rule != "classic" else None, radius_rule=rule, camera_model="fisheye",
        distortion=k)
    radii = radii[0].cpu().numpy()
    rx = radii if rule == "classic" else radii[:, 0]
    vis = rx > 0
    assert not (vis & past).any(), "a Gaussian past theta_max has a radius"
    flips = vis_ref != vis
    # fp32 rounding of u is about 1e-6 relative: only within 1e-5 u_max of u_max may it decide the cull differently
    unexplained = int((flips & ~band).sum())
    print(f"\n{lens} {rule} aa={aa}: visible {int(vis_ref.sum())}, past theta_max {int(past.sum())}, in the band "
          f"{int(band.sum())}, flips {int(flips.sum())} ({unexplained} outside the band)")
    assert unexplained <= max(1, n // 5000), f"{unexplained} visibility flips of {n}"
    both = vis & vis_ref
    assert (np.abs(radii[both] - ref["radii"][both]) > 0).sum() <= max(2, n // 1000)
    np.testing.assert_allclose(means2d[0].cpu().numpy()[both], ref["means2d"][both], rtol=2e-5, atol=2e-3)
    np.testing.assert_allclose(depths[0].cpu().numpy()[both], ref["depths"][both], rtol=1e-5, atol=1e-5)
    np.testing.assert_allclose(conics[0].cpu().numpy()[both], ref["conics"][both], rtol=2e-4, atol=1e-6)
    if aa:
        np.testing.assert_allclose(comps[0].cpu().numpy()[both], ref["compensations"][both], rtol=2e-4, atol=1e-6)
    culled = ~vis
    assert np.all(means2d[0].cpu().numpy()[culled] == 0) and np.all(conics[0].cpu().numpy()[culled] == 0)
    assert np.all(depths[0].cpu().numpy()[culled] == 0)
    # the lens is not the ideal one: the same Gaussians land elsewhere
    ideal = ops.fully_fused_projection(_t(g.means), None, _t(g.quats), _t(g.scales), _t(vm)[None], _t(K)[None], w, h,
                                       near_plane=near, camera_model="fisheye")
    assert not torch.equal(ideal[1], means2d)


# ---- 2. the whole forward path -------------------------------------------------------------------------------------------
def _check_path(lens, g, vm, K, w, h, near, deg, mode, aa, what):
    from robosimgs_amd import rasterization
    k = LENSES[lens]
    t = g.to_torch(DEV, deg)
    rm = "antialiased" if aa else "classic"
    colors, alphas, meta = rasterization(t["means"], t["quats"], t["scales"], t["opacities"], t["colors"], _t(vm)[None],
                                         _t(K)[None], w, h, sh_degree=deg, render_mode=mode, rasterize_mode=rm,
                                         tile_bounds="classic", camera_model="fisheye", distortion=k, near_plane=near)
    with LR.lens(k):
        ref, ref_alpha, rmeta = O.render(g.means, g.quats, g.scales, g.opacities, g.sh_coeffs[:, :(deg + 1) ** 2],
                                         _f32(vm), _f32(K), w, h, sh_degree=deg, render_mode=mode, rasterize_mode=rm,
                                         margins=True, flip_eps=O.EPS_PATH, camera_model="fisheye", near_plane=near)
    assert rmeta["n_vis"] > 1500
    assert abs(int(meta["radii"][0].gt(0).sum()) - rmeta["n_vis"]) <= 1
    assert torch.isfinite(colors).all() and torch.isfinite(alphas).all()
    st = O.check_frame(colors[0].cpu().numpy(), alphas[0].cpu().numpy(), ref, ref_alpha, rmeta["margins"], O.EPS_PATH,
                       rmeta["edge_mask"], expected_depth="E" in mode, what=what, flip_weight=rmeta["flip_weight"],
                       feat_max=rmeta["feat_max"], require_flip_bound=True)
    print(f"\n{what}: {st}; n_vis {rmeta['n_vis']} n_isect {int(meta['n_isects'][0])}")
    return colors, alphas, meta, rmeta


@pytest.mark.parametrize("lens", list(LENSES))
@pytest.mark.parametrize("mode,deg,aa", [("RGB", 0, False), ("RGB+ED", 3, False), ("RGB+D", 3, True), ("RGB+ED", 0, True)])
def test_rasterization_matches_fp64_render(lens, mode, deg, aa):
    """The whole forward path under the lens vs the fp64 render under the lens: zero unexplained pixels over 1e-4."""
    w, h = 192, 144
    g, vm, K, near = _lens_scene(lens, 8000, deg, w, h)
    _check_path(lens, g, vm, K, w, h, near, deg, mode, aa, f"{lens} lens {mode} deg {deg} aa {aa}")


# ---- 3. the same pixels on every path --------------------------------------------------------------------------------------
def test_same_pixels_on_every_path():
    """Per-camera path (tight and classic tile bounds), the one-call inference path and the batched training path with
    three cameras whose [C,4] coefficients differ, Trainer, and FrameRenderer(distortion=): the same frames bit for bit."""
    from robosimgs_amd import FrameRenderer, rasterization
    from robosimgs_amd.training import Trainer
    w, h, deg, mode = 160, 128, 3, "RGB+ED"
    g, _ = _scene(8000, 0.05, deg, w, h)
    cams = [c.viewmat() for c in camera_ring(3, w, h, thetas=[0.3, 1.4, 2.9])]
    K = _K("fisheye", w, h)
    lenses = np.array([LR.MILD, LR.FOLDING, (0.03, -0.01, 0.002, 0.0)])
    t = g.to_torch(DEV, deg)
    vms, Ks = _t(np.stack(cams)), _t(np.stack([K] * 3))
    kw = dict(sh_degree=deg, render_mode=mode, camera_model="fisheye")
    args = (t["means"], t["quats"], t["scales"], t["opacities"], t["colors"])

    def one(c, lens):
        ct, at, _ = rasterization(*args, vms[c:c + 1], Ks[c:c + 1], w, h, distortion=lens, **kw)
        cc, ac, _ = rasterization(*args, vms[c:c + 1], Ks[c:c + 1], w, h, distortion=lens, tile_bounds="classic", **kw)
        assert torch.equal(ct, cc) and torch.equal(at, ac)
        return ct[0], at[0]
    per_cam = [one(c, lenses[c]) for c in range(3)]
    assert not torch.equal(per_cam[0][0], one(0, lenses[1])[0])
    c3, a3, m3 = rasterization(*args, vms, Ks, w, h, isect_capacity=400_000, lean_meta=True, distortion=lenses, **kw)
    assert m3["n_isects"].shape == (3,) and int(m3["isect_status"].max()) == 0
    for c in range(3):
        assert torch.equal(c3[c], per_cam[c][0]) and torch.equal(a3[c], per_cam[c][1]), c
    # one lens for all three cameras, given as [4]
    c1, a1, _ = rasterization(*args, vms, Ks, w, h, isect_capacity=400_000, lean_meta=True, distortion=LR.FOLDING, **kw)
    assert torch.equal(c1[1], per_cam[1][0]) and torch.equal(a1[1], per_cam[1][1])
    fr = FrameRenderer(t, w, h, render_mode=mode, isect_capacity=400_000, frames_in_flight=2, reorder=None,
                       camera_model="fisheye", distortion=LR.FOLDING)
    for c in range(3):
        tk = fr.submit(cams[c], K)
        f = fr.fetch(tk)
        want = per_cam[1] if c == 1 else one(c, LR.FOLDING)
        assert torch.equal(f["colors"], want[0]) and torch.equal(f["alphas"], want[1]), c
        fr.release(tk)
    tg = {k: v.detach().clone().requires_grad_(True) if torch.is_tensor(v) and v.is_floating_point() else v
          for k, v in t.items()}
    ctr, atr, _ = rasterization(tg["means"], tg["quats"], tg["scales"], tg["opacities"], tg["colors"], vms, Ks, w, h,
                                isect_capacity=400_000, distortion=lenses, **kw)
    for c in range(3):
        assert torch.equal(ctr[c].detach(), per_cam[c][0]) and torch.equal(atr[c].detach(), per_cam[c][1]), c
    params = {k: t[k].detach().clone().requires_grad_(True) for k in Trainer.KEYS}
    tr = Trainer(params, None, w, h, auto_reorder_every=0, isect_capacity=400_000, distortion=lenses, **kw)
    cT, aT, _ = tr.render(vms, Ks)
    for c in range(3):
        assert torch.equal(cT[c].detach(), per_cam[c][0]) and torch.equal(aT[c].detach(), per_cam[c][1]), c


# ---- 4. backward -----------------------------------------------------------------------------------------------------------
def _plant(g, vm, lens, count=8):
    """Move the first 3 * count Gaussians onto the optical axis, just off it, and to 0.97 .. 0.995 of theta_max (85 degrees
    at most) left and right of it (within 12 degrees of the image's horizontal, where the 180-degree frame reaches the
    rim), at depths 1.5 .. 3 in front of the camera."""
    th_max = min(LR.theta_max(LENSES[lens]), math.radians(85.0) / 0.995)
    R, tvec = np.asarray(vm)[:3, :3], np.asarray(vm)[:3, 3]
    pts = []
    for i in range(count):
        d, phi = 1.5 + 1.5 * i / count, math.pi * (i % 2) + 0.06 * (i - 0.5 * count)
        pts.append((0.0, 0.0, d))
        pts.append((1e-4 * d * math.cos(phi), 1e-4 * d * math.sin(phi), d))
        th = th_max * (0.97 + 0.025 * i / (count - 1))
        pts.append((d * math.sin(th) * math.cos(phi), d * math.sin(th) * math.sin(phi), d * math.cos(th)))
    pc = np.array(pts)
    g.means[:len(pc)] = ((pc - tvec) @ R).astype(g.means.dtype)          # world = R^T (p - t)
    return len(pc)


def _ref_grads(lens, g, vm, K, w, h, near, deg, mode, aa, wr, wa, raw):
    r = {"means": _d(g.means, True), "quats": _d(g.quats, True), "colors": _d(g.sh_coeffs[:, :(deg + 1) ** 2], True)}
    if raw:          # leaves log_s, x with exp / sigmoid inside the graph, from the fp32 values the GPU is handed
        r["scales"] = _d(np.asarray(g.log_scales, np.float32).astype(np.float64), True)
        r["opacities"] = _d(np.asarray(g.opacity_logits, np.float32).astype(np.float64), True)
        scales, opac = torch.exp(r["scales"]), torch.sigmoid(r["opacities"])
    else:
        r["scales"], r["opacities"] = _d(g.scales, True), _d(g.opacities, True)
        scales, opac = r["scales"], r["opacities"]
    vmd = _d(_f32(vm), True)
    with LR.lens(LENSES[lens]):
        img, al, p = OT.render(r["means"], r["quats"], scales, opac, r["colors"], vmd, _d(_f32(K)), w, h, sh_degree=deg,
                               render_mode=mode, rasterize_mode="antialiased" if aa else "classic", camera_model="fisheye",
                               near_plane=near)
    ((img * _d(wr)).sum() + (al[..., 0] * _d(wa)).sum()).backward()
    return {k: v.grad.numpy() for k, v in r.items()}, vmd.grad.numpy(), p


@pytest.mark.parametrize("lens,raw,deg,mode,aa,cap", [("mild", False, 2, "RGB+ED", False, None), ("mild", True, 3, "RGB+D", False, 300_000),
                                                      ("folding", False, 3, "RGB+D", False, 300_000),
                                                      ("folding", True, 1, "RGB", True, None)])
def test_backward_matches_fp64_autograd(lens, raw, deg, mode, aa, cap):
    """Gradients of means, quats, scales, opacities, colours and the view matrix vs fp64 autograd of the torch oracle under
    the lens, activated and raw (gradients of log-scales and logits), with Gaussians planted on the axis and close to
    theta_max.  cap given: the batched training path (mgs_render_frames_train / _backward)."""
    from robosimgs_amd import rasterization
    w, h = 112, 80
    g, vm, K, near = _lens_scene(lens, 6000, deg, w, h, mu=0.07)
    planted = _plant(g, vm, lens)
    t = g.to_torch(DEV, deg, raw=raw)
    p = {k: t[k].detach().clone().requires_grad_(True) for k in NAMES}
    vmt = _t(vm)[None].requires_grad_(True)
    colors, alphas, meta = rasterization(p["means"], p["quats"], p["scales"], p["opacities"], p["colors"], vmt, _t(K)[None],
                                         w, h, sh_degree=deg, render_mode=mode, near_plane=near,
                                         rasterize_mode="antialiased" if aa else "classic", isect_capacity=cap,
                                         camera_model="fisheye", distortion=LENSES[lens], raw_params=raw)
    rng = np.random.default_rng(2)
    wr, wa = rng.normal(size=tuple(colors.shape[1:])), rng.normal(size=(h, w))
    ((colors[0] * _t(wr)).sum() + (alphas[0, ..., 0] * _t(wa)).sum()).backward()
    ref, ref_vm, pr = _ref_grads(lens, g, vm, K, w, h, near, deg, mode, aa, wr, wa, raw)
    vis_ref = pr["radii"].numpy() > 0
    assert vis_ref[:planted].all() and vis_ref.sum() > 1500
    assert np.abs(ref["means"][:planted]).max(axis=1).min() > 0, "every planted Gaussian takes part in the loss"
    assert int(((meta["radii"][0].cpu().numpy() > 0) != vis_ref).sum()) <= 1
    for k in NAMES:
        _gate(f"{lens} lens raw={raw} v_{k}", p[k].grad, ref[k])
    _gate(f"{lens} lens raw={raw} v_viewmat", vmt.grad[0, :3], ref_vm[:3])


@pytest.mark.parametrize("lens", list(LENSES))
def test_projection_operator_backward_matches_fp64_autograd(lens):
    """mgs_projection_bwd under the lens (fully_fused_projection(...).backward(), the operator's own backward kernel):
    gradients of means, quats, scales and the view matrix for random cotangents of means2d, depths and conics vs fp64
    autograd of the torch oracle's projection under the lens, planted Gaussians included."""
    from robosimgs_amd import ops
    w, h = 112, 80
    g, vm, K, near = _lens_scene(lens, 6000, 0, w, h, mu=0.07)
    planted = _plant(g, vm, lens)
    n = len(g)
    leaves = {k: _t(v).requires_grad_(True) for k, v in (("means", g.means), ("quats", g.quats), ("scales", g.scales))}
    vmt = _t(vm)[None].requires_grad_(True)
    radii, m2d, dep, con, _ = ops.fully_fused_projection(leaves["means"], None, leaves["quats"], leaves["scales"], vmt,
                                                         _t(K)[None], w, h, near_plane=near, camera_model="fisheye",
                                                         distortion=LENSES[lens])
    r = {k: _d(_f32(v), True) for k, v in (("means", g.means), ("quats", g.quats), ("scales", g.scales))}
    vmd = _d(_f32(vm), True)
    with LR.lens(LENSES[lens]):
        p = OT.project(r["means"], r["quats"], r["scales"], vmd, _d(_f32(K)), w, h, near_plane=near, camera_model="fisheye")
    vis_gpu, vis_ref = radii[0].cpu().numpy() > 0, p["radii"].numpy() > 0
    assert vis_ref[:planted].all() and vis_ref.sum() > 1500 and int((vis_gpu != vis_ref).sum()) <= 1
    mask = (vis_gpu & vis_ref).astype(np.float64)          # both sides sum over the same Gaussians
    rng = np.random.default_rng(4)
    c2, c1, c3 = rng.normal(size=(n, 2)) * mask[:, None], rng.normal(size=n) * mask, rng.normal(size=(n, 3)) * mask[:, None]
    ((m2d[0] * _t(c2)).sum() + (dep[0] * _t(c1)).sum() + (con[0] * _t(c3)).sum()).backward()
    ((p["means2d"] * _d(c2)).sum() + (p["depths"] * _d(c1)).sum() + (p["conics"] * _d(c3)).sum()).backward()
    for k in leaves:
        _gate(f"{lens} lens operator v_{k}", leaves[k].grad, r[k].grad.numpy())
    _gate(f"{lens} lens operator v_viewmat", vmt.grad[0, :3], vmd.grad.numpy()[:3])


def test_trainer_backward_matches_fp64_autograd():
    """The same gradients through Trainer.render / step (distortion= as a raster keyword, batched training path)."""
    from robosimgs_amd.training import Trainer
    w, h, deg, mode, lens = 112, 80, 2, "RGB+ED", "folding"
    g, vm, K, near = _lens_scene(lens, 6000, deg, w, h, mu=0.07)
    _plant(g, vm, lens)
    t = g.to_torch(DEV, deg)
    params = {k: t[k].detach().clone().requires_grad_(True) for k in Trainer.KEYS}
    tr = Trainer(params, None, w, h, sh_degree=deg, render_mode=mode, isect_capacity=300_000, camera_model="fisheye",
                 distortion=LENSES[lens], near_plane=near)
    colors, alphas, meta = tr.render(_t(vm)[None], _t(K)[None])
    rng = np.random.default_rng(3)
    wr, wa = rng.normal(size=tuple(colors.shape[1:])), rng.normal(size=(h, w))
    tr.step((colors[0] * _t(wr)).sum() + (alphas[0, ..., 0] * _t(wa)).sum())
    ref, _, _ = _ref_grads(lens, g, vm, K, w, h, near, deg, mode, False, wr, wa, False)
    for k in Trainer.KEYS:
        _gate(f"trainer lens v_{k}", tr.in_original_order(tr.params[k].grad), ref[k])


# ---- 5. nothing existing moved ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("cap", [None, 300_000])
def test_no_lens_is_the_ideal_fisheye_bit_for_bit(cap):
    from robosimgs_amd import rasterization
    w, h, deg = 128, 96, 3
    g, _ = _scene(5000, 0.06, deg, w, h)
    cams = [c.viewmat() for c in camera_ring(2, w, h, thetas=[0.3, 2.0])]
    vms, Ks = _t(np.stack(cams)), _t(np.stack([_K("fisheye", w, h)] * 2))
    outs = []
    for extra in ({}, {"distortion": None}, {"distortion": (0.0, 0.0, 0.0, 0.0)}, {"distortion": np.zeros((2, 4))},
                  {"distortion": LR.MILD}):
        t = g.to_torch(DEV, deg)
        for k in NAMES:
            t[k].requires_grad_(True)
        c, a, _ = rasterization(t["means"], t["quats"], t["scales"], t["opacities"], t["colors"], vms, Ks, w, h,
                                sh_degree=deg, render_mode="RGB+ED", isect_capacity=cap, camera_model="fisheye", **extra)
        (c.square().sum() + a.sum()).backward()
        outs.append([c.detach(), a.detach()] + [t[k].grad for k in NAMES])
    for other in outs[1:4]:
        for x, y in zip(outs[0], other):
            assert torch.equal(x, y)
    assert not torch.equal(outs[0][0], outs[4][0]) and not torch.equal(outs[0][2], outs[4][2])
    with torch.no_grad():          # and the inference path
        t = g.to_torch(DEV, deg)
        a0 = rasterization(t["means"], t["quats"], t["scales"], t["opacities"], t["colors"], vms, Ks, w, h, sh_degree=deg,
                           isect_capacity=300_000, lean_meta=True, camera_model="fisheye")
        a1 = rasterization(t["means"], t["quats"], t["scales"], t["opacities"], t["colors"], vms, Ks, w, h, sh_degree=deg,
                           isect_capacity=300_000, lean_meta=True, camera_model="fisheye", distortion=np.zeros(4))
    assert torch.equal(a0[0], a1[0]) and torch.equal(a0[1], a1[1])


# ---- 6. refusals; labels and groups under the lens ---------------------------------------------------------------------------
def test_refusals(monkeypatch):
    from robosimgs_amd import FrameRenderer, _lib, ops, rasterization
    w, h = 64, 48
    g, vm = _scene(500, 0.1, 0, w, h)
    t = g.to_torch(DEV, 0)
    K = _K("fisheye", w, h)
    args = (t["means"], t["quats"], t["scales"], t["opacities"], t["colors"], _t(vm)[None], _t(K)[None], w, h)
    rows = ops.lens_rows(args[6], LR.MILD)
    assert rows.shape == (1, 16) and torch.equal(rows[0, :9], args[6].reshape(9))
    np.testing.assert_allclose(rows[0, 9:].cpu().numpy(), np.float32(LR.lens_row(K, LR.MILD)[9:]), rtol=1e-7)
    rgba = torch.empty(1, h, w, 4, dtype=torch.uint8, device=DEV)
    dist = torch.empty(1, h, w, 1, dtype=torch.float32, device=DEV)
    with pytest.raises(ValueError, match="fisheye"):
        rasterization(*args, sh_degree=0, camera_model="ortho", distortion=LR.MILD)
    with pytest.raises(ValueError, match="fisheye"):
        ops.fully_fused_projection(t["means"], None, t["quats"], t["scales"], args[5], args[6], w, h, distortion=LR.MILD)
    with pytest.raises(ValueError, match="pinhole"):
        rasterization(*args, sh_degree=0, render_mode="RGB+ED", isect_capacity=100_000, lean_meta=True,
                      dataset_out=(rgba, dist, K, False), camera_model="fisheye", distortion=LR.MILD)
    with pytest.raises(ValueError, match="pinhole"):
        FrameRenderer(t, w, h, render_mode="RGB+ED", isect_capacity=100_000, dataset_output=torch.float32, dataset_K=K,
                      camera_model="fisheye", distortion=LR.MILD)
    with pytest.raises(ValueError, match="fisheye"):
        FrameRenderer(t, w, h, isect_capacity=100_000, distortion=LR.MILD)
    # a lens the process has not seen cannot be uploaded under graph capture; one it has seen only concatenates
    side = torch.cuda.Stream(DEV)
    with torch.cuda.stream(side):
        torch.cuda.synchronize()
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph, stream=side):
            with pytest.raises(ValueError, match="graph capture"):
                ops.lens_rows(args[6], (0.0123, -0.0045, 0.0, 0.00067))
            captured = ops.lens_rows(args[6], LR.MILD)
        graph.replay()
    torch.cuda.synchronize()
    assert torch.equal(captured, rows)
    # rows a caller keeps itself (FrameRenderer's camera slots): the same frame as the coefficients
    c0, a0, _ = rasterization(*args, sh_degree=0, camera_model="fisheye", distortion=LR.MILD)
    c1, a1, _ = rasterization(*args, sh_degree=0, camera_model="fisheye", distortion=ops.LensRows(rows))
    assert torch.equal(c0, c1) and torch.equal(a0, a1)
    with pytest.raises(ValueError, match="LensRows"):
        rasterization(*args, sh_degree=0, camera_model="fisheye", distortion=ops.LensRows(rows[:, :9].contiguous()))
    # the C ABI: dataset output under the lens -> MGS_ERR_UNSUPPORTED (-3); two camera bits -> MGS_ERR_INVALID_ARGUMENT (-1)
    raw = (t["means"], t["quats"], t["scales"], t["opacities"], 0, t["colors"])
    with pytest.raises(_lib.MgsError, match=r"status -3: .*pinhole"):
        ops.render_frames_raw(*raw, args[5], rows, w, h, 0.3, 0.01, 1e10, 0.0, False, True, 100_000, expected_last=True,
                              dataset=(rgba, dist, K), camera=ops.CAMERA_FISHEYE_KB)
    for other in (ops.FRAMES_CAMERA_ORTHO, ops.FRAMES_CAMERA_FISHEYE):
        monkeypatch.setitem(ops.CAMERA_FRAME_FLAGS, 5, ops.FRAMES_CAMERA_FISHEYE_KB | other)
        with pytest.raises(_lib.MgsError, match=r"status -1: .*more than one MGS_FRAMES_CAMERA_"):
            ops.render_frames_raw(*raw, args[5], rows, w, h, 0.3, 0.01, 1e10, 0.0, False, True, 100_000, camera=5)
    for other in (ops.BIN_CAMERA_ORTHO, ops.BIN_CAMERA_FISHEYE):
        monkeypatch.setitem(ops.CAMERA_BIN_FLAGS, 5, ops.BIN_CAMERA_FISHEYE_KB | other)
        with pytest.raises(_lib.MgsError, match=r"status -1: .*more than one MGS_BIN_CAMERA_"):
            ops.project_color_fwd_raw(*raw, args[5][0], rows[0], w, h, 0.3, 0.01, 1e10, 0.0, False, True, camera=5)
    monkeypatch.setitem(ops.CAMERA_FRAME_FLAGS, 5, 16 | 32)          # ORTHO | FISHEYE stays the error it was
    with pytest.raises(_lib.MgsError, match=r"status -1: .*MGS_FRAMES_CAMERA_ORTHO and MGS_FRAMES_CAMERA_FISHEYE"):
        ops.render_frames_raw(*raw, args[5], args[6], w, h, 0.3, 0.01, 1e10, 0.0, False, True, 100_000, camera=5)
    with pytest.raises(_lib.MgsError, match=r"status -1: .*camera_model 7"):
        ops.projection_fwd_raw(t["means"], t["quats"], t["scales"], args[5][0], rows[0], w, h, 0.3, 0.01, 1e10, 0.0, False, camera=7)
    torch.cuda.synchronize()


def test_frame_renderer_with_groups_and_labels_under_the_lens():
    """FrameRenderer(distortion=, group_ids=, labels=True): a posed frame under the lens is the eager frame of the posed
    scene bit for bit, colours and labels, and the labels pass the fp64 label gate on that frame's own projection."""
    from robosimgs_amd import FrameRenderer, rasterization, transform_gaussians
    w, h, lens = 112, 80, LR.MILD
    g = synthetic_scene(4000, math.log(0.08), 0, 7)
    t = g.to_torch(DEV, 0)
    z = g.means[:, 2]
    gid = np.where(z < np.quantile(z, 0.3), 0, np.where(z > np.quantile(z, 0.7), 1, -1)).astype(np.int32)
    cam = camera_ring(1, w, h, thetas=[0.4])[0]
    K = _K("fisheye", w, h)
    fr = FrameRenderer(t, w, h, render_mode="RGB+ED", frames_in_flight=2, isect_capacity=200_000, group_ids=_t(gid).to(torch.int32),
                       n_groups=2, labels=True, camera_model="fisheye", distortion=lens)
    c, s = math.cos(0.5), math.sin(0.5)
    Rs, ts = [np.array([[c, -s, 0.0], [s, c, 0.0], [0.0, 0.0, 1.0]]), np.eye(3)], [np.zeros(3), np.array([0.0, 0.0, 0.2])]
    tk = fr.submit(cam.viewmat(), K, rotations=Rs, translations=ts)
    f = fr.fetch(tk)
    got = {k: f[k].clone() for k in ("colors", "alphas", "labels", "label_weights")}
    fr.release(tk)
    posed = transform_gaussians(fr.t, Rs, ts, group_ids=fr.group_ids)
    colors, alphas, meta = rasterization(posed["means"], posed["quats"], posed["scales"], posed["opacities"], posed["colors"],
                                         _t(cam.viewmat())[None], _t(K)[None], w, h, sh_degree=fr.t["sh_degree"],
                                         render_mode="RGB+ED", class_ids=fr.class_ids, n_classes=3, camera_model="fisheye",
                                         distortion=lens)
    assert torch.equal(got["colors"], colors[0]) and torch.equal(got["alphas"], alphas[0])
    assert torch.equal(got["labels"], meta["labels"][0]) and torch.equal(got["label_weights"], meta["label_weights"][0])
    ideal, _, _ = rasterization(posed["means"], posed["quats"], posed["scales"], posed["opacities"], posed["colors"],
                                _t(cam.viewmat())[None], _t(K)[None], w, h, sh_degree=fr.t["sh_degree"], render_mode="RGB+ED",
                                camera_model="fisheye")
    assert not torch.equal(ideal[0], got["colors"])
    n = int(meta["n_isects"][0])
    tl = meta["tile_lists"][0]
    npy = lambda x: x.detach().cpu().numpy()
    ref = LG.LabelReference(npy(meta["means2d"][0]), npy(meta["conics"][0]), npy(meta["opacities"][0]), npy(tl.flatten_ids[:n]),
                            npy(tl.tile_offsets[:-1]), w, h, npy(fr.class_ids))
    LG.check_labels(ref.blend.img[..., :3], ref.flip_weight, npy(got["labels"]), npy(got["label_weights"]),
                    what="FrameRenderer labels under the lens")
    assert {0, 1, 2} <= set(np.unique(npy(got["labels"])).tolist())
