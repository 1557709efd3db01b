"""Camera models as a policy of the projection (include/mgs.h MGS_CAMERA_*): camera_model="ortho" / "fisheye" through
every entry point that projects (the operator, the per-camera SH path, the one-call inference path, FrameRenderer, the
batched training path, Trainer), against the fp64 oracle under the same model (oracle/gs_oracle_np.py and
oracle/gs_oracle_torch.py, camera_model=).  "pinhole" (the default) is what every other test file exercises; here it is
checked to be the default bit for bit."""
import math

import numpy as np
import pytest
import torch

from oracle import gs_oracle_np as O
from oracle import gs_oracle_torch as OT
from robosimgs_amd import camera_ring, synthetic_scene

pytestmark = pytest.mark.gpu

DEV = "cuda"


def _K(model, w, h):
    """pinhole 60 degrees; ortho w/6 pixels per world unit (the scene spans ~4 units at the ring's centre); fisheye
    180 degrees across the width (r = f theta)."""
    f = {"pinhole": (w / 2) / math.tan(math.radians(30)), "ortho": w / 6.0, "fisheye": w / math.pi}[model]
    return np.array([[f, 0, w / 2 + 0.25], [0, f * 1.03, h / 2 - 0.4], [0, 0, 1]])


def _scene(n=8000, mu=0.05, deg=0, w=192, h=144, theta=0.3, seed=0, radius=7.0):
    g = synthetic_scene(n, math.log(mu), deg, seed)
    cam = camera_ring(1, w, h, thetas=[theta], radius=radius)[0]
    return g, cam.viewmat()


def _f32(a):
    return np.asarray(a, dtype=np.float32).astype(np.float64)


def _t(a, dtype=torch.float32):
    return torch.from_numpy(np.ascontiguousarray(a)).to(dtype).to(DEV)


def _d(a, grad=False):
    return torch.tensor(np.asarray(a), dtype=torch.float64, requires_grad=grad)


@pytest.mark.parametrize("model", ["ortho", "fisheye"])
@pytest.mark.parametrize("rule", ["classic", "opacity_aware"])
@pytest.mark.parametrize("aa", [False, True])
def test_projection_operator_matches_fp64(model, rule, aa):
    from robosimgs_amd import ops
    n, w, h = 10_000, 256, 192
    g, vm = _scene(n, 0.05, 0, w, h)
    K = _K(model, w, h)
    op = np.asarray(g.opacities, dtype=np.float32)
    ref = O.project(_f32(g.means), _f32(g.quats), _f32(g.scales), _f32(vm), _f32(K), w, h, radius_rule=rule,
                    opacities=op.astype(np.float64) if rule != "classic" else None, antialiased=aa, camera_model=model)
    radii, means2d, depths, conics, comps = ops.fully_fused_projection(
        _t(g.means), None, _t(g.quats), _t(g.scales), _t(vm)[None], _t(K)[None], w, h, calc_compensations=aa,
        opacities=_t(op) if rule != "classic" else None, radius_rule=rule, camera_model=model)
    radii = radii[0].cpu().numpy()
    rx, rr = (radii, ref["radii"]) if rule == "classic" else (radii[:, 0], ref["radii"][:, 0])
    vis, vis_ref = rx > 0, rr > 0
    assert vis_ref.sum() > 2000
    flips = int((vis_ref != vis).sum())
    assert flips <= max(1, n // 5000), f"{flips} visibility flips of {n}"
    both = vis & vis_ref
    assert (np.abs(radii[both] - ref["radii"][both]) > 0).sum() <= max(2, n // 1000)
    np.testing.assert_allclose(means2d[0].cpu().numpy()[both], ref["means2d"][both], rtol=2e-5, atol=2e-3)
    np.testing.assert_allclose(depths[0].cpu().numpy()[both], ref["depths"][both], rtol=1e-5, atol=1e-5)
    np.testing.assert_allclose(conics[0].cpu().numpy()[both], ref["conics"][both], rtol=2e-4, atol=1e-6)
    if aa:
        np.testing.assert_allclose(comps[0].cpu().numpy()[both], ref["compensations"][both], rtol=2e-4, atol=1e-6)
    # the model is not pinhole's: the same Gaussians land elsewhere
    pin = ops.fully_fused_projection(_t(g.means), None, _t(g.quats), _t(g.scales), _t(vm)[None], _t(K)[None], w, h)
    assert not torch.equal(pin[1], means2d)


def _check_path(model, g, vm, K, w, h, deg, mode, aa, what, **kw):
    from robosimgs_amd import rasterization
    t = g.to_torch(DEV, deg)
    rm = "antialiased" if aa else "classic"
    colors, alphas, meta = rasterization(t["means"], t["quats"], t["scales"], t["opacities"], t["colors"], _t(vm)[None],
                                         _t(K)[None], w, h, sh_degree=deg, render_mode=mode, rasterize_mode=rm,
                                         tile_bounds="classic", camera_model=model, **kw)
    ref, ref_alpha, rmeta = O.render(g.means, g.quats, g.scales, g.opacities, g.sh_coeffs[:, :(deg + 1) ** 2],
                                     _f32(vm), _f32(K), w, h, sh_degree=deg, render_mode=mode, rasterize_mode=rm,
                                     margins=True, flip_eps=O.EPS_PATH, camera_model=model, **kw)
    assert abs(int(meta["radii"][0].gt(0).sum()) - rmeta["n_vis"]) <= 1
    assert torch.isfinite(colors).all() and torch.isfinite(alphas).all()
    st = O.check_frame(colors[0].cpu().numpy(), alphas[0].cpu().numpy(), ref, ref_alpha, rmeta["margins"], O.EPS_PATH,
                       rmeta["edge_mask"], expected_depth="E" in mode, what=what, flip_weight=rmeta["flip_weight"],
                       feat_max=rmeta["feat_max"], require_flip_bound=True)
    print(f"\n{what}: {st}; n_vis {rmeta['n_vis']} n_isect {int(meta['n_isects'][0])}")
    return colors, alphas, meta, rmeta


@pytest.mark.parametrize("model", ["ortho", "fisheye"])
@pytest.mark.parametrize("mode,deg,aa", [("RGB", 0, False), ("RGB+ED", 3, False), ("RGB+D", 3, True), ("RGB+ED", 0, True)])
def test_rasterization_matches_fp64_render(model, mode, deg, aa):
    """The whole forward path under the model vs the fp64 render under the model: zero unexplained pixels over 1e-4."""
    w, h = 192, 144
    g, vm = _scene(8000, 0.05, deg, w, h)
    _check_path(model, g, vm, _K(model, w, h), w, h, deg, mode, aa, f"{model} {mode} deg {deg} aa {aa}")


def test_fisheye_180_degrees_inside_a_surrounding_scene():
    """A fisheye of 180 degrees horizontal field of view standing inside the scene: Gaussians all around it, behind the
    lens included.  Those behind the near plane are culled, no pixel is NaN, and the frame is the fp64 one."""
    w, h = 200, 160
    g = synthetic_scene(6000, math.log(0.04), 3, 4)
    c2w = np.eye(4)
    c2w[:3, 3] = (0.2, -0.1, 0.3)                            # inside the scene's cube
    from robosimgs_amd import Camera
    vm = Camera(c2w, 1, 1, 0, 0, w, h).viewmat()
    K = np.array([[w / math.pi, 0, w / 2], [0, w / math.pi, h / 2], [0, 0, 1]])   # 180 degrees across the width
    z = (_f32(g.means) @ _f32(vm)[:3, :3].T + _f32(vm)[:3, 3])[:, 2]
    assert (z < 0.0).sum() > 1000 and (z > 0.2).sum() > 1000
    colors, alphas, meta, rmeta = _check_path("fisheye", g, vm, K, w, h, 3, "RGB+ED", False, "fisheye 180 surround",
                                              near_plane=0.2)
    radii = meta["radii"][0].cpu().numpy()
    assert not (radii[z < 0.2 * (1 - 1e-5)] > 0).any()
    assert (radii[z > 0.2] > 0).sum() > 500
    assert not torch.isnan(colors).any() and not torch.isnan(alphas).any()
    # the frame does reach the rim: something near the left and right edges of the image
    m2d = meta["means2d"][0].cpu().numpy()[radii > 0]
    assert (m2d[:, 0] < 0.1 * w).any() and (m2d[:, 0] > 0.9 * w).any()


@pytest.mark.parametrize("model", ["ortho", "fisheye"])
def test_same_pixels_on_every_path(model):
    """Per-camera path (tight and classic tile bounds), one-call inference path (three cameras), FrameRenderer and the
    batched training path: the same frame bit for bit under the model."""
    from robosimgs_amd import FrameRenderer, rasterization
    w, h, deg, mode = 160, 128, 3, "RGB+ED"
    g, _ = _scene(8000, 0.05, deg, w, h)
    cams = [c.viewmat() for c in camera_ring(3, w, h, thetas=[0.3, 1.4, 2.9])]
    K = _K(model, w, h)
    t = g.to_torch(DEV, deg)
    vms, Ks = _t(np.stack(cams)), _t(np.stack([K] * 3))
    kw = dict(sh_degree=deg, render_mode=mode, camera_model=model)
    per_cam = []
    for c in range(3):
        ct, at, _ = rasterization(t["means"], t["quats"], t["scales"], t["opacities"], t["colors"], vms[c:c + 1],
                                  Ks[c:c + 1], w, h, **kw)
        cc, ac, _ = rasterization(t["means"], t["quats"], t["scales"], t["opacities"], t["colors"], vms[c:c + 1],
                                  Ks[c:c + 1], w, h, tile_bounds="classic", **kw)
        assert torch.equal(ct, cc) and torch.equal(at, ac)
        per_cam.append((ct[0], at[0]))
    c3, a3, m3 = rasterization(t["means"], t["quats"], t["scales"], t["opacities"], t["colors"], vms, Ks, w, h,
                               isect_capacity=400_000, lean_meta=True, **kw)
    assert "lean" not in m3 and m3["n_isects"].shape == (3,)
    for c in range(3):
        assert torch.equal(c3[c], per_cam[c][0]) and torch.equal(a3[c], per_cam[c][1]), c
    fr = FrameRenderer(t, w, h, render_mode=mode, isect_capacity=400_000, frames_in_flight=2, reorder=None,
                       camera_model=model)
    for c in range(3):
        tk = fr.submit(cams[c], K)
        f = fr.fetch(tk)
        assert torch.equal(f["colors"], per_cam[c][0]) and torch.equal(f["alphas"], per_cam[c][1]), c
        fr.release(tk)
    tg = {k: v.detach().clone().requires_grad_(True) if torch.is_tensor(v) and v.is_floating_point() else v
          for k, v in t.items()}
    ctr, atr, _ = rasterization(tg["means"], tg["quats"], tg["scales"], tg["opacities"], tg["colors"], vms, Ks, w, h,
                                isect_capacity=400_000, **kw)
    for c in range(3):
        assert torch.equal(ctr[c].detach(), per_cam[c][0]) and torch.equal(atr[c].detach(), per_cam[c][1]), c
    # and not the pinhole frame
    cp, _, _ = rasterization(t["means"], t["quats"], t["scales"], t["opacities"], t["colors"], vms[:1], _t(_K("pinhole", w, h))[None],
                             w, h, sh_degree=deg, render_mode=mode)
    assert not torch.equal(cp[0], per_cam[0][0])


def _ref_grads(model, g, vm, K, w, h, deg, mode, aa, wr, wa):
    r = {k: _d(v, True) for k, v in (("means", g.means), ("quats", g.quats), ("scales", g.scales),
                                      ("opacities", g.opacities), ("colors", g.sh_coeffs[:, :(deg + 1) ** 2]))}
    vmd = _d(_f32(vm), True)
    img, al, p = OT.render(r["means"], r["quats"], r["scales"], r["opacities"], r["colors"], vmd,
                           _d(_f32(K)), w, h, sh_degree=deg, render_mode=mode,
                           rasterize_mode="antialiased" if aa else "classic", camera_model=model)
    ((img * _d(wr)).sum() + (al[..., 0] * _d(wa)).sum()).backward()
    return {k: v.grad.numpy() for k, v in r.items()}, vmd.grad.numpy(), p


def _gate(name, got, ref):
    from grad_gate import compare
    compare(name, got, ref if ref.ndim > 1 else ref.reshape(-1, 1), row_tol=5e-3, bad_frac=1e-2, cos_min=0.999)


@pytest.mark.parametrize("model", ["ortho", "fisheye"])
@pytest.mark.parametrize("deg,mode,aa,cap", [(2, "RGB+ED", False, None), (1, "RGB", True, None), (3, "RGB+D", False, 300_000)])
def test_backward_matches_fp64_autograd(model, deg, mode, aa, cap):
    """Gradients of means, quats, scales, opacities, colours and the view matrix vs fp64 autograd of the torch
    restatement.  cap given: the batched training path (mgs_render_frames_train / _backward)."""
    from robosimgs_amd import rasterization
    w, h = 112, 80
    g, vm = _scene(6000, 0.07, deg, w, h)
    K = _K(model, w, h)
    t = g.to_torch(DEV, deg)
    names = ["means", "quats", "scales", "opacities", "colors"]
    for k in names:
        t[k].requires_grad_(True)
    vmt = _t(vm)[None].requires_grad_(True)
    colors, alphas, meta = rasterization(t["means"], t["quats"], t["scales"], t["opacities"], t["colors"], vmt,
                                         _t(K)[None], w, h, sh_degree=deg, render_mode=mode,
                                         rasterize_mode="antialiased" if aa else "classic", isect_capacity=cap,
                                         camera_model=model)
    rng = np.random.default_rng(2)
    wr, wa = rng.normal(size=tuple(colors.shape[1:])), rng.normal(size=(h, w))
    ((colors[0] * _t(wr)).sum() + (alphas[0, ..., 0] * _t(wa)).sum()).backward()
    ref, ref_vm, p = _ref_grads(model, g, vm, K, w, h, deg, mode, aa, wr, wa)
    assert int(((meta["radii"][0].cpu().numpy() > 0) != (p["radii"].numpy() > 0)).sum()) <= 1
    for k in names:
        _gate(f"{model} v_{k}", t[k].grad, ref[k])
    _gate(f"{model} v_viewmat", vmt.grad[0, :3], ref_vm[:3])


@pytest.mark.parametrize("model", ["ortho", "fisheye"])
def test_trainer_backward_matches_fp64_autograd(model):
    """The same gradients through Trainer.render / step (camera_model= as a raster keyword, batched training path)."""
    from robosimgs_amd.training import Trainer
    w, h, deg, mode = 112, 80, 2, "RGB+ED"
    g, vm = _scene(6000, 0.07, deg, w, h)
    K = _K(model, w, h)
    t = g.to_torch(DEV, deg)
    params = {k: t[k].detach().clone().requires_grad_(True) for k in Trainer.KEYS}
    tr = Trainer(params, None, w, h, sh_degree=deg, render_mode=mode, isect_capacity=300_000, camera_model=model)
    colors, alphas, meta = tr.render(_t(vm)[None], _t(K)[None])
    rng = np.random.default_rng(3)
    wr, wa = rng.normal(size=tuple(colors.shape[1:])), rng.normal(size=(h, w))
    tr.step((colors[0] * _t(wr)).sum() + (alphas[0, ..., 0] * _t(wa)).sum())
    ref, _, _ = _ref_grads(model, g, vm, K, w, h, deg, mode, False, wr, wa)
    for k in Trainer.KEYS:
        _gate(f"trainer {model} v_{k}", tr.in_original_order(tr.params[k].grad), ref[k])


@pytest.mark.parametrize("cap", [None, 300_000])
def test_pinhole_is_the_default_bit_for_bit(cap):
    from robosimgs_amd import rasterization
    w, h, deg = 128, 96, 3
    g, vm = _scene(5000, 0.06, deg, w, h)
    K = _K("pinhole", w, h)
    outs = []
    for extra in ({}, {"camera_model": "pinhole"}):
        t = g.to_torch(DEV, deg)
        for k in ("means", "quats", "scales", "opacities", "colors"):
            t[k].requires_grad_(True)
        vmt = _t(vm)[None].requires_grad_(True)
        c, a, _ = rasterization(t["means"], t["quats"], t["scales"], t["opacities"], t["colors"], vmt, _t(K)[None], w, h,
                                sh_degree=deg, render_mode="RGB+ED", isect_capacity=cap, **extra)
        (c.square().sum() + a.sum()).backward()
        outs.append([c.detach(), a.detach()] + [t[k].grad for k in ("means", "quats", "scales", "opacities", "colors")]
                    + [vmt.grad])
    for x, y in zip(outs[0][:-1], outs[1][:-1]):
        assert torch.equal(x, y)
    # (the view-matrix gradient is summed with float atomics: its order, and so its last bits, vary from run to run)
    a, b = outs[0][-1], outs[1][-1]
    assert float((a - b).abs().max()) <= 1e-5 * float(a.abs().max())


def test_errors(monkeypatch):
    from robosimgs_amd import FrameRenderer, _lib, ops, rasterization
    w, h = 64, 48
    g, vm = _scene(500, 0.1, 0, w, h)
    t = g.to_torch(DEV, 0)
    args = (t["means"], t["quats"], t["scales"], t["opacities"], t["colors"], _t(vm)[None], _t(_K("fisheye", w, h))[None],
            w, h)
    with pytest.raises(ValueError, match="camera_model"):
        rasterization(*args, sh_degree=0, camera_model="equirect")
    with pytest.raises(ValueError, match="camera_model"):
        ops.fully_fused_projection(t["means"], None, t["quats"], t["scales"], args[5], args[6], w, h, camera_model="x")
    rgba = torch.empty(1, h, w, 4, dtype=torch.uint8, device=DEV)
    dist = torch.empty(1, h, w, 1, dtype=torch.float32, device=DEV)
    with pytest.raises(ValueError, match="pinhole"):
        rasterization(*args, sh_degree=0, render_mode="RGB+ED", isect_capacity=100_000, lean_meta=True,
                      dataset_out=(rgba, dist, _K("fisheye", w, h), False), camera_model="fisheye")
    with pytest.raises(ValueError, match="pinhole"):
        FrameRenderer(t, w, h, render_mode="RGB+ED", isect_capacity=100_000, dataset_output=torch.float32,
                      dataset_K=_K("fisheye", w, h), camera_model="fisheye")
    # the C ABI: both camera bits -> MGS_ERR_INVALID_ARGUMENT (-1); dataset output under fisheye -> MGS_ERR_UNSUPPORTED (-3)
    L = _lib.lib()
    monkeypatch.setitem(ops.CAMERA_FRAME_FLAGS, 3, 16 | 32)        # both MGS_FRAMES_CAMERA_* bits
    monkeypatch.setitem(ops.CAMERA_BIN_FLAGS, 3, 4 | 8)            # both MGS_BIN_CAMERA_* bits
    with pytest.raises(_lib.MgsError, match=r"status -1: .*MGS_FRAMES_CAMERA_ORTHO and MGS_FRAMES_CAMERA_FISHEYE"):
        ops.render_frames_raw(t["means"], t["quats"], t["scales"], t["opacities"], 0, t["colors"], args[5], args[6],
                              w, h, 0.3, 0.01, 1e10, 0.0, False, True, 100_000, camera=3)
    with pytest.raises(_lib.MgsError, match=r"status -1: .*MGS_BIN_CAMERA_ORTHO and MGS_BIN_CAMERA_FISHEYE"):
        ops.project_color_fwd_raw(t["means"], t["quats"], t["scales"], t["opacities"], 0, t["colors"], args[5][0],
                                  args[6][0], w, h, 0.3, 0.01, 1e10, 0.0, False, True, camera=3)
    with pytest.raises(_lib.MgsError, match=r"status -1: .*camera_model 7"):
        ops.projection_fwd_raw(t["means"], t["quats"], t["scales"], args[5][0], args[6][0], w, h, 0.3, 0.01, 1e10, 0.0,
                               False, camera=7)
    with pytest.raises(_lib.MgsError, match=r"status -3: .*pinhole"):
        ops.render_frames_raw(t["means"], t["quats"], t["scales"], t["opacities"], 0, t["colors"], args[5], args[6], w, h,
                              0.3, 0.01, 1e10, 0.0, False, True, 100_000, expected_last=True,
                              dataset=(rgba, dist, _K("fisheye", w, h)), camera=2)
    torch.cuda.synchronize()
