"""ssim / l1_ssim_loss on the GPU (loss.hip ssim_kernel): loss against the fp64 oracle (tests/ssim_ref.py), gradient
against fp64 autograd, the fused form against its parts, reproducibility, the cotangent handling of the stored gradient,
and a Trainer step end to end, eager and captured in a HIP graph."""
import math

import numpy as np
import pytest
import torch

import ssim_ref as S
from robosimgs_amd import camera_ring, synthetic_scene

DEV = "cuda"
pytestmark = pytest.mark.gpu

SHAPES = [(11, 11, 3), (13, 17, 3), (37, 29, 3), (1080, 1920, 3), (3, 64, 96, 3), (40, 50, 1), (40, 50, 4)]


def _pair(shape, kind, seed=0):
    g = torch.Generator(DEV).manual_seed(seed)
    x = torch.rand(shape, device=DEV, generator=g)
    n = torch.rand(shape, device=DEV, generator=g)
    if kind == "near-constant":          # sigma^2 ~ 1e-5 << C2: the variances are differences of nearly equal moments
        return 0.5 + 0.01 * x, 0.5 + 0.01 * n
    return x, 0.7 * x + 0.3 * n


def _ref(x, y, lam, padding):
    """fp64 loss (ssim when lam is None) and its gradient in x."""
    xd = x.detach().double().requires_grad_(True)
    yd = y.detach().double()
    v = S.ssim_torch(xd, yd, padding) if lam is None else S.l1_ssim_torch(xd, yd, lam, padding)
    v.backward()
    return float(v), xd.grad


def _check_grad(g, g_ref, what):
    assert torch.isfinite(g).all(), what
    err = float((g.double() - g_ref).abs().max())
    scale = float(g_ref.abs().max())
    assert err <= 1e-5 * scale, (what, err, scale)


# near-constant images on the small shapes
CASES = [(s, k) for s in SHAPES for k in ("random", "near-constant") if k == "random" or s[0] != 1080]


@pytest.mark.parametrize("padding", ["valid", "same"])
@pytest.mark.parametrize("shape,kind", CASES, ids=lambda v: "x".join(map(str, v)) if isinstance(v, tuple) else v)
def test_loss_and_gradient_match_the_fp64_oracle(shape, padding, kind):
    from robosimgs_amd import l1_ssim_loss, ssim
    x, y = _pair(shape, kind)
    if shape[0] <= 64:           # the NumPy direct windowed sum as well (the torch oracle is its fp64 restatement)
        assert S.ssim_np(x.cpu().numpy(), y.cpu().numpy(), padding) == pytest.approx(_ref(x, y, None, padding)[0], rel=1e-12)
    for lam in (None, 0.2):
        xr = x.clone().requires_grad_(True)
        v = ssim(xr, y, padding) if lam is None else l1_ssim_loss(xr, y, lam, padding)
        v.backward()
        torch.cuda.synchronize()
        v_ref, g_ref = _ref(x, y, lam, padding)
        assert abs(float(v) - v_ref) <= 1e-5 * abs(v_ref), (lam, float(v), v_ref)
        _check_grad(xr.grad, g_ref, f"lambda={lam}")


@pytest.mark.parametrize("lam", [0.0, 0.2, 1.0])
@pytest.mark.parametrize("padding", ["valid", "same"])
def test_fused_loss_is_l1_plus_d_ssim(lam, padding):
    from robosimgs_amd import l1_loss, l1_ssim_loss, ssim
    x, y = _pair((2, 45, 70, 3), "random", 3)
    xa, xb = x.clone().requires_grad_(True), x.clone().requires_grad_(True)
    fused = l1_ssim_loss(xa, y, lam, padding)
    fused.backward()
    parts = (1 - lam) * l1_loss(xb, y) + lam * (1 - ssim(xb, y, padding))
    parts.backward()
    assert abs(float(fused) - float(parts)) <= 2e-6 * max(abs(float(parts)), 1e-3)
    assert float((xa.grad - xb.grad).abs().max()) <= 1e-5 * float(xb.grad.abs().max())


def test_bits_reproduce_across_calls_and_forms():
    from robosimgs_amd import l1_ssim_loss
    x, y = _pair((1080, 1920, 3), "random", 4)
    out = []
    for _ in range(2):
        xr = x.clone().requires_grad_(True)
        v = l1_ssim_loss(xr, y)
        v.backward()
        out.append((v.detach(), xr.grad))
    assert torch.equal(out[0][0], out[1][0]) and torch.equal(out[0][1], out[1][1])
    assert torch.equal(l1_ssim_loss(x, y), out[0][0])              # the forward-only kernel: the same sums
    with torch.no_grad():
        assert torch.equal(l1_ssim_loss(x.clone().requires_grad_(True), y), out[0][0])


def test_cotangents_and_a_second_backward():
    from robosimgs_amd import l1_ssim_loss, unit_gradient
    x, y = _pair((2, 40, 52, 3), "random", 5)
    grads = []
    for cot in ("unit", "ones", 2.5):
        xr = x.clone().requires_grad_(True)
        v = l1_ssim_loss(xr, y, 0.2, "same")
        gr = unit_gradient(v) if cot == "unit" else (torch.ones_like(v) if cot == "ones" else torch.full_like(v, cot))
        v.backward(gradient=gr)
        grads.append(xr.grad)
    assert torch.equal(grads[0], grads[1])                          # unit_gradient: the stored gradient as it is
    assert torch.equal(grads[2], grads[0] * 2.5)                    # any other cotangent scales it once
    xr = x.clone().requires_grad_(True)
    v = l1_ssim_loss(xr, y, 0.2, "same")
    (g1,) = torch.autograd.grad(v, xr, retain_graph=True)
    (g2,) = torch.autograd.grad(v, xr, grad_outputs=torch.full_like(v, 2.5), retain_graph=True)   # mgs_l1_loss_bwd
    (g3,) = torch.autograd.grad(v, xr)
    assert torch.equal(g1, grads[0]) and torch.equal(g2, grads[2]) and torch.equal(g3, grads[0])


def test_rgb_of_an_rgb_ed_frame():
    from robosimgs_amd import l1_ssim_loss
    c4 = torch.rand(1, 40, 50, 4, device=DEV, generator=torch.Generator(DEV).manual_seed(6)).requires_grad_(True)
    target = torch.rand(1, 40, 50, 3, device=DEV, generator=torch.Generator(DEV).manual_seed(7))
    v = l1_ssim_loss(c4[..., :3], target)
    v.backward()
    c3 = c4.detach()[..., :3].contiguous().requires_grad_(True)
    v3 = l1_ssim_loss(c3, target)
    v3.backward()
    assert torch.equal(v.detach(), v3.detach())
    assert torch.equal(c4.grad[..., :3], c3.grad) and not c4.grad[..., 3].any()


def test_invalid_inputs_raise():
    from robosimgs_amd import l1_ssim_loss, ssim
    from robosimgs_amd._lib import MgsError
    a = torch.rand(20, 20, 3, device=DEV)
    with pytest.raises(ValueError, match="shape mismatch"):
        l1_ssim_loss(a, torch.rand(20, 21, 3, device=DEV))
    with pytest.raises(ValueError, match=">= 11"):
        ssim(a[:10], a[:10])
    assert torch.isfinite(ssim(a[:10], a[:10], padding="same"))
    with pytest.raises(MgsError, match="GPU only"):
        l1_ssim_loss(a, a.cpu())


def _conv2d_loss(render, target, lam=0.2):
    """The same loss in fp32 eager torch: pytorch_msssim's separable grouped conv2d ("valid")."""
    x, y = render.permute(0, 3, 1, 2), target.permute(0, 3, 1, 2)
    c = x.shape[1]
    g = torch.from_numpy(S.window()).float().to(render.device)
    wh, ww = g.view(1, 1, -1, 1).repeat(c, 1, 1, 1), g.view(1, 1, 1, -1).repeat(c, 1, 1, 1)
    f = lambda t: torch.nn.functional.conv2d(torch.nn.functional.conv2d(t, wh, groups=c), ww, groups=c)
    mx, my = f(x), f(y)
    vxx, vyy, vxy = f(x * x) - mx * mx, f(y * y) - my * my, f(x * y) - mx * my
    s = (2 * mx * my + S.C1) * (2 * vxy + S.C2) / ((mx * mx + my * my + S.C1) * (vxx + vyy + S.C2))
    return (1 - lam) * (render - target).abs().mean() + lam * (1 - s.mean())


def test_trainer_step_end_to_end_eager_and_captured():
    from robosimgs_amd import Trainer, l1_ssim_loss
    W, H = 160, 112
    g = synthetic_scene(6000, math.log(0.08), 2, 12)
    cam = camera_ring(1, W, H, thetas=[0.5])[0]
    vm = torch.from_numpy(cam.viewmat().astype(np.float32)).to(DEV)[None]
    K = torch.from_numpy(cam.K.astype(np.float32)).to(DEV)[None]
    names = ("means", "quats", "scales", "opacities", "colors")
    t = g.to_torch(DEV, 2)
    params = {k: t[k].detach().clone().requires_grad_(True) for k in names}
    target = torch.rand(1, H, W, 3, device=DEV, generator=torch.Generator(DEV).manual_seed(8))
    tr = Trainer(params, None, W, H, auto_reorder_every=0, sh_degree=2, render_mode="RGB+ED", isect_capacity=400_000)

    def step(loss_fn):
        for p in params.values():
            p.grad = None
        colors, alphas, meta = tr.render(vm, K)
        loss = loss_fn(colors[..., :3], target)
        tr.step(loss)
        return loss

    ref = step(_conv2d_loss).detach()
    g_ref = {k: params[k].grad.clone() for k in names}
    loss = step(l1_ssim_loss).detach()
    g_fused = {k: params[k].grad.clone() for k in names}
    assert abs(float(loss) - float(ref)) <= 1e-5 * float(ref)
    for k in names:
        err, scale = float((g_fused[k] - g_ref[k]).abs().max()), float(g_ref[k].abs().max())
        assert scale > 0 and err <= 1e-4 * scale, (k, err, scale)

    side = torch.cuda.Stream(DEV)
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        step(l1_ssim_loss)
        torch.cuda.synchronize()
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph, stream=side):
            captured = step(l1_ssim_loss)
    torch.cuda.synchronize()
    graph.replay()
    torch.cuda.synchronize()
    assert torch.equal(captured.detach(), loss)
    for k in names:
        assert torch.equal(params[k].grad, g_fused[k]), k
