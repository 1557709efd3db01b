"""rgbd_loss on the GPU (loss.hip ssim_kernel<., true>): loss, terms and the complete gradient against the fp64 reference
(tests/rgbd_loss_ref.py), the same bits as l1_ssim_loss where the two coincide, invariance under the mask, reproducibility,
the cotangent handling of the stored gradient, the Python refusals, and a Trainer step end to end, eager and captured."""
import math

import numpy as np
import pytest
import torch

import rgbd_loss_ref as R
import ssim_ref as S
from robosimgs_amd import camera_ring, synthetic_scene

DEV = "cuda"
pytestmark = pytest.mark.gpu

SHAPES = [(11, 11), (13, 17), (37, 29), (2, 45, 70), (40, 50)]


def _gen(seed):
    return torch.Generator(DEV).manual_seed(seed)


def _pair(shape, kind, seed=0):
    """test_gpu_ssim's image pairs: random, or near-constant (sigma^2 ~ 1e-5 << C2)."""
    g = _gen(seed)
    x = torch.rand(shape, device=DEV, generator=g)
    n = torch.rand(shape, device=DEV, generator=g)
    if kind == "near-constant":
        return 0.5 + 0.01 * x, 0.5 + 0.01 * n
    return x, 0.7 * x + 0.3 * n


def _blobs(lead, seed, zeros=0.3):
    """A binary float mask [lead] with about `zeros` of it 0, in 4 x 4 blobs."""
    h, w = lead[-2:]
    coarse = torch.rand(lead[:-2] + ((h + 3) // 4, (w + 3) // 4), device=DEV, generator=_gen(seed)) >= zeros
    return coarse.repeat_interleave(4, -2).repeat_interleave(4, -1)[..., :h, :w].float().contiguous()


def _mask(lead, kind, seed=11):
    if kind is None:
        return None
    b = _blobs(lead, seed)
    return b if kind == "binary" else b * torch.rand(lead, device=DEV, generator=_gen(seed + 1))


def _frame(lead, cr, kind, seed=0):
    """render [lead, cr] (depth 1..3 in channel 3), target_rgb, target_depth with about 10 % invalid (0, negative, NaN, inf)."""
    c, t = _pair(lead + (3,), kind, seed)
    g = _gen(seed + 100)
    d = 1.0 + 2.0 * torch.rand(lead, device=DEV, generator=g)
    dt = d + 0.2 * (torch.rand(lead, device=DEV, generator=g) - 0.5)
    u = torch.rand(lead, device=DEV, generator=g)
    for lo, bad in ((0.0, 0.0), (0.025, -1.0), (0.05, float("nan")), (0.075, float("inf"))):
        dt = torch.where((u >= lo) & (u < lo + 0.025), torch.full_like(dt, bad), dt)
    render = c if cr == 3 else torch.cat([c, d[..., None]], -1)
    return render.contiguous(), t.contiguous(), dt.contiguous()


def _ref(render, target, depth, mask, lam, lam_d, padding):
    xd = render.detach().double().requires_grad_(True)
    v, terms = R.rgbd_loss_torch(xd, target.double(), None if depth is None else depth.double(),
                                 None if mask is None else mask.double(), lam, lam_d, padding)
    v.backward()
    return float(v.detach()), [float(t) for t in terms], xd.grad


def _close(got, want, what):
    assert abs(got - want) <= 1e-5 * abs(want), (what, got, want)


@pytest.mark.parametrize("mkind", [None, "binary", "soft"], ids=["no-mask", "binary", "soft"])
@pytest.mark.parametrize("kind", ["random", "near-constant"])
@pytest.mark.parametrize("padding", ["valid", "same"])
@pytest.mark.parametrize("lead", SHAPES, ids=lambda v: "x".join(map(str, v)))
def test_loss_terms_and_gradient_match_the_fp64_reference(lead, padding, kind, mkind):
    """Each frame with Cr = 3, with Cr = 4 and lambda_d = 0, and with Cr = 4 and lambda_d = 0.5 (about 10 % of d* invalid).
    Gates: loss and terms 1e-5 relative, the colour and the depth gradient each 1e-5 of its own maximum.  Every figure is
    printed before the verdict (pytest -s)."""
    from robosimgs_amd import rgbd_loss
    mask = _mask(lead, mkind)
    bad = []

    def gate(name, err, bound, what):
        print(what, name, "error", err, "bound", bound)
        if not err <= bound:
            bad.append((what, name, err, bound))

    for cr, lam_d in ((3, 0.0), (4, 0.0), (4, 0.5)):
        what = (cr, lam_d)
        render, target, depth = _frame(lead, cr, kind)
        xr = render.clone().requires_grad_(True)
        v, terms = rgbd_loss(xr, target, depth if lam_d else None, mask, 0.2, lam_d, padding, return_terms=True)
        v.backward()
        torch.cuda.synchronize()
        v_ref, t_ref, g_ref = _ref(render, target, depth if lam_d else None, mask, 0.2, lam_d, padding)
        g, t = xr.grad, terms.tolist()
        assert g.shape == render.shape and torch.isfinite(g).all(), what
        gate("loss", abs(float(v.detach()) - v_ref), 1e-5 * abs(v_ref), what)
        gate("colour gradient", float((g[..., :3].double() - g_ref[..., :3]).abs().max()), 1e-5 * float(g_ref[..., :3].abs().max()), what)
        gate("mean|x - y|", abs(t[0] - t_ref[0]), 1e-5 * abs(t_ref[0]), what)
        gate("SSIM", abs(t[1] - t_ref[1]), 1e-5 * abs(t_ref[1]), what)
        if lam_d:
            # channel 3 is lambda_d w / sum w up to a fixed-order fp32 sum of non-negative terms: a relative error of about
            # log2(n) 2^-24 < 2e-6 at these sizes.  Scaled by its own maximum, not the colour channels'.
            scale_d = float(g_ref[..., 3].abs().max())
            assert scale_d > 0
            gate("depth gradient", float((g[..., 3].double() - g_ref[..., 3]).abs().max()), 1e-5 * scale_d, what)
            gate("D", abs(t[2] - t_ref[2]), 1e-5 * abs(t_ref[2]), what)
            gate("sum w", abs(t[3] - t_ref[3]), 1e-5 * abs(t_ref[3]) if mkind == "soft" else 0.0, what)   # an integer < 2^24: exact
        else:
            assert t[2] == 0.0 and t[3] == 0.0, what
            if cr == 4:
                assert not g[..., 3].any(), what
    assert not bad, bad


@pytest.mark.parametrize("padding", ["valid", "same"])
def test_same_bits_as_l1_ssim_loss_where_the_two_coincide(padding):
    from robosimgs_amd import l1_ssim_loss, rgbd_loss
    lead = (2, 45, 70)
    render, target, _ = _frame(lead, 4, "random", 3)
    c3 = render[..., :3].contiguous().requires_grad_(True)
    want = l1_ssim_loss(c3, target, 0.2, padding)
    want.backward()
    for mask in (None, torch.ones(lead, device=DEV), torch.ones(lead, device=DEV, dtype=torch.bool)):
        x3 = render[..., :3].contiguous().requires_grad_(True)
        v = rgbd_loss(x3, target, mask=mask, ssim_lambda=0.2, padding=padding)
        v.backward()
        assert torch.equal(v.detach(), want.detach()) and torch.equal(x3.grad, c3.grad)
        x4 = render.clone().requires_grad_(True)
        seen = []
        hook = x4.register_hook(lambda g: seen.append(g))
        v4 = rgbd_loss(x4, target, mask=mask, ssim_lambda=0.2, padding=padding)
        # the render the kernel was handed (the node saves it for a second backward): the frame's own storage, not a copy
        assert v4.grad_fn.saved_tensors[0].data_ptr() == x4.data_ptr()
        v4.backward()
        hook.remove()
        assert torch.equal(v4.detach(), want.detach())
        assert torch.equal(x4.grad[..., :3], c3.grad) and not x4.grad[..., 3].any()
        assert seen[0].shape == x4.shape and seen[0].is_contiguous()      # the cotangent arrives complete, four channels


def test_what_the_mask_hides_changes_nothing():
    from robosimgs_amd import rgbd_loss
    lead = (2, 45, 70)
    render, target, depth = _frame(lead, 4, "random", 4)
    for mkind in ("binary", "soft"):
        mask = _mask(lead, mkind, 21)
        off = mask == 0
        assert 0.2 < float(off.float().mean()) < 0.4

        def run(r, t, d):
            xr = r.clone().requires_grad_(True)
            v, terms = rgbd_loss(xr, t, d, mask, 0.2, 0.5, "same", return_terms=True)
            v.backward()
            return v.detach(), terms, xr.grad

        v0, t0, g0 = run(render, target, depth)
        assert torch.isfinite(v0) and torch.isfinite(g0).all()
        r2, t2, d2 = render.clone(), target.clone(), depth.clone()
        noise = torch.rand(lead, device=DEV, generator=_gen(5))
        for buf, vals in ((r2, (float("nan"), float("inf"), -7.0)), (t2, (float("inf"), float("nan"), 3.0)),
                          (d2, (float("nan"), 5.0, float("-inf")))):
            for k, val in enumerate(vals):
                buf[off & (noise >= k / 3) & (noise < (k + 1) / 3)] = val
        v1, t1, g1 = run(r2, t2, d2)
        assert torch.equal(v1, v0) and torch.equal(t1, t0)
        assert torch.equal(g1, g0)                                  # where m > 0: the same bits ...
        assert not g0[off].any() and not g1[off].any()              # ... and exactly 0 where m == 0

    zero = torch.zeros(lead, device=DEV)
    for pad in ("valid", "same"):
        xr = render.clone().requires_grad_(True)
        v, terms = rgbd_loss(xr, target, depth, zero, 0.2, 0.5, pad, return_terms=True)
        v.backward()
        # lambda (1 - 1) + 0 and D = 0; S = (C1 C2) (1 / (C1 C2)) and its mean are 1 up to a few fp32 roundings
        tl = terms.tolist()
        assert abs(float(v)) <= 1e-6 and tl[0] == 0.0 and abs(tl[1] - 1.0) <= 1e-6 and tl[2:] == [0.0, 0.0], (float(v), tl)
        assert not xr.grad.any()
    # no valid depth anywhere: D = 0 and a zero depth gradient, decided on the device
    xr = render.clone().requires_grad_(True)
    v, terms = rgbd_loss(xr, target, torch.full_like(depth, float("nan")), None, 0.2, 0.5, return_terms=True)
    v.backward()
    assert torch.equal(v.detach(), rgbd_loss(render, target).detach()) and terms.tolist()[2:] == [0.0, 0.0]
    assert not xr.grad[..., 3].any() and xr.grad[..., :3].any()


def test_bits_reproduce_across_calls_and_forms():
    from robosimgs_amd import rgbd_loss
    lead = (2, 45, 70)
    render, target, depth = _frame(lead, 4, "random", 6)
    mask = _mask(lead, "soft", 31)
    out = []
    for _ in range(2):
        xr = render.clone().requires_grad_(True)
        v = rgbd_loss(xr, target, depth, mask, depth_lambda=0.5)
        v.backward()
        out.append((v.detach(), xr.grad))
    assert torch.equal(out[0][0], out[1][0]) and torch.equal(out[0][1], out[1][1])
    assert torch.equal(rgbd_loss(render, target, depth, mask, depth_lambda=0.5), out[0][0])      # mgs_rgbd_loss_fwd
    with torch.no_grad():
        assert torch.equal(rgbd_loss(render.clone().requires_grad_(True), target, depth, mask, depth_lambda=0.5), out[0][0])


def test_cotangents_and_a_second_backward():
    from robosimgs_amd import rgbd_loss, unit_gradient
    lead = (2, 40, 52)
    render, target, depth = _frame(lead, 4, "random", 7)
    mask = _mask(lead, "soft", 41)
    loss = lambda xr: rgbd_loss(xr, target, depth, mask, 0.2, 0.5, "same")
    grads = []
    for cot in ("unit", "ones", 2.5):
        xr = render.clone().requires_grad_(True)
        v = loss(xr)
        gr = unit_gradient(v) if cot == "unit" else (torch.ones_like(v) if cot == "ones" else torch.full_like(v, cot))
        v.backward(gradient=gr)
        grads.append(xr.grad)
    assert grads[0][..., 3].any()
    assert torch.equal(grads[0], grads[1])                          # unit_gradient: the stored gradient as it is
    assert torch.equal(grads[2], grads[0] * 2.5)                    # any other cotangent scales it once
    xr = render.clone().requires_grad_(True)
    v = loss(xr)
    (g1,) = torch.autograd.grad(v, xr, retain_graph=True)
    (g2,) = torch.autograd.grad(v, xr, grad_outputs=torch.full_like(v, 2.5), retain_graph=True)   # mgs_rgbd_loss_bwd
    (g3,) = torch.autograd.grad(v, xr)
    assert torch.equal(g1, grads[0]) and torch.equal(g2, grads[2]) and torch.equal(g3, grads[0])


def test_invalid_inputs_raise():
    from robosimgs_amd import rgbd_loss
    from robosimgs_amd._lib import MgsError
    r4, t3, d = torch.rand(20, 20, 4, device=DEV), torch.rand(20, 20, 3, device=DEV), torch.rand(20, 20, device=DEV)
    with pytest.raises(ValueError, match="shape mismatch"):
        rgbd_loss(r4, torch.rand(20, 21, 3, device=DEV))
    with pytest.raises(ValueError, match="shape mismatch: target_depth"):
        rgbd_loss(r4, t3, d[:19], depth_lambda=0.5)
    with pytest.raises(ValueError, match="shape mismatch: mask"):
        rgbd_loss(r4, t3, mask=torch.ones(20, 20, 1, device=DEV))
    with pytest.raises(ValueError, match="four-channel"):
        rgbd_loss(r4[..., :3], t3, d, depth_lambda=0.5)
    with pytest.raises(ValueError, match="needs target_depth"):
        rgbd_loss(r4, t3, depth_lambda=0.5)
    with pytest.raises(MgsError, match="GPU only"):
        rgbd_loss(r4, t3.cpu())
    with pytest.raises(MgsError, match="GPU only"):
        rgbd_loss(r4, t3, mask=torch.ones(20, 20))
    with pytest.raises(ValueError, match=">= 11"):
        rgbd_loss(r4[:10], t3[:10])
    assert torch.isfinite(rgbd_loss(r4[:10], t3[:10], padding="same"))
    assert torch.isfinite(rgbd_loss(r4, t3, d, torch.ones(20, 20, device=DEV, dtype=torch.uint8), depth_lambda=0.5))


def _composed_loss(colors, target, depth_t, mask, lam=0.2, lam_d=0.5):
    """The same loss composed in fp32 eager torch: torch.where masking, pytorch_msssim's separable grouped conv2d
    ("valid") for SSIM, a masked mean for the depth term."""
    on, zero = (mask > 0)[..., None], torch.zeros((), device=colors.device)
    xm = torch.where(on, mask[..., None] * colors[..., :3], zero)
    ym = torch.where(on, mask[..., None] * target, zero)
    x, y = xm.permute(0, 3, 1, 2), ym.permute(0, 3, 1, 2)
    g = torch.from_numpy(S.window()).float().to(colors.device)
    wh, ww = g.view(1, 1, -1, 1).repeat(3, 1, 1, 1), g.view(1, 1, 1, -1).repeat(3, 1, 1, 1)
    f = lambda t: torch.nn.functional.conv2d(torch.nn.functional.conv2d(t, wh, groups=3), ww, groups=3)
    mx, my = f(x), f(y)
    vxx, vyy, vxy = f(x * x) - mx * mx, f(y * y) - my * my, f(x * y) - mx * my
    s = (2 * mx * my + S.C1) * (2 * vxy + S.C2) / ((mx * mx + my * my + S.C1) * (vxx + vyy + S.C2))
    w = torch.where(torch.isfinite(depth_t) & (depth_t > 0), mask, zero)
    diff = torch.where(w > 0, colors[..., 3], zero) - torch.where(w > 0, depth_t, zero)
    return (1 - lam) * (xm - ym).abs().mean() + lam * (1 - s.mean()) + lam_d * (w * diff.abs()).sum() / w.sum()


def test_trainer_step_end_to_end_eager_and_captured():
    from robosimgs_amd import Trainer, rgbd_loss
    W, H = 160, 112
    g = synthetic_scene(6000, math.log(0.08), 2, 12)
    cam = camera_ring(1, W, H, thetas=[0.5])[0]
    vm = torch.from_numpy(cam.viewmat().astype(np.float32)).to(DEV)[None]
    K = torch.from_numpy(cam.K.astype(np.float32)).to(DEV)[None]
    names = ("means", "quats", "scales", "opacities", "colors")
    t = g.to_torch(DEV, 2)
    params = {k: t[k].detach().clone().requires_grad_(True) for k in names}
    target = torch.rand(1, H, W, 3, device=DEV, generator=_gen(8))
    tr = Trainer(params, None, W, H, auto_reorder_every=0, sh_degree=2, render_mode="RGB+ED", isect_capacity=400_000)
    with torch.no_grad():
        depth0 = tr.render(vm, K)[0][..., 3].clone()
    u = torch.rand(1, H, W, device=DEV, generator=_gen(9))
    depth_t = depth0 * (0.9 + 0.2 * u)
    depth_t[u < 0.05] = float("nan")                  # besides the zeros of pixels the scene does not cover
    mask = _blobs((1, H, W), 10)

    def step(loss_fn):
        for p in params.values():
            p.grad = None
        colors, alphas, meta = tr.render(vm, K)
        loss = loss_fn(colors)
        tr.step(loss)
        return loss

    fused = lambda colors: rgbd_loss(colors, target, depth_t, mask, 0.2, 0.5)
    ref = step(lambda colors: _composed_loss(colors, target, depth_t, mask)).detach()
    g_ref = {k: params[k].grad.clone() for k in names}
    loss = step(fused).detach()
    g_fused = {k: params[k].grad.clone() for k in names}
    print("loss", float(loss), float(ref))
    assert abs(float(loss) - float(ref)) <= 1e-5 * float(ref)
    for k in names:
        err, scale = float((g_fused[k] - g_ref[k]).abs().max()), float(g_ref[k].abs().max())
        print(k, err, scale)
        assert scale > 0 and err <= 1e-4 * scale, (k, err, scale)

    side = torch.cuda.Stream(DEV)
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        step(fused)
        torch.cuda.synchronize()
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph, stream=side):
            captured = step(fused)
    torch.cuda.synchronize()
    graph.replay()
    torch.cuda.synchronize()
    assert torch.equal(captured.detach(), loss)
    for k in names:
        assert torch.equal(params[k].grad, g_fused[k]), k
