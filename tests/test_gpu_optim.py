"""GaussianAdam / mgs_adam_step on the GPU (include/mgs_optim.h, csrc/optim.hip).

The reference is never the code under test: torch.optim.Adam on the CPU in float64 where the learning rate is constant,
a plain fp64 restatement of the update for the schedule and the row split.  Bounds are rounding analysis with
u = 2^-24 (one fp32 rounding), written next to each use."""
import copy
import math

import numpy as np
import pytest
import torch

from robosimgs_amd import GaussianAdam, Trainer, camera_ring, reorder_parameters, splatfacto_groups, synthetic_scene

# tests/adam_ref.py: the fp64 update and the per-element bounds, shared with test_gpu_training_loop.py
from adam_ref import B1, B2, EPS, U, first_moment_bound, param_bound, second_moment_bound
from adam_ref import update64 as _update64

pytestmark = pytest.mark.gpu
DEV = "cuda"
SHAPES = {1: lambda n: (n,), 3: lambda n: (n, 3), 4: lambda n: (n, 4), 48: lambda n: (n, 16, 3)}


def _rand(shape, seed, scale=1.0):
    return torch.randn(shape, generator=torch.Generator().manual_seed(seed), dtype=torch.float32) * scale


def _problem(n, row, seed):
    """fp32 p, g, m, v on the CPU: gradients of both signs with a few exact zeros, v >= 0."""
    shape = SHAPES[row](n)
    p, g, m = _rand(shape, seed), _rand(shape, seed + 1, 1e-2), _rand(shape, seed + 2, 3e-3)
    v = _rand(shape, seed + 3, 1e-2) ** 2
    g.view(-1)[::7] = 0.0
    return p, g, m, v


def _optimizer(problems, t_before, groups=None, **kw):
    """A GaussianAdam over GPU copies of `problems` (one param group each), its moments preset to the given m, v and its
    counter to t_before steps taken -- through load_state_dict, like a resumed run."""
    ps = [p.to(DEV).clone().requires_grad_(True) for p, _, _, _ in problems]
    for q, (_, g, _, _) in zip(ps, problems):
        q.grad = g.to(DEV).clone()
    groups = groups or [dict(lr=1e-3 * (k + 1)) for k in range(len(ps))]
    opt = GaussianAdam([dict(params=[q], **o) for q, o in zip(ps, groups)], betas=(B1, B2), eps=EPS, **kw)
    sd = opt.state_dict()
    sd["state"] = {k: {"exp_avg": m.clone(), "exp_avg_sq": v.clone()} for k, (_, _, m, v) in enumerate(problems)}
    sd["step_state"] = torch.tensor([t_before, 0], dtype=torch.int32)
    opt.load_state_dict(sd)
    return opt, ps


def _moments(opt, ps):
    return [opt.state[q]["exp_avg"] for q in ps], [opt.state[q]["exp_avg_sq"] for q in ps]


def _snapshot(opt, ps):
    m, v = _moments(opt, ps)
    return [x.detach().clone() for x in (*ps, *m, *v)]


@pytest.mark.parametrize("t", [1, 2, 1000])
@pytest.mark.parametrize("n", [1, 5, 257, 4099])
def test_one_step_matches_fp64_adam(n, t):
    """Row widths 1, 3, 4 and 48 as four groups of ONE launch, update number t, against torch.optim.Adam in fp64 on the
    CPU from the same fp32 p, g, m, v.  No element may exceed a bound (u = 2^-24):

      m' : 4u (b1 |m| + (1 - b1) |g|)   -- b1 and 1 - b1 rounded to fp32 (u each), the product b1 m (u), the fma (u): 3u
      v' : 4u v'64                      -- b2, 1 - b2 rounded (u each), (1 - b2) g (u), b2 v (u), the fma (exact product,
           one rounding of the sum of two non-negative terms, u): 3u
      p' : u |p'64| + 16u |D64|         -- p'64 = p - D64 in fp64 from the GPU's own m', v'.  Roundings of the step D:
           sqrtf (1 ulp = 2u), sqrt(1 - b2^t) to fp32 (u), the division by it (2.5 ulp = 5u), + eps (u, and eps itself
           to fp32, below u of the sum), m' / denominator (5u), lr / (1 - b1^t) to fp32 (u), the final fma (exact
           product; its rounding is the u |p'64|): 2 + 1 + 5 + 1 + 5 + 1 = 15u <= 16u at HIP's documented worst case,
           9 roundings; with the correctly rounded division and square root the build uses, 6u."""
    problems = [_problem(n, row, 100 * row + n) for row in SHAPES]
    opt, ps = _optimizer(problems, t - 1)
    opt.step()
    torch.cuda.synchronize()
    assert opt.steps_taken() == t
    ms, vs = _moments(opt, ps)
    for k, (p, g, m, v) in enumerate(problems):
        lr = 1e-3 * (k + 1)
        q = p.double().clone().requires_grad_(True)
        q.grad = g.double()
        ref = torch.optim.Adam([q], lr=lr, betas=(B1, B2), eps=EPS, foreach=False)
        ref.state[q] = {"step": torch.tensor(float(t - 1)), "exp_avg": m.double().clone(), "exp_avg_sq": v.double().clone()}
        ref.step()
        m64, v64 = ref.state[q]["exp_avg"], ref.state[q]["exp_avg_sq"]
        # the restatement used for p (and by the schedule / split tests) is torch's update, up to the ~1e-13 relative
        # that torch's own 1 - b2**t loses in fp64 at small t
        d_ref = _update64(m64, v64, t, lr)
        assert bool((((p.double() - d_ref) - q.detach()).abs() <= 1e-12 * (d_ref.abs() + p.double().abs())).all())
        gm, gv, gp = ms[k].cpu(), vs[k].cpu(), ps[k].detach().cpu()
        err_m = (gm.double() - m64).abs() - first_moment_bound(m, g)
        err_v = (gv.double() - v64).abs() - second_moment_bound(v64)
        d64 = _update64(gm, gv, t, lr)
        p64 = p.double() - d64
        err_p = (gp.double() - p64).abs() - param_bound(p64, d64)
        what = f"n={n} t={t} row={list(SHAPES)[k]}"
        print(f"{what}: worst excess over the bound m {float(err_m.max()):.3e} v {float(err_v.max()):.3e} p {float(err_p.max()):.3e}")
        assert int((err_m > 0).sum()) == 0, what
        assert int((err_v > 0).sum()) == 0, what
        assert int((err_p > 0).sum()) == 0, what
        assert float(d64.abs().max()) > 0


def test_bias_correction_at_the_first_step():
    """t = 1, b2 = 0.999, gradients of one sign per tensor, p = m = v = 0: the update is lr g / (|g| + eps) = lr sign(g)
    to 16u relative (the step's roundings as above, plus those of m' and v' from zero moments: about 11u).  1 - b2^t
    evaluated in fp32 is off by ~6e-5 relative (half of that in the update) and fails."""
    n, lr = 4099, 1e-2
    mag = torch.rand(n, 3, generator=torch.Generator().manual_seed(5)) * 1.5 + 0.5
    problems = [(torch.zeros(n, 3), s * mag, torch.zeros(n, 3), torch.zeros(n, 3)) for s in (1.0, -1.0)]
    opt, ps = _optimizer(problems, 0, groups=[dict(lr=lr), dict(lr=lr)])
    opt.step()
    for q, (_, g, _, _) in zip(ps, problems):
        want = lr * g.double() / (g.double().abs() + EPS)
        rel = ((-q.detach().cpu().double()) - want).abs() / want.abs()
        print(f"bias correction: worst relative error {float(rel.max()) / U:.2f} u")
        assert float(rel.max()) <= 16 * U


def test_schedule_follows_the_exponential_decay_and_then_stays_flat():
    """12 steps with decay_steps = 8, p reset to zero before each so that p' = -D exactly: the learning rate implied by the
    step, D (1 - b1^t) (sqrt(v') / sqrt(1 - b2^t) + eps) / m' in fp64 from the GPU's m', v', is
    lr r^(min(t - 1, 8) / 8) with r = lr_final / lr, to 16u relative (the roundings of D listed in
    test_one_step_matches_fp64_adam), and the same from update 9 on."""
    n, lr, lr_final, steps = 257, 1e-2, 1e-3, 8
    g = _rand((n, 3), 11, 1e-2) + 2e-2                                    # away from zero: m' / denominator is O(1)
    problems = [(torch.zeros(n, 3), g, torch.zeros(n, 3), torch.zeros(n, 3))]
    opt, (q,) = _optimizer(problems, 0, groups=[dict(lr=lr, lr_final=lr_final, decay_steps=steps)])
    implied = []
    for t in range(1, 13):
        q.data.zero_()
        opt.step()
        m, v = opt.state[q]["exp_avg"].cpu(), opt.state[q]["exp_avg_sq"].cpu()
        unit = _update64(m, v, t, 1.0)
        got = -q.detach().cpu().double() / unit
        want = lr * (lr_final / lr) ** (min(t - 1, steps) / steps)
        implied.append(want)
        rel = (got / want - 1).abs()
        print(f"schedule t={t}: lr {want:.6e}, worst relative error {float(rel.max()) / U:.2f} u")
        assert float(rel.max()) <= 16 * U, t
    assert all(a > b for a, b in zip(implied[:8], implied[1:9])) and implied[0] == lr
    assert all(math.isclose(x, lr_final, rel_tol=1e-12) for x in implied[8:])
    assert opt.steps_taken() == 12


@pytest.mark.parametrize("shape,head", [((257, 16, 3), 3), ((257, 5, 3), 3), ((259, 7), 2)])
def test_row_split_trains_head_and_rest_at_two_rates(shape, head):
    """t = 1 from p = m = v = 0: the first head_floats of every row move by lr g / (|g| + eps), the rest by a twentieth of
    that, each to 16u relative (as test_bias_correction_at_the_first_step; lr / 20 / (1 - b1) is rounded once like lr /
    (1 - b1)).  Row widths 15 and 7 put float4s across the split and across rows."""
    lr, scale = 2.5e-3, 1 / 20
    g = _rand(shape, 21)
    g = torch.where(g.abs() < 0.1, torch.full_like(g, 0.1), g)
    z = torch.zeros(shape)
    opt, (q,) = _optimizer([(z, g, z, z)], 0, groups=[dict(lr=lr, head_floats=head, rest_lr_scale=scale)])
    opt.step()
    moved = -q.detach().cpu().double().reshape(shape[0], -1)
    g2 = g.double().reshape(shape[0], -1)
    want = lr * g2 / (g2.abs() + EPS)
    want[:, head:] *= scale
    rel = (moved / want - 1).abs()
    print(f"split {shape}: worst relative error head {float(rel[:, :head].max()) / U:.2f} u, rest {float(rel[:, head:].max()) / U:.2f} u")
    assert float(rel.max()) <= 16 * U


def _radii(n, seed, cams=2):
    """[cams, n] int32 radii, about half of the Gaussians visible in no camera."""
    gen = torch.Generator().manual_seed(seed)
    seen = torch.rand(cams, n, generator=gen) < 1 - 0.5 ** (1 / cams)
    r = torch.randint(1, 40, (cams, n), generator=gen, dtype=torch.int32) * seen.to(torch.int32)
    r[:, 1::11] = -r[:, 1::11]                     # a negative radius is not visible either
    return r


def _visibility_forms(r):
    """The same visible set as radii [C,N] (contiguous, and rows of a wider tensor), as [C,N,2] whose two axes each carry
    part of it (interleaved, and the planar view rasterization returns), and as a bool [N] mask."""
    c, n = r.shape
    coin = torch.rand(c, n, generator=torch.Generator().manual_seed(3)) < 0.5
    rx, ry = r * coin.to(torch.int32), r * (~coin).to(torch.int32)
    wide = torch.zeros(c, n + 5, dtype=torch.int32)
    wide[:, :n] = r
    wide[:, n:] = 7
    return {"radii [C,N]": r.to(DEV), "radii rows of [C,N+5]": wide.to(DEV)[:, :n],
            "radii [C,N,2] interleaved": torch.stack([rx, ry], -1).to(DEV),
            "radii [C,N,2] planar view": torch.stack([rx, ry], 1).to(DEV).permute(0, 2, 1),
            "bool [N]": (r > 0).any(0).to(DEV), "radii [N]": torch.where((r > 0).any(0), 3, 0).to(torch.int32).to(DEV)}


def test_invisible_gaussians_are_left_bit_identical():
    """Row widths 1, 3, 4 and 48 in one masked launch at N = 4099 (float4s across visible and invisible rows, the tail):
    p, m, v of the rows no camera saw are the bits they were; the visible rows are the bits of the unmasked launch; the
    counter advanced.  Every accepted form of the visibility argument selects the same rows."""
    n = 4099
    problems = [_problem(n, row, 7 * row) for row in SHAPES]
    r = _radii(n, 1)
    vis = (r > 0).any(0).to(DEV)
    assert 0.4 * n < int(vis.sum()) < 0.6 * n
    full, fps = _optimizer(problems, 2)
    before = _snapshot(full, fps)
    full.step()
    after = _snapshot(full, fps)
    assert all(not torch.equal(a[vis], b[vis]) for a, b in zip(before, after))
    for name, form in _visibility_forms(r).items():
        opt, ps = _optimizer(problems, 2, selective=True)
        opt.step(visibility=form)
        got = _snapshot(opt, ps)
        assert opt.steps_taken() == 3, name
        for x, b, a in zip(got, before, after):
            assert torch.equal(x[~vis], b[~vis]), name
            assert torch.equal(x[vis], a[vis]), name
    # nothing visible: only the counter moves
    opt, ps = _optimizer(problems, 2, selective=True)
    opt.step(visibility=torch.zeros(n, dtype=torch.bool, device=DEV))
    assert all(torch.equal(x, b) for x, b in zip(_snapshot(opt, ps), before)) and opt.steps_taken() == 3
    with pytest.raises(Exception, match="visibility"):
        opt.step()
    with pytest.raises(Exception, match="visibility"):
        opt.step(visibility=torch.zeros(n + 1, dtype=torch.bool, device=DEV))


def test_a_parameter_without_a_gradient_is_left_out():
    problems = [_problem(257, 3, 1), _problem(257, 4, 2)]
    opt, ps = _optimizer(problems, 0)
    ps[1].grad = None
    before = _snapshot(opt, ps)
    opt.step()
    got = _snapshot(opt, ps)
    assert not torch.equal(got[0], before[0]) and opt.steps_taken() == 1
    for k in (1, 3, 5):
        assert torch.equal(got[k], before[k])


@pytest.mark.parametrize("masked", [False, True])
def test_five_eager_steps_equal_one_captured_step_replayed_five_times(masked):
    """The schedule active (decay over 3 steps, then flat), a split SH tensor, and the counter on the device: p, m, v and
    the counter after five replays of ONE captured step are the bits of five eager steps.  A counter kept on the host
    would replay update 1 five times."""
    n = 4099
    problems = [_problem(n, 3, 31), _problem(n, 48, 32), _problem(n, 1, 33)]
    groups = [dict(lr=1e-2, lr_final=1e-4, decay_steps=3), dict(lr=2.5e-3, head_floats=3, rest_lr_scale=0.05), dict(lr=5e-2)]
    vis = _radii(n, 2).to(DEV) if masked else None
    eager, eager_ps = _optimizer(problems, 0, groups=groups, selective=masked)
    first = None
    for k in range(5):
        eager.step(visibility=vis)
        first = first or _snapshot(eager, eager_ps)
    want = _snapshot(eager, eager_ps)
    assert not torch.equal(first[0], want[0])
    opt, ps = _optimizer(problems, 0, groups=groups, selective=masked)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        opt.step(visibility=vis)
    torch.cuda.synchronize()
    assert opt.steps_taken() == 0                                   # capturing ran nothing
    for _ in range(5):
        graph.replay()
    torch.cuda.synchronize()
    assert opt.steps_taken() == eager.steps_taken() == 5
    assert torch.equal(opt.step_state, eager.step_state) and int(opt.step_state[1]) == 0
    for x, w in zip(_snapshot(opt, ps), want):
        assert torch.equal(x, w)


def _scene_params(n, seed):
    shapes = {"means": (n, 3), "quats": (n, 4), "scales": (n, 3), "opacities": (n,), "colors": (n, 16, 3)}
    return {k: _rand(s, seed + i).to(DEV).requires_grad_(True) for i, (k, s) in enumerate(shapes.items())}


def test_reorder_parameters_carries_the_moments():
    """Two steps, a Morton reorder, two more steps: parameters and moments equal the un-reordered run's mapped through the
    permutation, bit for bit (the update is elementwise), under the schedule and the split."""
    n = 1237
    a = _scene_params(n, 40)
    b = {k: v.detach().clone().requires_grad_(True) for k, v in a.items()}
    oa, ob = (GaussianAdam(splatfacto_groups(p, decay_steps=3)) for p in (a, b))
    grads = [{k: _rand(v.shape, 50 + 10 * s + i, 1e-2).to(DEV) for i, (k, v) in enumerate(a.items())} for s in range(4)]
    order = torch.arange(n, device=DEV)
    for s in range(4):
        if s == 2:
            order = reorder_parameters(b, ob, per_gaussian=list(Trainer.KEYS))
            assert not torch.equal(order, torch.arange(n, device=DEV))
        for k in a:
            a[k].grad, b[k].grad = grads[s][k].clone(), grads[s][k][order].clone()
        oa.step()
        ob.step()
    for k in a:
        assert torch.equal(b[k].detach(), a[k].detach()[order]), k
        for key in ("exp_avg", "exp_avg_sq"):
            assert torch.equal(ob.state[b[k]][key], oa.state[a[k]][key][order]), (k, key)
    assert oa.steps_taken() == ob.steps_taken() == 4


def test_state_dict_round_trip():
    """Moments and counter survive state_dict() -> load_state_dict() into a fresh optimiser: the resumed run's next step is
    the original's, bit for bit (the schedule is mid-decay, so a lost counter would show)."""
    a = _scene_params(257, 60)
    oa = GaussianAdam(splatfacto_groups(a, decay_steps=5), selective=False)
    for s in range(2):
        for i, k in enumerate(a):
            a[k].grad = _rand(a[k].shape, 70 + 10 * s + i, 1e-2).to(DEV)
        oa.step()
    sd = copy.deepcopy(oa.state_dict())
    assert sd["step_state"].tolist() == [2, 0] and len(sd["state"]) == 5
    b = {k: v.detach().clone().requires_grad_(True) for k, v in a.items()}
    ob = GaussianAdam(splatfacto_groups(b, decay_steps=5))
    ob.load_state_dict(sd)
    assert ob.steps_taken() == 2
    for k in a:
        for key in ("exp_avg", "exp_avg_sq"):
            assert torch.equal(ob.state[b[k]][key], oa.state[a[k]][key])
    for i, k in enumerate(a):
        a[k].grad = _rand(a[k].shape, 90 + i, 1e-2).to(DEV)
        b[k].grad = a[k].grad.clone()
    oa.step()
    ob.step()
    assert oa.steps_taken() == ob.steps_taken() == 3
    for k in a:
        assert torch.equal(a[k].detach(), b[k].detach()), k


def test_trainer_steps_a_selective_gaussian_adam_inside_a_hip_graph():
    """The scene of test_raw_trainer_step_captures_in_a_hip_graph_and_descends (8 000 Gaussians, 160 x 112, raw leaves) with
    GaussianAdam(splatfacto_groups(...), selective=True): render -> l1_loss -> step captured once and replayed five times.
    Everything stays finite, the loss ends lower, the counter counted every step, and the Gaussians the camera never saw
    are bit-unchanged from the start, moments included (zero)."""
    from robosimgs_amd import l1_loss
    names = Trainer.KEYS
    g = synthetic_scene(8000, math.log(0.08), 2, 12)
    cam = camera_ring(1, 160, 112, thetas=[0.5])[0]
    as_t = lambda a: torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32)).to(DEV)
    vm, K = as_t(cam.viewmat())[None], as_t(cam.K)[None]
    target = torch.rand(1, 112, 160, 4, device=DEV, generator=torch.Generator(DEV).manual_seed(2))
    t = g.to_torch(DEV, 2, raw=True)
    p = {k: t[k].detach().clone().requires_grad_(True) for k in names}
    start = {k: p[k].detach().clone() for k in names}
    opt = GaussianAdam(splatfacto_groups(p), selective=True)
    tr = Trainer(p, opt, 160, 112, auto_reorder_every=500, sh_degree=2, render_mode="RGB+ED", isect_capacity=400_000,
                 raw_params=True)
    loss_buf = torch.zeros((), device=DEV)
    seen = torch.zeros(8000, dtype=torch.bool, device=DEV)

    def step():
        c, a, meta = tr.render(vm, K)
        seen.logical_or_((meta["radii"] > 0).reshape(1, 8000, -1).any(-1).any(0))
        loss = l1_loss(c, target)
        loss_buf.copy_(loss.detach())
        tr.step(loss)

    # warm-up and capture on ONE side stream: autograd pins each leaf's gradient accumulation to the stream of the leaf's
    # first use, so a step warmed up on another stream than the capturing one would leave the capture
    side = torch.cuda.Stream(DEV)
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        for _ in range(3):                       # the first render reorders (Morton), allocations settle
            step()
        torch.cuda.synchronize()
        assert tr.reorders == 1 and opt.steps_taken() == 3
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph, stream=side):
            step()
    torch.cuda.synchronize()
    losses = []
    for _ in range(5):
        graph.replay()
        torch.cuda.synchronize()
        losses.append(float(loss_buf))
    assert tr.reorders == 1 and opt.steps_taken() == 8
    for k in names:
        assert torch.isfinite(p[k]).all(), k
        for key in ("exp_avg", "exp_avg_sq"):
            assert torch.isfinite(opt.state[p[k]][key]).all(), (k, key)
    assert all(math.isfinite(x) for x in losses) and losses[-1] < losses[0], losses
    never = tr.in_original_order(seen.to(torch.uint8)) == 0
    print(f"trainer: {int(never.sum())} of 8000 Gaussians never visible; losses {losses}")
    assert 0 < int(never.sum()) < 8000
    for k in names:
        now = tr.in_original_order(p[k].detach())
        assert torch.equal(now[never], start[k][never]), k
        assert not torch.equal(now[~never], start[k][~never]), k
        for key in ("exp_avg", "exp_avg_sq"):
            assert not tr.in_original_order(opt.state[p[k]][key])[never].any(), (k, key)
