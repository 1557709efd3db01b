"""A short training loop through Trainer, every link of every step held to fp64 (teacher-forced).

Trainer chains render -> loss -> backward -> GaussianAdam, eagerly or as one captured HIP graph that is replayed.  Each
piece has its own single-call gate (test_gpu_raw_params.py, test_gpu_ssim.py, test_gpu_optim.py ...); this module checks
what lives BETWEEN steps: a buffer a replay does not clear, a gradient that accumulates, the previous render's radii as
this step's mask, a camera read at capture time, moments out of step with a reordered scene, an update number off by one.
Adam divides by the gradient's own magnitude, so none of those stops the loss from descending.

The loop is observed, not changed: parameters, moments, counter and original_index are cloned before and after a step;
the frame, alphas, radii, loss, d loss / d frame (a tensor hook on `colors`) and the five gradients the optimiser consumed
(post-accumulate hooks on the leaves) are copied into static buffers inside the step -- ordinary device copies, so a
captured graph records them.  After every step each link is compared with a plain fp64 reference whose INPUTS are the
GPU's own (the pre-step parameters, the captured frame, the captured cotangent, the captured gradients), so that errors
neither compound nor hide:

  1 frame       O.render + O.check_frame, as test_raw_frame_passes_the_forward_gate
  2 visibility  radii against the oracle projection's (test_raw_projection_matches_oracle's allowance, per camera), and
                against the GPU's own radii for each camera rendered alone, bit for bit
  3 loss        value and d loss / d frame at the captured frame (test_gpu_ssim.py's bounds; test_fused_l1_loss_matches_torch's
                for the plain L1)
  4 gradients   fp64 autograd of OT.render for loss = <w, frame>, w the captured cotangent, summed over the step's cameras;
                test_raw_gradients_match_autograd_through_the_activations' gate with summed flip budgets
  5 update      fp64 Adam (tests/adam_ref.py) from the captured gradients and pre-step moments at update number
                counter + 1: test_one_step_matches_fp64_adam's per-element bounds on the rows the captured radii mark
                visible, every other row of all fifteen tensors bit-identical, the counter advanced by one, a Morton
                reorder carried through parameters, moments and original_index bit for bit.

Every gate and number is one the project already uses.  Worst ratios measured on an MI355X: profiles/training_loop/.

Cost: 19 camera-steps of the CPU oracles at 3 000 Gaussians, 96 x 64 -- 4.0-7.1 s for case A and 6.3-6.8 s for case B next to
an MI355X, against 2.2-2.7 s for the six cases of test_raw_gradients_match_autograd_through_the_activations.  In a CPU
profile of one camera-step, 0.85 of about 1.2 s was the per-entry Python loop of O.render's blend with margins (link 1); the
C++ port could take its place only by changing the reference."""
import math

import numpy as np
import pytest
import torch

import ssim_ref as S
from oracle import gs_oracle_np as O
from oracle import gs_oracle_torch as OT
from robosimgs_amd import GaussianAdam, Trainer, camera_ring, rasterization, splatfacto_groups, synthetic_scene
from robosimgs_amd.gaussians import Gaussians

import adam_ref as A
from grad_gate import compare, oracle_budgets, parameter_budgets
from test_gpu_raw_params import _activated64        # exp / sigmoid in fp64 of the fp32 raw values
from test_gpu_ssim import _check_grad                # 1e-5 of the gradient's largest entry

pytestmark = pytest.mark.gpu
DEV = "cuda"
W, H, N = 96, 64, 3000                               # 6 x 4 tiles
NAMES = Trainer.KEYS
MODE = "RGB+ED"
ADAM_EPS = 1e-15                                     # splatfacto's


def _t(a):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32))


def _f32(a):
    """What the GPU is given: the matrix rounded to fp32 (the oracle then computes in fp64 from it)."""
    return np.asarray(a, dtype=np.float32).astype(np.float64)


def _d(a, grad=False):
    return torch.tensor(np.asarray(a, dtype=np.float64), requires_grad=grad)


def _visible(radii):
    """[C,N] or [C,N,2] radii -> [C,N] bool: what GaussianAdam's mask reads (a positive extent on either axis)."""
    r = torch.as_tensor(radii)
    return (r.reshape(r.shape[0], r.shape[1], -1) > 0).any(-1)


def _ratio(err, bound):
    """max err / bound over the elements; an element with no allowance must have no error."""
    r = torch.where(bound > 0, err / bound.clamp(min=1e-300), torch.where(err > 0, torch.full_like(err, math.inf), torch.zeros_like(err)))
    return float(r.max()) if r.numel() else 0.0


class _Loop:
    """A Trainer over this module's scene, with the observation buffers and hooks (hooks=False: the bare loop)."""

    def __init__(self, deg, n_cams, loss_fn, loss_channels, hooks=True, groups_kw=None, **trainer_kw):
        self.deg, self.loss_fn, self.loss_channels = deg, loss_fn, loss_channels
        self.rule = trainer_kw.get("radius_rule", "classic")
        self.scene = synthetic_scene(N, math.log(0.1), deg, seed=12)
        self.cams = camera_ring(4, W, H)
        t = self.scene.to_torch(DEV, deg, raw=True)
        self.p = {k: t[k].detach().clone().requires_grad_(True) for k in NAMES}
        self.opt = GaussianAdam(splatfacto_groups(self.p, **(groups_kw or {})), eps=ADAM_EPS, selective=True)
        self.tr = Trainer(self.p, self.opt, W, H, raw_params=True, sh_degree=deg, render_mode=MODE, **trainer_kw)
        gen = torch.Generator().manual_seed(5)
        self.targets = torch.rand(4, H, W, loss_channels, generator=gen)       # one fixed random image per camera
        if loss_channels == 4:
            self.targets[..., 3] = 4.0 + 6.0 * self.targets[..., 3]            # expected depths: both signs of the residual
        self.vm = torch.zeros(n_cams, 4, 4, device=DEV)
        self.K = torch.zeros(n_cams, 3, 3, device=DEV)
        self.target = torch.zeros(n_cams, H, W, loss_channels, device=DEV)
        self.obs = None
        self.mid = None                                  # eager only: the state between render() and step()
        self.snap_mid = False
        if hooks:
            per_axis = (2,) if self.rule == "opacity_aware" else ()
            self.obs = {"frame": torch.zeros(n_cams, H, W, 4, device=DEV), "alphas": torch.zeros(n_cams, H, W, 1, device=DEV),
                        "radii": torch.zeros((n_cams, N) + per_axis, dtype=torch.int32, device=DEV),
                        "loss": torch.zeros((), device=DEV), "v_frame": torch.zeros(n_cams, H, W, 4, device=DEV)}
            for k in NAMES:
                self.obs["g_" + k] = torch.zeros_like(self.p[k].detach())
                self.p[k].register_post_accumulate_grad_hook(self._grad_hook(k))

    def _grad_hook(self, k):
        def hook(leaf):
            self.obs["g_" + k].copy_(leaf.grad)
        return hook

    def _frame_hook(self, g):
        self.obs["v_frame"].copy_(g)

    def set_cameras(self, idx):
        """Copy the step's cameras and targets into the static tensors the step reads."""
        self.vm.copy_(torch.stack([_t(self.cams[i].viewmat()) for i in idx]))
        self.K.copy_(torch.stack([_t(self.cams[i].K) for i in idx]))
        self.target.copy_(self.targets[list(idx)])

    def step(self):
        c, a, meta = self.tr.render(self.vm, self.K)
        if self.snap_mid:
            self.mid = self.snapshot()
        if self.obs is not None:
            self.obs["frame"].copy_(c.detach())
            self.obs["alphas"].copy_(a.detach())
            self.obs["radii"].copy_(meta["radii"])
            c.register_hook(self._frame_hook)
        loss = self.loss_fn(c[..., :self.loss_channels] if self.loss_channels < 4 else c, self.target)
        if self.obs is not None:
            self.obs["loss"].copy_(loss.detach())
        self.tr.step(loss)

    def snapshot(self):
        """Clones of the fifteen tensors (moments that do not exist yet are zero), the counter and original_index."""
        st = self.opt.state
        z = lambda k, key: st[self.p[k]][key].clone() if key in st[self.p[k]] else torch.zeros_like(self.p[k].detach())
        counter = self.opt.step_state.clone() if self.opt.step_state is not None else torch.zeros(2, dtype=torch.int32, device=DEV)
        return {"p": {k: self.p[k].detach().clone() for k in NAMES}, "m": {k: z(k, "exp_avg") for k in NAMES},
                "v": {k: z(k, "exp_avg_sq") for k in NAMES}, "counter": counter, "index": self.tr.original_index.clone()}


def _assert_scene_conditions(loop):
    """On the oracle's radii of the start scene, all four cameras: the mask checks below can never pass on an empty set."""
    g = loop.scene
    s64, o64 = _activated64(g)
    vis = []
    for cam in loop.cams:
        pr = O.project(g.means, g.quats, s64, _f32(cam.viewmat()), _f32(cam.K), W, H, radius_rule=loop.rule, opacities=o64)
        vis.append(np.asarray(pr["radii"]).reshape(N, -1)[:, 0] > 0)
    invisible = [int((~v).sum()) for v in vis]
    pairs = [(vis[i], vis[(i + 1) % 4]) for i in range(4)]
    entering = [int((~a & b).sum()) for a, b in pairs]
    leaving = [int((a & ~b).sum()) for a, b in pairs]
    neither = [int((~a & ~b).sum()) for a, b in pairs]
    print(f"\nscene ({loop.rule}): invisible per camera {invisible}; from one camera to the next entering {entering}, leaving {leaving}; "
          f"invisible to both of a consecutive pair {neither}")
    assert min(invisible) >= 100 and min(leaving) >= 100 and min(neither) >= 30


def _same_bits(a, b, rows=None):
    return all(torch.equal(a[part][k] if rows is None else a[part][k][rows], b[part][k] if rows is None else b[part][k][rows])
               for part in ("p", "m", "v") for k in NAMES)


def _check_step(loop, what, cam_idx, pre, post):
    """Links 1-5 of one step.  pre: the state the step rendered from and updated (after a reorder, if one fell in this
    step); post: the state it left; the observations are read from loop.obs.  Returns the worst ratio per link."""
    deg, rule = loop.deg, loop.rule
    obs = {k: v.detach().cpu() for k, v in loop.obs.items()}
    cpu = lambda s: {part: {k: s[part][k].cpu() for k in NAMES} for part in ("p", "m", "v")}
    pre_c, post_c = cpu(pre), cpu(post)
    P = {k: pre_c["p"][k].numpy() for k in NAMES}
    g = Gaussians(P["means"], P["scales"], P["quats"], P["opacities"], P["colors"][:, 0], P["colors"][:, 1:])
    s64, o64 = _activated64(g)
    worst = {}

    # ---- 1 frame, 2 visibility -----------------------------------------------------------------------------------------
    frame_ratio, flips_all, dr_all = 0.0, [], []
    gpu_p = pre["p"]
    for j, ci in enumerate(cam_idx):
        cam = loop.cams[ci]
        vm64, K64 = _f32(cam.viewmat()), _f32(cam.K)
        ref, ref_alpha, rmeta = O.render(g.means, g.quats, s64, o64, g.sh_coeffs, vm64, K64, W, H, sh_degree=deg,
                                         render_mode=MODE, margins=True, flip_eps=O.EPS_PATH, radius_rule=rule)
        st = O.check_frame(obs["frame"][j].numpy(), obs["alphas"][j].numpy(), ref, ref_alpha, rmeta["margins"], O.EPS_PATH,
                           rmeta["edge_mask"], expected_depth=True, what=f"{what} camera {ci}", flip_weight=rmeta["flip_weight"],
                           feat_max=rmeta["feat_max"], require_flip_bound=True)
        assert st["unexplained"] == 0 and st["flip_over_bound"] == 0
        frame_ratio = max(frame_ratio, st["max_err_over_tol_nonflip"], st["max_flip_err_over_bound"])
        # the allowance of test_raw_projection_matches_oracle, for every camera of the batch
        radii = obs["radii"][j].numpy().reshape(N, -1)
        ref_radii = np.asarray(rmeta["radii"]).reshape(N, -1)
        vis_ref, vis = ref_radii[:, 0] > 0, radii[:, 0] > 0
        assert ((radii > 0).all(1) == (radii > 0).any(1)).all()
        flips = int((vis_ref != vis).sum())
        both = vis_ref & vis
        dr = np.abs(radii[both] - ref_radii[both]).max(axis=1)
        flips_all.append(flips)
        dr_all.append(int((dr > 0).sum()))
        assert flips <= max(1, N // 5000), f"{what} camera {ci}: {flips} visibility flips of {N}"
        assert dr.max() <= 1 and (dr > 0).sum() <= max(1, N // 2000), f"{what} camera {ci}: radius mismatches {(dr > 0).sum()} (max {dr.max()})"
        # the same parameters rendered for this camera alone report the same rows, bit for bit
        with torch.no_grad():
            solo = rasterization(gpu_p["means"], gpu_p["quats"], gpu_p["scales"], gpu_p["opacities"], gpu_p["colors"],
                                 _t(cam.viewmat())[None].to(DEV), _t(cam.K)[None].to(DEV), W, H, **loop.tr.raster_kwargs)[2]["radii"]
        assert torch.equal(solo[0].cpu(), obs["radii"][j]), f"{what} camera {ci}: the step's radii are not this camera's"
    worst["frame"] = frame_ratio
    visible = _visible(obs["radii"]).any(0)
    n_inv = int((~visible).sum())
    assert 0 < n_inv < N

    # ---- 3 loss at the GPU's own frame -----------------------------------------------------------------------------------
    ch = loop.loss_channels
    x = obs["frame"][..., :ch].double().requires_grad_(True)
    y = loop.targets[list(cam_idx)].double()
    loss = float(obs["loss"])
    if ch == 3:                                          # l1_ssim_loss(colors[..., :3], target, 0.2)
        v = S.l1_ssim_torch(x, y, 0.2)
        v.backward()
        v = float(v.detach())
        assert abs(loss - v) <= 1e-5 * abs(v), (what, loss, v)                              # test_gpu_ssim.py's bound on the value
        _check_grad(obs["v_frame"][..., :3], x.grad, what)
        assert not obs["v_frame"][..., 3].any(), what     # the channel the loss does not read
        worst["loss"] = abs(loss - v) / (1e-5 * abs(v))
        worst["d loss"] = float((obs["v_frame"][..., :3].double() - x.grad).abs().max()) / (1e-5 * float(x.grad.abs().max()))
    else:                                                # l1_loss on the four-channel frame: plain fp64 L1
        v = (x - y).abs().mean()
        v.backward()
        v = float(v.detach())
        assert abs(loss - v) <= 2e-6 * max(1.0, v), (what, loss, v)                         # test_fused_l1_loss_matches_torch's
        torch.testing.assert_close(obs["v_frame"].double(), x.grad, rtol=1e-6, atol=0)
        worst["loss"] = abs(loss - v) / (2e-6 * max(1.0, v))
        rel = (obs["v_frame"].double() - x.grad).abs() / x.grad.abs().clamp(min=1e-300)
        worst["d loss"] = float(rel[x.grad != 0].max()) / 1e-6
    assert math.isfinite(loss) and float(x.grad.abs().max()) > 0

    # ---- 4 gradients: loss = <w, frame>, w the GPU's own cotangent, summed over the step's cameras -------------------------
    r = {"means": _d(g.means, True), "quats": _d(g.quats, True), "scales": _d(P["scales"], True),
         "opacities": _d(P["opacities"], True), "colors": _d(P["colors"], True)}
    total = 0.0
    budgets = {k: 0.0 for k in NAMES}
    f32 = lambda m: np.asarray(m, dtype=np.float32)
    for j, ci in enumerate(cam_idx):
        cam = loop.cams[ci]
        wr = obs["v_frame"][j].double().numpy()
        img, _, _ = OT.render(r["means"], r["quats"], torch.exp(r["scales"]), torch.sigmoid(r["opacities"]), r["colors"],
                              _d(f32(cam.viewmat())), _d(f32(cam.K)), W, H, sh_degree=deg, render_mode=MODE, radius_rule=rule)
        total = total + (img * _d(wr)).sum()
        info = oracle_budgets(g, f32(cam.viewmat()), f32(cam.K), W, H, deg, MODE, wr, np.zeros((H, W)), O.EPS_PATH_GRAD,
                              radius_rule=rule)
        bud = info["budget"]
        b = parameter_budgets(g, f32(cam.viewmat()), f32(cam.K), W, H, deg, True, bud, radius_rule=rule)
        b["scales"] = b["scales"] * s64                       # |d s / d log_s| = s
        b["opacities"] = bud[:, 3] * o64 * (1.0 - o64)         # |d o / d x| = o (1 - o)
        for k in NAMES:
            budgets[k] = budgets[k] + b[k]
    total.backward()
    worst["gradients"] = 0.0
    for k in NAMES:
        ref = r[k].grad.numpy()
        st = compare(f"{what} v_{k}", obs["g_" + k], ref if ref.ndim > 1 else ref.reshape(-1, 1), row_tol=5e-3, bad_frac=1e-2,
                     cos_min=0.999, budget=budgets[k], verbose=False)
        worst["gradients"] = max(worst["gradients"], st["worst_ratio"])
        assert float(np.abs(ref).max()) > 0, k

    # ---- 5 update ------------------------------------------------------------------------------------------------------
    t = int(pre["counter"][0]) + 1
    assert post["counter"].tolist() == [t, 0], (what, pre["counter"].tolist(), post["counter"].tolist())
    assert _same_bits(pre_c, post_c, rows=~visible), f"{what}: a row no camera of the step saw has changed"
    b1, b2 = loop.opt.betas
    worst.update({"m'": 0.0, "v'": 0.0, "p'": 0.0})
    for group in loop.opt.param_groups:
        k = group["name"]
        p0, m0, v0, grad = pre_c["p"][k], pre_c["m"][k], pre_c["v"][k], obs["g_" + k]
        lr = A.scheduled_lr(group["lr"], group["lr_final"], group["decay_steps"], t)
        rates = torch.full((p0[0].numel(),), lr, dtype=torch.float64)
        if group["head_floats"]:
            rates[group["head_floats"]:] *= group["rest_lr_scale"]
        rates = rates.reshape(p0.shape[1:])
        m64, v64 = A.moments64(m0, v0, grad, b1, b2)
        gm, gv, gp = post_c["m"][k], post_c["v"][k], post_c["p"][k]
        d64 = A.update64(gm, gv, t, rates, b1, b2, loop.opt.eps)
        p64 = p0.double() - d64
        for name, err, bound in (("m'", (gm.double() - m64).abs(), A.first_moment_bound(m0, grad, b1)),
                                 ("v'", (gv.double() - v64).abs(), A.second_moment_bound(v64)),
                                 ("p'", (gp.double() - p64).abs(), A.param_bound(p64, d64))):
            err, bound = err[visible], bound[visible]
            worst[name] = max(worst[name], _ratio(err, bound))
            assert int((err > bound).sum()) == 0, f"{what} {k} {name}: {int((err > bound).sum())} elements over their bound (update {t})"
        assert float(d64[visible].abs().max()) > 0, k
    print(f"{what} cameras {list(cam_idx)} update {t}: visible {int(visible.sum())} invisible {n_inv}; oracle flips {flips_all} "
          f"radius mismatches {dr_all}; worst ratio to the gate: " + ", ".join(f"{k} {v:.3f}" for k, v in worst.items()))
    return worst


def _report(case, rows):
    keys = list(rows[0])
    print(f"{case}: worst ratio over the run: " + ", ".join(f"{k} {max(r[k] for r in rows):.3f}" for k in keys))


def test_eager_loop_with_reorders_is_held_to_fp64_at_every_step():
    """Case A.  Raw parameters, sh_degree 2, RGB+ED, l1_ssim_loss(colors[..., :3], target, 0.2), a selective GaussianAdam over
    splatfacto_groups(decay_steps=4) with eps 1e-15, Trainer(auto_reorder_every=3): seven eager steps, one camera per step
    cycling through the ring of four.  Reorders fall at steps 0, 3 and 6 and the decay ends inside the run.  Links 1-5 at
    every step; parameters, moments and original_index are the pre-render ones mapped through last_order, bit for bit,
    exactly in the steps that reorder.  A second run of the same seven steps without any hook gives the same bits."""
    from robosimgs_amd import l1_ssim_loss
    make = lambda hooks: _Loop(2, 1, lambda c, y: l1_ssim_loss(c, y, 0.2), 3, hooks=hooks, groups_kw=dict(decay_steps=4),
                               auto_reorder_every=3)
    loop = make(True)
    _assert_scene_conditions(loop)
    loop.snap_mid = True
    rows, reordered_at = [], []
    for s in range(7):
        loop.set_cameras([s % 4])
        torch.cuda.synchronize()
        before, reorders = loop.snapshot(), loop.tr.reorders
        loop.step()
        torch.cuda.synchronize()
        after, mid = loop.snapshot(), loop.mid
        if loop.tr.reorders > reorders:
            assert loop.tr.reorders == reorders + 1
            order = loop.tr.last_order
            moved = int((order != torch.arange(N, device=DEV)).sum())
            print(f"\nA step {s}: Morton reorder, {moved} of {N} rows moved")
            reordered_at.append(s)
            mapped = {part: {k: before[part][k][order] for k in NAMES} for part in ("p", "m", "v")}
            assert _same_bits(mid, mapped), f"step {s}: the reorder did not carry every tensor"
            assert torch.equal(mid["index"], before["index"][order])
        else:
            assert _same_bits(mid, before) and torch.equal(mid["index"], before["index"])
        assert torch.equal(after["index"], mid["index"]) and torch.equal(mid["counter"], before["counter"])
        rows.append(_check_step(loop, f"A step {s}", [s % 4], mid, after))
    assert reordered_at == [0, 3, 6] and loop.opt.steps_taken() == 7
    assert torch.equal(loop.tr.in_original_order(loop.tr.original_index), torch.arange(N, device=DEV))
    _report("A", rows)
    bare = make(False)
    for s in range(7):
        bare.set_cameras([s % 4])
        bare.step()
    torch.cuda.synchronize()
    assert _same_bits(bare.snapshot(), loop.snapshot()) and torch.equal(bare.tr.original_index, loop.tr.original_index)
    assert torch.equal(bare.opt.step_state, loop.opt.step_state)


def test_captured_loop_replayed_with_fresh_cameras_is_held_to_fp64_at_every_replay():
    """Case B.  The same scene with sh_degree 3, radius_rule="opacity_aware" (radii [C,N,2]), l1_loss on the four-channel
    frame, two cameras per step behind a fixed isect_capacity: warmed up and captured on one side stream, replayed six
    times.  View matrices, K and targets live in static tensors; before each replay the next camera pair and its targets
    are copied into them, and links 1, 2 and 4 use THAT pair -- a graph that baked the capture-time cameras in fails at the
    first replay.  Links 1-5 after every replay."""
    from robosimgs_amd import l1_loss
    loop = _Loop(3, 2, l1_loss, 4, radius_rule="opacity_aware", isect_capacity=40_000, auto_reorder_every=500)
    _assert_scene_conditions(loop)
    pair = lambda r: [r % 4, (r + 1) % 4]
    loop.set_cameras(pair(0))
    # warm-up and capture on ONE side stream (see test_trainer_steps_a_selective_gaussian_adam_inside_a_hip_graph)
    side = torch.cuda.Stream(DEV)
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        for _ in range(3):                       # the first render reorders (Morton), allocations settle
            loop.step()
        torch.cuda.synchronize()
        assert loop.tr.reorders == 1 and loop.opt.steps_taken() == 3
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph, stream=side):
            loop.step()
    torch.cuda.synchronize()
    assert loop.opt.steps_taken() == 3                                   # capturing ran nothing
    index = loop.tr.original_index.clone()
    rows = []
    for r in range(6):
        cams = pair(r + 1)                       # never the capture-time pair twice in a row; the first replay differs from it
        loop.set_cameras(cams)
        torch.cuda.synchronize()
        before = loop.snapshot()
        graph.replay()
        torch.cuda.synchronize()
        after = loop.snapshot()
        assert loop.tr.reorders == 1 and torch.equal(after["index"], index)
        rows.append(_check_step(loop, f"B replay {r}", cams, before, after))
    assert loop.opt.steps_taken() == 9 and int(loop.tr.last_meta["isect_status"].max()) == 0
    _report("B", rows)
