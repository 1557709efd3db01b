"""MCMCStrategy / mgs_mcmc_* on the GPU (include/mgs_refine.h, csrc/refine.hip).

The reference is never the code under test: tests/mcmc_ref.py states the three operations in NumPy fp64.  Bounds are
rounding analysis with u = 2^-24 (one fp32 rounding), written next to each use or in mcmc_ref.py next to the quantity.

Sizes: 1, 5, 257 and 4099; 1025, one more than the scan's block of 1024 Gaussians; 262145 = 1024 * 256 + 1, the smallest
count whose block sums need a second round (the carry) of the one-workgroup scan over them."""
import math

import numpy as np
import pytest
import torch

import mcmc_ref as R
from mcmc_ref import U
from robosimgs_amd import GaussianAdam, MCMCStrategy, Trainer, camera_ring, rasterization, splatfacto_groups, synthetic_scene
from robosimgs_amd import _lib
from robosimgs_amd.strategy import KEYS, mcmc_noise, mcmc_relocate, mcmc_weights

pytestmark = pytest.mark.gpu
DEV = "cuda"
MIN_O = 0.005
THRESHOLD = math.log(MIN_O / (1 - MIN_O))          # the logit of min_opacity
SIZES = [1, 5, 257, 1025, 4099, 262145]
SHAPES = {"means": (3,), "quats": (4,), "scales": (3,), "opacities": (), "colors": (4, 3)}
GUARD = 8                                          # rows of 0xA5 behind `capacity`


def _logits(n, seed, max_dead=600):
    """logits ~ N(-1, 3) as fp32, none within 1e-3 of the threshold (fp32 and fp64 then agree on who is dead: the
    activation's 4u relative is 2e-7 in the logit), at most max_dead of them dead (the others mirrored to the live side)."""
    x = np.random.default_rng(seed).normal(-1.0, 3.0, n).astype(np.float32)
    x[np.abs(x - THRESHOLD) < 1e-3] += np.float32(0.01)
    dead = np.flatnonzero(x < THRESHOLD)
    if len(dead) > max_dead:
        keep = dead[:: len(dead) // max_dead + 1]
        mirror = np.setdiff1d(dead, keep)
        x[mirror] = -x[mirror]
    return x


def _scene(n, capacity, seed, logits=None):
    """-> (storage, moments, full): the five tensors of `capacity` rows (n of them in use) and their moments, every one a
    view of a tensor of capacity + GUARD rows whose last rows are 0xA5 bytes.  The moments are non-zero everywhere."""
    gen = torch.Generator().manual_seed(seed)
    storage, moments, full = {}, {}, []

    def guarded(values):
        t = torch.empty((capacity + GUARD, *values.shape[1:]), dtype=torch.float32)
        t.view(-1).view(torch.uint8).fill_(0xA5)
        t[:capacity] = values
        t = t.to(DEV)
        full.append(t)
        return t[:capacity]

    for k, tail in SHAPES.items():
        v = torch.randn((capacity, *tail), generator=gen)
        if k == "scales":
            v = v * 0.5 + math.log(0.05)
        if k == "opacities" and logits is not None:
            v[:n] = torch.from_numpy(np.asarray(logits, dtype=np.float32))
        storage[k] = guarded(v)
        moments[k] = (guarded(torch.randn((capacity, *tail), generator=gen) * 1e-2 + 0.5),
                      guarded(torch.rand((capacity, *tail), generator=gen) * 1e-3 + 1e-4))
    return storage, moments, full


def _snapshot(storage, moments, full):
    return ({k: v.clone() for k, v in storage.items()}, {k: (m.clone(), v.clone()) for k, (m, v) in moments.items()},
            [t.clone() for t in full])


def _guards_intact(full, capacity):
    return all(bool((t[capacity:].reshape(-1).view(torch.uint8) == 0xA5).all()) for t in full)


# ---- 1. dead list and weights ----------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", [R.RELOCATE, R.ADD])
@pytest.mark.parametrize("n", SIZES)
def test_weights_and_dead_list(n, mode):
    """The dead list is the fp64 reference's, ascending, and its count is on the device; w is exactly 0 on dead rows in
    relocate mode; elsewhere |w - sigmoid64| <= 4u sigmoid64: expf (1 ulp = 2u), the sum 1 + e and the division (u each).
    T is the fp64 sum of the stored w to n 2^-53 T (at most n additions of non-negative numbers, in whatever order)."""
    x = _logits(n, 10 + n, max_dead=10**9)
    w64, dead64, o64 = R.weights(x, MIN_O, mode)
    assert float(np.abs(o64 / MIN_O - 1).min()) > 8 * U                    # nobody within the activation's error of dead
    s = mcmc_weights(torch.from_numpy(x).to(DEV), MIN_O, mode)
    total, n_dead, n_live = s.counts()
    assert n_dead == len(dead64)
    got_dead = s.dead[:n_dead].cpu().numpy()
    assert got_dead.dtype == np.int32 and np.array_equal(got_dead, dead64)
    w = s.w[:n].cpu().numpy()
    if mode == R.RELOCATE:
        assert not w[dead64].any() and n_live == n - n_dead
    rel = np.abs(w.astype(np.float64) - w64) / np.where(w64 > 0, w64, 1.0)
    print(f"weights n={n} mode={mode}: {n_dead} dead, worst error {rel.max() / U:.2f} u of 4 u")
    assert float(rel.max()) <= 4 * U
    assert n_live == int((w > 0).sum())
    exact = math.fsum(w.astype(np.float64))
    assert abs(total - exact) <= n * 2.0 ** -53 * exact


# ---- 2. sampling -----------------------------------------------------------------------------------------------------
def _check_sources(w, u, sources, n, what):
    """sources == searchsorted(cumsum(w64), u T, 'right'), after asserting that no sample sits within n 2^-52 T of a
    bucket edge (the two cumulative sums differ by the order of at most n additions: n 2^-53 T each)."""
    idx, margin, total = R.sample(w, u)
    print(f"{what}: {len(u)} samples, T = {total:.6g}, smallest margin {margin.min() / total:.3e} T "
          f"({margin.min() / (n * 2.0 ** -52 * total):.3g} x the bound)")
    assert float(margin.min()) > n * 2.0 ** -52 * total, what
    assert np.array_equal(sources.astype(np.int64), idx), what
    assert bool((w[idx] > 0).all())


@pytest.mark.parametrize("mode", [R.RELOCATE, R.ADD])
@pytest.mark.parametrize("n", SIZES)
def test_sampled_sources_are_bit_equal_to_searchsorted(n, mode):
    rng = np.random.default_rng(n % 7 + 2)
    x = _logits(n, 20 + n, max_dead=200 if n > 100_000 else 600)
    n_new = 0 if mode == R.RELOCATE else (200 if n > 100_000 else max(1, n // 10))
    storage, moments, full = _scene(n, n + n_new, 30 + n, x)
    u = rng.random(n if mode == R.RELOCATE else n_new, dtype=np.float32)
    s = mcmc_relocate(mode, n, n_new, storage, moments, MIN_O, torch.from_numpy(u).to(DEV))
    total, n_dead, n_live = s.counts()
    targets = n_dead if mode == R.RELOCATE else n_new
    assert n_dead == int((x < THRESHOLD).sum())
    if targets == 0 or n_live == 0:
        assert n <= 5                                                     # only the smallest cases may be empty
        return
    _check_sources(s.w[:n].cpu().numpy(), u[:targets], s.sources[:targets].cpu().numpy(), n, f"n={n} mode={mode}")
    assert _guards_intact(full, n + n_new)


def test_sampling_edge_cases():
    """u = 0 draws the first row of positive weight; u = nextafter(1, 0) the last one (u T is 2^-24 T short of T, the last
    weight here is a hundred times that); one live row among 60 dead is drawn 60 times and its ratio clamps at 51."""
    n = 64
    x = np.full(n, 0.3, dtype=np.float32)
    x[:3] = -9.0                                     # dead head
    x[-4:] = -9.0                                    # dead tail: the last positive row is n - 5
    x[20] = -9.0
    for u_value, want in ((np.float32(0.0), 3), (np.nextafter(np.float32(1), np.float32(0)), n - 5)):
        storage, moments, full = _scene(n, n, 1, x)
        u = np.full(n, u_value, dtype=np.float32)
        s = mcmc_relocate(R.RELOCATE, n, 0, storage, moments, MIN_O, torch.from_numpy(u).to(DEV))
        total, n_dead, n_live = s.counts()
        assert (n_dead, n_live) == (8, 56)
        w = s.w[:n].cpu().numpy()
        assert float(w[n - 5]) > 100 * 2.0 ** -24 * total
        assert s.sources[:8].cpu().tolist() == [want] * 8
        ref = R.relocated(x[want], 8, MIN_O)
        assert abs(float(R.sigmoid(storage["opacities"][want].cpu().numpy())) - ref["kept"]) <= R.relocated_bounds(ref, 0.0)[0]
    x = np.full(61, -9.0, dtype=np.float32)
    x[17] = 1.5
    storage, moments, full = _scene(61, 61, 2, x)
    before = storage["scales"][17].cpu().numpy().astype(np.float64)
    s = mcmc_relocate(R.RELOCATE, 61, 0, storage, moments, MIN_O, torch.rand(61, device=DEV))
    assert s.counts()[1:] == (60, 1) and s.sources[:60].cpu().tolist() == [17] * 60
    ref = R.relocated(x[17], 60, MIN_O)
    assert ref["r"] == 51
    o_bound, s_bound = R.relocated_bounds(ref, before)
    got_o = R.sigmoid(storage["opacities"].cpu().numpy())
    assert np.all(got_o == got_o[17]) and abs(got_o[17] - ref["kept"]) <= o_bound      # all 61 rows are the source's now
    got_s = storage["scales"].cpu().numpy().astype(np.float64)
    assert np.all(got_s == got_s[17]) and np.all(np.abs(np.expm1(got_s[17] - (before + ref["shift"]))) <= s_bound)
    assert _guards_intact(full, 61)


@pytest.mark.parametrize("case", ["no dead row", "no live row", "no new row"])
def test_nothing_to_do_leaves_every_buffer_bitwise_unchanged(case):
    n, cap = 257, 300
    x = np.abs(_logits(n, 3)) if case != "no live row" else np.full(n, -7.5, dtype=np.float32)
    storage, moments, full = _scene(n, cap, 4, x)
    _, _, before = _snapshot(storage, moments, full)
    mode, n_new = (R.ADD, 0) if case == "no new row" else (R.RELOCATE, 0)
    s = mcmc_relocate(mode, n, n_new, storage, moments, MIN_O, torch.rand(n, device=DEV))
    total, n_dead, n_live = s.counts()
    assert (n_dead, n_live) == ((n, 0) if case == "no live row" else (0, n))
    assert (total == 0.0) == (case == "no live row")
    for a, b in zip(full, before):
        assert torch.equal(a.view(-1).view(torch.int32), b.view(-1).view(torch.int32)), case


# ---- 3. relocated values ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("r", [1, 2, 3, 51])
@pytest.mark.parametrize("o", [0.006, 0.5, 0.999, 1.0])
def test_relocated_opacity_and_scale_match_fp64(o, r):
    """One live row of opacity o among r - 1 dead rows (60 for the clamp at 51): it is drawn by every one of them.  The
    new opacity sigmoid(stored logit) and the new scales exp(stored log-scale) against mcmc_ref.relocated, within
    mcmc_ref.relocated_bounds: the reference's own condition number of D, D's sensitivity to an fp32 powf in o_new, and
    the fp32 roundings of what is stored.  o = 1.0 is a logit of 20: sigmoid rounds to 1.0f, the source clamp applies.
    r = 1 is a row nobody drew: it keeps its bits (o_new = o, s_new = s)."""
    n_dead = 60 if r == 51 else r - 1
    n = n_dead + 1
    live = n // 2
    x = np.full(n, -9.0, dtype=np.float32)
    x[live] = np.float32(20.0) if o == 1.0 else np.float32(math.log(o / (1 - o)))
    storage, moments, full = _scene(n, n, 40 + r, x)
    before_s = storage["scales"][live].cpu().numpy()
    before_o = storage["opacities"][live].cpu().numpy()
    s = mcmc_relocate(R.RELOCATE, n, 0, storage, moments, MIN_O, torch.rand(n, device=DEV))
    assert s.counts()[1:] == (n_dead, 1)
    got_logit = storage["opacities"][live].cpu().numpy()
    got_s = storage["scales"][live].cpu().numpy()
    if r == 1:
        assert got_logit.tobytes() == before_o.tobytes() and got_s.tobytes() == before_s.tobytes()
        ref = R.relocated(x[live], 0, MIN_O)
        assert ref["r"] == 1 and abs(ref["shift"]) <= 1e-15
        return
    ref = R.relocated(x[live], n_dead, MIN_O)
    assert ref["r"] == r
    o_bound, s_bound = R.relocated_bounds(ref, before_s.astype(np.float64))
    err_o = abs(float(R.sigmoid(got_logit)) - ref["kept"])
    err_s = np.abs(np.expm1(got_s.astype(np.float64) - (before_s.astype(np.float64) + ref["shift"])))
    print(f"o={o} r={r}: cond(D) {ref['cond']:.3g}, o_new {ref['o_new']:.6g} kept {ref['kept']:.6g}: error "
          f"{err_o:.3e} of {o_bound:.3e} ({err_o / o_bound:.3f}); scales {err_s.max():.3e} of {s_bound.min():.3e} "
          f"({(err_s / s_bound).max():.3f})")
    assert err_o <= o_bound
    assert bool((err_s <= s_bound).all())
    assert MIN_O - o_bound <= float(R.sigmoid(got_logit)) <= R.O_MAX + o_bound


# ---- 4. bookkeeping --------------------------------------------------------------------------------------------------
def _bits(t):
    return t.contiguous().view(-1).view(torch.int32)


@pytest.mark.parametrize("mode", [R.RELOCATE, R.ADD])
@pytest.mark.parametrize("n", [257, 4099])
def test_bookkeeping_of_rows_and_moments(n, mode):
    """Targets are bitwise copies of their sources' updated rows in all five tensors; relocate zeroes the sources'
    moments and leaves the dead rows' alone, add zeroes the new rows' and leaves the sources' alone; a row that is neither
    keeps every bit (a source changes in opacity and scale only); the guard rows behind `capacity` are 0xA5; a second run
    from the same bits gives the same bits."""
    n_new = 0 if mode == R.RELOCATE else n // 10
    cap = n + n_new + 13                               # rows [n + n_new, cap) exist and are nobody's
    x = _logits(n, 50 + n)
    u = torch.rand(max(n, n_new), generator=torch.Generator().manual_seed(n)).to(DEV)
    runs = []
    for _ in range(2):
        storage, moments, full = _scene(n, cap, 60 + n, x)
        p0, m0, _ = _snapshot(storage, moments, full)
        s = mcmc_relocate(mode, n, n_new, storage, moments, MIN_O, u)
        total, n_dead, n_live = s.counts()
        targets = s.dead[:n_dead].long() if mode == R.RELOCATE else torch.arange(n, n + n_new, device=DEV)
        sources = s.sources[:len(targets)].long()
        assert len(targets) > 10 and int(sources.min()) >= 0 and int(sources.max()) < n
        runs.append((storage, moments, sources.clone()))
    (storage, moments, sources), second = runs
    drawn = torch.zeros(cap, dtype=torch.bool, device=DEV)
    drawn[sources] = True
    target = torch.zeros(cap, dtype=torch.bool, device=DEV)
    target[targets] = True
    assert not bool((drawn & target).any())
    other = ~(drawn | target)
    for k in KEYS:
        p, (m, v) = storage[k], moments[k]
        assert torch.equal(_bits(p[targets]), _bits(p[sources])), k
        assert torch.equal(_bits(p[other]), _bits(p0[k][other])), k
        changed = k in ("opacities", "scales")
        assert torch.equal(_bits(p[drawn]), _bits(p0[k][drawn])) != changed, k
        for got, was in ((m, m0[k][0]), (v, m0[k][1])):
            assert torch.equal(_bits(got[other]), _bits(was[other])), k
            if mode == R.RELOCATE:
                assert not bool(got[drawn].any()) and torch.equal(_bits(got[target]), _bits(was[target])), k
            else:
                assert not bool(got[target].any()) and torch.equal(_bits(got[drawn]), _bits(was[drawn])), k
        assert torch.equal(_bits(p), _bits(second[0][k])), k
        assert torch.equal(_bits(m), _bits(second[1][k][0])) and torch.equal(_bits(v), _bits(second[1][k][1])), k
    assert torch.equal(sources, second[2])
    assert _guards_intact(full, cap)


# ---- 5. noise --------------------------------------------------------------------------------------------------------
NOISE_LR, LR, LR_FINAL, DECAY = 5e5, 1.6e-4, 1.6e-6, 7


def _noise_inputs(n, seed):
    gen = torch.Generator().manual_seed(seed)
    means = torch.randn(n, 3, generator=gen)
    quats = torch.randn(n, 4, generator=gen) * 3.0                            # un-normalised
    scales = torch.randn(n, 3, generator=gen) * 0.5 + math.log(0.05)
    knee = [0.003, 0.0049, 0.005, 0.0051, 0.008, 0.5]                         # both sides of the gate's knee, and 0.5
    o = torch.tensor([knee[(i + seed) % len(knee)] for i in range(n)], dtype=torch.float64)
    opacities = torch.log(o / (1 - o)).float()
    z = torch.randn(n, 3, generator=gen)
    return means, quats, scales, opacities, z


def _check_noise(before, after, quats, scales, opacities, z, lam, what):
    """|means' - (means + d64)| <= bound(d) + u |means'| per component: mcmc_ref.noise's bound on the displacement and
    the rounding of the final addition."""
    d, gate, bound = R.noise(quats.numpy(), scales.numpy(), opacities.numpy(), z.numpy(), lam)
    want = before.numpy().astype(np.float64) + d
    err = np.abs(after.numpy().astype(np.float64) - want)
    allowed = bound[:, None] + U * np.abs(want)
    print(f"{what}: lambda {lam:.6g}, gate {gate.min():.3g} .. {gate.max():.3g}, |d| up to {np.abs(d).max():.3g}, "
          f"worst error / bound {(err / allowed).max():.3f}")
    assert bool((err <= allowed).all()), what
    return d, gate


@pytest.mark.parametrize("t", [None, 0, 1, DECAY, DECAY + 5])
@pytest.mark.parametrize("n", [1, 5, 257, 4099])
def test_noise_matches_fp64_at_the_rate_of_the_counter(n, t):
    """t = None passes no counter: lambda is the host's noise_lr * lr.  Otherwise the counter of a GaussianAdam is preset
    to t updates taken through load_state_dict, lambda = noise_lr * lr (lr_final / lr)^(min(t, 7) / 7), and the launch
    leaves the counter as it was."""
    means, quats, scales, opacities, z = _noise_inputs(n, 70 + n)
    g = [x.to(DEV) for x in (means, quats, scales, opacities, z)]
    state = None
    if t is not None:
        opt = GaussianAdam([g[0].clone().requires_grad_(True)], lr=LR, lr_final=LR_FINAL, decay_steps=DECAY)
        sd = opt.state_dict()
        sd["step_state"] = torch.tensor([t, 0], dtype=torch.int32)
        opt.load_state_dict(sd)
        state = opt.step_state
        assert state.is_cuda and opt.steps_taken() == t
    mcmc_noise(*g, NOISE_LR, LR, LR_FINAL, DECAY, state)
    lam = NOISE_LR * (LR if t is None else R.next_rate(LR, LR_FINAL, DECAY, t))
    d, gate = _check_noise(means, g[0].cpu(), quats, scales, opacities, z, lam, f"noise n={n} t={t}")
    if n >= 5:
        assert gate.max() > 0.5 and gate.min() < 1e-10 and float(np.abs(d).max()) > 1e-3
    if t is not None:
        assert state.cpu().tolist() == [t, 0]
        assert lam == pytest.approx(NOISE_LR * LR * (LR_FINAL / LR) ** (min(t, DECAY) / DECAY), rel=1e-14)
    for a, b in zip(g[1:], (quats, scales, opacities, z)):
        assert torch.equal(a.cpu(), b)                                      # only the means are written


# ---- 6. replay -------------------------------------------------------------------------------------------------------
def test_replayed_trainer_step_injects_noise_at_the_rate_of_each_replay():
    """One captured Trainer.step (a toy render whose loss does not see the means, GaussianAdam over all five leaves with
    the means' rate decaying over 5 updates, the strategy's noise) replayed four times.  Adam leaves the means alone (no
    gradient), so each replay's displacement of the means is the noise alone: it matches fp64 from the quats, scales
    and opacities as that replay's Adam update left them, the normals that replay drew, and the rate at that replay's
    counter value t = 3, 4, 5, 6 -- a rate frozen at capture would be off by the decay."""
    n = 1237
    means, quats, scales, opacities, _ = _noise_inputs(n, 5)
    p = {"means": means, "quats": quats, "scales": scales, "opacities": opacities,
         "colors": torch.randn(n, 4, 3, generator=torch.Generator().manual_seed(6))}
    p = {k: v.to(DEV).requires_grad_(True) for k, v in p.items()}
    opt = GaussianAdam(splatfacto_groups(p, decay_steps=5))
    strategy = MCMCStrategy(cap_max=n + 100, refine_start_iter=10**6, refine_stop_iter=10**6 + 1)
    p = strategy.initialize(p, opt)

    def toy_render(means, quats, scales, opacities, colors, viewmats, Ks, width, height, **kw):
        img = (colors.sum() + opacities.sum() + scales.sum() + (quats ** 2).sum()).reshape(1, 1, 1, 1)
        return img, img, {}

    tr = Trainer(p, opt, 4, 4, auto_reorder_every=0, render_fn=toy_render, raw_params=True, strategy=strategy)

    def step():
        c, _a, _m = tr.render(None, None)
        tr.step(c.sum() * 1e-3)

    side = torch.cuda.Stream(DEV)
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        for _ in range(2):
            step()
        torch.cuda.synchronize()
        assert opt.steps_taken() == 2 and tr.params["means"].grad is None
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph, stream=side):
            step()
    torch.cuda.synchronize()
    rates = []
    for k in range(4):
        before = tr.params["means"].detach().cpu()
        graph.replay()
        torch.cuda.synchronize()
        t = opt.steps_taken()
        assert t == 3 + k
        rate = R.next_rate(1.6e-4, 1.6e-6, 5, t)
        rates.append(rate)
        now = {k_: tr.params[k_].detach().cpu() for k_ in KEYS}
        d, gate = _check_noise(before, now["means"], now["quats"], now["scales"], now["opacities"], strategy.last_z.cpu(),
                               strategy.noise_lr * rate, f"replay {k} (t = {t})")
        assert float(np.abs(d).max()) > 100 * U * float(before.abs().max())      # the displacement is there to be checked
    assert rates[0] > rates[1] > rates[2] == rates[3] == pytest.approx(1.6e-6, rel=1e-12)
    assert tr.params["means"].data_ptr() == strategy.storage["means"].data_ptr()


# ---- 7. a short loop -------------------------------------------------------------------------------------------------
def test_a_short_training_loop_relocates_grows_and_never_reads_past_n():
    """2 000 Gaussians at 64 x 64, cap_max 3 000, a refinement every 5 steps from step 5 on, 30 steps.  After every step
    the count is n_after(step) (2000, 2100, 2205, 2315, 2430, 2551), everything in use is finite, the storage never
    moves, and -- rows >= n poisoned with NaN before every render -- the frame is finite: nothing reads past n.  At the end
    a render of params[:n] cloned into fresh tensors is the trainer's own, bit for bit."""
    from robosimgs_amd import l1_loss
    n0, cap, W, H = 2000, 3000, 64, 64
    g = synthetic_scene(n0, math.log(0.08), 2, 12)
    cam = camera_ring(1, W, H, thetas=[0.5])[0]
    as_t = lambda a: torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32)).to(DEV)
    vm, K = as_t(cam.viewmat())[None], as_t(cam.K)[None]
    target = torch.rand(1, H, W, 3, device=DEV, generator=torch.Generator(DEV).manual_seed(2))
    t = g.to_torch(DEV, 2, raw=True)
    t["opacities"][::9] = -7.0                                              # some Gaussians are dead from the start
    p = {k: t[k].detach().clone().requires_grad_(True) for k in KEYS}
    opt = GaussianAdam(splatfacto_groups(p))
    strategy = MCMCStrategy(cap_max=cap, refine_every=5, refine_start_iter=0, refine_stop_iter=1000)
    p = strategy.initialize(p, opt)
    tr = Trainer(p, opt, W, H, auto_reorder_every=500, sh_degree=2, isect_capacity=400_000, raw_params=True,
                 strategy=strategy)
    pointers = {k: strategy.storage[k].data_ptr() for k in KEYS}
    counts = []
    for step in range(1, 31):
        n = tr.params["means"].shape[0]
        for k in KEYS:
            strategy.storage[k][n:] = float("nan")
        colors, alphas, meta = tr.render(vm, K)
        assert bool(torch.isfinite(colors).all()) and bool(torch.isfinite(alphas).all()), step
        tr.step(l1_loss(colors, target))
        n = tr.params["means"].shape[0]
        counts.append(n)
        assert n == strategy.n_after(step) == strategy.n, step
        for k in KEYS:
            assert tr.params[k].shape[0] == n and tr.params[k].data_ptr() == pointers[k], (step, k)
            assert strategy.storage[k].data_ptr() == pointers[k]
            assert bool(torch.isfinite(tr.params[k]).all()), (step, k)
            for key in ("exp_avg", "exp_avg_sq"):
                st = opt.state[tr.params[k]][key]
                assert st.shape[0] == n and bool(torch.isfinite(st).all()), (step, k, key)
    assert counts[4] == 2000 and counts[5] == 2100 and counts[-1] == 2551 and strategy.refinements == 5
    assert sorted(set(counts)) == [2000, 2100, 2205, 2315, 2430, 2551]
    assert opt.steps_taken() == 30 and len(opt.state) == 5
    n = counts[-1]
    for k in KEYS:
        strategy.storage[k][n:] = float("nan")
    with torch.no_grad():
        own, own_a, _ = tr.render(vm, K)
        fresh = [tr.params[k].detach().clone() for k in KEYS]
        again, again_a, _ = rasterization(*fresh, vm, K, W, H, sh_degree=2, isect_capacity=400_000, raw_params=True)
    assert torch.equal(own, again) and torch.equal(own_a, again_a) and bool(torch.isfinite(own).all())
