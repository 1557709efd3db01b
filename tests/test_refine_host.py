"""The refinement's boundary without a GPU: include/mgs_refine.h <-> libmgs.so / libmgs_debug.so <-> the third ctypes table
(_lib.REFINE_EXPORTS), the argument checks of the three entry points, the fp64 reference's own identities
(tests/mcmc_ref.py), MCMCStrategy's host arithmetic, and Trainer(strategy=None)."""
import ctypes
import math
import os
import re
import subprocess

import numpy as np
import pytest
import torch

import mcmc_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "mgs_refine.h")


def _code():
    return re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)


def _declared():
    decls = re.findall(r"\b(?:int|void|size_t|const char \*)\s*\*?\s*(mgs_\w+)\s*\(([^;]*?)\)\s*;", _code(), flags=re.S)
    return {name: 0 if args.strip() == "void" else len([a for a in args.split(",") if a.strip()]) for name, args in decls}


def test_refine_header_symbols_are_exported_and_bound_in_both_libraries():
    from robosimgs_amd import _lib
    decl = _declared()
    assert sorted(decl) == sorted(_lib.REFINE_EXPORTS) == ["mgs_mcmc_noise", "mgs_mcmc_relocate", "mgs_mcmc_weights"]
    assert not set(_lib.REFINE_EXPORTS) & (set(_lib.EXPORTS) | set(_lib.OPTIM_EXPORTS))
    for L in (_lib.lib(), _lib.debug_lib()):
        for name, nargs in decl.items():
            assert len(getattr(L, name).argtypes) == nargs, name
    nm = lambda path: subprocess.run(["nm", "-D", "--defined-only", path], capture_output=True, text=True).stdout
    for path in (_lib.LIB_PATH, _lib.DEBUG_LIB_PATH):
        assert all(name in nm(path) for name in decl), path
    define = lambda name: int(re.search(rf"#define\s+{name}\s+(\d+)", _code()).group(1))
    assert define("MGS_MCMC_RELOCATE") == _lib.MCMC_RELOCATE == R.RELOCATE == 0
    assert define("MGS_MCMC_ADD") == _lib.MCMC_ADD == R.ADD == 1
    assert define("MGS_MCMC_MAX_RATIO") == _lib.MCMC_MAX_RATIO == R.MAX_RATIO == 51
    assert define("MGS_REFINE_MAX_GROUPS") == _lib.REFINE_MAX_GROUPS == _lib.ADAM_MAX_GROUPS
    assert "MGS_VERSION" not in _code()                                   # the version is mgs.h's alone


@pytest.mark.parametrize("struct,ctype,offsets,size", [
    ("mgs_refine_group", "RefineGroup", [0, 8, 16, 24], 32),
    ("mgs_mcmc_stats", "McmcStats", [0, 8, 12], 16),
])
def test_structs_match_the_header(struct, ctype, offsets, size):
    """The ctypes structures have the header's fields, in its order, at a C compiler's offsets."""
    from robosimgs_amd import _lib
    body = re.search(rf"typedef struct {struct} \{{(.*?)\}} {struct};", _code(), flags=re.S).group(1)
    names = [re.search(r"(\w+)\s*$", d).group(1) for d in body.split(";") if d.strip()]
    S = getattr(_lib, ctype)
    assert names == [f[0] for f in S._fields_]
    assert [getattr(S, n).offset for n in names] == offsets and ctypes.sizeof(S) == size


def _relocate(mode=0, n=10, n_new=0, capacity=16, opacities=0x1000, scales=0x2000, groups="one", n_groups=None,
              min_opacity=0.005, u=0x3000, w=0x4000, dead=0x5000, stats=0x6000, sources=0x7000, workspace=0x10000, **group):
    """mgs_mcmc_relocate on made-up addresses: every case here must be refused before anything is launched."""
    from robosimgs_amd import _lib
    L = _lib.lib()
    if groups == "one":
        f = dict(param=0x8000, exp_avg=0x9000, exp_avg_sq=0xa000, row_floats=3)
        f.update(group)
        groups = [_lib.RefineGroup(**f)]
    table = (_lib.RefineGroup * len(groups))(*groups) if groups else None
    nbytes = ctypes.c_size_t(1 << 30)
    rc = L.mgs_mcmc_relocate(mode, n, n_new, capacity, opacities, scales, (len(groups) if groups else 1) if n_groups is None
                             else n_groups, table, min_opacity, u, w, dead, stats, sources, workspace, ctypes.byref(nbytes), None)
    return rc, L.mgs_last_error_string()


@pytest.mark.parametrize("kw,word", [
    (dict(groups=None), b"groups is null"),
    (dict(n_groups=9), b"n_groups"),
    (dict(mode=1, n=10, n_new=7, capacity=16), b"does not fit capacity"),
    (dict(capacity=9), b"capacity"),
    (dict(mode=2), b"mode"),
    (dict(min_opacity=0.0), b"min_opacity"),
    (dict(min_opacity=1.0), b"min_opacity"),
    (dict(min_opacity=-0.5), b"min_opacity"),
    (dict(opacities=0x1004), b"opacities is not 16-byte aligned"),
    (dict(w=0x4008), b"w is not 16-byte aligned"),
    (dict(param=0x8004), b"groups[0].param"),
    (dict(exp_avg=0x9008), b"exp_avg "),
    (dict(exp_avg_sq=0xa00c), b"exp_avg_sq"),
    (dict(exp_avg=None), b"one moment"),
    (dict(row_floats=0), b"row_floats"),
    (dict(capacity=1 << 30, row_floats=4), b"2^32"),
    (dict(u=None), b"null"),
    (dict(workspace=0x10010), b"256-byte"),
])
def test_relocate_argument_errors_are_reported_without_a_gpu(kw, word):
    rc, msg = _relocate(**kw)
    assert rc == -1 and word in msg, (rc, msg)


def test_size_queries_and_the_other_two_entry_points_check_their_arguments():
    from robosimgs_amd import _lib
    L = _lib.lib()
    nbytes = ctypes.c_size_t(0)
    # the size queries launch nothing: n rows of cdf (8 B), live and draw counts (4 B each), targets (4 B), block records
    assert L.mgs_mcmc_weights(4099, None, 0.005, 0, None, None, None, None, ctypes.byref(nbytes), None) == 0
    assert 16 * 4099 <= nbytes.value <= 16 * 4099 + 5 * 256 + 16 * 5
    assert L.mgs_mcmc_relocate(1, 4099, 300, 5000, None, None, 0, None, 0.005, None, None, None, None, None, None,
                               ctypes.byref(nbytes), None) == 0
    assert 16 * 4099 + 4 * 300 <= nbytes.value <= 16 * 4099 + 4 * 300 + 5 * 256 + 16 * 5
    assert L.mgs_mcmc_relocate(1, 4099, 902, 5000, None, None, 0, None, 0.005, None, None, None, None, None, None,
                               ctypes.byref(nbytes), None) == -1 and b"capacity" in L.mgs_last_error_string()
    for args, word in (((10, 0x1000, 1.5, 0, 0x2000, 0x3000, 0x4000, 0x10000), b"min_opacity"),
                       ((10, 0x1004, 0.005, 0, 0x2000, 0x3000, 0x4000, 0x10000), b"opacities"),
                       ((-1, 0x1000, 0.005, 0, 0x2000, 0x3000, 0x4000, 0x10000), b"n -1"),
                       ((10, 0x1000, 0.005, 0, 0x2000, None, 0x4000, 0x10000), b"null")):
        nbytes = ctypes.c_size_t(1 << 30)
        assert L.mgs_mcmc_weights(*args, ctypes.byref(nbytes), None) == -1 and word in L.mgs_last_error_string(), args
    noise = dict(n=10, means=0x1000, quats=0x2000, scales=0x3000, opacities=0x4000, z=0x5000, noise_lr=5e5, lr=1e-4,
                 lr_final=1e-6, decay_steps=100, step_state=0x6000)
    for kw, word in ((dict(means=0x1004), b"means is not 16-byte aligned"), (dict(z=0x5008), b"z is not"),
                     (dict(quats=None), b"null"), (dict(lr_final=0.0), b"lr_final"), (dict(lr=0.0), b"schedule"),
                     (dict(lr=-1.0, decay_steps=0), b"lr"), (dict(decay_steps=-1), b"decay_steps"),
                     (dict(noise_lr=-1.0), b"noise_lr"), (dict(n=1 << 30), b"n ")):
        a = dict(noise, **kw)
        assert L.mgs_mcmc_noise(*a.values(), None) == -1 and word in L.mgs_last_error_string(), kw
    assert L.mgs_mcmc_noise(*dict(noise, n=0).values(), None) == 0            # nothing to do: nothing launched


@pytest.mark.parametrize("o", [0.005, 0.006, 0.3, 0.5, 0.9, 0.999, 1 - 2.0 ** -23, 1 - 2.0 ** -24])
def test_reference_single_sum_equals_the_double_sum(o):
    """sum_{i=k+1..r} C(i-1, k) = C(r, k+1) (the hockey stick): the r-term sum the kernel evaluates is gsplat's double
    loop, to 1e-12 relative for every r <= 51 and every opacity a source can have (o <= 1 - 2^-23, the clamp).  Both are
    summed exactly (fsum) from terms that carry up to four roundings each (the power, the square root, the product, the
    division), so they may differ by 2^-51 times the condition number: that bound holds everywhere, also at
    o = 1 - 2^-24, beyond the clamp, where the condition number reaches 4e4 and the two sums differ by 1.1e-12."""
    worst = 0.0
    for r in range(1, R.MAX_RATIO + 1):
        o_new = -math.expm1(math.log1p(-o) / r)
        D2, mag2 = R.denominator_double_sum(o_new, r)
        D1, mag1, _ = R.denominator_single_sum(o_new, r)
        assert D2 > 0 and (o > R.O_MAX or abs(D1 / D2 - 1) <= 1e-12), (o, r, D1, D2)
        assert abs(D1 / D2 - 1) <= 2.0 ** -51 * mag2 / D2 + 2.0 ** -52
        worst = max(worst, mag2 / D2)
    assert worst < 5e4
    if o == 1 - 2.0 ** -24:
        assert worst > 3e4                       # the ill-conditioned corner is really in the cases


def test_reference_r_1_is_the_identity_and_the_clamps_hold():
    for logit in (-5.0, -0.3, 0.0, 2.5, 9.0):
        ref = R.relocated(np.float32(logit), 0, 0.005)
        o = float(R.sigmoid(np.float32(logit)))
        assert ref["r"] == 1 and ref["o_new"] == pytest.approx(o, rel=1e-15) and ref["D"] == pytest.approx(o, rel=1e-15)
        assert abs(ref["shift"]) <= 1e-15 and ref["logit"] == pytest.approx(float(np.float32(logit)), abs=2.0 ** -51 / (1 - o))  # 1 - o is formed in fp64
    hot = R.relocated(np.float32(30.0), 0, 0.005)             # o = 1.0f: the source clamp
    assert hot["o"] == R.O_MAX and hot["kept"] == R.O_MAX and math.isfinite(hot["shift"])
    many = R.relocated(np.float32(-5.0), 1000, 0.005)         # r clamps at 51, the new opacity at min_opacity
    assert many["r"] == 51 and many["o_new"] < 0.005 and many["kept"] == 0.005
    # (1 - o_new)^r = 1 - o: r copies at o_new cover what the source covered
    for count in (1, 2, 50):
        ref = R.relocated(np.float32(1.0), count, 0.005)
        assert (1 - ref["o_new"]) ** ref["r"] == pytest.approx(1 - ref["o"], rel=1e-13)


def test_reference_sampling_picks_the_bucket_and_never_a_zero_weight():
    w = np.array([0, 0.5, 0, 0, 0.25, 0.25, 0], dtype=np.float32)
    u = np.array([0.0, 0.49, 0.5, 0.74, 0.75, np.nextafter(np.float32(1), np.float32(0))], dtype=np.float32)
    idx, margin, total = R.sample(w, u)
    assert idx.tolist() == [1, 1, 4, 4, 5, 5] and total == 1.0
    assert margin[0] == 0.5 and margin[2] == 0.0               # u = 0: the exact lower edge does not count; 0.5 sits on one


def test_n_after_is_host_arithmetic_and_saturates():
    from robosimgs_amd import MCMCStrategy
    s = MCMCStrategy(cap_max=3000, refine_every=5, refine_start_iter=0, refine_stop_iter=10**6)
    n, want = 2000, []
    for step in range(1, 101):                     # `step` steps done: step numbers 0 .. step - 1
        if (step - 1) % 5 == 0 and step - 1 > 0:
            n = min(3000, math.floor(1.05 * n))
        want.append(n)
    assert [s.n_after(k, 2000) for k in range(1, 101)] == want
    assert want[4] == 2000 and want[5] == 2100 and want[10] == 2205 and want[-1] == 3000 and s.n_after(0, 2000) == 2000
    assert s.grown(2999) == 3000 and s.grown(3000) == 3000 and s.grown(10) == 10 and s.grown(20) == 21
    d = MCMCStrategy(cap_max=10**6)                # gsplat's defaults: every 100 from 600 to 24 900
    assert not d.due(500) and d.due(600) and d.due(24900) and not d.due(25000) and not d.due(650)
    assert d.n_after(600, 1000) == 1000 and d.n_after(601, 1000) == 1050 and d.n_after(701, 1000) == 1102
    assert d.n_after(10**9, 1000) == d.n_after(25000, 1000)
    n = 1000
    for _ in range(244):
        n = min(10**6, math.floor(1.05 * n))
    assert d.n_after(10**9, 1000) == n == 10**6
    with pytest.raises(Exception, match="initialize"):
        d.n_after(10)
    with pytest.raises(ValueError):
        MCMCStrategy(cap_max=0)
    with pytest.raises(ValueError):
        MCMCStrategy(cap_max=10, min_opacity=1.0)


def _cpu_params(n=7):
    return {"means": torch.zeros(n, 3), "quats": torch.ones(n, 4), "scales": torch.zeros(n, 3),
            "opacities": torch.zeros(n), "colors": torch.zeros(n, 4, 3)}


def test_strategy_is_exported_lazily_and_refuses_activated_params_and_cpu_tensors():
    import robosimgs_amd
    from robosimgs_amd import MCMCStrategy
    from robosimgs_amd._lib import MgsError
    assert MCMCStrategy is robosimgs_amd.strategy.MCMCStrategy
    s = MCMCStrategy(cap_max=10)
    with pytest.raises(MgsError, match="raw"):
        s.initialize(_cpu_params(), None, raw_params=False)
    with pytest.raises(MgsError, match="CPU tensor"):
        s.initialize(_cpu_params(), None)
    with pytest.raises(KeyError):
        s.initialize({"means": torch.zeros(3, 3)}, None)

    class _Trainer:
        raw_params, it, params, optimizer = False, 1, _cpu_params(), None
    with pytest.raises(MgsError, match="raw"):
        s.step(_Trainer())
    _Trainer.raw_params = True
    with pytest.raises(MgsError, match="CPU tensor"):
        s.step(_Trainer())


def test_trainer_without_a_strategy_takes_the_same_trajectory_and_with_one_calls_it_after_each_step():
    """The CPU loop of test_training_host.py (a toy, permutation-equivariant render function in fp64): strategy=None is
    bit for bit the trainer without the argument, and a strategy object is stepped once per step, after the optimiser,
    with the step count already advanced."""
    from robosimgs_amd.training import Trainer
    n = 300

    def make():
        g = torch.Generator().manual_seed(3)
        P = {"means": torch.randn(n, 3, generator=g, dtype=torch.float64), "quats": torch.randn(n, 4, generator=g, dtype=torch.float64),
             "scales": torch.rand(n, 3, generator=g, dtype=torch.float64), "opacities": torch.rand(n, generator=g, dtype=torch.float64),
             "colors": torch.randn(n, 4, 3, generator=g, dtype=torch.float64)}
        return {k: v.requires_grad_(True) for k, v in P.items()}

    def toy_render(means, quats, scales, opacities, colors, viewmats, Ks, width, height, gain=1.0):
        w = torch.sigmoid(means @ viewmats[0, :3, :3].T).sum(-1) * opacities
        img = (w[:, None] * colors[:, 0] * scales).sum(0) * gain + (quats ** 2).sum()
        return img[None], w.sum()[None], {"n": means.shape[0]}

    vm = torch.eye(4, dtype=torch.float64)[None]
    target = torch.tensor([0.3, -0.2, 0.9], dtype=torch.float64)

    class Recorder:
        def __init__(self):
            self.calls = []

        def step(self, trainer):
            self.calls.append((trainer.it, trainer.params["means"].grad is None,
                               trainer.params["means"].detach().clone()))

    def run(**kw):
        P = make()
        tr = Trainer(P, torch.optim.Adam(P.values(), lr=1e-2), 4, 4, auto_reorder_every=3, render_fn=toy_render, gain=2.0, **kw)
        for _ in range(8):
            c, a, _m = tr.render(vm, None)
            tr.step((c[0] - target).abs().sum() + 0.1 * a.sum())
        return tr, P

    plain, A = run()
    none, B = run(strategy=None)
    rec = Recorder()
    with_rec, C = run(strategy=rec)
    assert plain.strategy is None and none.strategy is None and with_rec.strategy is rec
    for k in Trainer.KEYS:
        assert torch.equal(A[k], B[k]) and torch.equal(A[k], C[k]), k
    assert torch.equal(plain.original_index, none.original_index) and plain.reorders == none.reorders == 3
    assert [c[0] for c in rec.calls] == list(range(1, 9)) and all(c[1] for c in rec.calls)
    assert torch.equal(rec.calls[-1][2], C["means"].detach())              # called after the last optimiser step
