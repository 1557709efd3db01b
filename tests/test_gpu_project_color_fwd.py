"""Stage tests of robosimgs_amd/csrc/projection.hip -- mgs_project_color_fwd, mgs_projection_fwd, mgs_sh_fwd -- against the
fp64 reference of tests/project_color_fwd_ref.py (checked on the CPU by tests/test_project_color_fwd_host.py).

Every row of every launch is held: radii, visibility and the colour clamp's state exactly (no row of any case is within 8 x the
float32 oracle's error of a threshold: the host test asserts it), every output of every visible row at 8 x the family's rounding
floor, every culled row bit for bit.  Beyond the numbers: which rows a launch may write (every output is n + 64 rows long and
prefilled), that the packed records are the arrays of the same launch, that the nullable outputs change nothing in the ones
that stay, the binning seed's sums, and the SH rows' way through LDS when only some rows of a wave are visible.  The launches
go to the C ABI directly, since the ops wrappers allocate their own outputs; test_ops_wrappers_agree ties the wrappers in.
"""
import functools

import numpy as np
import pytest
import torch

import project_color_fwd_ref as FR
import project_color_ref as R

pytestmark = pytest.mark.gpu
DEV = "cuda"
PAD = 64
F = np.float32
BIN_TIGHT, BIN_PER_AXIS, PARAMS_RAW, PARAMS_OPAC_PLAIN = 1, 2, 64, 128


def _t(a):
    return torch.from_numpy(np.array(a, order="C")).to(DEV)


@functools.lru_cache(maxsize=None)
def _prefill(shape, seed=0, integer=False):
    """Finite, non-zero, every entry different: what a launch must leave in place is recognised by its bits."""
    if integer:
        a = (np.int32(0x5A5A0000) + np.arange(int(np.prod(shape)), dtype=np.int32) * np.int32(7 + seed)).reshape(shape)
    else:
        a = (np.random.default_rng(199 + seed).normal(size=shape) * 0.25).astype(F)
        a[a == 0] = 0.125
    a.setflags(write=False)
    return a


def _upload(case):
    d = {k: _t(case[k]) for k in ("means", "quats", "scales", "opac", "sh", "viewmat")}
    d["K"] = _t(R.camera_row(case))
    return d


def opac_form(case, aa):
    return "aa" if aa else ("plain" if case["raw"] else "absent")


def launch(case, deg, rule="classic", *, form="aa", width=4, records=True, seed="tight", lean=False, n=None, near=FR.NEAR,
           far=FR.FAR, clip=0.0, with_opacities=True, dev=None):
    """One mgs_project_color_fwd launch on the first n rows.  form: opac_out "absent" | "aa" | "plain" (kept plain: raw only).
    Every output is n + PAD rows long and prefilled.  Returns {name: numpy of n + PAD rows} and "_pre", the prefills."""
    from robosimgs_amd import _lib, ops
    from robosimgs_amd._lib import check, ptr, stream_handle
    d = dev or _upload(case)
    n = case["means"].shape[0] if n is None else n
    m, per_axis = n + PAD, rule == "opacity_aware"
    pre = {"depths": _prefill((m,), 1)}
    if not lean:
        pre.update(radii=_prefill((m,), 2, True), means2d=_prefill((m, 2), 3), conics=_prefill((m, 3), 4), feats=_prefill((m, width), 5))
        if per_axis:
            pre["radii_y"] = _prefill((m,), 6, True)
    if form != "absent":
        pre["opac_out"] = _prefill((m,), 7)
    if records:
        pre["record"] = _prefill((m, 12), 8)
    if seed is not None:
        pre["bin_info"], pre["bin_sums"] = _prefill((m, 2), 9, True), _prefill((-(-n // 64) + PAD,), 10, True)
    out = {k: _t(v) for k, v in pre.items()}
    flags = ((BIN_TIGHT if seed == "tight" else 0) | (BIN_PER_AXIS if per_axis else 0) | ops.camera_bin_flags(R.CAMERA_ID[case["model"]])
             | (PARAMS_RAW if case["raw"] else 0) | (PARAMS_OPAC_PLAIN if form == "plain" else 0))
    g = lambda k: ptr(out.get(k))
    check(_lib.lib().mgs_project_color_fwd(
        n, ptr(d["means"]), ptr(d["quats"]), ptr(d["scales"]), ptr(d["opac"]) if with_opacities else None, deg, d["sh"].shape[1],
        ptr(d["sh"]), ptr(d["viewmat"]), ptr(d["K"]), FR.W, FR.H, FR.EPS2D, near, far, clip, g("radii"), g("means2d"), g("depths"),
        g("conics"), g("opac_out"), width, g("feats"), g("record"), flags, g("bin_info"), g("bin_sums"), g("radii_y"),
        stream_handle()), "mgs_project_color_fwd")
    torch.cuda.synchronize()
    res = {k: v.cpu().numpy() for k, v in out.items()}
    res["_pre"] = pre
    return res


def launch_run(run, **kw):
    case = run["case"]
    kw.setdefault("form", opac_form(case, run["aa"]))
    kw.setdefault("width", 4 if run["with_depth"] else 3)
    return launch(case, run["deg"], run["rule"], near=run["near"], far=run["far"], clip=run["radius_clip"], **kw)


def check_launch(name, ref, out, n, what, form, full=None):
    """The whole contract of one launch against the float64 reference `ref` (FR.forward): rows past n untouched; radii,
    visibility, clamp state exact; visible rows inside the gates; culled rows bit for bit; the records are this launch's own
    arrays; the seed's words.  form: "absent" | "aa" | "plain", what the launch was given for opac_out.  full: the arrays of the full form, for a launch that leaves some out."""
    pre = out["_pre"]
    assert ("opac_out" in out) == (form != "absent"), f"{what}: opac_out against the form {form}"
    for k, p in pre.items():
        rows = n if k != "bin_sums" else -(-n // 64)
        assert np.array_equal(out[k][rows:].view(np.int32), p[rows:].view(np.int32)), f"{what} {k}: written past its {rows} rows"
    vis = ref["vis"][:n]
    got = {k: out[k][:n] for k in ("radii", "radii_y", "means2d", "depths", "conics", "opac_out", "feats") if k in out}
    if "radii" not in got:                                   # lean: the decisions are read off the records' rows
        got["radii"] = ref["radii"][:n]
    ratios = FR.hold_rows(name, ref, got, what, rows=n)
    src = dict(full or {}, **{k: v for k, v in out.items() if not k.startswith("_")})
    if "record" in out:
        rec, p = out["record"][:n], pre["record"][:n]
        assert np.array_equal(FR.bits(rec[~vis]), FR.bits(p[~vis])), f"{what}: the record of a culled row was written"
        v = np.flatnonzero(vis)
        op = src["opac_out"][v] if "opac_out" in src else None
        want = np.zeros((len(v), 12), F)
        want[:, 0:2], want[:, 2:5], want[:, 6:9] = src["means2d"][v], src["conics"][v], src["feats"][v, :3]
        want[:, 9] = src["depths"][v] if ref["settings"]["with_depth"] else 0
        cols = [c for c in range(12) if c != 5 or op is not None]
        if op is not None:
            want[:, 5] = op
        assert np.array_equal(FR.bits(rec[v][:, cols]), FR.bits(want[:, cols])), f"{what}: a record is not the arrays of its launch"
        if op is None:                                       # opac_out absent: the record holds the activated opacity itself
            e = FR.row_error("comp", rec[v, 5], ref["opacity"][v])
            assert e.size == 0 or e.max() <= FR.gate(name, "comp"), f"{what}: the record's opacity"
    if "bin_info" in out:
        info, sums = out["bin_info"][:n].view(np.uint32), out["bin_sums"][: -(-n // 64)].view(np.uint32)
        assert (info[~vis, 0] == FR.EMPTY_WORD).all() and not info[~vis, 1].any(), f"{what}: the seed of a culled row"
        per_wave = np.add.reduceat(info[:, 1].astype(np.uint64), np.arange(0, n, 64))
        assert np.array_equal(per_wave, sums.astype(np.uint64)), f"{what}: seed sums"
    return ratios


# ---------------------------------------------------------------------------------------------------------------------
# a. the instantiation sweep
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mu", R.SWEEP_MU)
@pytest.mark.parametrize("raw", [False, True])
@pytest.mark.parametrize("model", R.CAMERAS)
def test_instantiation_sweep(model, raw, mu):
    """n = 333, degree 3 at stride 16 (the staged fetch): camera x raw x anti-aliased x both radius rules."""
    tag = f"{model}-{'raw' if raw else 'act'}-{mu} "
    runs = [r for r in FR.family("sweep") if r["label"].startswith(tag)]
    assert len(runs) == 4
    dev = _upload(runs[0]["case"])
    for run in runs:
        out = launch_run(run, dev=dev)
        check_launch("sweep", FR.reference(run), out, 333, f"sweep {run['label']}", opac_form(run["case"], run["aa"]))


@pytest.mark.parametrize("deg,stride", [(0, 1), (1, 4), (2, 9), (3, 20), (2, 16), (0, 16), (1, 16)])
def test_degrees_and_strides(deg, stride):
    """Degrees 0..2 at their own strides, degree 3 unstaged (stride 20), and the stride-16 rows at the degrees below 3 (degree 2
    staged; degrees 0 and 1 never are)."""
    for raw in (False, True):
        case = FR.sweep_case("pinhole", raw, 0.1, stride, deg)
        for run in FR._both(f"pinhole-{raw}-deg{deg}-stride{stride}", case, deg):
            out = launch_run(run)
            check_launch("sweep", FR.reference(run), out, 333, f"sweep {run['label']}", opac_form(case, run["aa"]))


# ---------------------------------------------------------------------------------------------------------------------
# b. the families
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", FR.FAMILIES[1:])
def test_families(name):
    """Every run of the family; cull_margin / cull_exact: the rows either side of (and on) each threshold come out as the
    reference decides; sparse_waves: the NaN coefficient rows of culled Gaussians reach no output."""
    worst = {}
    for run in FR.family(name):
        ref = FR.reference(run)
        out = launch_run(run)
        n = len(ref["vis"])
        for k, v in check_launch(name, ref, out, n, f"{name} {run['label']}", opac_form(run["case"], run["aa"])).items():
            worst[k] = max(worst.get(k, 0.0), v)
        for k, v in out.items():
            if not k.startswith("_") and v.dtype == F:
                assert np.isfinite(v).all(), f"{name} {run['label']} {k}: not finite"
        if name == "sparse_waves":
            assert np.array_equal(out["radii"][:n] > 0, FR.sparse_keep(run))
        if name == "cull_exact":
            for row, visible in FR.EXACT_EXPECT:
                assert (out["radii"][row] > 0) == visible, (run["label"], row)
    print(f"PCF-worst {name} " + " ".join(f"{k}={v:.2f}" for k, v in worst.items()))


# ---------------------------------------------------------------------------------------------------------------------
# c. output forms of one case
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("rule", FR.RULES)
def test_output_forms(rule):
    """One case (a third of its rows culled), raw parameters: feats 3 / 4 wide, opac_out absent / anti-aliased / kept plain,
    with / without records, seeded tight / classic / not at all, lean.  Every array a form writes is bit-identical to the full
    form's of the same anti-aliasing (full: 4 wide, records, tight seed)."""
    case = FR.mixed_case()
    n, dev = 257, _upload(FR.mixed_case())
    for aa in (True, False):
        forms = ("aa",) if aa else ("plain", "absent")
        ref = FR.forward(case, 3, aa, True, rule)
        assert 60 < (~ref["vis"]).sum() < 120
        full = launch(case, 3, rule, form=forms[0], dev=dev)
        check_launch("sweep", ref, full, n, f"forms {rule} full {forms[0]}", forms[0])
        for form in forms:
            for width in (4, 3):
                for records in (True, False):
                    for seed in ("tight", "classic", None):
                        for lean in (False, True):
                            if lean and not (records and seed):
                                continue
                            if lean and form == "plain":
                                continue                      # (kept plain is the training form: never lean)
                            what = f"forms {rule} {form} width={width} records={records} seed={seed} lean={lean}"
                            out = launch(case, 3, rule, form=form, width=width, records=records, seed=seed, lean=lean, dev=dev)
                            r = ref if width == 4 else FR.forward(case, 3, aa, False, rule)
                            f3 = dict({k: v for k, v in full.items() if not k.startswith("_")}, feats=full["feats"][:, :width])
                            check_launch("sweep", r, out, n, what, form, full=f3)
                            same = ["radii", "radii_y", "means2d", "depths", "conics"] + (["opac_out"] if form == forms[0] else [])
                            if seed == "tight":
                                same += ["bin_info", "bin_sums"]
                            for k in same:
                                if k in out and k in full:
                                    rows = n if k != "bin_sums" else -(-n // 64)
                                    assert np.array_equal(out[k][:rows].view(np.int32), full[k][:rows].view(np.int32)), f"{what}: {k}"
                            if "feats" in out:
                                assert np.array_equal(FR.bits(out["feats"][:n, :3]), FR.bits(full["feats"][:n, :3])), what
                            if "record" in out and form == forms[0]:
                                cols = [c for c in range(12) if c != 9 or width == 4]
                                v = ref["vis"]
                                assert np.array_equal(FR.bits(out["record"][:n][v][:, cols]), FR.bits(full["record"][:n][v][:, cols])), what


# ---------------------------------------------------------------------------------------------------------------------
# d. row ownership
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [1, 63, 64, 65, 257])
def test_row_ownership(n):
    """The first n rows of one case: rows n .. n + 63 of every output keep their prefill, bin_sums has exactly ceil(n / 64) words
    written, and they are the sums of the seed's per-row counts (all inside check_launch)."""
    case = FR.mixed_case()
    dev = _upload(case)
    for rule in FR.RULES:
        for aa, form in ((True, "aa"), (False, "plain")):
            ref = FR.forward(case, 3, aa, True, rule)
            for seed in ("tight", "classic"):
                out = launch(case, 3, rule, form=form, seed=seed, n=n, dev=dev)
                check_launch("sweep", ref, out, n, f"ownership n={n} {rule} {form} {seed}", form)
            out = launch(case, 3, rule, form="aa" if aa else "absent", seed="tight", lean=True, n=n, dev=dev)
            check_launch("sweep", ref, out, n, f"ownership n={n} {rule} lean", "aa" if aa else "absent",
                         full={k: v for k, v in launch(case, 3, rule, form="aa" if aa else "absent", n=n, dev=dev).items() if not k.startswith("_")})


# ---------------------------------------------------------------------------------------------------------------------
# e. mgs_projection_fwd
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [1, 65, 257])
def test_projection_fwd(n):
    """The unfused projection on the projection-stage case: with / without compensations, classic and per-axis (radii_y),
    with / without opacities under the per-axis rule; the same gates and ownership.  (Against the fused kernel bit for bit:
    test_projection_fwd_is_the_fused_kernel_bit_for_bit.)"""
    from robosimgs_amd import _lib
    from robosimgs_amd._lib import check, ptr, stream_handle
    case = FR.projection_case()
    dev = _upload(case)
    m = n + PAD
    for rule in FR.RULES:
        for comp in (False, True):
            for with_op in ((True, False) if rule == "opacity_aware" else (False,)):
                what = f"projection_fwd n={n} {rule} comp={comp} opacities={with_op}"
                pre = {"radii": _prefill((m,), 2, True), "means2d": _prefill((m, 2), 3), "depths": _prefill((m,), 1),
                       "conics": _prefill((m, 3), 4)}
                if comp:
                    pre["comp"] = _prefill((m,), 7)
                if rule == "opacity_aware":
                    pre["radii_y"] = _prefill((m,), 6, True)
                out = {k: _t(v) for k, v in pre.items()}
                g = lambda k: ptr(out.get(k))
                check(_lib.lib().mgs_projection_fwd(
                    n, ptr(dev["means"]), ptr(dev["quats"]), ptr(dev["scales"]), ptr(dev["viewmat"]), ptr(dev["K"]), FR.W, FR.H, FR.EPS2D,
                    FR.NEAR, FR.FAR, 0.0, g("radii"), g("means2d"), g("depths"), g("conics"), g("comp"), ptr(dev["opac"]) if with_op else None,
                    FR.RULE_ID[rule], g("radii_y"), 0, stream_handle()), "mgs_projection_fwd")
                torch.cuda.synchronize()
                res = {k: v.cpu().numpy() for k, v in out.items()}
                for k, p in pre.items():
                    assert np.array_equal(res[k][n:].view(np.int32), p[n:].view(np.int32)), f"{what} {k}: rows past n"
                ref = FR.forward(case, 0, comp, True, rule, has_opacity=with_op)
                FR.hold_rows("sweep", ref, {k: v[:n] for k, v in res.items()}, what, rows=n)


def test_projection_fwd_is_the_fused_kernel_bit_for_bit():
    """mgs_projection_fwd against mgs_project_color_fwd on the same inputs, bit for bit (anti-aliased <=> compensations; without
    opacities the fused kernel can write neither opac_out nor records nor a tight seed): both call project_gaussian with the
    same arguments.  What keeps that true: csrc/mgs_math.h MGS_FP_CONTRACT_IN_EXPRESSION (profiles/project_color_fwd/README.md)."""
    from robosimgs_amd import _lib
    from robosimgs_amd._lib import check, ptr, stream_handle
    case, n = FR.projection_case(), 257
    dev = _upload(case)
    bad = []
    for rule in FR.RULES:
        for comp in (False, True):
            for with_op in ((True, False) if rule == "opacity_aware" else (False,)):
                out = {"radii": torch.zeros(n, dtype=torch.int32, device=DEV), "means2d": torch.zeros(n, 2, device=DEV),
                       "depths": torch.zeros(n, device=DEV), "conics": torch.zeros(n, 3, device=DEV)}
                if comp:
                    out["comp"] = torch.zeros(n, device=DEV)
                if rule == "opacity_aware":
                    out["radii_y"] = torch.zeros(n, dtype=torch.int32, device=DEV)
                g = lambda k: ptr(out.get(k))
                check(_lib.lib().mgs_projection_fwd(
                    n, ptr(dev["means"]), ptr(dev["quats"]), ptr(dev["scales"]), ptr(dev["viewmat"]), ptr(dev["K"]), FR.W, FR.H, FR.EPS2D,
                    FR.NEAR, FR.FAR, 0.0, g("radii"), g("means2d"), g("depths"), g("conics"), g("comp"), ptr(dev["opac"]) if with_op else None,
                    FR.RULE_ID[rule], g("radii_y"), 0, stream_handle()), "mgs_projection_fwd")
                torch.cuda.synchronize()
                res = {k: v.cpu().numpy() for k, v in out.items()}
                if with_op or rule == "classic":
                    fused = launch(case, 0, rule, form="aa" if comp else "absent", dev=dev)
                else:
                    fused = launch(case, 0, rule, form="absent", records=False, seed=None, with_opacities=False, dev=dev)
                if comp and "opac_out" in fused:        # opacities are 1: the fused opac_out IS the compensation
                    fused["comp"] = fused["opac_out"]
                for k in ("radii", "radii_y", "means2d", "depths", "conics", "comp"):
                    if k in res and k in fused:
                        a, b = res[k].view(np.int32).reshape(n, -1), fused[k][:n].view(np.int32).reshape(n, -1)
                        rows = np.flatnonzero((a != b).any(1))
                        if len(rows):
                            bad.append(f"{rule} comp={comp} opacities={with_op} {k}: {len(rows)} rows (first {rows[:4]}), up to "
                                       f"{np.abs(a.astype(np.int64) - b).max()} ulp")
    print("PCF projection_fwd against the fused kernel:", bad)
    assert not bad, bad


# ---------------------------------------------------------------------------------------------------------------------
# f. mgs_sh_fwd
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [1, 64, 65, 257])
def test_sh_fwd(n):
    """SH_STRIDES x n against fp64 at the colour gate: directions of every length, a zero-length direction (the basis at the
    zero vector: C0 x coeff_0, and from degree 2 on Y_6's constant), masked rows exactly zero whatever their coefficients are
    (NaN included), rows past n untouched."""
    from robosimgs_amd import _lib
    from robosimgs_amd._lib import check, ptr, stream_handle
    dirs, coeffs, _ = R.sh_case(257)
    dirs = dirs[:n].copy()
    dirs[n // 2] = 0.0
    gate = FR.GATE_FACTOR * FR.FWD_FLOORS["sh_stage"]["colour"]
    assert gate <= FR.CEILING["colour"]
    d_dirs = _t(dirs)
    for deg, stride in R.SH_STRIDES:
        co = np.zeros((n, stride, 3), F)
        co[:, :min(stride, 16)] = coeffs[:n, :stride]
        for name in ("no mask", "all", "none", "alternating", "last"):
            m = {"no mask": None, "all": np.ones(n, bool), "none": np.zeros(n, bool), "alternating": np.arange(n) % 2 == 0,
                 "last": np.arange(n) == n - 1}[name]
            c = co.copy()
            if m is not None:
                c[~m] = np.nan
            pre = _prefill((n + PAD, 3), 11)
            out = _t(pre)
            d_c, d_m = _t(c), None if m is None else _t(m.astype(np.uint8))
            check(_lib.lib().mgs_sh_fwd(n, deg, stride, ptr(d_dirs), ptr(d_c), ptr(d_m), ptr(out), stream_handle()), "mgs_sh_fwd")
            torch.cuda.synchronize()
            got = out.cpu().numpy()
            what = f"sh_fwd n={n} deg={deg} stride={stride} {name}"
            assert np.array_equal(FR.bits(got[n:]), FR.bits(pre[n:])), f"{what}: rows past n"
            live = np.ones(n, bool) if m is None else m
            assert np.array_equal(FR.bits(got[:n][~live]), FR.bits(np.zeros(((~live).sum(), 3), F))), f"{what}: masked rows"
            assert np.isfinite(got[:n]).all(), what
            if live.any():
                want = FR.sh_colors(deg, dirs, c, m)
                e = FR.row_error("colour", got[:n][live], want[live])
                print(f"PCF sh_stage colour {e.max():.3e} gate {gate:.2e} [{what}]")
                assert e.max() <= gate, f"{what}: off by {e.max():.3e} > {gate:.2e}"
            if live[n // 2]:
                z = 0.2820947917738781 * c[n // 2, 0].astype(np.float64)
                if deg >= 2:
                    z = z - 0.3153915652525201 * c[n // 2, 6].astype(np.float64)
                assert np.abs(got[n // 2] - z).max() <= gate * np.abs(z).max(), f"{what}: the zero-length direction"


def test_ops_wrappers_agree():
    """ops.project_color_fwd_raw, ops.projection_fwd_raw and ops.spherical_harmonics return, bit for bit, what the direct calls
    above wrote."""
    from robosimgs_amd import ops
    case = FR.mixed_case()
    d = _upload(case)
    for per_axis in (False, True):
        rule = FR.RULES[per_axis]
        for aa in (False, True):
            direct = launch(case, 3, rule, form="aa" if aa else "plain", dev=d)
            radii, means2d, depths, conics, opac, feats, splats, seed = ops.project_color_fwd_raw(
                d["means"], d["quats"], d["scales"], d["opac"], 3, d["sh"], d["viewmat"], d["K"], FR.W, FR.H, FR.EPS2D, FR.NEAR, FR.FAR,
                0.0, aa, True, want_splats=True, bin_seed="tight", per_axis=per_axis, camera=0, raw=True)
            torch.cuda.synchronize()
            rr = radii.cpu().numpy()
            vis = direct["radii"][:257] > 0
            assert np.array_equal(rr[0] if per_axis else rr, direct["radii"][:257])
            if per_axis:
                assert np.array_equal(rr[1], direct["radii_y"][:257])
            for k, v in (("means2d", means2d), ("depths", depths), ("conics", conics), ("opac_out", opac), ("feats", feats)):
                assert np.array_equal(FR.bits(v.cpu().numpy()), FR.bits(direct[k][:257])), (rule, aa, k)
            assert np.array_equal(FR.bits(splats.cpu().numpy()[vis]), FR.bits(direct["record"][:257][vis]))
            assert np.array_equal(seed[0].cpu().numpy(), direct["bin_info"][:257]) and np.array_equal(seed[1].cpu().numpy(), direct["bin_sums"][:5])
    pc = FR.projection_case()
    dp = _upload(pc)
    radii, means2d, depths, conics, comp = ops.projection_fwd_raw(dp["means"], dp["quats"], dp["scales"], dp["viewmat"], dp["K"], FR.W,
                                                                  FR.H, FR.EPS2D, FR.NEAR, FR.FAR, 0.0, True)
    torch.cuda.synchronize()
    ref = FR.forward(pc, 0, True, True, "classic", has_opacity=False)
    FR.hold_rows("sweep", ref, {"radii": radii.cpu().numpy(), "means2d": means2d.cpu().numpy(), "depths": depths.cpu().numpy(),
                                "conics": conics.cpu().numpy(), "comp": comp.cpu().numpy()}, "ops.projection_fwd_raw")
    dirs, coeffs, _ = R.sh_case(257)
    got = ops.spherical_harmonics(3, _t(dirs), _t(coeffs)).cpu().numpy()
    e = FR.row_error("colour", got, FR.sh_colors(3, dirs, coeffs))
    assert e.max() <= FR.GATE_FACTOR * FR.FWD_FLOORS["sh_stage"]["colour"]
