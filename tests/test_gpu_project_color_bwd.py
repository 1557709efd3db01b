"""Stage tests of robosimgs_amd/csrc/backward.hip -- mgs_project_color_bwd, mgs_projection_bwd, mgs_sh_bwd -- against the
fp64 reference of tests/project_color_ref.py (checked on the CPU by tests/test_project_color_bwd_host.py).

The fused backward takes radii, conics and feats as inputs: every test feeds it the reference's own forward products rounded
to fp32, so kernel and reference decide visibility and clamping from identical bits and EVERY row is held
(grad_gate.compare with bad_frac=0) at 8 x the family's rounding floor (project_color_ref.FLOORS); nothing here is sized for
alpha-threshold flips.  What is checked beyond the numbers: which rows and columns a launch may write (tails, invisible
rows, padding columns, rows past n), overwrite against accumulate, and the wave reduction of the camera-pose gradient.
"""
import functools

import numpy as np
import pytest
import torch

import project_color_ref as R
from grad_gate import compare

pytestmark = pytest.mark.gpu
DEV = "cuda"
PAD = 64                 # rows every output is allocated past n; they must come back bit-identical
F = np.float32


def _t(a):
    return torch.from_numpy(np.array(a, order="C")).to(DEV)        # (a copy: the cached prefills are read-only)


def _bits(a):
    return np.ascontiguousarray(a, dtype=F).view(np.int32)


@functools.lru_cache(maxsize=None)
def _prefill(shape, seed=0):
    """Finite, non-zero, every entry different: what a launch must leave in place is recognised by its bits."""
    a = (np.random.default_rng(99 + seed).normal(size=shape) * 0.25).astype(F)
    a[a == 0] = 0.125
    a.setflags(write=False)
    return a


def _upload(case, stride=None):
    c = case if stride is None else R.with_stride(case, stride)
    d = {k: _t(c[k]) for k in ("means", "quats", "scales", "opac", "sh", "viewmat")}
    d["K"] = _t(R.camera_row(c))
    d["camera"], d["raw"], d["n"] = R.CAMERA_ID[c["model"]], c["raw"], c["means"].shape[0]
    return d


def run_fused(d, deg, aa, radii, conics, feats, ct, accumulate=False, view=None, v_depths=None, n=None):
    """One mgs_project_color_bwd launch on the first n rows of the uploaded case `d`.  Outputs are n + PAD rows long and
    prefilled; view: the [4,4] prefill of v_viewmat, or None for a launch without it.  Returns ({name: numpy}, prefill)."""
    from robosimgs_amd import ops
    n = d["n"] if n is None else n
    stride = d["sh"].shape[1]
    pre = {"v_means": _prefill((n + PAD, 3), 1), "v_quats": _prefill((n + PAD, 4), 2), "v_scales": _prefill((n + PAD, 3), 3),
           "v_sh": _prefill((n + PAD, stride, 3), 4), "v_opacities": _prefill((n + PAD,), 5)}
    out = {k: _t(v) for k, v in pre.items()}
    vv = None if view is None else _t(np.asarray(view, dtype=F))
    cut = lambda x: None if x is None else _t(np.asarray(x)[:n])
    ops.project_color_bwd_raw(d["means"][:n], d["quats"][:n], d["scales"][:n], d["opac"][:n], deg, d["sh"][:n], d["viewmat"],
                              d["K"], R.W, R.H, R.EPS2D, cut(radii), cut(conics), aa, cut(feats), cut(ct["v_feats"]),
                              cut(ct["v_means2d"]), cut(ct["v_conics"]), cut(ct["v_opac_out"]), out["v_means"], out["v_quats"],
                              out["v_scales"], out["v_sh"], out["v_opacities"], v_viewmat=vv, accumulate=accumulate,
                              camera=d["camera"], raw=d["raw"], v_depths=cut(v_depths))
    torch.cuda.synchronize()
    res = {k: v.cpu().numpy() for k, v in out.items()}
    if vv is not None:
        res["v_viewmat"] = vv.cpu().numpy()
    return res, pre


def hold(family, tensor, got, want, what):
    """Every row within the family's gate; a tensor the reference has as all zeros must be all zeros."""
    want = np.asarray(want, dtype=np.float64)
    if not want.any():
        assert not np.asarray(got).any(), f"{what} {tensor}: the reference is zero"
        return
    g = R.gate(family, tensor)
    print(f"PCB {family} {tensor} {R.scaled_error(got, want):.3e} gate {g:.2e} [{what}]")
    compare(f"{what} {tensor}", got, want, row_tol=g, bad_frac=0.0, verbose=False)


def hold_added(family, tensor, got, pre, want, what):
    """Accumulate mode: got = fp32(pre + v) with v within the family's gate of `want` -- the gate on what was added, scaled
    as grad_gate.compare scales it by the reference of what was added, plus the one rounding of the sum itself."""
    want = np.asarray(want, dtype=np.float64).reshape(len(want), -1)
    got, pre = (np.asarray(a, dtype=np.float64).reshape(want.shape) for a in (got, pre))
    g = R.gate(family, tensor)
    scale = np.abs(want).max(axis=1, keepdims=True) + 1e-3 * np.abs(want).max() + 1e-30
    raw = np.abs(got - pre - want)
    d = np.maximum(raw - 0.5 * np.finfo(F).eps * np.abs(got), 0.0)
    err = float((d / scale).max())
    carried = int((((raw / scale) > g) & ((d / scale) <= g)).any(axis=1).sum())      # rows inside only thanks to the rounding term
    print(f"PCB {family} {tensor} {err:.3e} gate {g:.2e} [{what}] without the sum's rounding: {float((raw / scale).max()):.3e}, "
          f"rows it carries: {carried}")
    assert np.isfinite(got).all() and err <= g, f"{what} {tensor}: added rows off by {err:.3e} > {g:.2e}"


def check_launch(family, res, pre, ref, n, vis, deg, stride, accumulate, own_opac, what, view_pre=None):
    """The whole contract of one launch.  ref: R.vjp's result for n rows (or more: rows are independent) with every row
    visible or already gated by `vis`; vis [n] bool: the rows whose radii were > 0."""
    kc = (deg + 1) ** 2
    vis = np.asarray(vis, dtype=bool)[:n]
    names = ["v_means", "v_quats", "v_scales", "v_sh"] + (["v_opacities"] if own_opac else [])
    for k in ("v_means", "v_quats", "v_scales", "v_sh", "v_opacities"):
        assert np.array_equal(_bits(res[k][n:]), _bits(pre[k][n:])), f"{what} {k}: rows past n were written"
    if not own_opac:
        assert np.array_equal(_bits(res["v_opacities"]), _bits(pre["v_opacities"])), f"{what}: v_opacities is not this launch's"
    for k in names:
        got, p = res[k][:n], pre[k][:n]
        r = np.asarray(ref[k][:n], dtype=np.float64)
        if k == "v_sh":
            assert not r[:, kc:].any()
            r = np.concatenate([r, np.zeros((n, max(0, stride - r.shape[1]), 3))], axis=1)[:, :stride]
        want = np.where(vis.reshape((n,) + (1,) * (got.ndim - 1)), r.reshape(got.shape), 0.0)
        if accumulate:
            assert np.array_equal(_bits(got[~vis]), _bits(p[~vis])), f"{what} {k}: accumulate touched an invisible row"
            if k == "v_sh":
                assert np.array_equal(_bits(got[:, kc:]), _bits(p[:, kc:])), f"{what}: accumulate touched padding columns"
            if vis.any():
                hold_added(family, k, got[vis], p[vis], want[vis], what + " accumulate")
        else:
            assert not got[~vis].any(), f"{what} {k}: invisible rows are not zero"
            if k == "v_sh":
                assert not got[:, kc:].any(), f"{what}: padding columns are not zero"
            if vis.any():
                hold(family, k, got[vis], want[vis], what)
    if view_pre is not None:
        hold_view(family, res["v_viewmat"], view_pre, ref["view"][:n][vis], n, what)


def hold_view(family, got, view_pre, contrib, n, what):
    """v_viewmat = prefill + the sum of `contrib` [m,3,4] on rows 0..2, the bottom row bit-unchanged.  Cancellation-safe:
    |got - ref| <= tol x sum_g |contribution_g| per entry, plus the rounding of the atomic adds into the prefill itself
    (one per wave, each half an ulp of a running total the prefill dominates when the contributions are small).  With rows
    0..2 of the prefill zero (VIEW_BOTTOM) that term is zero and the gate is the bare one."""
    view_pre = np.asarray(view_pre, dtype=F)
    assert np.array_equal(_bits(got[3]), _bits(view_pre[3])), f"{what}: v_viewmat's bottom row was written"
    tol = R.gate(family, "v_viewmat")
    d = np.abs(got[:3].astype(np.float64) - view_pre[:3].astype(np.float64) - R.view_sum(contrib))
    strict = tol * R.view_abs(contrib)
    extra = np.finfo(F).eps * -(-n // 64) * np.abs(view_pre[:3])
    allow = strict + extra
    if contrib.size:
        carried = int(((d > strict) & (d <= allow)).sum())            # entries inside only thanks to the prefill term
        print(f"PCB {family} v_viewmat {float((d / allow).max()) * tol:.3e} gate {tol:.2e} [{what}] prefill share of the "
              f"allowance: max {float((extra / allow).max()):.3f}, entries it carries: {carried}")
    assert (d <= allow).all(), f"{what} v_viewmat: |got - ref| is {(d / allow).max():.3f} x what sum|contribution| allows at {tol:.2e}"


VIEW_PRE = (np.arange(16, dtype=F).reshape(4, 4) - 7.5) * F(0.125)      # non-zero everywhere
VIEW_BOTTOM = VIEW_PRE * np.array([[0], [0], [0], [1]], dtype=F)        # only the bottom row: the first atomic add is exact


# ---------------------------------------------------------------------------------------------------------------------
# a. the instantiation sweep
# ---------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=4)
def _sweep_ref(model, raw, aa, mu, deg, width):
    case = R.scene_case(model, raw, n=333, mu=mu)
    fp = R.forward_products(case, deg, aa, width == 4)
    ct = R.cotangents(333, 0, width == 4)
    ref = R.vjp(case, deg, aa, fp["radii"], fp["feats"], ct["v_means2d"], ct["v_conics"], ct["v_feats"], None, ct["v_opac_out"])
    return case, fp, ct, ref


@pytest.mark.parametrize("mu", R.SWEEP_MU)
@pytest.mark.parametrize("aa", [False, True])
@pytest.mark.parametrize("raw", [False, True])
@pytest.mark.parametrize("model", R.CAMERAS)
def test_instantiation_sweep(model, raw, aa, mu):
    """n = 333 (one full block and a 77-row tail): every degree x coefficient stride (16: the LDS-staged rows; otherwise the
    plain path: degree 1 at stride 9 and degree 3 at stride 20, both with padding) x feats 3 / 4 wide x with / without
    v_viewmat x overwrite / accumulate -- with the decorator's camera x raw x anti-aliased, all 256 instantiations of
    project_color_bwd_kernel (DEG x STAGED x ACCUM x VIEWGRAD x CAM x RAW)."""
    own = aa or raw
    for deg, stride in R.SH_STRIDES:
        d = None
        for width in (3, 4):
            case, fp, ct, ref = _sweep_ref(model, raw, aa, mu, deg, width)
            d = d or _upload(case, stride)
            vis = fp["radii"] > 0
            assert vis.sum() > 100                     # (pinhole and ortho cull some rows too; the fisheyes see the whole scene)
            for view in (None, VIEW_PRE):
                for acc in (False, True):
                    what = f"{model} raw={raw} aa={aa} mu={mu} deg={deg} stride={stride} feats={width} view={view is not None}"
                    res, pre = run_fused(d, deg, aa, fp["radii"], fp["conics"], fp["feats"], ct, accumulate=acc, view=view)
                    check_launch("sweep", res, pre, ref, 333, vis, deg, stride, acc, own, what, view_pre=view)
                    if view is not None and not acc:                    # the same twelve sums by the issue's plain row gate
                        hold("sweep", "v_viewmat", (res["v_viewmat"] - VIEW_PRE)[:3].reshape(1, 12),
                             R.view_sum(ref["view"][vis]).reshape(1, 12), what)


# ---------------------------------------------------------------------------------------------------------------------
# b. row ownership and tails
# ---------------------------------------------------------------------------------------------------------------------
SIZES = (1, 63, 64, 65, 255, 256, 257)
PATTERNS = ("none", "last", "lane63", "row64", "alternating", "all")


def _pattern(name, n):
    """bool [n], or None when the pattern's row does not exist at this n."""
    m = np.zeros(n, bool)
    if name == "last":
        m[n - 1] = True
    elif name in ("lane63", "row64"):
        r = 63 if name == "lane63" else 64
        if r >= n:
            return None
        m[r] = True
    elif name == "alternating":
        m[::2] = True
    elif name == "all":
        m[:] = True
    return m


@functools.lru_cache(maxsize=None)
def _owned_ref(deg, aa):
    case = R.visible_case(257)
    fp = R.forward_products(case, deg, aa, True)
    assert (fp["radii"] > 0).all()
    ct = R.cotangents(257, 1, True)
    ref = R.vjp(case, deg, aa, fp["radii"], fp["feats"], ct["v_means2d"], ct["v_conics"], ct["v_feats"], None, ct["v_opac_out"])
    return case, fp, ct, ref


@pytest.mark.parametrize("n", SIZES)
def test_fused_row_ownership(n):
    """Rows of the reference are independent, so one reference of 257 visible Gaussians serves every size and every
    visibility pattern: the pattern is put into `radii` alone."""
    for deg, stride in ((3, 16), (3, 20), (1, 9), (1, 16)):
        for aa in (False, True):
            case, fp, ct, ref = _owned_ref(deg, aa)
            d = _upload(case, stride)
            for name in PATTERNS:
                vis = _pattern(name, n)
                if vis is None:
                    continue
                radii = np.where(vis, fp["radii"][:n], 0).astype(np.int32)
                for view in (None, VIEW_PRE):
                    for acc in (False, True):
                        what = f"n={n} {name} deg={deg} stride={stride} aa={aa} view={view is not None}"
                        res, pre = run_fused(d, deg, aa, radii, fp["conics"], fp["feats"], ct, accumulate=acc, view=view, n=n)
                        check_launch("sweep", res, pre, ref, n, vis, deg, stride, acc, aa, what, view_pre=view)


@pytest.mark.parametrize("n", SIZES)
def test_sh_bwd_row_ownership(n):
    """mgs_sh_bwd overwrites: masked rows are exact zeros (v_dirs too), padding columns zero, rows past n untouched."""
    from robosimgs_amd import _lib
    from robosimgs_amd._lib import check, ptr, stream_handle
    dirs, coeffs, v = R.sh_case(257)
    for deg, stride in R.SH_STRIDES:
        kc = (deg + 1) ** 2
        co = np.zeros((n, stride, 3), F)                     # (a stride over 16: zero padding)
        co[:, :min(stride, 16)] = coeffs[:n, :stride]
        want_c, want_d = R.sh_vjp(deg, dirs[:n], co, None, v[:n])
        d_dirs, d_co, d_v = _t(dirs[:n]), _t(co), _t(v[:n])
        for name in PATTERNS + ("no mask",):
            m = np.ones(n, bool) if name == "no mask" else _pattern(name, n)
            if m is None:
                continue
            d_m = None if name == "no mask" else _t(m.astype(np.uint8))
            for with_dirs in (False, True):
                pc, pd = _prefill((n + PAD, stride, 3), 6), _prefill((n + PAD, 3), 7)
                oc, od = _t(pc), _t(pd)
                check(_lib.lib().mgs_sh_bwd(n, deg, stride, ptr(d_dirs), ptr(d_co), ptr(d_m), ptr(d_v), ptr(oc),
                                            ptr(od) if with_dirs else None, stream_handle()), "mgs_sh_bwd")
                torch.cuda.synchronize()
                gc, gd = oc.cpu().numpy(), od.cpu().numpy()
                what = f"sh_bwd n={n} {name} deg={deg} stride={stride} v_dirs={with_dirs}"
                assert np.array_equal(_bits(gc[n:]), _bits(pc[n:])) and np.array_equal(_bits(gd[n:]), _bits(pd[n:])), what
                assert not gc[:n][~m].any() and not gc[:n, kc:].any(), what
                if m.any():
                    hold("sh_stage", "v_coeffs", gc[:n][m], want_c[m], what)
                if with_dirs:
                    assert not gd[:n][~m].any(), what
                    if m.any():
                        hold("sh_stage", "v_dirs", gd[:n][m], want_d[m], what)
                else:
                    assert np.array_equal(_bits(gd), _bits(pd)), what


@functools.lru_cache(maxsize=None)
def _projection_ref(aa, with_depth):
    case = R.projection_case(257)
    fp = R.forward_products(case, 0, aa, True)
    assert (fp["radii"] > 0).all()
    ct = R.cotangents(257, 2, True)
    vf = np.zeros((257, 4), F)
    vd = ct["v_feats"][:, 3].copy() if with_depth else None
    ref = R.vjp(case, 0, aa, fp["radii"], np.zeros((257, 4), F), ct["v_means2d"], ct["v_conics"], vf, vd,
                ct["v_opac_out"] if aa else None)
    return case, fp, ct, vd, ref


@pytest.mark.parametrize("n", SIZES)
def test_projection_bwd_row_ownership(n):
    """mgs_projection_bwd always ADDS: prefilled buffers, invisible rows and rows past n bit-unchanged, v_viewmat present and
    absent, compensations / v_compensations / v_depths null and non-null."""
    from robosimgs_amd import _lib
    from robosimgs_amd._lib import check, ptr, stream_handle
    for aa in (False, True):
        for with_depth in (False, True):
            case, fp, ct, vd, ref = _projection_ref(aa, with_depth)
            d = _upload(case)
            cut = lambda x: None if x is None else _t(np.asarray(x)[:n])
            con, comp, vm2, vcon = cut(fp["conics"]), cut(fp["compensations"]), cut(ct["v_means2d"]), cut(ct["v_conics"])
            vcomp, vdep = cut(ct["v_opac_out"]), cut(vd)
            for name in PATTERNS:
                vis = _pattern(name, n)
                if vis is None:
                    continue
                radii = _t(np.where(vis, fp["radii"][:n], 0).astype(np.int32))
                for view in (None, VIEW_PRE):
                    pre = {"v_means": _prefill((n + PAD, 3), 1), "v_quats": _prefill((n + PAD, 4), 2), "v_scales": _prefill((n + PAD, 3), 3)}
                    out = {k: _t(v) for k, v in pre.items()}
                    vv = None if view is None else _t(view)
                    check(_lib.lib().mgs_projection_bwd(
                        n, ptr(d["means"]), ptr(d["quats"]), ptr(d["scales"]), ptr(d["viewmat"]), ptr(d["K"]), R.W, R.H, R.EPS2D,
                        ptr(radii), ptr(con), ptr(comp) if aa else None, ptr(vm2), ptr(vdep), ptr(vcon), ptr(vcomp) if aa else None,
                        ptr(out["v_means"]), ptr(out["v_quats"]), ptr(out["v_scales"]), ptr(vv), 0, stream_handle()), "mgs_projection_bwd")
                    torch.cuda.synchronize()
                    what = f"projection_bwd n={n} {name} comp={aa} v_depths={with_depth} view={view is not None}"
                    for k, p in pre.items():
                        got = out[k].cpu().numpy()
                        assert np.array_equal(_bits(got[n:]), _bits(p[n:])), f"{what} {k}: rows past n"
                        assert np.array_equal(_bits(got[:n][~vis]), _bits(p[:n][~vis])), f"{what} {k}: invisible rows"
                        if vis.any():
                            hold_added("projection_stage", k, got[:n][vis], p[:n][vis], ref[k][:n][vis], what)
                    if view is not None:
                        hold_view("projection_stage", vv.cpu().numpy(), view, ref["view"][:n][vis], n, what)


# ---------------------------------------------------------------------------------------------------------------------
# c. two cameras, one buffer
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("raw,aa", [(False, True), (True, False)])
def test_two_cameras_one_buffer(raw, aa):
    """Camera 0 overwrites, camera 1 accumulates into the same buffers (rendering.py's loop): the fp64 sum of both VJPs; a
    Gaussian only one camera sees carries that camera's gradient alone, one neither sees is zero."""
    from robosimgs_amd import ops
    n, deg = 333, 2
    cams = [R.scene_case("pinhole", raw, n=n, mu=0.1, stride=9, theta=th, radius=4.0) for th in (0.3, 2.4)]       # close: each camera misses a part of the scene
    ct = [R.cotangents(n, s, True) for s in (0, 1)]
    fps = [R.forward_products(c, deg, aa, True) for c in cams]
    refs = [R.vjp(c, deg, aa, fp["radii"], fp["feats"], t["v_means2d"], t["v_conics"], t["v_feats"], None, t["v_opac_out"], view=False)
            for c, fp, t in zip(cams, fps, ct)]
    v0, v1 = fps[0]["radii"] > 0, fps[1]["radii"] > 0
    assert (v0 & ~v1).sum() > 5 and (v1 & ~v0).sum() > 5 and (~v0 & ~v1).sum() > 5 and (v0 & v1).sum() > 5
    out = {"v_means": torch.full((n, 3), 7.0, device=DEV), "v_quats": torch.full((n, 4), 7.0, device=DEV),
           "v_scales": torch.full((n, 3), 7.0, device=DEV), "v_sh": torch.full((n, 9, 3), 7.0, device=DEV),
           "v_opacities": torch.full((n,), 7.0, device=DEV)}
    for i, (c, fp, t) in enumerate(zip(cams, fps, ct)):
        d = _upload(c)
        ops.project_color_bwd_raw(d["means"], d["quats"], d["scales"], d["opac"], deg, d["sh"], d["viewmat"], d["K"], R.W, R.H,
                                  R.EPS2D, _t(fp["radii"]), _t(fp["conics"]), aa, _t(fp["feats"]), _t(t["v_feats"]),
                                  _t(t["v_means2d"]), _t(t["v_conics"]), _t(t["v_opac_out"]), out["v_means"], out["v_quats"],
                                  out["v_scales"], out["v_sh"], out["v_opacities"], accumulate=i > 0, camera=0, raw=raw)
    torch.cuda.synchronize()
    for k in ("v_means", "v_quats", "v_scales", "v_sh", "v_opacities"):
        got = out[k].cpu().numpy()
        hold("sweep", k, got, refs[0][k] + refs[1][k], f"two cameras raw={raw} aa={aa}")
        hold("sweep", k, got[v0 & ~v1], refs[0][k][v0 & ~v1], "camera 0 alone")
        hold("sweep", k, got[v1 & ~v0], refs[1][k][v1 & ~v0], "camera 1 alone")
        assert not got[~v0 & ~v1].any()


# ---------------------------------------------------------------------------------------------------------------------
# d. the camera-pose gradient
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n,only_row_64", [(65, True), (257, False)])
@pytest.mark.parametrize("term", ["projection", "direction"])
def test_camera_pose_gradient(term, n, only_row_64):
    """v_viewmat[:3] = prefill + the sum of the Gaussians' contributions, the bottom row untouched; lanes past n and
    invisible lanes take part in the wave reduction with zeros.  Order is free under atomics, so the gate is
    |got - ref| <= tol x sum_g |contribution_g| per entry, both sums from the reference.  "projection": degree 0, no
    direction term; "direction": degree 3 with every projection cotangent zero -- dir = mean + R^T t alone."""
    deg = 0 if term == "projection" else 3
    case = R.visible_case(257)
    fp = R.forward_products(case, deg, False, term == "projection")
    ct = R.cotangents(257, 3, term == "projection")
    if term == "direction":
        ct["v_means2d"][:], ct["v_conics"][:] = 0, 0
    vis = np.ones(n, bool)
    if only_row_64:
        vis[:64] = False
    radii = np.where(vis, fp["radii"][:n], 0).astype(np.int32)
    ref = R.vjp(case, deg, False, fp["radii"], fp["feats"], ct["v_means2d"], ct["v_conics"], ct["v_feats"], None, None)
    assert np.abs(R.view_sum(ref["view"][:n][vis])).min() > 0
    d = _upload(case, (deg + 1) ** 2)
    for acc in (False, True):
        res, pre = run_fused(d, deg, False, radii, fp["conics"], fp["feats"], ct, accumulate=acc, view=VIEW_PRE, n=n)
        check_launch("sweep", res, pre, ref, n, vis, deg, (deg + 1) ** 2, acc, False, f"pose {term} n={n} acc={acc}", view_pre=VIEW_PRE)
        # the bare gate, |got - ref| <= tol x sum |contribution|: nothing in rows 0..2 for the sums to round into
        res, pre = run_fused(d, deg, False, radii, fp["conics"], fp["feats"], ct, accumulate=acc, view=VIEW_BOTTOM, n=n)
        hold_view("sweep", res["v_viewmat"], VIEW_BOTTOM, ref["view"][:n][vis], n, f"pose {term} n={n} acc={acc} bare")


# ---------------------------------------------------------------------------------------------------------------------
# e. the colour clamp
# ---------------------------------------------------------------------------------------------------------------------
def test_colour_clamp_gate():
    """feats written by hand: +0.0, -0.0 and a negative value are dead, the smallest normal float and 1.0 live, per channel.
    One channel dead, then all three: with all three dead at degree 3 the v_sh row is exactly zero and v_means is the
    projection's alone."""
    n, deg = 130, 3
    case = R.visible_case(n)
    fp = R.forward_products(case, deg, False, True)
    ct = R.cotangents(n, 4, True)
    vals = np.array([0.0, -0.0, np.finfo(F).tiny, -1.0, 1.0], dtype=F)
    feats = fp["feats"].copy()
    i = np.arange(n)
    feats[:, 0], feats[:, 1], feats[:, 2] = vals[i % 5], vals[(i // 5) % 5], vals[(i // 25 + i) % 5]
    all_dead = np.flatnonzero(~(feats[:, :3] > 0).any(1))
    one_dead = np.flatnonzero((feats[:, :3] > 0).sum(1) == 2)
    assert len(all_dead) >= 5 and len(one_dead) >= 20 and np.signbit(feats[all_dead, :3]).any()
    ref = R.vjp(case, deg, False, fp["radii"], feats, ct["v_means2d"], ct["v_conics"], ct["v_feats"], None, None)
    no_rgb = dict(ct, v_feats=np.concatenate([np.zeros((n, 3), F), ct["v_feats"][:, 3:]], 1))
    proj = R.vjp(case, deg, False, fp["radii"], feats, no_rgb["v_means2d"], no_rgb["v_conics"], no_rgb["v_feats"], None, None)
    d = _upload(case)
    for acc in (False, True):
        res, pre = run_fused(d, deg, False, fp["radii"], fp["conics"], feats, ct, accumulate=acc, view=VIEW_PRE)
        check_launch("sweep", res, pre, ref, n, np.ones(n, bool), deg, 16, acc, False, f"clamp acc={acc}", view_pre=VIEW_PRE)
        if not acc:
            assert not res["v_sh"][all_dead].any()
            dead_ch = ~(feats[:n, :3] > 0)
            assert not res["v_sh"][:n].transpose(0, 2, 1)[dead_ch].any()          # a dead channel's column of every coefficient
            assert res["v_sh"][:n].transpose(0, 2, 1)[~dead_ch][:, 0].all()
            hold("sweep", "v_means", res["v_means"][all_dead], proj["v_means"][all_dead], "all channels dead: projection only")


# ---------------------------------------------------------------------------------------------------------------------
# f. the depth cotangent
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("where", ["v_feats", "v_depths 3 wide", "v_depths 4 wide", "both"])
def test_depth_cotangent(where):
    """d/d depth arrives in v_feats[:,3], in v_depths (with 3- and 4-wide feats), or in both, which add."""
    n, deg = 257, 1
    case = R.visible_case(n, model="fisheye")
    wide = where != "v_depths 3 wide"
    fp = R.forward_products(case, deg, True, wide)
    ct = R.cotangents(n, 5, wide)
    vd = None if where == "v_feats" else np.random.default_rng(11).normal(size=n).astype(F) * F(3.0)
    if where == "v_depths 4 wide":
        ct["v_feats"][:, 3] = 0
    ref = R.vjp(case, deg, True, fp["radii"], fp["feats"], ct["v_means2d"], ct["v_conics"], ct["v_feats"], vd, ct["v_opac_out"])
    none = R.vjp(case, deg, True, fp["radii"], fp["feats"], ct["v_means2d"], ct["v_conics"], ct["v_feats"][:, :3], None,
                 ct["v_opac_out"], view=False)
    assert R.scaled_error(none["v_means"], ref["v_means"]) > 1e-2          # the depth term is a visible share of v_means
    d = _upload(case, 4)
    vis = fp["radii"] > 0
    for acc in (False, True):
        res, pre = run_fused(d, deg, True, fp["radii"], fp["conics"], fp["feats"], ct, accumulate=acc, view=VIEW_PRE, v_depths=vd)
        check_launch("sweep", res, pre, ref, n, vis, deg, 4, acc, True, f"depth in {where} acc={acc}", view_pre=VIEW_PRE)


# ---------------------------------------------------------------------------------------------------------------------
# g. numerical edges
# ---------------------------------------------------------------------------------------------------------------------
def _family_launch(name, label, case, deg, aa, wd, ct=None, acc=False):
    n = case["means"].shape[0]
    fp = R.forward_products(case, deg, aa, wd)
    ct = R.cotangents(n, 0, wd) if ct is None else ct
    ref = R.vjp(case, deg, aa, fp["radii"], fp["feats"], ct["v_means2d"], ct["v_conics"], ct["v_feats"], None, ct["v_opac_out"])
    d = _upload(case)
    res, pre = run_fused(d, deg, aa, fp["radii"], fp["conics"], fp["feats"], ct, accumulate=acc, view=VIEW_PRE)
    check_launch(name, res, pre, ref, n, fp["radii"] > 0, deg, case["sh"].shape[1], acc, aa or case["raw"], f"{name} {label}",
                 view_pre=VIEW_PRE)
    return fp, ref, res


@pytest.mark.parametrize("name", R.FAMILIES)
def test_numerical_edges(name):
    """project_color_ref.family(name): hand-placed Gaussians at the edge, padded with ordinary ones that share their wave;
    every output at 8 x the family's own floor."""
    for label, case, deg, aa, wd in R.family(name):
        n = case["means"].shape[0]
        ct = R.triplet_cotangents(n, wd) if name == "quat_norm" else None
        for acc in (True, False):                       # (overwrite last: its result is what the property checks below read)
            fp, ref, res = _family_launch(name, label, case, deg, aa, wd, ct=ct, acc=acc)
            placed = {"aa_subpixel": 32, "quat_norm": 6, "pinhole_clamp": 8, "near_far": 4, "fisheye_axis": 6, "ortho_depths": 2,
                      "raw_range": 8}[name]
            assert (fp["radii"][:placed] > 0).all(), f"{name} {label}: a placed Gaussian is culled"
            for k in ("v_means", "v_quats", "v_scales", "v_sh", "v_opacities"):
                assert np.isfinite(res[k]).all(), (name, label, k)
        if name == "aa_subpixel":
            assert fp["compensations"][:32].min() < 2e-4
        if name == "quat_norm":
            q, vq = case["quats"].astype(np.float64), res["v_quats"].astype(np.float64)
            g = R.gate(name, "v_quats")
            cosine = np.abs((q[:6] * vq[:6]).sum(-1)) / (np.linalg.norm(q[:6], axis=1) * np.linalg.norm(vq[:6], axis=1))
            assert cosine.max() <= g, f"v_quats is not orthogonal to q: {cosine.max():.3e}"
            for b in (0, 3):
                s = np.abs(vq[b + 1]).max()
                assert np.abs(vq[b] * 0.1 - vq[b + 1]).max() <= 2 * g * s and np.abs(vq[b + 2] * 10 - vq[b + 1]).max() <= 2 * g * s


def test_pinhole_clamp_kills_the_clamped_coordinate():
    """Outside the 1.3 x frustum clamp the Jacobian is that of the clamped point: a cotangent of the conic alone then gives
    the camera-space x (or y) of the mean nothing; just inside it does."""
    label, case, deg, aa, wd = R.family("pinhole_clamp")[0]
    n = case["means"].shape[0]
    fp = R.forward_products(case, 0, False, False)
    z = lambda *s: np.zeros(s, F)
    ct = {"v_means2d": z(n, 2), "v_conics": R.cotangents(n)["v_conics"], "v_feats": z(n, 3), "v_opac_out": None}
    res, _ = run_fused(_upload(case, 1), 0, False, fp["radii"], fp["conics"], fp["feats"], ct)
    v_cam = res["v_means"][:8].astype(np.float64) @ case["viewmat"][:3, :3].astype(np.float64).T
    big = np.abs(v_cam).max()
    for i in range(8):                      # x+ inside, x+ outside, x- inside, x- outside, then y
        axis, outside = (0 if i < 4 else 1), i % 2 == 1
        # (v_means is R^T of the camera-space cotangent, rounded to fp32: rotating it back leaves that rounding)
        assert (abs(v_cam[i, axis]) <= 8 * np.finfo(F).eps * np.abs(v_cam[i]).max()) == outside, (i, v_cam[i], big)


def test_ortho_depth_does_not_enter_the_mean():
    """Two Gaussians that differ in depth alone: the same cotangent of means2d gives bit-identical v_means rows."""
    label, case, deg, aa, wd = R.family("ortho_depths")[0]
    n = case["means"].shape[0]
    fp = R.forward_products(case, 0, False, False)
    z = lambda *s: np.zeros(s, F)
    vm = R.cotangents(n)["v_means2d"]
    vm[1] = vm[0]
    ct = {"v_means2d": vm, "v_conics": z(n, 3), "v_feats": z(n, 3), "v_opac_out": None}
    res, _ = run_fused(_upload(case, 1), 0, False, fp["radii"], fp["conics"], fp["feats"], ct)
    assert res["v_means"][0].any() and np.array_equal(_bits(res["v_means"][0]), _bits(res["v_means"][1]))
    assert not res["v_scales"][:2].any() and not res["v_quats"][:2].any()


@pytest.mark.parametrize("raw", [False, True])
def test_zero_inputs(raw):
    """All cotangents zero: every output exactly zero.  Opacity 0 (a logit of -120 when raw: the sigmoid underflows to 0)
    under anti-aliasing: finite, and the reference's."""
    n, deg = 100, 3
    case = R.visible_case(n, raw=raw)
    case["opac"] = case["opac"].copy()
    case["opac"][::3] = -120.0 if raw else 0.0
    fp = R.forward_products(case, deg, True, True)
    z = lambda *s: np.zeros(s, F)
    zero = {"v_means2d": z(n, 2), "v_conics": z(n, 3), "v_feats": z(n, 4), "v_opac_out": z(n)}
    d = _upload(case)
    res, _ = run_fused(d, deg, True, fp["radii"], fp["conics"], fp["feats"], zero, view=np.zeros((4, 4), F))
    for k, v in res.items():
        assert not v[:n].any(), k
    ct = R.cotangents(n, 6, True)
    ref = R.vjp(case, deg, True, fp["radii"], fp["feats"], ct["v_means2d"], ct["v_conics"], ct["v_feats"], None, ct["v_opac_out"])
    res, pre = run_fused(d, deg, True, fp["radii"], fp["conics"], fp["feats"], ct, view=VIEW_PRE)
    for k in ("v_means", "v_quats", "v_scales", "v_sh", "v_opacities"):
        assert np.isfinite(res[k]).all(), k
    check_launch("sweep", res, pre, ref, n, fp["radii"] > 0, deg, 16, False, True, f"opacity 0 raw={raw}", view_pre=VIEW_PRE)
