"""CPU tests of tests/project_color_ref.py, the fp64 reference the GPU stage tests of the fused projection + colour
backward (tests/test_gpu_project_color_bwd.py) hold the kernels to: central finite differences under every camera model,
the device math compiled for the host (hh_project_vjp + hh_sh composed as the kernel composes them), the mask and clamp
semantics, and the rounding floor of every case family with its ceiling."""
import ctypes
import os
import subprocess

import numpy as np
import pytest
import torch

import project_color_ref as R

HERE = os.path.dirname(os.path.abspath(__file__))


def _args(case, deg, aa, with_depth=True, seed=0, v_depths=False):
    fp = R.forward_products(case, deg, aa, with_depth)
    ct = R.cotangents(case["means"].shape[0], seed, with_depth)
    vd = np.random.default_rng(7).normal(size=len(fp["radii"])).astype(np.float32) if v_depths else None
    return fp, (case, deg, aa, fp["radii"], fp["feats"], ct["v_means2d"], ct["v_conics"], ct["v_feats"], vd, ct["v_opac_out"])


@pytest.mark.parametrize("model", R.CAMERAS)
@pytest.mark.parametrize("raw,aa", [(False, False), (False, True), (True, False), (True, True)])
def test_vjp_matches_central_finite_differences(model, raw, aa):
    """<vjp, delta> against (L(p + h delta) - L(p - h delta)) / 2h in float64 for random directions of every leaf and for each
    of the twelve entries of viewmat[:3].  The exact square root here (guard=False): the guard is not the derivative of
    anything, and test_compensation_guard pins what it changes."""
    case = R.scene_case(model, raw, n=20, mu=0.1, seed=3)
    fp, args = _args(case, 3, aa, v_depths=True)
    assert (fp["radii"] > 0).sum() >= 12
    ref = R.vjp(*args, guard=False)
    rng = np.random.default_rng(0)
    leaves = {"means": "v_means", "quats": "v_quats", "scales": "v_scales", "sh": "v_sh", "opac": "v_opacities"}

    def fd(key, delta, h):
        c64 = {k: (v.astype(np.float64) if isinstance(v, np.ndarray) else v) for k, v in case.items()}
        up, dn = dict(c64), dict(c64)
        up[key], dn[key] = c64[key] + h * delta, c64[key] - h * delta
        return (_loss64(up, args) - _loss64(dn, args)) / (2 * h)

    for key, name in leaves.items():
        for _ in range(3):
            delta = rng.normal(size=case[key].shape)
            want, got = fd(key, delta, 1e-6), float((ref[name] * delta).sum())
            assert abs(got - want) <= 2e-7 * (np.abs(ref[name] * delta).sum() + 1e-12), (key, got, want)
    total, mags = R.view_sum(ref["view"]), R.view_abs(ref["view"])
    for r in range(3):
        for c in range(4):
            delta = np.zeros((4, 4))
            delta[r, c] = 1.0
            want = fd("viewmat", delta, 1e-6)
            assert abs(total[r, c] - want) <= 2e-7 * (mags[r, c] + 1e-12), (r, c, total[r, c], want)


def _loss64(case64, args):
    """The scalar R.vjp differentiates, on a case whose arrays are float64 (make_case rounds to fp32, which a finite
    difference must not)."""
    with torch.no_grad():
        _, o = R._graph(case64, args[1], args[2], torch.float64, False)
        return float(R.loss_rows(o, len(args[3]), *args[3:], torch.float64).sum())


def test_compensation_guard():
    """With v_opac_out the only cotangent, activated opacities and anti-aliasing, the geometry hears of the loss through
    the compensation alone: the guarded backward is the exact one times comp / (comp + 1e-6), row by row, and
    v_opacities = v_opac_out x comp either way."""
    case = R.family("aa_subpixel")[0][1]
    n = case["means"].shape[0]
    fp = R.forward_products(case, 0, True, False)
    z = lambda *s: np.zeros(s, np.float32)
    vo = R.cotangents(n)["v_opac_out"]
    a = (case, 0, True, fp["radii"], fp["feats"], z(n, 2), z(n, 3), z(n, 3), None, vo)
    g, e = R.vjp(*a), R.vjp(*a, guard=False)
    comp = fp["compensations"].astype(np.float64)
    vis = fp["radii"] > 0
    assert comp[vis].min() < 2e-4 and vis[:32].all()
    f = (comp / (comp + 1e-6))[:, None]
    for k in ("v_scales", "v_quats", "v_means"):
        np.testing.assert_allclose(g[k][vis], (e[k] * f)[vis], rtol=1e-6, atol=1e-12 * np.abs(e[k]).max())
    np.testing.assert_allclose(g["v_opacities"][vis], (vo * comp)[vis], rtol=1e-6)
    assert (g["v_opacities"][~vis] == 0).all()


@pytest.fixture(scope="module")
def hh(tmp_path_factory):
    so = tmp_path_factory.mktemp("hh_pcb") / "libhh.so"
    subprocess.run(["g++", "-O2", "-std=c++17", "-shared", "-fPIC", os.path.join(HERE, "host_harness", "harness.cpp"),
                    "-o", str(so)], check=True)
    return ctypes.CDLL(str(so))


def _p(a):
    return a.ctypes.data_as(ctypes.c_void_p)


def host_fused(hh, case, deg, aa, radii, conics, feats, v_means2d, v_conics, v_feats, v_depths, v_opac_out):
    """project_color_bwd_kernel's body on the host, pinhole and activated: the device math (csrc/mgs_math.h through
    tests/host_harness) around the kernel's own few lines, restated in fp32 numpy -- the clamp gate, the compensation
    rebuilt from the blurred conic as det(I - eps Q), v_comp = v_opac_out x opacity, the view direction's share of v_means and v_viewmat.
    A check of the COMPOSITION at the harness's 2e-3, not of the compensation's precision: the det(I - eps Q) lines are a copy
    of the kernel's, kept by hand, and at 2e-3 the old form and the new are alike.  What holds the kernel's own lines to the
    fp32 conic's limit is the anti-aliased sweep and the sub-pixel family on the GPU."""
    assert case["model"] == "pinhole" and not case["raw"]
    f32 = np.float32
    n = case["means"].shape[0]
    vm = case["viewmat"]
    Rm, t = vm[:3, :3], vm[:3, 3]
    campos = -(Rm.T @ t).astype(f32)
    dirs = np.ascontiguousarray(case["means"] - campos, dtype=f32)
    v_rgb = np.ascontiguousarray(np.where(feats[:, :3] > 0, v_feats[:, :3], 0), dtype=f32)
    v_depth = (v_feats[:, 3] if v_feats.shape[1] == 4 else np.zeros(n, f32)).astype(f32)
    if v_depths is not None:
        v_depth = v_depth + v_depths
    comp, v_comp = np.zeros(n, f32), np.zeros(n, f32)
    if aa:
        e, c64 = float(f32(R.EPS2D)), conics.astype(np.float64)
        p0, p2 = (1.0 - e * c64[:, 0]).astype(f32), (1.0 - e * c64[:, 2]).astype(f32)          # fmaf(-eps, q, 1): one rounding
        q1 = (f32(R.EPS2D) * conics[:, 1]).astype(f32)
        comp = np.sqrt(np.maximum(0, (p0.astype(np.float64) * p2 - (q1 * q1).astype(np.float64)).astype(f32))).astype(f32)
        comp = np.where(radii > 0, comp, 0).astype(f32)
        v_comp = (v_opac_out * case["opac"]).astype(f32)
    K = case["sh"].shape[1]
    colors, v_sh, v_dirs = np.zeros((n, 3), f32), np.zeros((n, K, 3), f32), np.zeros((n, 3), f32)
    hh.hh_sh(n, deg, K, _p(dirs), _p(case["sh"]), _p(v_rgb), _p(colors), _p(v_sh), _p(v_dirs))
    v_means, v_quats, v_scales = np.zeros((n, 3), f32), np.zeros((n, 4), f32), np.zeros((n, 3), f32)
    v_R, v_t = np.zeros(9, f32), np.zeros(3, f32)
    c = np.ascontiguousarray
    hh.hh_project_vjp(n, _p(case["means"]), _p(case["quats"]), _p(case["scales"]), _p(c(vm)), _p(c(case["K"])), R.W, R.H,
                      ctypes.c_float(R.EPS2D), _p(c(radii.astype(np.int32))), _p(c(conics)), _p(c(comp)), _p(c(v_means2d)),
                      _p(c(v_depth.astype(f32))), _p(c(v_conics)), _p(c(v_comp)), _p(v_means), _p(v_quats), _p(v_scales),
                      _p(v_R), _p(v_t))
    vis = (radii > 0)[:, None]
    v_dirs = np.where(vis, v_dirs, 0)
    v_sh = np.where(vis[:, :, None], v_sh, 0)
    view = np.concatenate([v_R.reshape(3, 3) + np.outer(t, v_dirs.sum(0)), (v_t + Rm @ v_dirs.sum(0))[:, None]], axis=1)
    return {"v_means": v_means + v_dirs, "v_quats": v_quats, "v_scales": v_scales, "v_sh": v_sh,
            "v_opacities": (v_opac_out * comp).astype(f32), "v_viewmat": view}


@pytest.mark.parametrize("aa", [False, True])
@pytest.mark.parametrize("deg", [0, 3])
def test_vjp_matches_the_device_math_on_the_host(hh, aa, deg):
    """The existing harness at the existing tolerance (tests/test_host_math.py: 2e-3 scaled), composed as the kernel does."""
    assert R.EPS2D == float(np.float32(R.EPS2D))        # the reference's eps2d is the C float the kernel is handed
    case = R.scene_case("pinhole", False, n=333, mu=0.1)
    fp, args = _args(case, deg, aa, v_depths=True)
    ref = R.vjp(*args)
    got = host_fused(hh, case, deg, aa, fp["radii"], fp["conics"], fp["feats"], *args[5:])
    for k in ("v_means", "v_quats", "v_scales", "v_sh") + (("v_opacities",) if aa else ()):
        err = R.scaled_error(got[k], ref[k])
        print(f"host harness aa={aa} deg={deg} {k}: {err:.3e}")
        assert err < 2e-3, (k, err)
    err = R.scaled_error(got["v_viewmat"].reshape(1, 12), R.view_sum(ref["view"]).reshape(1, 12))
    print(f"host harness aa={aa} deg={deg} v_viewmat: {err:.3e}")
    assert err < 2e-3, err


def test_mask_and_clamp_semantics():
    """Rows whose radii are 0 are zero rows whatever the oracle itself would decide; a dead channel (feats <= 0) gives
    nothing to v_sh, v_means or v_viewmat: the result is that of the same cotangents with the channel's set to zero."""
    case = R.scene_case("pinhole", True, n=64, mu=0.1, seed=1)
    fp, args = _args(case, 2, True)
    radii, feats = fp["radii"].copy(), fp["feats"].copy()
    assert (radii > 0).sum() > 40
    vis_rows = np.flatnonzero(radii > 0)
    radii[vis_rows[::3]] = 0                                    # hidden by the gate alone
    feats[vis_rows[1::3], 1] = 0.0                              # +0.0: dead
    feats[vis_rows[2::3], :3] = -0.0
    feats[vis_rows[4::6], 0] = np.finfo(np.float32).tiny        # the smallest normal: live
    a = list(args)
    a[3], a[4] = radii, feats
    out = R.vjp(*a)
    hidden = radii == 0
    for k in ("v_means", "v_quats", "v_scales", "v_sh", "v_opacities", "view"):
        assert (out[k][hidden] == 0).all(), k
        assert np.abs(out[k][~hidden]).reshape((~hidden).sum(), -1).max(1).min() > 0 or k == "v_sh", k
    assert (out["v_sh"][vis_rows[1::3], :, 1] == 0).all() and (out["v_sh"][vis_rows[2::3]] == 0).all()
    live_tiny = [r for r in vis_rows[4::6] if radii[r] > 0]
    assert len(live_tiny) and all(np.abs(out["v_sh"][r, :, 0]).max() > 0 for r in live_tiny)
    vf = a[7].copy()
    vf[:, :3] = np.where(feats[:, :3] > 0, vf[:, :3], 0)
    b = list(a)
    b[7] = vf
    b[4] = np.where(feats > 0, feats, 1.0).astype(np.float32)    # every channel live, the dead ones' cotangents zeroed
    same = R.vjp(*b)
    for k in ("v_means", "v_quats", "v_scales", "v_sh", "v_opacities", "view"):
        np.testing.assert_array_equal(out[k], same[k])
    all_dead = vis_rows[2::3]
    c = list(a)
    c[1] = 0                                                     # degree 0: no direction term at all
    c[0] = R.with_stride(case, 1)
    c[7] = np.concatenate([np.zeros_like(vf[:, :3]), vf[:, 3:]], axis=1)
    proj_only = R.vjp(*c)
    np.testing.assert_allclose(out["v_means"][all_dead], proj_only["v_means"][all_dead], rtol=1e-13, atol=1e-13)


def _measure(name):
    worst = {}
    if name == "sweep":
        cases = [(f"{m}-{raw}-{mu}-{aa}", R.scene_case(m, raw, mu=mu), 3, aa, True) for m in R.CAMERAS for raw in (False, True)
                 for mu in R.SWEEP_MU for aa in (False, True)]
    else:
        cases = R.family(name)
    for label, case, deg, aa, with_depth in cases:
        for k, v in R.floors_of(case, deg, aa, with_depth).items():
            worst[k] = max(worst.get(k, 0.0), v)
    return worst


@pytest.mark.parametrize("name", ("sweep",) + R.FAMILIES)
def test_rounding_floors(name):
    """Every family's floor -- the float32 oracle against the float64 one on the same fp32 inputs -- is what the table says
    (the last bits of a float32 torch reduction depend on the CPU's vector width: a measured floor may sit up to 1.5 x
    over its entry, never more), and no entry is over the ceiling: 8 x floor <= 2e-3."""
    worst = _measure(name)
    print(name, {k: f"{v:.2e}" for k, v in worst.items()})
    table = R.FLOORS[name]
    assert set(worst) == set(table), (sorted(worst), sorted(table))
    for k, v in worst.items():
        assert table[k] <= R.CEILING / R.GATE_FACTOR, (name, k, table[k])
        assert v <= R.CEILING / R.GATE_FACTOR, f"{name} {k}: the float32 oracle itself is at {v:.3e}, over the ceiling"
        assert v <= 1.5 * table[k], f"{name} {k}: measured floor {v:.3e} over the table's {table[k]:.3e}"
        assert R.gate(name, k) <= R.CEILING


@pytest.mark.parametrize("name", ["sh_stage", "projection_stage"])
def test_stage_floors(name):
    """The same for the two unfused entry points (mgs_sh_bwd, mgs_projection_bwd)."""
    worst = R.sh_floors() if name == "sh_stage" else R.projection_floors()
    print(name, {k: f"{v:.2e}" for k, v in worst.items()})
    assert set(worst) == set(R.FLOORS[name])
    for k, v in worst.items():
        assert R.FLOORS[name][k] <= R.CEILING / R.GATE_FACTOR and v <= 1.5 * R.FLOORS[name][k], (k, v)
        assert v <= R.CEILING / R.GATE_FACTOR, (k, v)


def test_quaternion_scale_and_clamp_properties():
    """The reference has the two properties the GPU test asks of the kernel: v_quats is orthogonal to q and scales with
    1 / |q|; outside the pinhole frustum clamp the conic does not depend on the clamped camera coordinate."""
    label, case, deg, aa, wd = R.family("quat_norm")[0]
    fp = R.forward_products(case, deg, aa, wd)
    ct = R.triplet_cotangents(case["means"].shape[0], wd)
    out = R.vjp(case, deg, aa, fp["radii"], fp["feats"], ct["v_means2d"], ct["v_conics"], ct["v_feats"], None, ct["v_opac_out"])
    q, vq = case["quats"].astype(np.float64), out["v_quats"]
    assert np.abs((q * vq).sum(-1)).max() <= 1e-12 * np.abs(vq).max()
    for base in (0, 3):
        np.testing.assert_allclose(vq[base] * 0.1, vq[base + 1], rtol=1e-6)      # quats are fp32-rounded multiples of one another
        np.testing.assert_allclose(vq[base + 2] * 10, vq[base + 1], rtol=1e-6)
    label, case, deg, aa, wd = R.family("pinhole_clamp")[0]
    n = case["means"].shape[0]
    fp = R.forward_products(case, 0, False, False)
    z = lambda *s: np.zeros(s, np.float32)
    out = R.vjp(case, 0, False, fp["radii"], fp["feats"], z(n, 2), R.cotangents(n)["v_conics"], z(n, 3), None, None)
    v_cam = out["v_means"] @ case["viewmat"][:3, :3].astype(np.float64).T        # cotangent of the camera point
    big = np.abs(v_cam[:8]).max()
    for i in range(8):                                                           # (xp in, xp out, xn in, xn out, yp .., yn ..)
        axis, outside = (0 if i < 4 else 1), i % 2 == 1
        assert (abs(v_cam[i, axis]) <= 1e-8 * big) == outside, (i, v_cam[i])
