"""CPU tests of tests/project_color_fwd_ref.py, the fp64 reference the GPU stage tests of the fused projection + colour
forward (tests/test_gpu_project_color_fwd.py) hold the kernels to: the restatement against the oracle's own project, the
rounding floor of every family with its ceiling, that every row of every family is decided, the reference's semantics (culled
rows, the clamp at 0, the depth channel, radii_y), and the device math compiled for the host (tests/host_harness/
project_color_fwd.cpp: project_gaussian<CAM>, the activations, sh_dot and the clamp chained as the kernel chains them) inside
the very gates the GPU test uses -- before any GPU run."""
import ctypes
import os
import subprocess

import numpy as np
import pytest
import torch

import project_color_fwd_ref as FR
import project_color_ref as R
from oracle import gs_oracle_torch as OT

HERE = os.path.dirname(os.path.abspath(__file__))
F = np.float32


@pytest.mark.parametrize("name", FR.FAMILIES)
def test_forward_floors(name):
    """Every FWD_FLOORS entry is what the float32 run measures (committed within [measured, 1.5 x measured]: the last bits of
    a float32 torch reduction depend on the CPU's vector width), every gate is under its ceiling, the float32 run takes every
    decision as the float64 run does, and EVERY row of every run is decided: the cap on undecided rows is zero."""
    worst = FR.family_floors(name)
    table = FR.FWD_FLOORS[name]
    print(name, {k: f"{v:.2e}" for k, v in worst.items()})
    assert set(table) == set(FR.OUTPUTS + FR.DECISIONS)
    for k, v in worst.items():
        assert v <= table[k] <= 1.5 * v, f"{name} {k}: measured {v:.3e}, committed {table[k]:.3e}"
    for k in FR.OUTPUTS:
        assert FR.gate(name, k) <= FR.CEILING[k], (name, k)
    for run in FR.family(name):
        r64, r32 = FR.reference(run), FR.reference(run, torch.float32)
        for k in ("vis", "radii", "radii_y"):
            assert np.array_equal(r64[k], r32[k]), f"{name} {run['label']}: the float32 run differs in {k}"
        assert np.array_equal(r64["pre"][r64["vis"]] > 0, r32["pre"][r64["vis"]] > 0), f"{name} {run['label']}: clamp state"
        for k, ok in FR.decided(run, r64, table).items():
            bad = np.flatnonzero(~ok)
            assert not len(bad), f"{name} {run['label']}: rows {bad[:8]} are undecided in {k} (margins {FR.margins(r64)[k][bad[:8]]})"
        if name == "sweep":
            assert r64["vis"].sum() > 100
        if name == "aa_subpixel":                   # the regime the family exists for: every placed row seen, compensations to 1e-4
            placed = slice(0, FR.SUBPIXEL_PLACED)
            if run["rule"] == "classic":
                assert r64["vis"][placed].all(), run["label"]
                assert 0 < r64["comp"][placed].min() < 2e-4, run["label"]
            elif run["aa"]:                             # and under the per-axis rule the anti-aliased opacity drops under 1 / 255
                assert (~r64["vis"][placed]).any() and r64["vis"][placed].any(), run["label"]


@pytest.mark.parametrize("name", FR.FAMILIES)
def test_forward_restates_the_oracle(name):
    """forward() is OT.project + OT.spherical_harmonics (under lens_ref's lens for fisheye_kb) with the kernel's fp32 thresholds:
    the same decisions, the same numbers to 1e-9 -- to 1e-5 under the lens, whose coefficients and u_max are the fp32 ones here
    and the double ones there (3e-8 apart, and amplified next to the fold)."""
    for run in FR.family(name):
        case, ref = run["case"], FR.reference(run)
        t = lambda a: torch.tensor(np.asarray(a, np.float64))
        s = torch.exp(t(case["scales"])) if case["raw"] else t(case["scales"])
        o = torch.sigmoid(t(case["opac"])) if case["raw"] else t(case["opac"])
        model = "fisheye" if case["model"] == "fisheye_kb" else case["model"]
        with R._lens_ctx(case):
            p = OT.project(t(case["means"]), t(case["quats"]), s, t(case["viewmat"]), t(case["K"]), FR.W, FR.H, eps2d=FR.EPS2D,
                           near_plane=FR.f32(run["near"]), far_plane=FR.f32(run["far"]), radius_clip=run["radius_clip"],
                           radius_rule=run["rule"], opacities=o, antialiased=run["aa"], camera_model=model)
        radii = p["radii"].numpy()
        rx, ry = (radii, radii) if run["rule"] == "classic" else (radii[:, 0], radii[:, 1])
        what = f"{name} {run['label']}"
        rtol = 1e-5 if case["model"] == "fisheye_kb" else 1e-9
        assert np.array_equal(rx, ref["radii"]) and np.array_equal(ry, ref["radii_y"]), what
        for mine, theirs in (("means2d", "means2d"), ("depths", "depths"), ("conics", "conics"), ("comp", "compensations")):
            np.testing.assert_allclose(ref[mine], p[theirs].numpy(), rtol=rtol, atol=1e-12, err_msg=f"{what} {mine}")
        if run["rule"] == "classic":
            assert np.array_equal(ref["radii"], ref["radii_y"]), what
        vis = ref["vis"]
        vm = t(case["viewmat"])
        campos = -vm[:3, :3].T @ vm[:3, 3]
        sh = torch.nan_to_num(t(case["sh"]))
        pre = (OT.spherical_harmonics(run["deg"], t(case["means"]) - campos, sh) + 0.5).numpy()
        np.testing.assert_allclose(ref["pre"][vis], pre[vis], rtol=1e-12, atol=1e-13, err_msg=what)


def test_reference_semantics():
    """What a culled row holds, the depth channel, the record's layout, and the clamp at exactly 0."""
    for run in FR.family("sparse_waves")[:3]:
        ref, keep = FR.reference(run), FR.sparse_keep(run)
        assert np.array_equal(ref["vis"], keep)
        cul = ~ref["vis"]
        for k in ("radii", "radii_y", "means2d", "depths", "conics", "comp", "feats", "record"):
            assert not np.asarray(ref[k])[cul].any(), k
            assert np.isfinite(np.asarray(ref[k], np.float64)).all(), k
        if run["aa"]:
            assert not ref["opac_out"][cul].any() and np.array_equal(FR.culled(ref, "opac_out"), np.zeros(193))
        else:                                                                   # the kept-plain form: the activated opacity
            assert np.array_equal(ref["opac_out"], ref["opacity"]) and (FR.culled(ref, "opac_out")[cul] > 0).all()
        assert ref["feats"].shape[1] == (4 if run["with_depth"] else 3)
        v = ref["vis"]
        rec = ref["record"][v]
        assert np.array_equal(rec[:, 0:2], ref["means2d"][v]) and np.array_equal(rec[:, 2:5], ref["conics"][v])
        assert np.array_equal(rec[:, 5], ref["opac_out"][v]) and np.array_equal(rec[:, 6:9], ref["feats"][v, :3])
        assert np.array_equal(rec[:, 9], ref["depths"][v] if run["with_depth"] else np.zeros(v.sum())) and not rec[:, 10:].any()
        if run["with_depth"]:
            assert np.array_equal(ref["feats"][:, 3], ref["depths"])
    # the clamp: a channel whose colour is exactly 0 before the clamp is dead (0, not > 0), one below it as well.  Degree 0
    # with a float64 coefficient c such that C0 x c is exactly -0.5 in float64
    c0 = -0.5 / 0.2820947917738781
    for _ in range(64):
        if 0.2820947917738781 * c0 == -0.5:
            break
        c0 = np.nextafter(c0, 0.0 if 0.2820947917738781 * c0 < -0.5 else -10.0)
    assert 0.2820947917738781 * c0 == -0.5
    case = dict(R.with_stride(R.visible_case(4), 1))
    sh = np.zeros((4, 1, 3))
    sh[0, 0] = (c0, c0 * (1 + 1e-12), c0 * (1 - 1e-12))
    sh[1, 0] = 1.0
    case["sh"] = sh
    ref = FR.forward(case, 0, False, False)
    assert ref["vis"].all() and ref["pre"][0, 0] == 0.0 and ref["pre"][0, 1] < 0.0 < ref["pre"][0, 2]
    assert ref["feats"][0, 0] == 0.0 and ref["feats"][0, 1] == 0.0 and ref["feats"][0, 2] == ref["pre"][0, 2] > 0
    assert not np.signbit(ref["feats"][0, :2]).any()
    assert np.array_equal(ref["feats"][0] > 0, [False, False, True])


def test_cull_exact_is_exact():
    """On cull_exact's placed rows the float32 and float64 runs form the decided quantities without any rounding -- bit-equal --
    and take the comparison the same way: `<=` / `>=` cull ON the screen edge, `>=` / `<=` keep ON the near / far plane, a
    radius equal to radius_clip is culled, an opacity one ulp under 1/255 is culled under the per-axis rule."""
    for run in FR.family("cull_exact"):
        r64, r32 = FR.reference(run), FR.reference(run, torch.float32)
        for row, visible in FR.EXACT_EXPECT:
            assert r64["vis"][row] == visible == r32["vis"][row], (run["label"], row)
        q6, q3 = r64["q"], r32["q"]
        for k in ("mx", "my", "z"):
            rows = sorted(set(run["exact"]["edge"] + run["exact"]["near"] + run["exact"]["far"]))
            assert np.array_equal(q6[k][rows], q3[k][rows]) and np.array_equal(q6[k][rows], q6[k][rows].astype(F)), (run["label"], k)
        assert np.array_equal(q6["mx"][[0, 2]] + q6["rx"][[0, 2]] * [1, -1], [0.0, FR.W])
        assert np.array_equal(q6["my"][[4, 6]] + q6["ry"][[4, 6]] * [1, -1], [0.0, FR.H])
        assert np.array_equal(q6["z"][8:12].astype(F), np.array([4.0, 20.0, np.nextafter(F(4), F(0)), np.nextafter(F(20), F(30))], F))
        assert max(q6["rx"][12], q6["ry"][12]) == FR.EXACT_CLIP and min(q6["rx"][:12].min(), q6["ry"][:12].min()) > FR.EXACT_CLIP
        if run["rule"] == "opacity_aware":
            assert not r64["vis"][13] and r64["vis"][14] and not r32["vis"][13] and r32["vis"][14]
            if not run["aa"]:
                assert q6["op"][13] == float(np.nextafter(F(FR.T255), F(0))) == q3["op"][13]


# ---------------------------------------------------------------------------------------------------------------------
# the device math on the host
# ---------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def hh(tmp_path_factory):
    so = tmp_path_factory.mktemp("hh_pcf") / "libhh_pcf.so"
    subprocess.run(["g++", "-O2", "-std=c++17", "-shared", "-fPIC", os.path.join(HERE, "host_harness", "project_color_fwd.cpp"),
                    "-o", str(so)], check=True)
    return ctypes.CDLL(str(so))


def _p(a):
    return a.ctypes.data_as(ctypes.c_void_p)


def host_forward(hh, run, opac=None):
    case = run["case"]
    n, stride = case["means"].shape[0], case["sh"].shape[1]
    c = lambda a: np.ascontiguousarray(a, dtype=F)
    out = {"radii": np.zeros(n, np.int32), "radii_y": np.zeros(n, np.int32), "means2d": np.zeros((n, 2), F), "depths": np.zeros(n, F),
           "conics": np.zeros((n, 3), F), "comp": np.zeros(n, F), "opac_out": np.zeros(n, F), "pre": np.zeros((n, 3), F),
           "feats": np.zeros((n, 4), F)}
    keep = [c(case[k]) for k in ("means", "quats", "scales")] + [c(case["opac"] if opac is None else opac), c(case["sh"]),
                                                                  c(case["viewmat"]), c(R.camera_row(case))]
    rc = hh.hh_project_color_fwd(R.CAMERA_ID[case["model"]], run["deg"], n, _p(keep[0]), _p(keep[1]), _p(keep[2]), _p(keep[3]), stride,
                                 _p(keep[4]), _p(keep[5]), _p(keep[6]), FR.W, FR.H, ctypes.c_float(FR.EPS2D), ctypes.c_float(run["near"]),
                                 ctypes.c_float(run["far"]), ctypes.c_float(run["radius_clip"]), FR.RULE_ID[run["rule"]],
                                 (1 if case["raw"] else 0) | (2 if run["aa"] else 0), *[_p(v) for v in out.values()])
    assert rc == 0
    if not run["with_depth"]:
        out["feats"] = out["feats"][:, :3]
    return out


@pytest.mark.parametrize("name", FR.FAMILIES)
def test_device_math_on_the_host(hh, name):
    """The shipped arithmetic (csrc/mgs_math.h, g++) on every run of every family, held exactly as the GPU test holds the kernel:
    radii, visibility and clamp state exact, every row of every output inside 8 x floor."""
    worst = {}
    for run in FR.family(name):
        got = host_forward(hh, run)
        for k, v in FR.hold_rows(name, FR.reference(run), got, f"host {run['label']}", tag="PCF-host").items():
            worst[k] = max(worst.get(k, 0.0), v)
    print(f"PCF-host-worst {name} " + " ".join(f"{k}={v:.2f}" for k, v in worst.items()))


def test_opacity_exactly_at_the_threshold_is_culled_by_its_extent(hh):
    """Why cull_exact has no `opacity == 1/255 is kept` row: 255 x fp32(1/255) rounds to 1.0f, the extent sqrt(2 ln 1) is exactly
    0 and the device math culls the row by `radius > 0` -- whichever way the opacity itself compares -- while in float64 the
    product is 1 + 5.9e-8, the extent 3.4e-4 and the radius 1.  One ulp above the threshold the same happens; the opacity test's
    own `>=` cannot be seen in any output."""
    run = [r for r in FR.family("cull_exact") if r["rule"] == "opacity_aware" and not r["aa"]][0]
    opac = run["case"]["opac"].copy()
    opac[13] = F(FR.T255)
    got = host_forward(hh, run, opac=opac)
    ref = FR.forward(dict(run["case"], opac=opac), run["deg"], False, True, "opacity_aware", near=run["near"], far=run["far"],
                     radius_clip=0.0)
    assert got["radii"][13] == 0 and ref["radii"][13] == 1 and ref["q"]["op"][13] == FR.T255
    assert float(F(FR.T255) * F(255)) == 1.0


def test_sh_stage_floor():
    v = FR.sh_floor()
    table = FR.FWD_FLOORS["sh_stage"]["colour"]
    print(f"sh_stage colour {v:.2e}")
    assert v <= table <= 1.5 * v and FR.GATE_FACTOR * table <= FR.CEILING["colour"]


def test_sh_colors_is_the_oracle():
    dirs, coeffs, _ = R.sh_case(65)
    for deg in range(4):
        want = OT.spherical_harmonics(deg, torch.tensor(dirs.astype(np.float64)), torch.tensor(coeffs.astype(np.float64))).numpy()
        np.testing.assert_allclose(FR.sh_colors(deg, dirs, coeffs), want, rtol=1e-13, atol=1e-14)
        z = FR.sh_colors(deg, np.zeros((65, 3)), coeffs)                        # a zero-length direction: the unit direction is 0
        want0 = 0.2820947917738781 * coeffs[:, 0].astype(np.float64)
        if deg >= 2:                                                            # (Y_6 = 0.946 z^2 - 0.315 keeps its constant)
            want0 = want0 - 0.3153915652525201 * coeffs[:, 6].astype(np.float64)
        np.testing.assert_allclose(z, want0, rtol=1e-14, atol=1e-15)
    m = np.arange(65) % 3 == 0
    assert not FR.sh_colors(3, dirs, coeffs, m)[~m].any()
