"""The fp64 reference of the fused projection + colour FORWARD (mgs_project_color_fwd, mgs_projection_fwd, mgs_sh_fwd in
robosimgs_amd/csrc/projection.hip).  A helper module, not a test file: tests/test_project_color_fwd_host.py keeps it honest on
the CPU (against oracle/gs_oracle_torch.py and against the device math compiled for the host),
tests/test_gpu_project_color_fwd.py holds the kernels to it row by row.

Built on tests/project_color_ref.py (cases, families, camera rows, the scaled error) and on the oracle's parts
(quat_to_rotmat, the camera models' mean and Jacobian, spherical_harmonics).  The projection is restated here and not called
as OT.project because the forward's DECISIONS need what OT.project does not return: the pre-ceil extents, theta^2, the culled
opacity, and every threshold as the fp32 constant the kernel compares with.  tests/test_project_color_fwd_host.py asserts that
the restatement and OT.project agree.

Method (that of project_color_ref, applied to the forward).  `forward(..., dtype=torch.float32)` is the same statement in
float32, an independent fp32 evaluation; its row error against the float64 run is the FLOOR of a family and output, the GPU gate
is GATE_FACTOR (8) x floor, and no gate exceeds CEILING -- what tests/test_gpu_forward.py already allows.  Every row is held;
nothing is sized for flips.  What makes that possible is the decision margin: for every row, the distance of each decided
quantity from its threshold, against 8 x the float32 run's own error in that quantity (`decided`).  No family has an undecided
row, so radii, visibility and the colour clamp's state are compared exactly.

The extent's margin and error under the per-axis rule are both divided by kappa = 1 + 1 / (2 ln(255 op)), the condition number
of the extent sqrt(2 ln(255 op)) in the opacity: next to op = 1/255 the extent goes to zero and ANY arithmetic loses its
relative accuracy there in proportion to kappa, so a family's one floor would otherwise be set by its faintest row.

Error measures (`row_error`):  means2d: largest |error| of the row in pixels;  depths, comp (compensation and opac_out):
relative;  conics, colour (the pre-clamp colour and feats): largest |error| of the row over the row's largest |entry|.
A floor below the format's own half ulp (2^-24 relative; 2^-24 x 256 px for the pixel quantities) is raised to it (UNIT): a row
family whose arithmetic happens to be exact in the float32 oracle says nothing about the rounding of a fused multiply-add.
"""
from __future__ import annotations

import functools
import math

import numpy as np
import torch

import lens_ref as LR
import project_color_ref as R
from oracle import camera_models as CM
from oracle import gs_oracle_torch as OT

W, H, EPS2D, NEAR = R.W, R.H, R.EPS2D, R.NEAR
FAR = 1e10
GATE_FACTOR = R.GATE_FACTOR
F32 = np.float32
# the kernel's own fp32 constants, held as Python floats (as EPS2D is)
T255 = float(F32(1) / F32(255))          # `op >= 1.0f / 255.0f`
EXTENT_MAX = float(F32(3.33))
EMPTY_WORD = 1 << 20                     # kEmptyTileRect (csrc/tile_rect.h)
RULE_ID = {"classic": 0, "opacity_aware": 1}
RULES = tuple(RULE_ID)

OUTPUTS = ("means2d", "depths", "conics", "comp", "colour")
DECISIONS = ("near", "far", "u", "op", "extent", "edge", "clamp")
# what tests/test_gpu_forward.py::test_projection_matches_oracle and ::test_spherical_harmonics_matches_oracle allow
CEILING = {"means2d": 2e-3, "depths": 1e-5, "conics": 2e-4, "comp": 2e-4, "colour": 1e-4}
_HALF_ULP = 2.0 ** -24
UNIT = {k: _HALF_ULP for k in OUTPUTS + DECISIONS}
UNIT["means2d"] = UNIT["edge"] = _HALF_ULP * 256.0


def f32(x):
    return float(F32(x))


# ------------------------------------------------------------------------------------------------------------------
# the forward
# ------------------------------------------------------------------------------------------------------------------
def forward(case, deg, aa, with_depth=True, rule="classic", dtype=torch.float64, *, near=NEAR, far=FAR, radius_clip=0.0,
            has_opacity=True):
    """Every product of mgs_project_color_fwd for one case, as float64 numpy arrays (evaluated in `dtype`):
    radii / radii_y i32 [N] (equal under "classic"), vis bool [N], means2d [N,2], depths [N], conics [N,3], comp [N] (the
    compensation), opacity [N] (activated), opac_out [N] (opacity x comp if aa else opacity), pre [N,3] (the colour before
    the clamp, unmasked), feats [N,3|4], record [N,12]; and `q`, the decided quantities with the masks of the rows that reach
    each decision.  Culled rows hold what the kernel writes (`culled`): zeros, but the ACTIVATED opacity in opac_out when not
    anti-aliased (the kept-plain form).  has_opacity=False: the per-axis rule without opacities (mgs_projection_fwd)."""
    t = lambda a: torch.tensor(np.asarray(a, dtype=np.float64), dtype=dtype)
    means, quats, scales, opac, sh, vm, K = (t(case[k]) for k in ("means", "quats", "scales", "opac", "sh", "viewmat", "K"))
    near, far, clip = f32(near), f32(far), f32(radius_clip)
    s = torch.exp(scales) if case["raw"] else scales
    o = torch.sigmoid(opac) if case["raw"] else opac
    Rcw, tcw = vm[:3, :3], vm[:3, 3]
    fx, fy, cx, cy = K[0, 0], K[1, 1], K[0, 2], K[1, 2]
    x, y, z = (means @ Rcw.T + tcw).unbind(-1)
    keep_z = (z >= near) & (z <= far)
    zs = torch.where(keep_z, z, torch.ones_like(z))
    M = OT.quat_to_rotmat(quats) * s[:, None, :]
    cov_c = Rcw @ (M @ M.transpose(1, 2)) @ Rcw.T
    model = case["model"]
    u, keep_u = None, torch.ones_like(keep_z)
    if model == "pinhole":
        tanx, tany = 0.5 * W / fx, 0.5 * H / fy
        lim_xp, lim_xn = (W - cx) / fx + 0.3 * tanx, cx / fx + 0.3 * tanx
        lim_yp, lim_yn = (H - cy) / fy + 0.3 * tany, cy / fy + 0.3 * tany
        rz = 1.0 / zs
        tx = zs * torch.minimum(lim_xp, torch.maximum(-lim_xn, x * rz))
        ty = zs * torch.minimum(lim_yp, torch.maximum(-lim_yn, y * rz))
        zero = torch.zeros_like(rz)
        Jt = (fx * rz, zero, -fx * tx * rz * rz, zero, fy * rz, -fy * ty * rz * rz)
        mu = (fx * x * rz + cx, fy * y * rz + cy)
    elif model == "fisheye_kb":
        k32 = [f32(v) for v in case["lens"]]                 # the camera row is fp32
        mu, Jt = LR.mean_and_J(x, y, zs, fx, fy, cx, cy, k32, torch)
        u = LR.u_of(x, y, zs, torch)
        keep_u = u < f32(LR.theta_max(case["lens"]) ** 2)
    else:
        mu, Jt = CM.mean_and_J(x, y, zs, fx, fy, cx, cy, model, torch)
    J = torch.stack(Jt, dim=-1).reshape(-1, 2, 3)
    cov2 = J @ cov_c @ J.transpose(1, 2)
    mx, my = mu
    a, b, c = cov2[:, 0, 0], cov2[:, 0, 1], cov2[:, 1, 1]
    det0 = a * c - b * b
    a, c = a + EPS2D, c + EPS2D
    det = a * c - b * b
    keep_det = det > 0
    dets = torch.where(keep_det, det, torch.ones_like(det))
    comp = torch.sqrt(torch.clamp(det0 / dets, min=0.0))
    conic = torch.stack([c / dets, -b / dets, a / dets], dim=-1)
    op, keep_op, kappa = None, torch.ones_like(keep_z), torch.ones_like(z)
    if rule == "classic":
        m = 0.5 * (a + c)
        pre_x = 3.0 * torch.sqrt(m + torch.sqrt(torch.clamp(m * m - dets, min=0.01)))
        pre_y = pre_x
    else:
        ext = torch.full_like(a, EXTENT_MAX)
        if has_opacity:
            op = o * comp if aa else o
            keep_op = op >= T255
            lg = 2.0 * torch.log(torch.where(keep_op, op, torch.ones_like(op)) * 255.0)
            ext = torch.minimum(ext, torch.sqrt(lg))
            kappa = torch.where(lg > 0, 1.0 + 1.0 / lg, kappa)
        pre_x, pre_y = ext * torch.sqrt(a), ext * torch.sqrt(c)
    rx, ry = torch.ceil(pre_x), torch.ceil(pre_y)
    if rule == "classic":
        keep_clip = rx > clip
    else:
        keep_clip = ((rx > clip) | (ry > clip)) & (rx > 0) & (ry > 0)
    keep_screen = ~((mx + rx <= 0) | (mx - rx >= W) | (my + ry <= 0) | (my - ry >= H))
    reach_u = keep_z
    reach_op = reach_u & keep_u & keep_det
    reach_clip = reach_op & keep_op
    reach_screen = reach_clip & keep_clip
    vis = reach_screen & keep_screen

    campos = -Rcw.T @ tcw
    d = means - campos
    n2 = (d * d).sum(-1, keepdim=True)
    inv = torch.where(n2 > 0, 1.0 / torch.sqrt(torch.where(n2 > 0, n2, torch.ones_like(n2))), torch.zeros_like(n2))
    pre = torch.einsum("nk,nkc->nc", OT.sh_basis(deg, d * inv), sh[:, :(deg + 1) ** 2]) + 0.5

    zero1 = torch.zeros_like(z)
    w1 = lambda v: torch.where(vis, v, zero1)
    w2 = lambda v: torch.where(vis[:, None], v, torch.zeros_like(v))
    comp_v = w1(comp)
    rgb = w2(torch.clamp(pre, min=0.0))
    out = {"vis": vis, "radii": w1(rx).to(torch.int32), "radii_y": w1(ry).to(torch.int32),
           "means2d": w2(torch.stack([mx, my], -1)), "depths": w1(z), "conics": w2(conic), "comp": comp_v, "opacity": o,
           "opac_out": o * comp_v if aa else o, "pre": pre,
           "feats": torch.cat([rgb, w1(z)[:, None]], -1) if with_depth else rgb}
    rec_op = out["opac_out"] if has_opacity else zero1
    out["record"] = w2(torch.stack([out["means2d"][:, 0], out["means2d"][:, 1], out["conics"][:, 0], out["conics"][:, 1],
                                    out["conics"][:, 2], rec_op, rgb[:, 0], rgb[:, 1], rgb[:, 2],
                                    w1(z) if with_depth else zero1, zero1, zero1], -1))
    res = {k: v.double().numpy() if v.dtype.is_floating_point else v.numpy() for k, v in out.items()}
    nan = torch.full_like(z, float("nan"))
    q = {"z": z, "u": nan if u is None else u, "op": nan if op is None else op, "pre_x": pre_x, "pre_y": pre_y, "mx": mx, "my": my,
         "rx": rx, "ry": ry, "kappa": kappa}
    res["q"] = {k: v.double().numpy() for k, v in q.items()}
    res["reach"] = {"near": np.ones(len(z), bool), "far": np.ones(len(z), bool),
                    "u": reach_u.numpy() & (u is not None), "op": reach_op.numpy() & (op is not None),
                    "extent": reach_clip.numpy(), "edge": reach_screen.numpy(), "clamp": vis.numpy()}
    res["settings"] = {"near": near, "far": far, "clip": clip, "aa": bool(aa), "rule": rule, "with_depth": bool(with_depth),
                       "u_max": f32(LR.theta_max(case["lens"]) ** 2) if model == "fisheye_kb" else None}
    return res


def culled(ref, name):
    """What a culled row holds in output `name`, [N, ...]: zeros; opac_out of the kept-plain form holds the activated opacity."""
    if name == "opac_out" and not ref["settings"]["aa"]:
        return ref["opacity"]
    return np.zeros_like(np.asarray(ref[name], dtype=np.float64))


def sh_colors(deg, dirs, coeffs, masks=None, dtype=torch.float64):
    """mgs_sh_fwd: sum_k Y_k(dir / |dir|) coeff_k.  A zero-length direction has the unit direction 0 (sh_dot: inv = 0), and the
    basis polynomials are evaluated there: C0 x coeff_0 at degrees 0 and 1, and from degree 2 on also Y_6(0) = -0.3154 times
    coeff_6 -- Y_6 = 0.946 z^2 - 0.315 is the one basis function with a constant term.  Masked rows are 0 whatever their
    coefficients hold (NaN included: they are not read)."""
    d = torch.tensor(np.asarray(dirs, np.float64), dtype=dtype)
    c = torch.tensor(np.asarray(coeffs, np.float64), dtype=dtype)
    n2 = (d * d).sum(-1, keepdim=True)
    inv = torch.where(n2 > 0, 1.0 / torch.sqrt(torch.where(n2 > 0, n2, torch.ones_like(n2))), torch.zeros_like(n2))
    col = torch.einsum("nk,nkc->nc", OT.sh_basis(deg, d * inv), torch.nan_to_num(c[:, :(deg + 1) ** 2], nan=0.0))
    col = col.double().numpy()
    if masks is not None:
        col = np.where(np.asarray(masks, bool)[:, None], col, 0.0)
    return col


# ------------------------------------------------------------------------------------------------------------------
# errors, margins, decisions
# ------------------------------------------------------------------------------------------------------------------
def row_error(key, got, ref, scale_ref=None):
    """[M] row errors of `got` against `ref` in the measure of `key` (module docstring).  colour: scale_ref = the pre-clamp
    reference whose largest entry scales the row (feats are compared against the clamped colour at the unclamped scale)."""
    ref = np.asarray(ref, dtype=np.float64)
    got = np.asarray(got, dtype=np.float64).reshape(ref.shape)
    d = np.abs(got - ref).reshape(len(ref), -1)
    with np.errstate(invalid="ignore", divide="ignore"):
        if key == "means2d":
            e = d.max(1)
        elif key in ("depths", "comp"):
            e = np.where(d[:, 0] == 0, 0.0, d[:, 0] / np.abs(ref.reshape(-1)))
        else:
            sc = np.abs(ref if scale_ref is None else np.asarray(scale_ref, np.float64)).reshape(len(ref), -1).max(1)
            e = np.where(d.max(1) == 0, 0.0, d.max(1) / sc)
    return np.where(np.isfinite(e), e, np.inf)


def margins(ref):
    """{decision: [N] distance of the decided quantity from its threshold} for a float64 `forward`, in the units of `errors`;
    inf where the row does not reach the decision."""
    q, st, reach = ref["q"], ref["settings"], ref["reach"]
    inf = np.full(len(q["z"]), np.inf)
    with np.errstate(invalid="ignore", divide="ignore"):
        m = {"near": np.abs(q["z"] - st["near"]) / abs(st["near"]), "far": np.abs(q["z"] - st["far"]) / abs(st["far"])}
        m["u"] = np.abs(q["u"] - st["u_max"]) / st["u_max"] if st["u_max"] is not None else inf
        m["op"] = np.abs(q["op"] - T255) / T255
        e = inf
        for p in (q["pre_x"], q["pre_y"]):                   # from the nearest integer and from radius_clip, relative
            e = np.minimum(e, np.minimum(np.abs(p - np.round(p)), np.abs(p - st["clip"]) if st["clip"] > 0 else np.inf) / p)
        m["extent"] = e / q["kappa"]
        m["edge"] = np.minimum.reduce([np.abs(q["mx"] + q["rx"]), np.abs(q["mx"] - q["rx"] - W), np.abs(q["my"] + q["ry"]),
                                       np.abs(q["my"] - q["ry"] - H)])
        m["clamp"] = np.abs(ref["pre"]).min(1) / np.abs(ref["pre"]).max(1)
    return {k: np.where(reach[k] & np.isfinite(v), v, np.inf) for k, v in m.items()}


def errors(r32, r64):
    """{decision: [N] error of the float32 run in the decided quantity}, nan-free: rows that do not reach the decision in the
    float64 run give 0."""
    q3, q6, st, reach = r32["q"], r64["q"], r64["settings"], r64["reach"]
    with np.errstate(invalid="ignore", divide="ignore"):
        dz = np.abs(q3["z"] - q6["z"])
        e = {"near": dz / abs(st["near"]), "far": dz / abs(st["far"]),
             "u": np.abs(q3["u"] - q6["u"]) / (st["u_max"] or 1.0), "op": np.abs(q3["op"] - q6["op"]) / T255,
             "extent": np.maximum(np.abs(q3["pre_x"] - q6["pre_x"]) / q6["pre_x"], np.abs(q3["pre_y"] - q6["pre_y"]) / q6["pre_y"]) / q6["kappa"],
             "edge": np.maximum(np.abs(q3["mx"] - q6["mx"]), np.abs(q3["my"] - q6["my"])),
             "clamp": np.abs(r32["pre"] - r64["pre"]).max(1) / np.abs(r64["pre"]).max(1)}
    return {k: np.where(reach[k], np.nan_to_num(v, nan=np.inf, posinf=np.inf), 0.0) for k, v in e.items()}


def exact_rows(run, n):
    """{decision: bool [N]}: the rows a builder placed so that the decided quantity is formed without any rounding in fp32
    (cull_exact).  There the float32 run's error is zero -- the host test asserts it, to the bit -- and a margin of zero, the
    threshold itself, is decided."""
    out = {}
    for k in DECISIONS:
        mk = np.zeros(n, bool)
        mk[list(run.get("exact", {}).get(k, ()))] = True
        out[k] = mk
    return out


def measure(run):
    """One run in float64 and float32 -> (r64, r32, {key: floor}, {decision: bool [N] decided})  -- the floors of this run
    alone, outputs on the rows visible in both."""
    r64, r32 = reference(run), reference(run, torch.float32)
    both = r64["vis"] & r32["vis"]
    fl = {"means2d": row_error("means2d", r32["means2d"][both], r64["means2d"][both]),
          "depths": row_error("depths", r32["depths"][both], r64["depths"][both]),
          "conics": row_error("conics", r32["conics"][both], r64["conics"][both]),
          "comp": np.maximum(row_error("comp", r32["comp"][both], r64["comp"][both]),
                             row_error("comp", r32["opac_out"][both], r64["opac_out"][both])),
          "colour": row_error("colour", r32["pre"][both], r64["pre"][both])}
    fl = {k: float(v.max()) if v.size else 0.0 for k, v in fl.items()}
    ex = exact_rows(run, len(both))
    for k, v in errors(r32, r64).items():
        fl[k] = float(v[~ex[k]].max()) if (~ex[k]).any() else 0.0
    return r64, r32, fl


def decided(run, r64, floors):
    """{decision: bool [N]}: margin >= GATE_FACTOR x the family's floor in that quantity (or a row placed exactly)."""
    ex = exact_rows(run, len(r64["vis"]))
    return {k: (v >= GATE_FACTOR * max(floors[k], UNIT[k])) | ex[k] for k, v in margins(r64).items()}


def gate(family_name, key):
    g = GATE_FACTOR * max(FWD_FLOORS[family_name][key], UNIT[key])
    assert key not in CEILING or g <= CEILING[key] * (1 + 1e-12), (family_name, key, g)
    return g


def bits(a):
    return np.ascontiguousarray(a, dtype=F32).view(np.int32)


# (gate key, name in `got`, name in the reference)
HELD = (("means2d", "means2d", "means2d"), ("depths", "depths", "depths"), ("conics", "conics", "conics"), ("comp", "comp", "comp"),
        ("comp", "opac_out", "opac_out"), ("colour", "pre", "pre"), ("colour", "feats", "feats"))


def hold_rows(name, ref, got, what, tag="PCF", rows=None):
    """One launch (or one host run) against the float64 reference `ref`, row by row.  got: {name: array} of whichever outputs
    exist (radii, radii_y, means2d, depths, conics, comp, opac_out, pre, feats [n,3|4]).  Radii, visibility and the clamp's
    state exactly; every visible row of every output within the family's gate; every culled row bit for bit what `culled`
    says (a kept-plain opac_out holds an fp32 activation there, which is held as a value).  rows: the first `rows` rows only.
    Prints one line per output and returns {output name: worst error / gate}."""
    n = len(ref["vis"]) if rows is None else rows
    vis = ref["vis"][:n]
    assert np.array_equal(np.asarray(got["radii"])[:n], ref["radii"][:n]), \
        f"{what}: radii differ on rows {np.flatnonzero(np.asarray(got['radii'])[:n] != ref['radii'][:n])[:8]}"
    if "radii_y" in got:
        assert np.array_equal(np.asarray(got["radii_y"])[:n], ref["radii_y"][:n]), f"{what}: radii_y differ"
    ratios = {}
    for key, gn, rn in HELD:
        if gn not in got:
            continue
        g, r = np.asarray(got[gn])[:n], np.asarray(ref[rn], dtype=np.float64)[:n]
        assert np.isfinite(g).all(), f"{what} {gn}: not finite on rows {np.flatnonzero(~np.isfinite(g).reshape(n, -1).all(1))[:8]}"
        if gn == "pre":
            r = np.where(vis[:, None], r, 0.0)                      # (the harness reports 0 where it does not evaluate)
        held = vis
        if gn == "opac_out" and not ref["settings"]["aa"]:
            held = np.ones(n, bool)
        else:
            want = culled(ref, rn)[:n][~held]
            assert np.array_equal(bits(g[~held]), bits(want)), f"{what} {gn}: a culled row does not hold {want[:1]}"
        if not held.any():
            continue
        if gn == "feats":
            live = g[vis, :3] > 0
            assert np.array_equal(live, ref["pre"][:n][vis] > 0), f"{what}: the clamp's state differs"
            e = row_error("colour", g[held, :3], r[held, :3], ref["pre"][:n][held])
            if g.shape[1] == 4:
                ed = row_error("depths", g[held, 3], r[held, 3])
                assert ed.max() <= gate(name, "depths"), f"{what} feats depth: {ed.max():.3e} > {gate(name, 'depths'):.2e}"
        else:
            e = row_error(key, g[held], r[held])
        gt = gate(name, key)
        worst = float(e.max())
        print(f"{tag} {name} {gn} {worst:.3e} gate {gt:.2e} [{what}]")
        assert worst <= gt, f"{what} {gn}: row {np.flatnonzero(held)[int(e.argmax())]} off by {worst:.3e} > {gt:.2e}"
        ratios[gn] = max(ratios.get(gn, 0.0), worst / gt)
    return ratios


# ------------------------------------------------------------------------------------------------------------------
# runs: a case with everything a launch is given.  family(name) -> [run]
# ------------------------------------------------------------------------------------------------------------------
def make_run(label, case, deg, aa, with_depth=True, rule="classic", near=NEAR, far=FAR, radius_clip=0.0, exact=None):
    return {"label": f"{label} {rule}{' aa' if aa else ''}", "case": case, "deg": deg, "aa": bool(aa), "with_depth": bool(with_depth),
            "rule": rule, "near": near, "far": far, "radius_clip": radius_clip, "exact": exact or {}}


_REF_CACHE = {}


def reference(run, dtype=torch.float64, has_opacity=True):
    """forward() of a run, computed once per run object and left unchanged."""
    key = (id(run["case"]), run["label"], dtype, has_opacity)
    if key not in _REF_CACHE:
        _REF_CACHE[key] = (run, forward(run["case"], run["deg"], run["aa"], run["with_depth"], run["rule"], dtype, near=run["near"],
                                        far=run["far"], radius_clip=run["radius_clip"], has_opacity=has_opacity))
    return _REF_CACHE[key][1]


def _both(label, case, deg, with_depth=True, **kw):
    """A case under both radius rules, anti-aliased and not."""
    return [make_run(label, case, deg, aa, with_depth, rule, **kw) for rule in RULES for aa in (False, True)]


# Ranges shrunk to meet the ceilings.
# near_far: project_color_ref's rows sit at z = 1.01 x 0.01 under a camera seven units from the scene.  Camera z then carries
# the absolute rounding of a sum of terms of magnitude 7 (4e-7), which is 3.5e-5 of z: over the depth ceiling (1e-5 / 8) by
# 30 x, and 6.8e-4 px in the mean, whatever the arithmetic.  The forward's family keeps the geometry (1.01 x the near plane;
# huge splats at z = 1e4) and moves the plane: near = 1.0 under the axis camera, where z = 1.01 is a sum of terms of
# magnitude 4.
NEAR_FAR_NEAR = 1.0
# aa_subpixel: every eigenvalue of project_color_ref's family (down to 3e-5 px^2, compensations down to 1e-4), at anisotropy 1
# and 30 only.  Dropped: the 1e3 : 1 needles below one pixel.  On those a c - b^2 cancels (csrc/mgs_math.h, the textbook order)
# and the float32 ORACLE itself is at 4.3e-5 in the relatively held compensation, 8 x which is over the 2e-4 ceiling; without
# them the family's floor is 2e-6.  (project_color_ref keeps 1e3 below a pixel for the backward, whose row-scaled gate is wider,
# and drops it from a pixel up: SUBPIXEL_ANISO_FROM_A_PIXEL_UP.)
FWD_SUBPIXEL_LAMBDA = R.SUBPIXEL_LAMBDA
FWD_SUBPIXEL_ANISO = R.SUBPIXEL_ANISO_FROM_A_PIXEL_UP
SUBPIXEL_PLACED = len(FWD_SUBPIXEL_LAMBDA) * len(FWD_SUBPIXEL_ANISO) * len(R.SUBPIXEL_ANGLES)


def _subpixel(model):
    z, pts, rots, scs = 5.0, [], [], []
    f = float(R.intrinsics("pinhole" if model == "pinhole" else "ortho" if model == "ortho" else "fisheye")[0, 0])
    px_per_unit = f if model == "ortho" else f / z
    for lam in FWD_SUBPIXEL_LAMBDA:
        for an in FWD_SUBPIXEL_ANISO:
            for ang in R.SUBPIXEL_ANGLES:
                s2 = math.sqrt(lam) / px_per_unit
                # (the ideal fisheye's rows stand at x = 0.31: at 0.3 its 100 px^2, 30 : 1 row at 45 degrees has a per-axis
                #  extent within 9e-6 of an integer -- undecided -- and a placed row is moved here, not by `settled`)
                pts.append((0.31 if model == "fisheye" else 0.3, -0.2, z))
                rots.append(R._rot_z(ang))
                scs.append((s2 * math.sqrt(an), s2, s2))
    return pts, rots, scs


# Random scenes put a row next to a threshold now and then (one in a few thousand has a pre-ceil extent within 1e-4 of an
# integer).  Such a row has its INPUT moved -- its scales grown by 0.7 % per step, an opacity next to 1/255 by 5 %, the constant
# colour term of a channel next to the clamp by 0.0028 -- until every margin under both rules, anti-aliased and not, is over
# SETTLE, which is far above any decision's 8 x floor.
SETTLE = {"near": 1e-2, "far": 1e-2, "u": 1e-3, "op": 1e-2, "extent": 1e-4, "edge": 1e-2, "clamp": 1e-4}


def settled(case, deg, placed=0, **kw):
    """placed: the first rows are hand-placed (next to a threshold on purpose) and stay where they are."""
    case = dict(case, scales=case["scales"].copy(), opac=case["opac"].copy(), sh=case["sh"].copy())
    for _ in range(40):
        bad_s, bad_o, bad_c = (np.zeros(len(case["means"]), bool) for _ in range(3))
        for rule in RULES:
            for aa in (False, True):
                for k, v in margins(forward(case, deg, aa, True, rule, **kw)).items():
                    v[:placed] = np.inf
                    {"op": bad_o, "clamp": bad_c}.get(k, bad_s)[v < SETTLE[k]] = True
        if not (bad_s.any() or bad_o.any() or bad_c.any()):
            return case
        case["sh"][bad_c, 0] += F32(0.01)                   # the colour's constant term: 0.0028 in every channel
        if case["raw"]:
            case["scales"][bad_s] += F32(0.007)
            case["opac"][bad_o] += F32(0.05)
        else:
            case["scales"][bad_s] *= F32(1.007)
            case["opac"][bad_o] *= F32(1.05)
    raise AssertionError("a row could not be moved off its thresholds")


@functools.lru_cache(maxsize=None)
def sweep_case(model, raw, mu, stride=16, deg=3):
    """scene_case, settled for the degree it is run at (the clamp's margins are the degree's)."""
    return settled(R.with_stride(R.scene_case(model, raw, mu=mu), stride), deg)


@functools.lru_cache(maxsize=None)
def mixed_case(n=257, raw=True):
    """visible_case with every third row moved behind the camera (reflected through the camera's centre): the case of the
    output-form and row-ownership tests."""
    base = R.visible_case(n, raw=raw)
    vm = base["viewmat"].astype(np.float64)
    campos = -vm[:3, :3].T @ vm[:3, 3]
    hide = np.arange(n) % 3 == 1
    c = dict(base, means=np.where(hide[:, None], (2.0 * campos - base["means"]).astype(F32), base["means"]).astype(F32))
    return settled(c, 3)


@functools.lru_cache(maxsize=None)
def projection_case(n=257):
    """project_color_ref.projection_case (opacities of one, one coefficient), settled."""
    return settled(R.projection_case(n), 0)


def sh_floor():
    """mgs_sh_fwd's floor: the float32 oracle against the float64 one on sh_case's directions (of every length), row-scaled."""
    dirs, coeffs, _ = R.sh_case()
    return max(float(row_error("colour", sh_colors(d, dirs, coeffs, dtype=torch.float32), sh_colors(d, dirs, coeffs)).max())
               for d in range(4))


@functools.lru_cache(maxsize=None)
def family(name):
    if name == "sweep":
        return tuple(r for m in R.CAMERAS for raw in (False, True) for mu in R.SWEEP_MU
                     for r in _both(f"{m}-{'raw' if raw else 'act'}-{mu}", sweep_case(m, raw, mu), 3))
    if name == "aa_subpixel":
        out = []
        for model in R.CAMERAS:
            pts, rots, scs = _subpixel(model)
            for raw in (False, True):
                out += _both(f"{model}-{'raw' if raw else 'act'}", settled(R.placed_case(model, raw, pts, rots, scs, pad_to=100), 0, SUBPIXEL_PLACED), 0, False)
        return tuple(out)
    if name == "near_far":
        out = []
        for model in ("pinhole", "fisheye"):
            n_ = NEAR_FAR_NEAR
            pts = [(0.0, 0.0, 1.01 * n_), (1e-2, -2e-2, 1.01 * n_), (30.0, -20.0, 1e4), (0.0, 0.0, 1e4)]
            scs = [(1e-1, 5e-2, 8e-2)] * 2 + [(300.0, 100.0, 200.0)] * 2
            case = R.placed_case(model, False, pts, [R._rot_z(25)] * 4, scs, viewmat=R.AXIS_VIEWMAT)
            out += _both(model, case, 1, True, near=n_)
        return tuple(out)
    if name in R.FAMILIES:
        return tuple(r for label, case, deg, aa, wd in R.family(name) for r in _both(label, case, deg, wd))
    if name == "cull_margin":
        return tuple(_cull_margin())
    if name == "cull_exact":
        return tuple(_cull_exact())
    if name == "sparse_waves":
        return tuple(_sparse_waves())
    raise KeyError(name)


FAMILIES = ("sweep",) + R.FAMILIES + ("cull_margin", "cull_exact", "sparse_waves")


# ---- cull_margin: two rows either side of every threshold ------------------------------------------------------
CULL_FAR = 20.0
CULL_NEAR = 2.0          # (not 0.01: see NEAR_FAR_NEAR -- a row at 1.01 x the plane must have a z of the plane's magnitude)
CULL_CLIP = 3.0
EDGE_FISHEYE_K = np.array([[80, 0, W / 2 + 0.25], [0, 82.4, H / 2 - 0.4], [0, 0, 1]], dtype=F32)     # the frame's edge at 1 rad


def _solve(case, run_kw, residual, setter, x0, iters=40, tol=1e-3, h=1e-3):
    """A few damped Newton steps in fp64 (slope by a forward difference) on the scalar input `setter(case, x)` writes, until
    |residual(forward)| <= tol.  The residual holds a ceil, so it is piecewise smooth: a step that lands on another radius is
    simply followed by the next."""
    def at(x):
        setter(case, x)
        return residual(forward(case, 0, run_kw.get("aa", False), False, run_kw.get("rule", "classic"),
                                near=run_kw.get("near", NEAR), far=run_kw.get("far", FAR), radius_clip=0.0))
    x = float(x0)
    for _ in range(iters):
        r = at(x)
        if abs(r) <= tol:
            return x
        slope = (at(x + h) - r) / h
        if not np.isfinite(slope) or abs(slope) < 1e-9:
            slope = 1.0
        x -= 0.8 * r / slope
    raise AssertionError(f"the placement did not converge ({r})")


def _set_cam_point(case, row, pc):
    vm = case["viewmat"].astype(np.float64)
    case["means"][row] = ((np.asarray(pc, np.float64) - vm[:3, 3]) @ vm[:3, :3]).astype(F32)


def _cull_margin():
    runs = []
    eye = np.eye(3)
    # near and far: z at 0.99 / 1.01 of each plane, on the optical axis' neighbourhood, small enough to stay on screen
    for model in ("pinhole", "fisheye"):
        zs = [0.99 * CULL_NEAR, 1.01 * CULL_NEAR, 0.99 * CULL_FAR, 1.01 * CULL_FAR]
        pts = [(0.05 * z, -0.03 * z, z) for z in zs]
        case = R.placed_case(model, False, pts, [R._rot_z(20)] * 4, [(0.02 * z, 0.01 * z, 0.015 * z) for z in zs],
                             viewmat=R.AXIS_VIEWMAT)
        runs += _both(f"planes-{model}", case, 1, True, near=CULL_NEAR, far=CULL_FAR)
    # the four screen edges: mean +- radius half a pixel either side.  The radius moves with the mean (the pinhole Jacobian,
    # the fisheye's), so the camera point is solved against the fp64 forward itself; per rule and aa, since the radius is.
    for model in ("pinhole", "fisheye"):
        for rule in RULES:
            for aa in (False, True):
                pts, targets = [], []
                for axis, side in ((0, -1), (0, 1), (1, -1), (1, 1)):
                    for off in (-0.5, 0.5):                 # outside (culled), inside (kept)
                        p = [0.1, -0.1, 5.0]
                        p[axis] = side * 3.0
                        pts.append(p)
                        targets.append((axis, side, off))
                case = R.placed_case(model, False, pts, [R._rot_z(30)] * 8, [(0.12, 0.06, 0.08)] * 8, viewmat=R.AXIS_VIEWMAT)
                if model == "fisheye":          # 180 degrees across the width puts the frame's edge at the horizon: a longer lens
                    case["K"] = EDGE_FISHEYE_K.copy()
                for row, (axis, side, off) in enumerate(targets):
                    def residual(r, row=row, axis=axis, side=side, off=off):
                        m, rad = r["q"]["mx" if axis == 0 else "my"][row], r["q"]["rx" if axis == 0 else "ry"][row]
                        lim = 0.0 if side < 0 else (W if axis == 0 else H)
                        return (m - side * rad) - (lim - side * off)         # the inner edge of the square, against the frame's

                    def setter(c, v, row=row, axis=axis):
                        p = list(pts[row])
                        p[axis] = v
                        _set_cam_point(c, row, p)

                    _solve(case, {"rule": rule, "aa": aa}, residual, setter, pts[row][axis])
                runs.append(make_run(f"edges-{model}", case, 1, aa, True, rule))
    # radius_clip = 3: rows of radius 3 (culled) and 4 (kept); the scale is solved so that the pre-ceil extent is 2.5 / 3.5
    for model in ("pinhole", "fisheye"):
        for rule in RULES:
            for aa in (False, True):
                case = R.placed_case(model, False, [(0.2, 0.1, 5.0), (-0.3, 0.2, 5.0)], [eye] * 2, [(0.02,) * 3] * 2,
                                     viewmat=R.AXIS_VIEWMAT)
                for row, want in ((0, 2.5), (1, 3.5)):
                    def residual(r, row=row, want=want):
                        return max(r["q"]["pre_x"][row], r["q"]["pre_y"][row]) - want

                    def setter(c, v, row=row):
                        c["scales"][row] = F32(v)

                    _solve(case, {"rule": rule, "aa": aa}, residual, setter, 0.02, h=1e-5)
                runs.append(make_run(f"clip-{model}", case, 1, aa, True, rule, radius_clip=CULL_CLIP))
    # opacity at 0.98 / 255 and 1.02 / 255 under the per-axis rule: plain, and times the compensation (anti-aliased)
    for model in ("pinhole", "fisheye"):
        for aa in (False, True):
            case = R.placed_case(model, False, [(0.2, 0.1, 5.0), (-0.3, 0.2, 5.0)], [R._rot_z(10)] * 2, [(0.05, 0.02, 0.03)] * 2,
                                 viewmat=R.AXIS_VIEWMAT)
            c64 = forward(case, 0, False, False, "classic")["comp"]
            for row, fac in ((0, 0.98), (1, 1.02)):
                case["opac"][row] = F32(fac / 255.0 / (c64[row] if aa else 1.0))
            runs.append(make_run(f"opacity-{model}", case, 1, aa, True, "opacity_aware"))
    # theta^2 at 0.99 / 1.01 of u_max under the lens: LR.MILD never folds, so its u_max is (pi/2)^2 and the row past it lies
    # BEHIND the lens plane -- reachable only with a near plane behind the camera; LR.FOLDING's lies in front of it
    for lens, near in ((LR.MILD, -10.0), (LR.FOLDING, NEAR)):
        u_max = LR.theta_max(lens) ** 2
        pts = []
        for fac in (0.99, 1.01):
            th = math.sqrt(fac * u_max)
            pts.append((2.0 * math.sin(th) * math.cos(0.4), 2.0 * math.sin(th) * math.sin(0.4), 2.0 * math.cos(th)))
        case = R.placed_case("fisheye_kb", False, pts, [R._rot_z(10)] * 2, [(0.05, 0.02, 0.03)] * 2, viewmat=R.AXIS_VIEWMAT, lens=lens)
        runs += _both(f"lens-{'mild' if lens is LR.MILD else 'folding'}", case, 1, True, near=near)
    done = {}                       # (the padding rows are random: moved off the thresholds like the sweep's)
    for r in runs:
        if id(r["case"]) not in done:
            placed = {"planes": 4, "edges": 8, "clip": 2, "opacity": 2, "lens": 2}[r["label"].split("-")[0]]
            done[id(r["case"])] = settled(r["case"], r["deg"], placed, near=r["near"], far=r["far"], radius_clip=r["radius_clip"])
        r["case"] = done[id(r["case"])]
    return runs


# ---- cull_exact: the comparisons themselves -----------------------------------------------------------------------
EXACT_NEAR, EXACT_FAR, EXACT_CLIP = 4.0, 20.0, 3.0
EXACT_K = np.array([[32, 0, 80], [0, 32, 60], [0, 0, 1]], dtype=F32)


def _cull_exact():
    """Ortho, the axis camera (identity rotation, t = (0, 0, 4)), fx = fy = 32, cx = 80, cy = 60, unit quaternions (1,0,0,0):
    camera x = mean x and z = mean z + 4 without rounding, mx = 32 x + 80 without rounding (dyadic means), so `mx + r <= 0`
    and `z >= near` compare exact numbers in fp32 and fp64 alike.  near = 4 and far = 20 because z = mean z + 4 must be able to
    stand one fp32 ulp off the plane: below 4 the ulp of z is 2^-22, and mean z = -2^-22 is representable; above 20 it is
    2^-19, the ulp of mean z = 16 as well.
    NOT here: an activated opacity of exactly 1/255 `kept`.  At op = fp32(1/255) the extent sqrt(2 ln(255 op)) is exactly 0
    in fp32 (255 x fp32(1/255) rounds to 1.0f) and 3.4e-4 in fp64, so the kernel culls the row by its zero extent whichever way
    it compares the opacity: `>=` against `>` is not observable there.  The rows are one ulp below (culled by the opacity) and
    the first opacity above it whose extent is decided (1/255 x (1 + 2^-6))."""
    runs = []
    for rule in RULES:
        for aa in (False, True):
            s_big, s_clip = 0.05, 0.0196
            n_rows = 8 + 4 + 1 + 2
            pts = [(0.0, 0.0, 8.0)] * 8 + [(0.25, 0.5, EXACT_NEAR), (0.25, 0.5, EXACT_FAR), (0.25, 0.5, EXACT_NEAR), (0.25, 0.5, EXACT_FAR),
                                           (-0.5, 0.25, 8.0), (1.0, -0.5, 8.0), (-1.0, 0.5, 8.0)]
            scs = [(s_big,) * 3] * 12 + [(s_clip,) * 3] + [(0.75,) * 3] * 2      # (rows 13, 14: an extent of 0.18 sigma must clear radius_clip)
            case = R.placed_case("ortho", False, pts, [np.eye(3)] * n_rows, scs, viewmat=R.AXIS_VIEWMAT)
            case["K"] = EXACT_K.copy()
            case["quats"][:n_rows] = np.array([1, 0, 0, 0], F32)
            below = np.nextafter(F32(T255), F32(0))
            case["opac"][13], case["opac"][14] = below, F32(T255 * (1 + 2.0 ** -6))
            if aa:      # op = opacity x compensation: not exact, so under aa rows 13, 14 are plain margin rows at -+2 %
                comp = forward(dict(case, opac=np.ones_like(case["opac"])), 0, True, False, "opacity_aware", near=EXACT_NEAR,
                               far=EXACT_FAR)["comp"]
                case["opac"][13], case["opac"][14] = F32(0.98 / 255 / comp[13]), F32(1.02 / 255 / comp[14])
            r0 = forward(case, 0, aa, False, rule, near=EXACT_NEAR, far=EXACT_FAR)
            rx, ry = r0["q"]["rx"], r0["q"]["ry"]
            m = case["means"]
            # rows 0..7: (mx = -r culled, mx = -r + 0.5 kept), (mx = W + r culled, W + r - 0.5 kept), the same in y
            for row, (axis, mval) in enumerate([(0, -rx[0]), (0, -rx[1] + 0.5), (0, W + rx[2]), (0, W + rx[3] - 0.5),
                                                (1, -ry[4]), (1, -ry[5] + 0.5), (1, H + ry[6]), (1, H + ry[7] - 0.5)]):
                m[row] = (0.0, 0.0, 4.0)
                m[row, axis] = (mval - (80 if axis == 0 else 60)) / 32.0
            m[10, 2] = -F32(2.0 ** -22)                                                        # z = 4 - 2^-22: one ulp under near
            m[11, 2] = F32(16.0) + F32(2.0 ** -19)                                             # z = 20 + 2^-19: one ulp over far
            exact = {"edge": list(range(8)), "near": [8, 10], "far": [9, 11]}
            if rule == "opacity_aware" and not aa:
                exact["op"] = [13]
            runs.append(make_run("exact", case, 1, aa, True, rule, near=EXACT_NEAR, far=EXACT_FAR, radius_clip=EXACT_CLIP, exact=exact))
    return runs


# what cull_exact's placed rows must come out as, (row, visible): checked by the host test on both dtypes
EXACT_EXPECT = ((0, False), (1, True), (2, False), (3, True), (4, False), (5, True), (6, False), (7, True),
                (8, True), (9, True), (10, False), (11, False), (12, False))


# ---- sparse_waves: which rows of a wave fetch their SH row -----------------------------------------------------
def _wave_masks(n=193):
    a = np.zeros(n, bool)
    a[0] = True                    # wave 0: only row 0
    a[127] = True                  # wave 1: only row 63
    a[128:192:2] = True            # wave 2: alternating; wave 3 (one row): none
    b = np.zeros(n, bool)          # wave 0: none
    b[65:128:2] = True             # wave 1: the odd rows
    b[128 + 63] = True             # wave 2: only row 63
    b[192] = True                  # the ragged wave's one row
    return (("a", a), ("b", b))


def _sparse_waves():
    runs = []
    base = R.visible_case(193)
    vm = base["viewmat"].astype(np.float64)
    campos = -vm[:3, :3].T @ vm[:3, 3]
    for deg, stride in ((3, 16), (2, 9)):
        for tag, keep in _wave_masks():
            c = R.with_stride(base, stride)
            c["means"] = np.where(keep[:, None], base["means"], (2.0 * campos - base["means"]).astype(F32)).astype(F32)     # behind the camera
            c["sh"][~keep] = np.nan
            for rule in RULES:
                runs.append(make_run(f"{tag}-deg{deg}-stride{stride}", c, deg, True, True, rule))
            runs.append(make_run(f"{tag}-deg{deg}-stride{stride}", c, deg, False, False, "classic"))
    return runs


def sparse_keep(run):
    tag = run["label"].split("-")[0]
    return dict(_wave_masks())[tag]


# ------------------------------------------------------------------------------------------------------------------
# floors: the largest row error of the float32 run against the float64 one over every run of the family, as
# tests/test_project_color_fwd_host.py::test_forward_floors measures it (x 1.2, two digits: a float32 torch reduction's last
# bits depend on the CPU's vector width).  gate = 8 x max(floor, UNIT).
# ------------------------------------------------------------------------------------------------------------------
def family_floors(name):
    worst = {k: 0.0 for k in OUTPUTS + DECISIONS}
    for run in family(name):
        _, _, fl = measure(run)
        for k, v in fl.items():
            worst[k] = max(worst[k], v)
    return worst


FWD_FLOORS = {
    "sweep": {"means2d": 1.7e-05, "depths": 1e-07, "conics": 1e-06, "comp": 1.1e-06, "colour": 4e-07, "near": 8e-05, "far": 8e-17, "u": 5.2e-08, "op": 5.3e-05, "extent": 1.9e-06, "edge": 2e-05, "clamp": 4e-07},
    "aa_subpixel": {"means2d": 1.5e-05, "depths": 9.8e-08, "conics": 2.5e-06, "comp": 2.2e-06, "colour": 2.2e-07, "near": 8.2e-05, "far": 8.2e-17, "u": 4.4e-08, "op": 6.7e-05, "extent": 1.9e-06, "edge": 1.5e-05, "clamp": 2.2e-07},
    "quat_norm": {"means2d": 1.5e-05, "depths": 7e-08, "conics": 3.5e-06, "comp": 2e-06, "colour": 3.7e-07, "near": 7.2e-05, "far": 7.2e-17, "u": 4.4e-08, "op": 0.00025, "extent": 7.1e-07, "edge": 1.5e-05, "clamp": 3.7e-07},
    "pinhole_clamp": {"means2d": 2.1e-05, "depths": 7e-08, "conics": 1.2e-06, "comp": 2e-07, "colour": 6.3e-07, "near": 7.2e-05, "far": 7.2e-17, "u": 0, "op": 1.9e-05, "extent": 4.2e-07, "edge": 2.1e-05, "clamp": 6.3e-07},
    "near_far": {"means2d": 1.4e-05, "depths": 6.9e-08, "conics": 8.1e-07, "comp": 4.8e-07, "colour": 2.8e-07, "near": 2.9e-07, "far": 2.9e-17, "u": 0, "op": 4.5e-05, "extent": 6.1e-07, "edge": 2.7e-05, "clamp": 2.8e-07},
    "fisheye_axis": {"means2d": 1.3e-05, "depths": 6.9e-08, "conics": 1.1e-06, "comp": 2.8e-07, "colour": 2.6e-07, "near": 2.9e-05, "far": 2.9e-17, "u": 1.3e-07, "op": 4.5e-05, "extent": 5.7e-07, "edge": 1.3e-05, "clamp": 2.6e-07},
    "ortho_depths": {"means2d": 1.3e-05, "depths": 6.9e-08, "conics": 6.9e-07, "comp": 1.2e-07, "colour": 1.5e-07, "near": 2.9e-05, "far": 2.9e-17, "u": 0, "op": 2.4e-05, "extent": 7.5e-07, "edge": 1.3e-05, "clamp": 1.5e-07},
    "raw_range": {"means2d": 1.5e-05, "depths": 7e-08, "conics": 1e-06, "comp": 2.1e-07, "colour": 3.9e-07, "near": 7.2e-05, "far": 7.2e-17, "u": 0, "op": 2.5e-05, "extent": 7.2e-07, "edge": 1.5e-05, "clamp": 3.9e-07},
    "cull_margin": {"means2d": 1.6e-05, "depths": 6.9e-08, "conics": 1.4e-06, "comp": 2.1e-05, "colour": 4.3e-07, "near": 2.9e-05, "far": 5.7e-08, "u": 1.9e-07, "op": 4.5e-05, "extent": 9.1e-06, "edge": 2.7e-05, "clamp": 4.3e-07},
    "cull_exact": {"means2d": 9.2e-06, "depths": 5.8e-08, "conics": 5.6e-07, "comp": 6.9e-08, "colour": 1.7e-07, "near": 7.2e-08, "far": 1.4e-08, "u": 0, "op": 1.7e-05, "extent": 7.1e-07, "edge": 9.2e-06, "clamp": 1.7e-07},
    "sparse_waves": {"means2d": 1.5e-05, "depths": 8.8e-08, "conics": 8.2e-07, "comp": 2.2e-07, "colour": 2.5e-07, "near": 0.00021, "far": 2.1e-16, "u": 0, "op": 5.1e-05, "extent": 4.5e-07, "edge": 1.5e-05, "clamp": 2.5e-07},
    "sh_stage": {"colour": 9.8e-07},
}
