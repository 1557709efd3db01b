"""The fp64 reference of the fused projection + colour backward (mgs_project_color_bwd, mgs_projection_bwd, mgs_sh_bwd in
robosimgs_amd/csrc/backward.hip).  A helper module, not a test file: tests/test_project_color_bwd_host.py keeps it honest
on the CPU, tests/test_gpu_project_color_bwd.py holds the kernels to it.

Built on oracle/gs_oracle_torch.py (`project`, `spherical_harmonics`) with leaves made from the fp32 values the kernel
receives.  The fused backward takes `radii`, `conics` and `feats` as INPUTS, so a test feeds it `forward_products` -- the
oracle's own forward rounded to fp32 -- and `vjp` takes the same fp32 `radii` and `feats` as its gate: a row is visible iff
radii > 0, a colour channel is live iff its feats > 0 (strictly); neither is decided again in fp64.  Kernel and reference
then branch on identical bits and no flip allowance is needed.

The compensation's square root uses the project's documented guard in its backward, 0.5 v / (comp + 1e-6)
(csrc/mgs_math.h project_gaussian_vjp, as the published algorithm does): against the exact square root the guard alone is
worth 1e-6 / comp, which at the compensations of the sub-pixel family (down to 1e-4) would mask every rounding error.

`vjp(..., dtype=torch.float32)` is the same oracle evaluated in float32: an independent fp32 statement of the operation,
whose scaled row error against the float64 run is the FLOOR of a case family (`scaled_error`, the scaling of
grad_gate.compare).  The GPU gate of a family and tensor is 8 x that floor (GATE_FACTOR): the three bits cover that the
kernel inverts the fp32-rounded conic instead of carrying cov2d forward, sums in another order and uses the device's
rsqrt / exp.  No gate may exceed CEILING (the project's row_tol of 2e-3), i.e. no floor 2.5e-4; a family whose float32
oracle does not stay under that has its range shrunk, which its builder says.
"""
from __future__ import annotations

import contextlib
import math

import numpy as np
import torch

import lens_ref as LR
from oracle import gs_oracle_torch as OT
from robosimgs_amd import camera_ring, synthetic_scene

W, H = 160, 120
EPS2D, NEAR = float(np.float32(0.3)), 0.01      # eps2d as the kernel receives it: a C float, 0.3 rounded to fp32
CAMERAS = ("pinhole", "ortho", "fisheye", "fisheye_kb")
CAMERA_ID = {"pinhole": 0, "ortho": 1, "fisheye": 2, "fisheye_kb": 3}      # include/mgs.h MGS_CAMERA_*
LENS = LR.MILD                       # the lens of "fisheye_kb" unless a case brings its own
ALL_K = (0.03, -0.01, 0.002, -0.0005)    # a second lens, all four k non-zero and of the other signs than LR.MILD; no fold below pi/2
GATE_FACTOR = 8.0
CEILING = 2e-3
TENSORS = ("v_means", "v_quats", "v_scales", "v_sh", "v_opacities", "v_viewmat")

# Floors: the largest scaled row error of the float32 oracle against the float64 one over every case of the family, as
# tests/test_project_color_bwd_host.py::test_rounding_floors measures it (rounded up to two digits); gate = 8 x floor.
# A tensor a family does not list is not produced by it (v_opacities when the kernel does not own it).
def _row(m, q, s, sh, o, v):
    return {"v_means": m, "v_quats": q, "v_scales": s, "v_sh": sh, "v_opacities": o, "v_viewmat": v}


FLOORS = {
    "sweep":         _row(4.9e-7, 1.6e-5, 7.0e-6, 3.7e-7, 2.2e-6, 2.8e-7),
    "aa_subpixel":   _row(2.7e-7, 6.9e-5, 9.3e-5, 1.1e-7, 3.9e-5, 9.3e-8),
    "quat_norm":     _row(2.4e-7, 9.6e-6, 1.4e-5, 1.2e-7, 2.3e-6, 2.5e-7),
    "pinhole_clamp": _row(2.0e-7, 1.6e-5, 2.8e-6, 2.5e-7, 2.5e-7, 8.9e-8),
    "near_far":      _row(3.6e-5, 6.8e-5, 9.5e-5, 5.1e-6, 2.0e-6, 5.2e-5),
    "fisheye_axis":  _row(3.0e-7, 4.2e-5, 3.3e-6, 2.9e-7, 2.1e-7, 1.8e-7),
    "ortho_depths":  {"v_means": 4.8e-8, "v_quats": 3.2e-6, "v_scales": 2.7e-6, "v_sh": 1.1e-7, "v_viewmat": 9.3e-8},
    "raw_range":     _row(2.1e-7, 1.7e-5, 7.3e-6, 1.4e-7, 6.7e-5, 5.4e-8),
    "projection_stage": {"v_means": 2.4e-7, "v_quats": 5.6e-6, "v_scales": 4.3e-6, "v_viewmat": 1.2e-7},
    "sh_stage":      {"v_coeffs": 5.4e-7, "v_dirs": 2.2e-6},
}
SWEEP_MU = (0.1, 0.01)               # the two scale settings of the random sweep (log 0.1, log 0.01)


def gate(family, tensor):
    g = GATE_FACTOR * FLOORS[family][tensor]
    assert g <= CEILING * (1 + 1e-12), (family, tensor, g)
    return g


# ------------------------------------------------------------------------------------------------------------------
# cases: everything the kernel receives, as fp32 arrays
# ------------------------------------------------------------------------------------------------------------------
def intrinsics(model, w=W, h=H):
    """pinhole 60 degrees; ortho w/6 pixels per world unit; fisheye 180 degrees across the width.  Off-centre principal
    point and fy != fx so that no term hides behind a symmetry."""
    f = {"pinhole": (w / 2) / math.tan(math.radians(30)), "ortho": w / 6.0, "fisheye": w / math.pi,
         "fisheye_kb": w / math.pi}[model]
    return np.array([[f, 0, w / 2 + 0.25], [0, f * 1.03, h / 2 - 0.4], [0, 0, 1]], dtype=np.float32)


def ring_viewmat(theta=0.3, radius=7.0):
    """A camera of the benchmark ring: rotation and a non-zero translation, rounded to fp32."""
    return camera_ring(1, W, H, thetas=[theta], radius=radius)[0].viewmat().astype(np.float32)


def make_case(model, means, quats, scales, opac, sh, raw, viewmat=None, K=None, lens=None):
    """scales / opac: log-scales / logits when raw.  sh [N,Kc,3] with Kc the coefficient stride."""
    f = lambda a: np.ascontiguousarray(a, dtype=np.float32)
    return {"model": model, "raw": bool(raw), "means": f(means), "quats": f(quats), "scales": f(scales), "opac": f(opac),
            "sh": f(sh), "viewmat": f(ring_viewmat() if viewmat is None else viewmat),
            "K": f(intrinsics(model) if K is None else K), "lens": tuple(LENS if lens is None else lens)}


def scene_case(model, raw, n=333, mu=0.1, stride=16, seed=0, theta=0.3, radius=7.0):
    g = synthetic_scene(n, math.log(mu), 3, seed)
    return make_case(model, g.means, g.quats, g.log_scales if raw else g.scales, g.opacity_logits if raw else g.opacities,
                     g.sh_coeffs[:, :stride], raw, viewmat=ring_viewmat(theta, radius))


def with_stride(case, stride):
    """The same case with its coefficient rows cut or zero-padded to `stride` coefficients."""
    c = dict(case)
    sh = np.zeros((case["sh"].shape[0], stride, 3), np.float32)
    k = min(stride, case["sh"].shape[1])
    sh[:, :k] = case["sh"][:, :k]
    c["sh"] = sh
    return c


def camera_row(case):
    """What the kernel takes as K: the 3x3, or under the lens the camera's 16-float row (include/mgs.h)."""
    if case["model"] == "fisheye_kb":
        return LR.lens_row(case["K"], case["lens"]).astype(np.float32)
    return case["K"].reshape(9)


def cotangents(n, seed=0, with_depth=True):
    rng = np.random.default_rng(1000 + seed)
    f = lambda *s: rng.normal(size=s).astype(np.float32)
    return {"v_means2d": f(n, 2), "v_conics": f(n, 3), "v_feats": f(n, 4 if with_depth else 3), "v_depths": None,
            "v_opac_out": f(n)}


# ------------------------------------------------------------------------------------------------------------------
# the graph
# ------------------------------------------------------------------------------------------------------------------
class _GuardedSqrt(torch.autograd.Function):
    """sqrt(max(x, 0)) whose backward is the project's guarded one: 0.5 v / (sqrt + 1e-6)."""
    generate_vmap_rule = True

    @staticmethod
    def forward(x):
        return torch.sqrt(torch.clamp(x, min=0.0))

    @staticmethod
    def setup_context(ctx, inputs, output):
        ctx.save_for_backward(output)

    @staticmethod
    def backward(ctx, v):
        (y,) = ctx.saved_tensors
        return 0.5 * v / (y + 1e-6)


def guarded_sqrt(x):
    return _GuardedSqrt.apply(x)


def _lens_ctx(case):
    return LR.lens(case["lens"]) if case["model"] == "fisheye_kb" else contextlib.nullcontext()


def _graph(case, deg, aa, dtype, grad, guard=True):
    t = lambda a: torch.tensor(np.asarray(a, dtype=np.float64), dtype=dtype, requires_grad=grad)
    P = {k: t(case[k]) for k in ("means", "quats", "scales", "opac", "sh", "viewmat")}
    K = torch.tensor(case["K"].astype(np.float64), dtype=dtype)
    s = torch.exp(P["scales"]) if case["raw"] else P["scales"]
    o = torch.sigmoid(P["opac"]) if case["raw"] else P["opac"]
    model = "fisheye" if case["model"] == "fisheye_kb" else case["model"]
    with _lens_ctx(case):
        p = OT.project(P["means"], P["quats"], s, P["viewmat"], K, W, H, eps2d=EPS2D, near_plane=NEAR, camera_model=model)
    c = p["compensations"]                          # sqrt(ratio) with the exact backward: undo it, redo it guarded
    comp = guarded_sqrt(c * c) if guard else c
    vm = P["viewmat"]
    campos = -vm[:3, :3].T @ vm[:3, 3]
    pre = OT.spherical_harmonics(deg, P["means"] - campos, P["sh"]) + 0.5
    out = {"radii": p["radii"], "means2d": p["means2d"], "depths": p["depths"], "conics": p["conics"], "comp": comp,
           "pre": pre, "opacity": o, "opac_out": o * comp if aa else o}
    return P, out


def forward_products(case, deg, aa, with_depth):
    """The fp32 inputs of the backward, from the float64 forward: radii i32 [N], conics [N,3], feats [N,3|4]
    (clamp_min(sh + 0.5, 0), zero rows where culled, depth in channel 3), opac_out [N] (activated opacity, x compensation
    when anti-aliased) and, for mgs_projection_bwd, compensations [N]."""
    with torch.no_grad():
        _, o = _graph(case, deg, aa, torch.float64, False)
    vis = (o["radii"] > 0).to(torch.float64)[:, None]
    feats = torch.clamp(o["pre"], min=0.0) * vis
    if with_depth:
        feats = torch.cat([feats, o["depths"][:, None]], dim=-1)
    f = lambda x: x.numpy().astype(np.float32)
    return {"radii": o["radii"].numpy().astype(np.int32), "conics": f(o["conics"]), "feats": f(feats),
            "opac_out": f(o["opac_out"] * vis[:, 0]), "compensations": f(o["comp"]), "means2d": f(o["means2d"])}


def loss_rows(o, n, radii, feats, v_means2d, v_conics, v_feats, v_depths, v_opac_out, dtype):
    """Per Gaussian: <cotangents, its forward outputs>, behind the fp32 gate (rows: radii > 0; channels: feats > 0)."""
    c = lambda a: torch.tensor(np.asarray(a, dtype=np.float64), dtype=dtype)
    vis = c(np.asarray(radii) > 0)
    live = c(np.asarray(feats)[:, :3] > 0)
    vf = np.asarray(v_feats, dtype=np.float64)
    v_depth = np.zeros(n) if vf.shape[1] == 3 else vf[:, 3].copy()
    if v_depths is not None:
        v_depth = v_depth + np.asarray(v_depths, dtype=np.float64)
    Lg = (o["means2d"] * c(v_means2d)).sum(-1) + (o["conics"] * c(v_conics)).sum(-1) + o["depths"] * c(v_depth) \
        + (o["pre"] * live * c(vf[:, :3])).sum(-1)
    if v_opac_out is not None:
        Lg = Lg + o["opac_out"] * c(v_opac_out)
    return Lg * vis


def vjp(case, deg, aa, radii, feats, v_means2d, v_conics, v_feats, v_depths=None, v_opac_out=None, dtype=torch.float64,
        view=True, guard=True):
    """The VJP of project + colour for the cotangents given (fp32 arrays; v_feats [N,3|4], channel 3 = d/d depth, which
    v_depths adds to).  radii / feats: the fp32 gate.  Returns float64 arrays v_means, v_quats, v_scales (of the
    log-scales when raw), v_sh [N,Kc,3] (zeros past (deg+1)^2), v_opacities (v_opac_out x d opac_out / d the opacity
    leaf: the logit when raw), `view` [N,3,4] -- each Gaussian's twelve contributions to v_viewmat[:3] -- and `agree`
    [N] bool: rows on which this evaluation's own visibility matches the gate (always all in float64 when the gate came from
    forward_products; a float32 run may cull a row at an edge, and such a row says nothing about rounding).
    guard=False: the exact square root's backward for the compensation (what finite differences see)."""
    n = case["means"].shape[0]
    P, o = _graph(case, deg, aa, dtype, True, guard)
    Lg = loss_rows(o, n, radii, feats, v_means2d, v_conics, v_feats, v_depths, v_opac_out, dtype)
    names = ("means", "quats", "scales", "sh", "opac")
    grads = torch.autograd.grad(Lg.sum(), [P[k] for k in names], retain_graph=view, allow_unused=True)
    g = {k: (torch.zeros_like(P[k]) if x is None else x).double().numpy() for k, x in zip(names, grads)}
    out = {"v_means": g["means"], "v_quats": g["quats"], "v_scales": g["scales"], "v_sh": g["sh"],
           "v_opacities": g["opac"], "agree": ((o["radii"] > 0).numpy() == (np.asarray(radii) > 0))}
    if view:
        (gv,) = torch.autograd.grad(Lg, P["viewmat"], grad_outputs=torch.eye(n, dtype=dtype), is_grads_batched=True)
        out["view"] = gv[:, :3, :].double().numpy()
    return out


def sh_vjp(deg, dirs, coeffs, masks, v_colors, dtype=torch.float64):
    """mgs_sh_bwd's reference: (v_coeffs [N,Kc,3], v_dirs [N,3]) of colours = SH(deg, normalize(dirs), coeffs) on the rows
    whose mask is set (None: all)."""
    t = lambda a: torch.tensor(np.asarray(a, dtype=np.float64), dtype=dtype, requires_grad=True)
    d, c = t(dirs), t(coeffs)
    m = torch.ones(len(dirs), dtype=dtype) if masks is None else torch.tensor(np.asarray(masks) != 0, dtype=dtype)
    L = ((OT.spherical_harmonics(deg, d, c) * torch.tensor(np.asarray(v_colors, np.float64), dtype=dtype)).sum(-1) * m).sum()
    gd, gc = torch.autograd.grad(L, [d, c], allow_unused=True)
    z = lambda x, like: (torch.zeros_like(like) if x is None else x).double().numpy()
    return z(gc, c), z(gd, d)


# ------------------------------------------------------------------------------------------------------------------
# measuring
# ------------------------------------------------------------------------------------------------------------------
def scaled_error(got, ref, rows=None):
    """The largest scaled row error, with the scaling of grad_gate.compare; `rows`: a bool mask of the rows measured (the
    scale still comes from the whole reference)."""
    ref = np.asarray(ref, dtype=np.float64)
    ref = ref.reshape(ref.shape[0], -1)
    got = np.asarray(got, dtype=np.float64).reshape(ref.shape)
    scale = np.abs(ref).max(axis=1, keepdims=True) + 1e-3 * np.abs(ref).max() + 1e-30
    err = (np.abs(got - ref) / scale).max(axis=1)
    if rows is not None:
        err = err[np.asarray(rows, dtype=bool)]
    return float(err.max()) if err.size else 0.0


def view_sum(view):
    return view.sum(axis=0)


def view_abs(view):
    return np.abs(view).sum(axis=0)


def floors_of(case, deg, aa, with_depth=True, seed=0, own_opac=None, feats=None):
    """{tensor: scaled error of the float32 oracle against the float64 one} for one case.  feats: a gate other than the
    forward's own (all zeros: the projection alone)."""
    fp = forward_products(case, deg, aa, with_depth)
    ct = cotangents(case["means"].shape[0], seed, with_depth)
    args = (case, deg, aa, fp["radii"], fp["feats"] if feats is None else feats, ct["v_means2d"], ct["v_conics"], ct["v_feats"],
            ct["v_depths"], ct["v_opac_out"])
    r64, r32 = vjp(*args), vjp(*args, dtype=torch.float32)
    assert r64["agree"].all()
    rows = r32["agree"]
    own = (aa or case["raw"]) if own_opac is None else own_opac
    out = {k: scaled_error(r32[k], r64[k], rows) for k in TENSORS[:4]}
    if own:
        out["v_opacities"] = scaled_error(r32["v_opacities"], r64["v_opacities"], rows)
    out["v_viewmat"] = scaled_error(view_sum(r32["view"][rows]).reshape(1, 12), view_sum(r64["view"][rows]).reshape(1, 12))
    return out


def visible_case(n=257, model="pinhole", raw=False, seed=2):
    """n Gaussians of a random scene that the camera sees, anti-aliased or not (the row-ownership tests then hide rows by
    the gate alone)."""
    big = scene_case(model, raw, n=4 * n, mu=0.1, seed=seed)
    keep = np.flatnonzero((forward_products(big, 0, True, False)["radii"] > 0) & (forward_products(big, 0, False, False)["radii"] > 0))[:n]
    assert len(keep) == n
    c = dict(big)
    for k in ("means", "quats", "scales", "opac", "sh"):
        c[k] = np.ascontiguousarray(big[k][keep])
    return c


def projection_case(n=257):
    """visible_case for mgs_projection_bwd: opacities of one, so that v_opac_out x opacity is a cotangent of the
    compensation itself, and one coefficient per row (there is no colour)."""
    c = with_stride(visible_case(n), 1)
    c["opac"] = np.ones(n, np.float32)
    return c


def projection_floors():
    c = projection_case()
    n = c["means"].shape[0]
    worst = {}
    for aa in (False, True):
        f = floors_of(c, 0, aa, True, feats=np.zeros((n, 4), np.float32))
        for k in ("v_means", "v_quats", "v_scales", "v_viewmat"):
            worst[k] = max(worst.get(k, 0.0), f[k])
    return worst


# ------------------------------------------------------------------------------------------------------------------
# the edge families of tests/test_gpu_project_color_bwd.py (section g): a handful of hand-placed Gaussians each, padded
# with ordinary ones so that neighbours share a wave.  family(name) -> [(label, case, deg, aa, with_depth)]
# ------------------------------------------------------------------------------------------------------------------
def _rotmat_to_quat(R):
    """wxyz of a rotation matrix (Shepperd's branch on the largest diagonal term)."""
    R = np.asarray(R, dtype=np.float64)
    tr = R[0, 0] + R[1, 1] + R[2, 2]
    if tr > 0:
        s = 2.0 * math.sqrt(1.0 + tr)
        q = [0.25 * s, (R[2, 1] - R[1, 2]) / s, (R[0, 2] - R[2, 0]) / s, (R[1, 0] - R[0, 1]) / s]
    else:
        i = int(np.argmax(np.diag(R)))
        j, k = (i + 1) % 3, (i + 2) % 3
        s = 2.0 * math.sqrt(1.0 + R[i, i] - R[j, j] - R[k, k])
        q = [0.0] * 4
        q[0] = (R[k, j] - R[j, k]) / s
        q[1 + i] = 0.25 * s
        q[1 + j] = (R[j, i] + R[i, j]) / s
        q[1 + k] = (R[k, i] + R[i, k]) / s
    return np.array(q)


def _rot_z(deg):
    a = math.radians(deg)
    return np.array([[math.cos(a), -math.sin(a), 0], [math.sin(a), math.cos(a), 0], [0, 0, 1.0]])


AXIS_VIEWMAT = np.array([[1, 0, 0, 0], [0, 1, 0, 0], [0, 0, 1, 4.0], [0, 0, 0, 1]], dtype=np.float32)   # camera at (0, 0, -4)


def placed_case(model, raw, pc, rot_cam, scales, viewmat=None, pad_to=65, deg_stride=16, seed=5, logits=None, lens=None,
                quat_norm=None):
    """Gaussians at the camera points pc [M,3] with camera-frame orientations rot_cam [M,3,3] and ACTIVATED scales [M,3],
    followed by ordinary Gaussians up to pad_to rows.  logits [M]: their opacity logits (default 1.0)."""
    vm = np.asarray(ring_viewmat() if viewmat is None else viewmat, dtype=np.float32).astype(np.float64)
    Rcw, t = vm[:3, :3], vm[:3, 3]
    pc = np.asarray(pc, dtype=np.float64)
    m = len(pc)
    means = (pc - t) @ Rcw                                      # R^T (pc - t)
    quats = np.stack([_rotmat_to_quat(Rcw.T @ np.asarray(r)) for r in rot_cam])
    if quat_norm is not None:
        quats = quats * np.asarray(quat_norm, dtype=np.float64)[:, None]
    g = synthetic_scene(max(pad_to - m, 1), math.log(0.1), 3, seed)
    logit = np.full(m, 1.0) if logits is None else np.asarray(logits, dtype=np.float64)
    sc = np.asarray(scales, dtype=np.float64)
    rng = np.random.default_rng(seed)
    sh = np.concatenate([rng.normal(size=(m, 16, 3)), g.sh_coeffs])[:, :deg_stride]
    return make_case(model, np.concatenate([means, g.means]), np.concatenate([quats, g.quats]),
                     np.concatenate([np.log(sc) if raw else sc, g.log_scales if raw else g.scales]),
                     np.concatenate([logit if raw else 1.0 / (1.0 + np.exp(-logit)), g.opacity_logits if raw else g.opacities]),
                     sh, raw, viewmat=vm, lens=lens)


SUBPIXEL_LAMBDA = (1e2, 1.0, 1e-2, 1e-3, 1e-4, 3e-5)        # the smaller eigenvalue of cov2d, px^2
SUBPIXEL_ANISO = (1.0, 30.0, 1e3)
# Range shrunk to meet the ceiling: anisotropy 1e3 only below one pixel.  A needle of 1 or 100 px^2 by 1e3 times that at
# 45 degrees has a cov2d whose determinant cancels to 1e-3 of its terms, and the float32 ORACLE itself is then at 1.0e-4 to
# 6.7e-3 in v_quats / v_scales (over 2.5e-4); below a pixel the blur eps2d conditions the determinant and 1e3 stays.
SUBPIXEL_ANISO_FROM_A_PIXEL_UP = (1.0, 30.0)
SUBPIXEL_ANGLES = (0.0, 45.0)


def _subpixel(model):
    z, pts, rots, scs = 5.0, [], [], []
    px_per_unit = {"pinhole": float(intrinsics("pinhole")[0, 0]) / z, "ortho": float(intrinsics("ortho")[0, 0]),
                   "fisheye": float(intrinsics("fisheye")[0, 0]) / z, "fisheye_kb": float(intrinsics("fisheye")[0, 0]) / z}[model]
    for lam in SUBPIXEL_LAMBDA:
        for an in (SUBPIXEL_ANISO if lam < 1.0 else SUBPIXEL_ANISO_FROM_A_PIXEL_UP):
            for ang in SUBPIXEL_ANGLES:
                s2 = math.sqrt(lam) / px_per_unit
                pts.append((0.3, -0.2, z))
                rots.append(_rot_z(ang))
                scs.append((s2 * math.sqrt(an), s2, s2))
    return pts, rots, scs


def family(name):
    eye = np.eye(3)
    if name == "aa_subpixel":
        out = []
        for model in CAMERAS:
            pts, rots, scs = _subpixel(model)
            for raw in (False, True):
                out.append((f"{model}-{'raw' if raw else 'act'}", placed_case(model, raw, pts, rots, scs, pad_to=100), 0, True, False))
        return out
    if name == "quat_norm":
        pts = [(0.4, 0.3, 5.0)] * 3 + [(-0.8, 0.1, 6.0)] * 3
        rots = [_rot_z(20) @ np.array([[1, 0, 0], [0, 0.8, -0.6], [0, 0.6, 0.8]])] * 3 + [_rot_z(-50)] * 3
        scs = [(0.3, 0.05, 0.1)] * 3 + [(0.02, 0.2, 0.07)] * 3
        return [(m, placed_case(m, False, pts, rots, scs, quat_norm=[0.1, 1, 10] * 2), 1, True, True) for m in ("pinhole", "fisheye_kb")]
    if name == "pinhole_clamp":
        K = intrinsics("pinhole")
        fx, fy, cx, cy = K[0, 0], K[1, 1], K[0, 2], K[1, 2]
        lims = {"xp": (W - cx) / fx + 0.15 * W / fx, "xn": -(cx / fx + 0.15 * W / fx),
                "yp": (H - cy) / fy + 0.15 * H / fy, "yn": -(cy / fy + 0.15 * H / fy)}
        z, pts = 5.0, []
        for k, lim in lims.items():
            for f in (0.99, 1.01):                              # just inside, just outside
                pts.append((lim * f * z, 0.1, z) if k[0] == "x" else (0.1, lim * f * z, z))
        rots = [_rot_z(30)] * len(pts)
        scs = [(1.0, 0.6, 0.8)] * len(pts)
        return [("pinhole", placed_case("pinhole", False, pts, rots, scs), 2, True, True)]
    if name == "near_far":
        out = []
        for model in ("pinhole", "fisheye"):
            pts = [(0.0, 0.0, 1.01 * NEAR), (1e-4, -2e-4, 1.01 * NEAR), (30.0, -20.0, 1e4), (0.0, 0.0, 1e4)]
            scs = [(1e-3, 5e-4, 8e-4)] * 2 + [(300.0, 100.0, 200.0)] * 2
            out.append((model, placed_case(model, False, pts, [_rot_z(25)] * 4, scs), 1, True, True))
        return out
    if name == "fisheye_axis":
        out = []
        th = math.pi / 2 - 0.02
        for model in ("fisheye", "fisheye_kb"):
            pts = [(0.0, 0.0, 3.0), (0.0, 0.0, 0.5), (3e-6, 0.0, 3.0), (-2e-6, 2e-6, 2.0),
                   (0.05 * math.tan(th), 0.0, 0.05), (0.0, -0.04 * math.tan(1.1), 0.04)]
            scs = [(0.1, 0.05, 0.08), (0.02, 0.03, 0.01), (0.1, 0.05, 0.08), (0.05, 0.05, 0.05), (0.02, 0.01, 0.015), (0.01, 0.02, 0.01)]
            out.append((model, placed_case(model, False, pts, [_rot_z(40)] * 6, scs, viewmat=AXIS_VIEWMAT, lens=ALL_K), 2, True, True))
        return out
    if name == "ortho_depths":
        pts = [(0.5, -0.3, 3.0), (0.5, -0.3, 9.0)]
        return [("ortho", placed_case("ortho", False, pts, [_rot_z(15)] * 2, [(0.2, 0.1, 0.15)] * 2, viewmat=AXIS_VIEWMAT), 0, False, True)]
    if name == "raw_range":
        logits = [15.0, -15.0, 0.0, 15.0, -15.0, 0.0, 2.0, -2.0]
        ls = [-7.0, -7.0, -4.0, 2.0, 0.0, 1.0, -7.0, 2.0]
        pts = [(0.3 * (i % 3 - 1), 0.2 * (i % 2), 5.0 + (8.0 if l > 0 else 0.0)) for i, l in enumerate(ls)]
        scs = [(math.exp(l), math.exp(l - 0.5), math.exp(min(l + 0.3, 2.0))) for l in ls]
        return [(f"{'aa' if aa else 'plain'}", placed_case("pinhole", True, pts, [_rot_z(35)] * 8, scs, logits=logits), 1, aa, True)
                for aa in (False, True)]
    raise KeyError(name)


def sh_case(n=257, seed=0):
    """mgs_sh_bwd's inputs: directions of every length (the kernel normalises), coefficient rows of 16, colour cotangents."""
    rng = np.random.default_rng(seed)
    dirs = rng.normal(size=(n, 3)) * np.exp(rng.normal(size=(n, 1)) * 2.0)
    f = lambda a: np.ascontiguousarray(a, dtype=np.float32)
    return f(dirs), f(rng.normal(size=(n, 16, 3))), f(rng.normal(size=(n, 3)))


# (degree, coefficient stride).  Stride 16 is the LDS-staged path, every other the plain one: (3, 20) is degree 3 unstaged.
SH_STRIDES = ((0, 1), (0, 16), (1, 4), (1, 9), (1, 16), (2, 9), (2, 16), (3, 16), (3, 20))


def sh_floors():
    dirs, coeffs, v = sh_case()
    worst = {"v_coeffs": 0.0, "v_dirs": 0.0}
    for deg in range(4):
        r64, r32 = sh_vjp(deg, dirs, coeffs, None, v), sh_vjp(deg, dirs, coeffs, None, v, dtype=torch.float32)
        worst["v_coeffs"] = max(worst["v_coeffs"], scaled_error(r32[0], r64[0]))
        if deg:
            worst["v_dirs"] = max(worst["v_dirs"], scaled_error(r32[1], r64[1]))
    return worst


def triplet_cotangents(n, with_depth=True):
    """cotangents(n) with rows 1, 2 (4, 5) made copies of row 0 (3): the quat_norm family's three norms of one Gaussian
    then differ in the quaternion's length alone."""
    ct = cotangents(n, 0, with_depth)
    for k, v in ct.items():
        if v is not None:
            v[1:3], v[4:6] = v[0], v[3]
    return ct


FAMILIES = ("aa_subpixel", "quat_norm", "pinhole_clamp", "near_far", "fisheye_axis", "ortho_depths", "raw_range")
