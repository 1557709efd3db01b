"""Differentiable group poses (include/mgs_pose.h, csrc/pose.hip): `pose_gaussians` is `transform_gaussians` with a
backward, so that a loss on a rendered image reaches the pose of a part -- a hinge angle, an object's position, the
similarity that aligns a scene -- and the Gaussians at rest.

    hinge = fit_hinge(...)
    theta = torch.tensor(0.1, device="cuda", dtype=torch.float64, requires_grad=True)
    R, t = hinge.pose_torch(theta)
    posed = pose_gaussians(tensors, R[None], t[None], group_ids=ids)
    colors, alphas, _ = rasterization(posed["means"], posed["quats"], posed["scales"], ...)
    l1_loss(colors, target).backward()                     # theta.grad

What is differentiated.  The pose gradient is taken in the tangent space at the current pose (R <- exp([d_omega]x) R,
t <- t + d_t, s <- s exp(d_lambda)): the kernel returns v_omega, v_t and v_lambda per group from the posed values and
their cotangents alone, and autograd receives

    v_R = 1/2 [v_omega]x R,     v_t,     v_s = v_lambda / s.

v_R is the tangent-projected gradient: <v_R, [d]x R> = v_omega . d for every d, so every parametrisation that stays on
SO(3) -- Rodrigues from an angle, a quaternion, a product of joint rotations -- gets its exact gradient.  Components
normal to SO(3) are zero by definition: a rotation matrix optimised entry by entry as nine free numbers would see no
pull off the manifold (and would not stay a rotation either).  Nothing differentiates `sh_rotation_matrices` or the
packing: `pack_transforms_torch` runs under no_grad.
"""
from __future__ import annotations

import math
from typing import Dict, Optional, Tuple

import numpy as np
import torch
from torch import Tensor
from torch.autograd.function import once_differentiable

from . import _lib
from ._lib import aligned_workspace, check, ptr, require_device, stream_handle
from .gaussians import _sh_fit_basis
from .ops import _f32c

POSE_FLOATS = 8          # include/mgs_pose.h: v_omega[3], v_t[3], v_lambda, 0
XFORM_FLOATS, SH_ROT_FLOATS = 20, 84

# csrc/pose.hip's kShGen: the generators L_k^(l) = d/d_eps M_l(exp(eps [e_k]x)) at 0 of the real-SH rotation, per axis k a
# list of (a, b, v) with L[a][b] = v and L[b][a] = -v; a < b count the coefficients above the DC term (degree 1: 0..2,
# degree 2: 3..7, degree 3: 8..14).
_S3, _S6, _S32, _S52 = math.sqrt(3.0), math.sqrt(6.0), math.sqrt(1.5), math.sqrt(2.5)
SH_GENERATORS = (
    ((0, 1, 1.0), (3, 6, 1.0), (4, 5, _S3), (4, 7, 1.0),
     (8, 13, _S32), (9, 12, _S52), (9, 14, _S32), (10, 11, _S6), (10, 13, _S52)),
    ((1, 2, 1.0), (3, 4, -1.0), (5, 6, _S3), (6, 7, 1.0),
     (8, 9, -_S32), (9, 10, -_S52), (11, 12, _S6), (12, 13, _S52), (13, 14, _S32)),
    ((0, 2, 1.0), (3, 7, 2.0), (4, 6, 1.0), (8, 14, 3.0), (9, 13, 2.0), (10, 12, 1.0)),
)


def sh_generator_matrices(degree: int = 3):
    """SH_GENERATORS as dense matrices: out[k][l] is the (2l+1) x (2l+1) float64 generator of axis k at degree l."""
    out = []
    for k in range(3):
        full = np.zeros((15, 15))
        for a, b, v in SH_GENERATORS[k]:
            full[a, b], full[b, a] = v, -v
        out.append([np.zeros((1, 1))] + [full[l * l - 1:(l + 1) ** 2 - 1, l * l - 1:(l + 1) ** 2 - 1].copy()
                                         for l in range(1, degree + 1)])
    return out


# ---- packing on the device ----------------------------------------------------------------------------------
_FIT_CACHE: dict = {}


def _fit_constants(degree: int, device):
    key = (degree, str(device))
    hit = _FIT_CACHE.get(key)
    if hit is None:
        d, pinv = _sh_fit_basis(degree)
        hit = _FIT_CACHE[key] = (torch.from_numpy(d).to(device), [torch.from_numpy(np.ascontiguousarray(p)).to(device)
                                                                  for p in pinv])
    return hit


def _sh_basis_torch(degree: int, dirs: Tensor) -> Tensor:
    """gaussians._sh_basis_np in torch: dirs [...,3] unit, float64 -> [...,(degree+1)^2]."""
    x, y, z = dirs[..., 0], dirs[..., 1], dirs[..., 2]
    Y = [torch.full_like(x, 0.28209479177387814)]
    if degree >= 1:
        c1 = 0.48860251190292
        Y += [-c1 * y, c1 * z, -c1 * x]
    if degree >= 2:
        z2, fC1, fS1 = z * z, x * x - y * y, 2 * x * y
        t = -1.092548430592079 * z
        Y += [0.5462742152960395 * fS1, t * y, 0.9461746957575601 * z2 - 0.3153915652525201, t * x,
              0.5462742152960395 * fC1]
    if degree >= 3:
        u = -2.285228997322329 * z2 + 0.4570457994644658
        w = 1.445305721320277 * z
        fC2, fS2 = x * fC1 - y * fS1, x * fS1 + y * fC1
        Y += [-0.5900435899266435 * fS2, w * fS1, u * y, z * (1.865881662950577 * z2 - 1.119528997770346),
              u * x, w * fC1, -0.5900435899266435 * fC2]
    return torch.stack(Y, dim=-1)


def _rotmat_to_quat_torch(R: Tensor) -> Tensor:
    """gaussians._rotmat_to_quat for R [G,3,3] float64, branch for branch: trace > 0, else the largest diagonal entry
    (the first of equal ones).  All four candidates are formed and one is selected: no synchronisation."""
    d0, d1, d2 = R[:, 0, 0], R[:, 1, 1], R[:, 2, 2]
    tr = d0 + d1 + d2
    cands = []
    s = torch.sqrt(torch.clamp(tr + 1.0, min=0.0)) * 2
    cands.append(torch.stack([0.25 * s, (R[:, 2, 1] - R[:, 1, 2]) / s, (R[:, 0, 2] - R[:, 2, 0]) / s,
                              (R[:, 1, 0] - R[:, 0, 1]) / s], dim=-1))
    for i in range(3):
        j, k = (i + 1) % 3, (i + 2) % 3
        s = torch.sqrt(torch.clamp(1.0 + R[:, i, i] - R[:, j, j] - R[:, k, k], min=0.0)) * 2
        q = [None] * 4
        q[0] = (R[:, k, j] - R[:, j, k]) / s
        q[1 + i] = 0.25 * s
        q[1 + j] = (R[:, j, i] + R[:, i, j]) / s
        q[1 + k] = (R[:, k, i] + R[:, i, k]) / s
        cands.append(torch.stack(q, dim=-1))
    first = (d0 >= d1) & (d0 >= d2)
    second = ~first & (d1 >= d2)
    by_diag = torch.where(first[:, None], cands[1], torch.where(second[:, None], cands[2], cands[3]))
    return torch.where((tr > 0)[:, None], cands[0], by_diag)


@torch.no_grad()
def pack_transforms_torch(rotations: Tensor, translations: Tensor, scales: Optional[Tensor] = None,
                          sh_degree: int = 0) -> Tuple[Tensor, Optional[Tensor]]:
    """`transform.pack_transforms` in torch ops on the inputs' device: (xforms [G,20], sh_rot [G,84] | None) float32, the
    same layout and values, with no host round trip and no synchronisation (so, unlike pack_transforms, it cannot refuse
    a matrix that is not a proper rotation: that is the caller's to ensure).  rotations [G,3,3], translations [G,3],
    scales [G] or None (= 1).  The arithmetic is float64 whatever the inputs' dtype.  Runs under no_grad: the pose
    gradient does not come through here (see pose_gaussians)."""
    R = rotations.detach().to(torch.float64).reshape(-1, 3, 3)
    G, dev = R.shape[0], R.device
    t = translations.detach().to(torch.float64).reshape(-1, 3)
    if t.shape[0] != G:
        raise ValueError(f"{G} rotations but {t.shape[0]} translations")
    s = torch.ones(G, dtype=torch.float64, device=dev) if scales is None else scales.detach().to(torch.float64).reshape(G)
    x = torch.zeros((G, XFORM_FLOATS), dtype=torch.float64, device=dev)
    x[:, :9] = (s[:, None, None] * R).reshape(G, 9)
    x[:, 9:12] = t
    x[:, 12:16] = _rotmat_to_quat_torch(R)
    x[:, 16] = s
    rot = None
    if sh_degree >= 1:
        d, pinv = _fit_constants(sh_degree, dev)
        Y_old = _sh_basis_torch(sh_degree, d[None] @ R)                 # [G,64,(deg+1)^2]: rows are (R^T d)^T
        rot = torch.zeros((G, SH_ROT_FLOATS), dtype=torch.float64, device=dev)
        off = 0
        for l in range(1, sh_degree + 1):
            m = 2 * l + 1
            rot[:, off:off + m * m] = (pinv[l][None] @ Y_old[:, :, l * l:(l + 1) * (l + 1)]).reshape(G, m * m)
            off += m * m
        rot = rot.float()
    return x.float(), rot


# ---- the backward call ---------------------------------------------------------------------------------------
def workspace_bytes(n: int, n_groups: int) -> int:
    """mgs_pose_bwd_workspace_bytes: what the backward of n Gaussians in n_groups groups needs."""
    return int(_lib.lib().mgs_pose_bwd_workspace_bytes(int(n), int(n_groups)))


def pose_bwd_raw(means: Tensor, quats: Tensor, scales: Tensor, sh: Optional[Tensor], sh_degree: int,
                 group_ids: Optional[Tensor], xforms: Tensor, sh_rot: Optional[Tensor],
                 ct_means: Optional[Tensor] = None, ct_quats: Optional[Tensor] = None, ct_scales: Optional[Tensor] = None,
                 ct_sh: Optional[Tensor] = None, rest: bool = True, out: Optional[Dict] = None,
                 workspace: Optional[Tensor] = None) -> Dict:
    """mgs_pose_bwd on torch's current stream: no synchronisation, nothing read back.  means / quats / scales / sh are the
    POSED float32 tensors (sh [N,K,3] or None), xforms / sh_rot what the forward read, ct_* the cotangents (None = zero, no
    zero tensor is made).  rest: also the rest-pose gradients.  out: dict of preallocated contiguous float32 results
    (v_pose [G,8], and v_means, v_quats, v_scales, v_sh) -- those missing are allocated; workspace: a uint8 tensor of at
    least workspace_bytes(n, G) + 256 bytes (otherwise one is allocated for the call).  Returns the dict."""
    require_device(means, quats, scales, sh, group_ids, xforms, sh_rot, ct_means, ct_quats, ct_scales, ct_sh, workspace)
    n, G, dev = int(means.shape[0]), int(xforms.shape[0]), means.device
    res = dict(out) if out is not None else {}
    if res.get("v_pose") is None:
        res["v_pose"] = torch.empty((G, POSE_FLOATS), dtype=torch.float32, device=dev)
    if rest:
        for name, like in (("v_means", means), ("v_quats", quats), ("v_scales", scales), ("v_sh", sh)):
            if like is not None and res.get(name) is None:
                res[name] = torch.empty_like(like)
    workspace, pad = aligned_workspace(workspace, workspace_bytes(n, G), dev)
    check(_lib.lib().mgs_pose_bwd(
        n, ptr(means), ptr(quats), ptr(scales), int(sh_degree), int(sh.shape[1]) if sh is not None else 1, ptr(sh),
        ptr(group_ids), G, ptr(xforms), ptr(sh_rot) if sh is not None else None,
        ptr(ct_means), ptr(ct_quats), ptr(ct_scales), ptr(ct_sh),
        ptr(res.get("v_means")) if rest else None, ptr(res.get("v_quats")) if rest else None,
        ptr(res.get("v_scales")) if rest else None, ptr(res.get("v_sh")) if rest and sh is not None else None,
        ptr(res["v_pose"]), workspace.data_ptr() + pad, max(0, workspace.numel() - pad), stream_handle()), "mgs_pose_bwd")
    return res


def _aligned(t: Optional[Tensor]) -> Optional[Tensor]:
    """A contiguous view at an odd storage offset is copied: the kernels load float4 (include/mgs_pose.h)."""
    return t.clone() if t is not None and t.data_ptr() % 16 else t


def _skew_times(v: Tensor, R: Tensor) -> Tensor:
    """[v]x R for v [G,3], R [G,3,3]: column c of the result is v x R[:, :, c]."""
    return torch.linalg.cross(v[:, :, None].expand(-1, -1, 3), R, dim=1)


class _PoseFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, means, quats, scl, sh, R, t, s, gids, deg):
        xd, rd = pack_transforms_torch(R, t, s, deg if sh is not None else 0)
        n, G = means.shape[0], xd.shape[0]
        m, q, c = _f32c(means.detach()), _f32c(quats.detach()), _f32c(scl.detach())
        c_sh = _f32c(sh.detach()) if sh is not None else None
        o_m, o_q, o_c = torch.empty_like(m), torch.empty_like(q), torch.empty_like(c)
        o_sh = torch.empty_like(c_sh) if c_sh is not None else None
        check(_lib.lib().mgs_transform_gaussians(
            n, ptr(m), ptr(q), ptr(c), deg, int(c_sh.shape[1]) if c_sh is not None else 1, ptr(c_sh), ptr(gids), G,
            ptr(xd), ptr(rd), ptr(o_m), ptr(o_q), ptr(o_c), ptr(o_sh), stream_handle()), "mgs_transform_gaussians")
        ctx.save_for_backward(o_m, o_q, o_c, o_sh, xd, rd, gids, R, s)
        ctx.set_materialize_grads(False)       # an output nobody used arrives as None: mgs_pose_bwd takes NULL for it
        ctx.deg, ctx.t_dtype = deg, t.dtype
        ctx.dtypes = (means.dtype, quats.dtype, scl.dtype, sh.dtype if sh is not None else None)
        outs = (o_m, o_q, o_c) + ((o_sh,) if o_sh is not None else ())
        return outs

    @staticmethod
    @once_differentiable                      # the results come from a C call: a double backward raises
    def backward(ctx, *cts):
        o_m, o_q, o_c, o_sh, xd, rd, gids, R, s = ctx.saved_tensors
        ct = [_aligned(_f32c(g)) for g in cts] + [None] * (4 - len(cts))
        rest = any(ctx.needs_input_grad[:4])
        res = pose_bwd_raw(o_m, o_q, o_c, o_sh, ctx.deg, gids, xd, rd, ct[0], ct[1], ct[2], ct[3], rest=rest)
        vp = res["v_pose"]
        grads = [None] * 9
        if rest:
            for i, name in enumerate(("v_means", "v_quats", "v_scales", "v_sh")):
                if ctx.needs_input_grad[i] and res.get(name) is not None:
                    grads[i] = res[name].to(ctx.dtypes[i])
        if ctx.needs_input_grad[4]:
            Rm = R.reshape(-1, 3, 3)
            grads[4] = (0.5 * _skew_times(vp[:, 0:3].to(R.dtype), Rm)).reshape(R.shape)
        if ctx.needs_input_grad[5]:
            grads[5] = vp[:, 3:6].to(ctx.t_dtype)
        if s is not None and ctx.needs_input_grad[6]:
            grads[6] = (vp[:, 6].to(s.dtype) / s.reshape(-1)).reshape(s.shape)
        return tuple(grads)


def pose_gaussians(tensors: Dict, rotations: Tensor, translations: Tensor, scales: Optional[Tensor] = None,
                   group_ids: Optional[Tensor] = None, rotate_sh: bool = True) -> Dict:
    """`transform_gaussians` that autograd can see through: x -> s_g R_g x + t_g for the Gaussians of every group g.

    tensors: dict(means, quats, scales, opacities, colors [N,K,3], sh_degree) on the GPU; rotations [G,3,3],
    translations [G,3] and scales [G] (None = 1) are torch tensors on the same device, of any float dtype, and may
    require grad -- as may the Gaussian tensors.  group_ids: int32 [N], ids outside [0, G) do not move; None = one group.
    Forward runs mgs_transform_gaussians into fresh buffers (never in place; the posed outputs are kept for the
    backward), backward runs mgs_pose_bwd and returns

        v_R = 1/2 [v_omega]x R,   v_t,   v_s = v_lambda / s

    and the rest-pose gradients of the Gaussians where they are asked for.  v_R is the gradient projected onto the tangent
    space of SO(3) at R: it pairs with any dR = [d]x R as v_omega . d, so a parametrisation that stays on SO(3) receives
    its exact gradient; the components normal to SO(3) are zero by definition.  Returns the dict transform_gaussians
    returns, `opacities` shared (and `colors` too where they are not rotated)."""
    require_device(tensors["means"], rotations, translations, scales, group_ids)
    deg = int(tensors.get("sh_degree") or 0)
    colors = tensors["colors"]
    do_sh = rotate_sh and colors.dim() == 3 and colors.shape[1] >= (deg + 1) ** 2 and deg >= 1
    if rotations.dim() != 3 or rotations.shape[1:] != (3, 3) or translations.shape != (rotations.shape[0], 3):
        raise ValueError("expected rotations [G,3,3] and translations [G,3]")
    if scales is not None and scales.shape != (rotations.shape[0],):
        raise ValueError(f"expected scales [{rotations.shape[0]}]")
    gids = group_ids.to(torch.int32).contiguous() if group_ids is not None else None
    outs = _PoseFn.apply(tensors["means"], tensors["quats"], tensors["scales"], colors if do_sh else None,
                         rotations, translations, scales, gids, deg)
    return {"means": outs[0], "quats": outs[1], "scales": outs[2], "opacities": tensors["opacities"],
            "colors": outs[3] if do_sh else colors, "sh_degree": tensors.get("sh_degree")}


__all__ = ["pose_gaussians", "pack_transforms_torch", "pose_bwd_raw", "workspace_bytes", "sh_generator_matrices",
           "SH_GENERATORS", "POSE_FLOATS"]
