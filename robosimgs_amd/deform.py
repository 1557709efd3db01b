"""Gaussians that follow simulated particles (include/mgs_deform.h, csrc/deform.hip): bind once, move per frame.

    binding = bind_particles(tensors["means"], particles_rest, select=soft_mask)       # once per object
    posed = deform_gaussians(tensors, binding, particles_now, mode="rigid", out=posed)   # every frame
    colors, alphas, _ = rasterization(posed["means"], posed["quats"], posed["scales"], ...)

A particle simulator (MPM, PBD) hands over a few tens of thousands of particle positions per step.  `bind_particles` ties
every Gaussian to its 8 nearest particles of the rest state (a brute-force search on the GPU, fp32 difference form, ties
to the lower index) and stores weights, weighted rest offsets and the neighbourhood's inverse moment matrix.
`deform_gaussians` then moves each Gaussian with its neighbours' current positions: mode "rigid" rotates it by shape
matching (Mueller et al. 2005), mode "affine" also stretches it, Sigma' = A Sigma A^T (PhysGaussian).  Stateless,
capturable, nothing is read back, no floating-point atomics: the same inputs give the same bytes.  Opacities and colours
are shared with the input and SH rows are not rotated: what transform_gaussians(rotate_sh=False) gives.

    posed = deform_gaussians(tensors, binding, particles_now, rotate_sh=True, out=posed)     # colours turn too

rotate_sh=True (include/mgs_deform_sh.h) turns every Gaussian's SH rows by the rotation its rigid branch applies -- in both
modes, so an affine frame has the colours of a rigid one -- in the same launch; the result then owns a `colors` tensor
(192 bytes per Gaussian at degree 3).  Rows of thin, unbound and non-finite Gaussians are the rest rows bit for bit.
`FrameRenderer(deform=binding[, deform_rotate_sh=True])` runs it inside every slot's graph (pipeline.py).
"""
from __future__ import annotations

import math
from typing import Dict, Optional

import torch
from torch import Tensor

from . import _lib
from ._lib import DEFORM_K, aligned_workspace, check, check_tensor, ptr, require_device, stream_handle
from .ops import _f32c

REST_ROWS = 12           # include/mgs_deform.h: d0 (3), Q^-1 (6), h^2, lambda_mid / lambda_max, lambda_min / lambda_max
FLAG_UNBOUND, FLAG_FLAT, FLAG_THIN = 1, 2, 4
STATUS_UNBOUND, STATUS_FALLBACK, STATUS_THIN, STATUS_NONFINITE = 1, 2, 4, 8
MODES = {"rigid": 0, "affine": 1}


def bind_workspace_bytes(n: int, m: int) -> int:
    """mgs_deform_bind_workspace_bytes: what binding n Gaussians to m particles needs."""
    return int(_lib.lib().mgs_deform_bind_workspace_bytes(int(n), int(m)))


def _rows(x: Tensor, cols: int, what: str) -> Tensor:
    if not torch.is_tensor(x) or x.dim() != 2 or x.shape[1] != cols:
        raise ValueError(f"{what} must be a tensor [n,{cols}], got {tuple(x.shape) if torch.is_tensor(x) else type(x).__name__}")
    if not x.dtype.is_floating_point:
        raise ValueError(f"{what} must be a floating-point tensor, got {x.dtype}")
    return x


def _particles(x: Tensor, m: Optional[int], what: str) -> Tensor:
    _rows(x, 3, what)
    if x.shape[0] < DEFORM_K:
        raise ValueError(f"{what}: {x.shape[0]} particles, at least {DEFORM_K} needed")
    if m is not None and x.shape[0] != m:
        raise ValueError(f"{what} must be [{m},3] (the particle set the binding was made for), got {tuple(x.shape)}")
    return x


class ParticleBinding:
    """What bind_particles made, neighbour-major device tensors (include/mgs_deform.h): idx int32 [8,N], w float32 [8,N],
    p float32 [8,3,N], rest float32 [12,N], flags uint8 [N]; n Gaussians, m particles.  `particles` (optional): the rest
    positions float32 [M,3] the binding was made from, which FrameRenderer(deform=) starts every slot with."""

    def __init__(self, idx: Tensor, w: Tensor, p: Tensor, rest: Tensor, flags: Tensor, n: int, m: int,
                 particles: Optional[Tensor] = None):
        self.idx, self.w, self.p, self.rest, self.flags, self.n, self.m = idx, w, p, rest, flags, int(n), int(m)
        self.particles = particles
        want = {"idx": ((DEFORM_K, self.n), torch.int32), "w": ((DEFORM_K, self.n), torch.float32),
                "p": ((DEFORM_K, 3, self.n), torch.float32), "rest": ((REST_ROWS, self.n), torch.float32),
                "flags": ((self.n,), torch.uint8)}
        for name, (shape, dtype) in want.items():
            check_tensor(f"binding.{name}", getattr(self, name), dtype, shape)

    def reordered(self, order: Tensor) -> "ParticleBinding":
        """The binding of the Gaussians taken in `order` (int64 [N']: new position -> old index; FrameRenderer's Morton
        order): an index_select on the last dimension of every array."""
        order = order.to(self.idx.device)
        sel = lambda t: t.index_select(t.dim() - 1, order).contiguous()
        return ParticleBinding(sel(self.idx), sel(self.w), sel(self.p), sel(self.rest), sel(self.flags),
                               int(order.shape[0]), self.m, self.particles)

    def n_bound(self) -> int:
        """How many Gaussians are bound (reads the flags back: one synchronising copy)."""
        return int(((self.flags & FLAG_UNBOUND) == 0).sum().item())

    def __repr__(self):
        return f"ParticleBinding(n={self.n}, m={self.m}, device={self.idx.device})"


def deform_bind_raw(means: Tensor, particles: Tensor, select: Optional[Tensor], max_distance: float, idx: Tensor,
                    w: Tensor, p: Tensor, rest: Tensor, flags: Tensor, workspace: Optional[Tensor] = None) -> None:
    """mgs_deform_bind on torch's current stream: no synchronisation, capturable.  means float32 [n,3] and particles
    float32 [m,3] contiguous on the GPU, select uint8 [n] or None, the five outputs as ParticleBinding describes them.
    workspace: a uint8 tensor of bind_workspace_bytes(n, m) + 256 bytes (a caller that captures a graph keeps its own);
    otherwise one is allocated for the call."""
    require_device(means, particles, select, idx, w, p, rest, flags, workspace)
    n, m, L = int(means.shape[0]), int(particles.shape[0]), _lib.lib()
    need = 0 if workspace is not None else int(L.mgs_deform_bind_workspace_bytes(n, m))
    workspace, pad = aligned_workspace(workspace, need, means.device)
    check(L.mgs_deform_bind(n, ptr(means), ptr(select), m, ptr(particles), float(max_distance),
                            workspace.data_ptr() + pad, max(0, workspace.numel() - pad), ptr(idx), ptr(w), ptr(p), ptr(rest),
                            ptr(flags), stream_handle()), "mgs_deform_bind")


def deform_apply_raw(means: Tensor, quats: Tensor, scales: Tensor, binding: ParticleBinding, mode: int, particles: Tensor,
                     out_means: Tensor, out_quats: Tensor, out_scales: Tensor, status: Optional[Tensor] = None) -> None:
    """mgs_deform_apply on torch's current stream: one launch, no workspace, capturable.  Everything float32, contiguous
    and on the GPU; mode 0 rigid, 1 affine; status uint8 [n] or None."""
    require_device(means, quats, scales, particles, out_means, out_quats, out_scales, status, binding.idx)
    check(_lib.lib().mgs_deform_apply(binding.n, ptr(means), ptr(quats), ptr(scales), ptr(binding.idx), ptr(binding.w),
                                      ptr(binding.p), ptr(binding.rest), ptr(binding.flags), int(mode), binding.m,
                                      ptr(particles), ptr(out_means), ptr(out_quats), ptr(out_scales), ptr(status),
                                      stream_handle()), "mgs_deform_apply")


def deform_apply_sh_raw(means: Tensor, quats: Tensor, scales: Tensor, binding: ParticleBinding, mode: int, particles: Tensor,
                        out_means: Tensor, out_quats: Tensor, out_scales: Tensor, sh_degree: int, colors: Tensor,
                        out_colors: Tensor, copy_unbound: bool = True, status: Optional[Tensor] = None) -> None:
    """mgs_deform_apply_sh on torch's current stream: deform_apply_raw that also turns the SH rows, one launch, no
    workspace, capturable.  colors and out_colors: float32 [n,K,3], contiguous, different buffers, K >= (sh_degree + 1)^2.
    copy_unbound=False leaves the rows of unbound Gaussians in out_colors as they are."""
    require_device(means, quats, scales, particles, out_means, out_quats, out_scales, status, binding.idx, colors, out_colors)
    for t, what in ((colors, "colors"), (out_colors, "out_colors")):
        check_tensor(what, t, torch.float32, (binding.n, -1, 3))
    if out_colors.shape != colors.shape:
        raise ValueError(f"out_colors {list(out_colors.shape)} is not the shape of colors {list(colors.shape)}")
    check(_lib.lib().mgs_deform_apply_sh(binding.n, ptr(means), ptr(quats), ptr(scales), ptr(binding.idx), ptr(binding.w),
                                         ptr(binding.p), ptr(binding.rest), ptr(binding.flags), int(mode), binding.m,
                                         ptr(particles), ptr(out_means), ptr(out_quats), ptr(out_scales), ptr(status),
                                         int(sh_degree), int(colors.shape[1]), ptr(colors), ptr(out_colors),
                                         int(bool(copy_unbound)), stream_handle()), "mgs_deform_apply_sh")


@torch.no_grad()
def bind_particles(means: Tensor, particles: Tensor, select: Optional[Tensor] = None,
                   max_distance: float = math.inf) -> ParticleBinding:
    """Tie Gaussians to the particles of a simulator's rest state.  means [N,3] and particles [M,3] (M >= 8) on the GPU;
    select: bool or integer [N], nonzero = bind this Gaussian (None: all); max_distance: a Gaussian whose nearest particle
    is farther away stays unbound (deform_gaussians passes it through).  A non-finite particle is nobody's neighbour and a
    Gaussian with a non-finite mean stays unbound.  No synchronisation."""
    _rows(means, 3, "means")
    _particles(particles, None, "particles")
    n = means.shape[0]
    if select is not None and (not torch.is_tensor(select) or tuple(select.shape) != (n,) or select.dtype.is_floating_point):
        raise ValueError(f"select must be a bool or integer tensor [{n}]")
    if not (max_distance > 0):                           # also refuses a NaN
        raise ValueError(f"max_distance {max_distance} is not a positive number")
    require_device(means, particles, select)
    dev, m = means.device, particles.shape[0]
    mu, x = _f32c(means.detach()), _f32c(particles.detach())
    sel = None if select is None else (select != 0).to(torch.uint8).contiguous()
    idx = torch.empty((DEFORM_K, n), dtype=torch.int32, device=dev)
    w = torch.empty((DEFORM_K, n), dtype=torch.float32, device=dev)
    p = torch.empty((DEFORM_K, 3, n), dtype=torch.float32, device=dev)
    rest = torch.empty((REST_ROWS, n), dtype=torch.float32, device=dev)
    flags = torch.empty((n,), dtype=torch.uint8, device=dev)
    deform_bind_raw(mu, x, sel, max_distance, idx, w, p, rest, flags)
    return ParticleBinding(idx, w, p, rest, flags, n, m, x.clone())      # (a copy: the simulator may step `particles` in place)


@torch.no_grad()
def deform_gaussians(tensors: Dict, binding: ParticleBinding, particles: Tensor, mode: str = "rigid",
                     out: Optional[Dict] = None, status: Optional[Tensor] = None, rotate_sh: bool = False,
                     copy_unbound: bool = True) -> Dict:
    """Move the Gaussians of `tensors` (the REST state: dict(means, quats, scales, opacities, colors, sh_degree) on the GPU,
    scales activated) with the particles' current positions [M,3].  The dictionary contract of transform_gaussians: returns
    a new dict that shares `opacities` and `colors`; pass out=<previous result> to reuse its buffers every frame.
    out=tensors is refused: the rest state must survive, every frame deforms it anew.  status: uint8 [N], receives per
    Gaussian 0 or the STATUS_* bits (unbound, affine fell back to rigid, thin: translated only, a neighbour was non-finite).
    rotate_sh=True, with colors [N,K,3], K >= (sh_degree + 1)^2 and sh_degree >= 1: every Gaussian's SH rows turn with it
    (mgs_deform_apply_sh, the same single launch) and the result has a `colors` tensor of its own: out["colors"] where it
    has the right shape and is not the rest state's buffer (a previous rotate_sh=False result shares the rest's colours),
    a new tensor otherwise.  copy_unbound=False then leaves the rows of unbound Gaussians in that tensor as they are (a
    caller that filled them once); bound rows are always rewritten.  Otherwise the call is the one without SH."""
    if mode not in MODES:
        raise ValueError(f"mode {mode!r} not in {tuple(MODES)}")
    if out is tensors and out is not None:
        raise ValueError("out is tensors: deform_gaussians deforms the rest state anew every frame and must not overwrite it")
    n = binding.n
    means, quats, scales = _rows(tensors["means"], 3, "means"), _rows(tensors["quats"], 4, "quats"), _rows(tensors["scales"], 3, "scales")
    for t, what in ((means, "means"), (quats, "quats"), (scales, "scales")):
        if t.shape[0] != n:
            raise ValueError(f"{what} has {t.shape[0]} rows, the binding was made for {n} Gaussians")
    _particles(particles, binding.m, "particles")
    if status is not None:
        check_tensor("status", status, torch.uint8, (n,))
    colors, deg = tensors["colors"], int(tensors.get("sh_degree") or 0)
    do_sh = bool(rotate_sh) and torch.is_tensor(colors) and colors.dim() == 3 and colors.shape[1] >= (deg + 1) ** 2 and deg >= 1
    if do_sh and (colors.shape[0] != n or colors.shape[2] != 3 or not colors.dtype.is_floating_point):
        raise ValueError(f"colors must be [{n},K,3], got {colors.dtype} {list(colors.shape)}")
    require_device(means, particles, status, colors if do_sh else None)
    means, quats, scales, x = _f32c(means), _f32c(quats), _f32c(scales), _f32c(particles)
    res = out if out is not None else {}
    outs = []
    for key, src in (("means", means), ("quats", quats), ("scales", scales)):
        o = res.get(key)
        if o is None:
            o = torch.empty_like(src)
        else:
            check_tensor(f"out[{key!r}]", o, torch.float32, src.shape)
            if o.data_ptr() == src.data_ptr():
                raise ValueError(f"out[{key!r}] is the rest state's own buffer: the rest state must survive")
        outs.append(o)
    if do_sh:
        sh_in = _f32c(colors)
        o = res.get("colors")
        if (not torch.is_tensor(o) or o.dtype != torch.float32 or o.shape != sh_in.shape or not o.is_contiguous()
                or not o.is_cuda or o.data_ptr() == sh_in.data_ptr() or o.data_ptr() == colors.data_ptr()):
            o = torch.empty_like(sh_in)
            copy_unbound = True                      # nobody has filled a fresh tensor's unbound rows
        deform_apply_sh_raw(means, quats, scales, binding, MODES[mode], x, *outs, deg, sh_in, o, copy_unbound, status=status)
        colors = o
    else:
        deform_apply_raw(means, quats, scales, binding, MODES[mode], x, *outs, status=status)
    return {"means": outs[0], "quats": outs[1], "scales": outs[2], "opacities": tensors["opacities"],
            "colors": colors, "sh_degree": tensors.get("sh_degree")}


__all__ = ["ParticleBinding", "bind_particles", "deform_gaussians", "deform_bind_raw", "deform_apply_raw", "deform_apply_sh_raw",
           "bind_workspace_bytes", "MODES", "REST_ROWS", "FLAG_UNBOUND", "FLAG_FLAT", "FLAG_THIN", "STATUS_UNBOUND",
           "STATUS_FALLBACK", "STATUS_THIN", "STATUS_NONFINITE"]
