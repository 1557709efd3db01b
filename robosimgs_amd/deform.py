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

    posed = deform_gaussians_autograd(tensors, binding, particles_now)                   # autograd sees through it

`deform_gaussians_autograd` (include/mgs_deform_bwd.h) is the rigid mode with a backward: gradients reach the particles'
current positions (state and system identification through a differentiable simulator) and the rest state's means, quats
and scales (training a soft object from frames in which it is deformed).  Two launches, no floating-point atomics: the
scatter from Gaussians to particles goes through the binding's transpose in a fixed order.
"""
from __future__ import annotations

import math
from typing import Dict, Optional

import torch
from torch import Tensor
from torch.autograd.function import once_differentiable

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


def _rest_state(tensors: Dict, binding: "ParticleBinding", particles: Tensor, status: Optional[Tensor]):
    """The checks deform_gaussians and deform_gaussians_autograd open with: rows for the binding's n Gaussians, its particle
    set, status uint8 [n] or None.  The device check stays the callers': deform_gaussians' colours ValueError precedes it."""
    means, quats, scales = _rows(tensors["means"], 3, "means"), _rows(tensors["quats"], 4, "quats"), _rows(tensors["scales"], 3, "scales")
    for t, what in ((means, "means"), (quats, "quats"), (scales, "scales")):
        if t.shape[0] != binding.n:
            raise ValueError(f"{what} has {t.shape[0]} rows, the binding was made for {binding.n} Gaussians")
    _particles(particles, binding.m, "particles")
    if status is not None:
        check_tensor("status", status, torch.uint8, (binding.n,))
    return means, quats, scales


class ParticleBinding:
    """What bind_particles made, neighbour-major device tensors (include/mgs_deform.h): idx int32 [8,N], w float32 [8,N],
    p float32 [8,3,N], rest float32 [12,N], flags uint8 [N]; n Gaussians, m particles.  `particles` (optional): the rest
    positions float32 [M,3] the binding was made from, which FrameRenderer(deform=) starts every slot with."""

    def __init__(self, idx: Tensor, w: Tensor, p: Tensor, rest: Tensor, flags: Tensor, n: int, m: int,
                 particles: Optional[Tensor] = None):
        self.idx, self.w, self.p, self.rest, self.flags, self.n, self.m = idx, w, p, rest, flags, int(n), int(m)
        self.particles = particles
        self._transposed = None
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

    def transposed(self):
        """The transposed binding mgs_deform_apply_bwd scatters through (include/mgs_deform_bwd.h): (t_start int32 [m + 1],
        t_entry int32 [8 n]).  t_entry lists k n + i for every (neighbour row k, Gaussian i), ordered by the particle
        idx[k][i] and ascending within a particle (a stable sort); entries t_start[j] .. t_start[j + 1] - 1 are particle
        j's.  Entries of unbound Gaussians (index -1) sort to the front, before t_start[0], and are never referenced.
        Built once and cached (reordered() makes a new binding, which builds its own); no synchronising call."""
        if self._transposed is None:
            with torch.no_grad():
                keys, order = torch.sort(self.idx.reshape(-1), stable=True)
                ids = torch.arange(self.m + 1, dtype=torch.int32, device=self.idx.device)
                t_start = torch.searchsorted(keys, ids).to(torch.int32)
                self._transposed = (t_start.contiguous(), order.to(torch.int32).contiguous())
        return self._transposed

    @torch.no_grad()
    def shift_offsets_(self, delta: Tensor) -> "ParticleBinding":
        """rest[0:3] += delta^T for delta [n,3], in place: the offsets d0 = mu - Xbar follow a change of the means with
        the neighbours and weights held fixed, which is the derivative deform_gaussians_autograd reports as the gradient
        of `means` -- so a trained mean takes effect without a re-bind.  Rows of unbound Gaussians stay zero."""
        _rows(delta, 3, "delta")
        if delta.shape[0] != self.n:
            raise ValueError(f"delta has {delta.shape[0]} rows, the binding was made for {self.n} Gaussians")
        bound = ((self.flags & FLAG_UNBOUND) == 0).to(self.rest.dtype)
        self.rest[0:3] += delta.to(self.rest.device, self.rest.dtype).t() * bound[None, :]
        return self

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


def apply_bwd_workspace_bytes(n: int) -> int:
    """mgs_deform_apply_bwd_workspace_bytes: what the backward of n Gaussians needs."""
    return int(_lib.lib().mgs_deform_apply_bwd_workspace_bytes(int(n)))


def deform_apply_bwd_raw(quats: Tensor, binding: ParticleBinding, particles: Tensor, status: Tensor,
                         ct_means: Optional[Tensor] = None, ct_quats: Optional[Tensor] = None,
                         ct_scales: Optional[Tensor] = None, rest: bool = True, out: Optional[Dict] = None,
                         bwd_status: Optional[Tensor] = None, workspace: Optional[Tensor] = None) -> Dict:
    """mgs_deform_apply_bwd on torch's current stream: two launches, no synchronisation, capturable.  quats: the REST
    quaternions float32 [n,4]; particles float32 [m,3]; status uint8 [n]: what the mode-0 forward wrote for these
    arguments; ct_*: the cotangents of the deformed means / quats / scales (None = zero, no zero tensor is made).  rest:
    also the rest-state gradients.  out: dict of preallocated contiguous float32 results (v_particles [m,3], and v_means,
    v_quats, v_scales) -- those missing are allocated; bwd_status uint8 [n] or None (bit 0: the guard dropped the row's
    rotation gradient); workspace: a uint8 tensor of at least apply_bwd_workspace_bytes(n) + 256 bytes (otherwise one is
    allocated for the call).  Returns the dict."""
    t_start, t_entry = binding.transposed()
    require_device(quats, particles, status, ct_means, ct_quats, ct_scales, bwd_status, workspace, binding.idx)
    n, m, dev = binding.n, binding.m, binding.idx.device
    check_tensor("quats", quats, torch.float32, (n, 4))
    check_tensor("particles", particles, torch.float32, (m, 3))
    check_tensor("status", status, torch.uint8, (n,))
    for name, t, cols in (("ct_means", ct_means, 3), ("ct_quats", ct_quats, 4), ("ct_scales", ct_scales, 3)):
        if t is not None:
            check_tensor(name, t, torch.float32, (n, cols))
    if bwd_status is not None:
        check_tensor("bwd_status", bwd_status, torch.uint8, (n,))
    res = dict(out) if out is not None else {}
    want = [("v_particles", (m, 3))] + ([("v_means", (n, 3)), ("v_quats", (n, 4)), ("v_scales", (n, 3))] if rest else [])
    for name, shape in want:
        if res.get(name) is None:
            res[name] = torch.empty(shape, dtype=torch.float32, device=dev)
        else:
            check_tensor(f"out[{name!r}]", res[name], torch.float32, shape)
    workspace, pad = aligned_workspace(workspace, apply_bwd_workspace_bytes(n) if workspace is None else 0, dev)
    g = (lambda name: ptr(res[name])) if rest else (lambda name: None)
    check(_lib.lib().mgs_deform_apply_bwd(
        n, ptr(quats), ptr(binding.idx), ptr(binding.w), ptr(binding.p), ptr(binding.rest), ptr(binding.flags), m,
        ptr(particles), ptr(status), ptr(ct_means), ptr(ct_quats), ptr(ct_scales), ptr(t_start), ptr(t_entry),
        g("v_means"), g("v_quats"), g("v_scales"), ptr(res["v_particles"]), ptr(bwd_status),
        workspace.data_ptr() + pad, max(0, workspace.numel() - pad), stream_handle()), "mgs_deform_apply_bwd")
    return res


def _aligned(t: Optional[Tensor]) -> Optional[Tensor]:
    """A contiguous view at an odd storage offset is copied: the kernels load float4 (include/mgs_deform_bwd.h)."""
    return t.clone() if t is not None and t.data_ptr() % 16 else t


class _DeformFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, means, quats, scales, particles, binding, status):
        mu, q, s, x = (_f32c(t.detach()) for t in (means, quats, scales, particles))
        q = _aligned(q)
        o_m, o_q, o_s = torch.empty_like(mu), torch.empty_like(q), torch.empty_like(s)
        deform_apply_raw(mu, q, s, binding, MODES["rigid"], x, o_m, o_q, o_s, status=status)
        ctx.save_for_backward(q, x, status)
        ctx.set_materialize_grads(False)       # an output nobody used arrives as None: mgs_deform_apply_bwd takes NULL
        ctx.binding = binding
        ctx.dtypes = (means.dtype, quats.dtype, scales.dtype, particles.dtype)
        return o_m, o_q, o_s

    @staticmethod
    @once_differentiable                      # the results come from a C call: a double backward raises
    def backward(ctx, ct_m, ct_q, ct_s):
        q, x, status = ctx.saved_tensors
        ct = [_aligned(_f32c(g)) if g is not None else None for g in (ct_m, ct_q, ct_s)]
        rest = any(ctx.needs_input_grad[:3])
        res = deform_apply_bwd_raw(q, ctx.binding, x, status, ct[0], ct[1], ct[2], rest=rest)
        names = ("v_means", "v_quats", "v_scales", "v_particles")
        grads = [res[name].to(ctx.dtypes[i]) if ctx.needs_input_grad[i] else None for i, name in enumerate(names)]
        return (*grads, None, None)


def deform_gaussians_autograd(tensors: Dict, binding: ParticleBinding, particles: Tensor, status: Optional[Tensor] = None,
                              mode: str = "rigid", rotate_sh: bool = False) -> Dict:
    """`deform_gaussians` in the rigid mode that autograd can see through.  The forward is mgs_deform_apply, mode 0; the
    backward is mgs_deform_apply_bwd (include/mgs_deform_bwd.h): a closed form on top of what the forward computes, and a
    scatter from Gaussians to particles through the binding's transpose -- no floating-point atomics, the same bits in
    every run.  `particles` and the rest state's `means`, `quats`, `scales` may each require grad; `opacities` and
    `colors` are shared with `tensors`, so autograd passes through them by identity.  status: uint8 [N] that receives the
    forward's STATUS_* bits (one is allocated where none is given: the backward follows the forward's branch from it, so
    do not overwrite it before backward()).

    The mean.  A bound Gaussian's position comes from the offset d0 in the binding, not from `means`: the gradient of a
    bound row of `means` is DEFINED as that of d0 -- the derivative with the binding's neighbours and weights held fixed
    and d0 = mu - Xbar following the mean.  After an optimiser step on the means, binding.shift_offsets_(delta) moves d0
    by the same amount, so that the trained mean takes effect without a re-bind.  Rows that pass through (unbound, or a
    non-finite neighbour this frame) take their cotangents bit for bit and give the particles exactly 0; thin rows are
    translated only.  Where an inverted neighbourhood (det P < 0) leaves the rotation undetermined the rotation's gradient
    is dropped for that row (the header's guard).

    The affine mode and rotate_sh=True have no backward: NotImplementedError."""
    if mode != "rigid":
        if mode not in MODES:
            raise ValueError(f"mode {mode!r} not in {tuple(MODES)}")
        raise NotImplementedError(f"deform_gaussians_autograd: mode {mode!r} has no backward, only 'rigid' (use "
                                  "deform_gaussians for a forward without gradients)")
    if rotate_sh:
        raise NotImplementedError("deform_gaussians_autograd: rotate_sh=True has no backward (use deform_gaussians for a "
                                  "forward without gradients)")
    means, quats, scales = _rest_state(tensors, binding, particles, status)
    require_device(means, quats, scales, particles, status, binding.idx)
    if status is None:
        status = torch.empty((binding.n,), dtype=torch.uint8, device=means.device)
    o_m, o_q, o_s = _DeformFn.apply(means, quats, scales, particles, binding, status)
    return {"means": o_m, "quats": o_q, "scales": o_s, "opacities": tensors["opacities"], "colors": tensors["colors"],
            "sh_degree": tensors.get("sh_degree")}


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
    means, quats, scales = _rest_state(tensors, binding, particles, status)
    n, colors, deg = binding.n, tensors["colors"], int(tensors.get("sh_degree") or 0)
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
           "deform_gaussians_autograd", "deform_apply_bwd_raw", "apply_bwd_workspace_bytes", "bind_workspace_bytes", "MODES", "REST_ROWS", "FLAG_UNBOUND", "FLAG_FLAT", "FLAG_THIN", "STATUS_UNBOUND",
           "STATUS_FALLBACK", "STATUS_THIN", "STATUS_NONFINITE"]
