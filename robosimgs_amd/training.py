"""Helpers for training loops on top of `rasterization()`.

`reorder_parameters`: put a trainer's Gaussians (and the optimiser state that belongs to them) in Morton order of the means.
The render path is faster on a spatially ordered scene -- SH rows of neighbours are contiguous, a binning workgroup's pairs
fall into few tile groups, a tile's list gathers from a narrow index range: the training step takes 0.84 instead of
0.87 ms at 1 M Gaussians (bench.py `fwd_bwd` / `fwd_bwd.morton_order`) -- and the order of the parameter tensors is the
trainer's to choose.  Gradient descent is equivariant under a permutation of the Gaussians, so re-ordering every few hundred
steps (e.g. where splatfacto densifies, which rebuilds the tensors anyway) changes nothing but memory order, up to which of
two Gaussians that tie in depth to the last bit is blended first.
"""
from __future__ import annotations

from typing import Dict, Iterable, Optional

import torch

from .optim import GaussianAdam
from .pipeline import locality_order


@torch.no_grad()
def reorder_parameters(params: Dict[str, torch.Tensor], optimizer: Optional[torch.optim.Optimizer] = None,
                       key: str = "means", bits: int = 10, per_gaussian: Optional[Iterable[str]] = None,
                       extra_state: Iterable[torch.Tensor] = ()) -> torch.Tensor:
    """Permute the per-Gaussian tensors of `params` into Morton order of params[key], in place (the tensors stay the same
    objects, so an optimiser keeps its references), together with the per-parameter state tensors of `optimizer` that
    have the Gaussian count as their first dimension (Adam's exp_avg / exp_avg_sq ...).  Returns the permutation (new
    position -> old index).

    per_gaussian: the keys of `params` that are per-Gaussian (first dimension = the Gaussian count).  None (default)
    takes every tensor whose first dimension equals the count -- a heuristic that also catches an unrelated parameter which
    happens to have N rows, so name the keys where that can be.  A tensor object listed under two keys is permuted once.
    extra_state: further per-Gaussian tensors that must follow -- a densification strategy's accumulators (gsplat's
    `grad2d`, `count`, `radii` ...), anything indexed like the Gaussians that lives outside `params` and the optimiser.
    Whatever is NOT handed over keeps the old order and no longer matches: permute it with the returned `order`."""
    n = params[key].shape[0]
    order = locality_order(params[key], bits)
    keys = list(per_gaussian) if per_gaussian is not None else [k for k, p in params.items()
                                                                  if torch.is_tensor(p) and p.dim() >= 1 and p.shape[0] == n]
    seen = set()                                   # (by storage: the same tensor under two keys is permuted once)

    def permute(t_):
        if not torch.is_tensor(t_) or (t_.data_ptr(), t_.device) in seen:
            return
        if t_.dim() < 1 or t_.shape[0] != n:
            raise ValueError(f"a tensor of shape {tuple(t_.shape)} is not per-Gaussian (first dimension {n})")
        seen.add((t_.data_ptr(), t_.device))
        t_.copy_(t_.index_select(0, order.to(t_.device)))

    for k in keys:
        p = params[k]
        first = (p.data_ptr(), p.device) not in seen
        permute(p.data)
        if not first:
            continue
        if p.grad is not None:
            permute(p.grad)
        if optimizer is not None and p in optimizer.state:
            for st in optimizer.state[p].values():
                if torch.is_tensor(st) and st.dim() >= 1 and st.shape[0] == n:
                    permute(st)
    for t_ in extra_state:
        permute(t_)
    return order


class Trainer:
    """A splatfacto-style loop's parameters, optimiser and render call in one place, so that the ordered rate is the DEFAULT
    rate: `Trainer.render()` is `rasterization()` on the trainer's parameters, and every `auto_reorder_every` steps (and at
    the first one) the parameters, the optimiser's per-Gaussian state and whatever `extra_state` was handed over are put
    into Morton order of the means first (`reorder_parameters`) -- the one thing a plain `rasterization()` caller has to
    remember to do to get the 4-5 % (uniform scene) to 25 % (a clustered export whose large Gaussians sit together in the
    index range) faster step.

        tr = Trainer(params, torch.optim.Adam(params.values(), lr=1e-3), width=W, height=H, sh_degree=3,
                     auto_reorder_every=500, isect_capacity=cap, render_mode="RGB+ED")
        for it in range(iters):
            colors, alphas, meta = tr.render(viewmats, Ks)          # reorders when due
            tr.step(l1_loss(colors, target))                        # backward, optimiser step, zero_grad

    Gradient descent is equivariant under the permutation: the trajectory is the un-reordered one up to the order of
    floating-point sums (tests/test_training_host.py, tests/test_gpu_backward.py).  `original_index[i]` is the index Gaussian
    i had when the trainer was built (or last `rebind`): per-Gaussian data kept OUTSIDE the trainer is brought along with
    `x[tr.last_order]` after a reorder, or looked up through `original_index`.

    DENSIFICATION rebuilds the parameter tensors (new objects, new count): call `rebind(params, optimizer, extra_state)`
    with the new ones; the next render reorders them.  A strategy that keeps per-Gaussian accumulators (gsplat's `grad2d`,
    `count`, `radii`) hands them over as `extra_state` so that they follow; anything not handed over keeps the old order.
    render_fn: the render call (default robosimgs_amd.rasterization) -- (means, quats, scales, opacities, colors, viewmats,
    Ks, width, height, **kw) -> (colors, alphas, meta).

    raw_params=True: params["scales"] / params["opacities"] hold log-scales / opacity logits, as splatfacto keeps them, and
    the render call gets raw_params=True (rasterization activates them inside its projection kernels).  The optimiser's
    leaves are then the very tensors handed in, with no activation graph in between: their .grad comes straight out of the
    library's backward.  KEYS, reorder_parameters and rebind work as in the activated form.

    optimizer = robosimgs_amd.GaussianAdam(..., selective=True): `step` hands it the radii of the last `render` as the
    visibility mask, so the Gaussians that render did not see keep their parameters and moments (gsplat's SelectiveAdam).
    Every other optimiser is stepped with no arguments.

    strategy = robosimgs_amd.MCMCStrategy(...): `step` ends with strategy.step(self) -- splatfacto-mcmc's relocation and
    growth when due (the strategy rebinds the trainer to the grown views of its storage) and its noise every step.
    None (default): nothing is called.

    raster_kwargs are rasterization's, the camera's among them: camera_model=, distortion= (the fisheye lens) and
    pinhole_distortion= (OpenCV's k1 k2 p1 p2 k3 of a calibrated pinhole camera), so a scene trains against raw captures."""

    KEYS = ("means", "quats", "scales", "opacities", "colors")

    def __init__(self, params: Dict[str, torch.Tensor], optimizer: Optional[torch.optim.Optimizer], width: int, height: int,
                 auto_reorder_every: int = 500, extra_state: Iterable[torch.Tensor] = (), render_fn=None, bits: int = 10,
                 raw_params: bool = False, strategy=None, **raster_kwargs):
        self.width, self.height = int(width), int(height)
        self.auto_reorder_every = int(auto_reorder_every)
        self.bits = int(bits)
        self.raw_params = bool(raw_params)
        self.raster_kwargs = dict(raster_kwargs, raw_params=True) if self.raw_params else dict(raster_kwargs)
        self._render_fn = render_fn
        self.strategy = strategy
        self.it = 0
        self.reorders = 0
        self.last_order: Optional[torch.Tensor] = None
        self.last_meta: Optional[dict] = None          # meta of the last render() under a selective GaussianAdam: its visibility
        self.rebind(params, optimizer, extra_state)

    def rebind(self, params: Dict[str, torch.Tensor], optimizer: Optional[torch.optim.Optimizer],
               extra_state: Iterable[torch.Tensor] = ()) -> None:
        """New parameter tensors / optimiser (after densification, pruning, a checkpoint load): the next render reorders."""
        missing = [k for k in self.KEYS if k not in params]
        if missing:
            raise KeyError(f"params lacks {missing} (needs {self.KEYS})")
        self.params, self.optimizer, self.extra_state = params, optimizer, list(extra_state)
        self.last_meta = None
        n = params["means"].shape[0]
        self.original_index = torch.arange(n, device=params["means"].device)
        self._due = self.auto_reorder_every > 0

    def reorder(self) -> torch.Tensor:
        """Morton order now (parameters, optimiser state, extra_state, original_index).  Returns the permutation."""
        order = reorder_parameters(self.params, self.optimizer, bits=self.bits, per_gaussian=[k for k in self.KEYS],
                                   extra_state=[*self.extra_state, self.original_index])
        self.last_order, self._due = order, False
        self.reorders += 1
        self._since = 0
        return order

    def render(self, viewmats, Ks, **kw):
        if self._due or (self.auto_reorder_every > 0 and getattr(self, "_since", 0) >= self.auto_reorder_every):
            self.reorder()
        fn = self._render_fn
        if fn is None:
            from .rendering import rasterization as fn
        p = self.params
        out = fn(p["means"], p["quats"], p["scales"], p["opacities"], p["colors"], viewmats, Ks, self.width, self.height,
                 **{**self.raster_kwargs, **kw})
        if self._selective():           # only then: a kept meta keeps the frame's per-camera state alive until the next render
            self.last_meta = out[2]
        return out

    def _selective(self) -> bool:
        return isinstance(self.optimizer, GaussianAdam) and self.optimizer.selective

    def step(self, loss: torch.Tensor) -> None:
        """loss.backward(), optimiser step, zero_grad(set_to_none=True); counts the step towards the next reorder.  A scalar loss
        is differentiated with losses.unit_gradient (no fill launch; l1_loss's backward skips its scale launch)."""
        if loss.dim() == 0 and loss.dtype == torch.float32 and loss.is_cuda:
            from .losses import unit_gradient
            loss.backward(gradient=unit_gradient(loss))
        else:
            loss.backward()
        if self.optimizer is not None:
            if self._selective():
                if self.last_meta is None or self.last_meta.get("radii") is None:
                    raise RuntimeError("a selective GaussianAdam steps on the radii of Trainer.render(): render first")
                self.optimizer.step(visibility=self.last_meta["radii"])
            else:
                self.optimizer.step()
            self.optimizer.zero_grad(set_to_none=True)
        self.it += 1
        self._since = getattr(self, "_since", 0) + 1
        if self.strategy is not None:
            self.strategy.step(self)

    def in_original_order(self, x: torch.Tensor) -> torch.Tensor:
        """A per-Gaussian tensor in the trainer's current order -> the order the trainer was built (or last rebound) with."""
        out = torch.empty_like(x)
        out.index_copy_(0, self.original_index.to(x.device), x)
        return out
