"""MCMCStrategy: splatfacto's `strategy="mcmc"` (gsplat's MCMCStrategy, "3D Gaussian Splatting as Markov Chain Monte
Carlo") on libmgs.so's refinement entry points (include/mgs_refine.h, csrc/refine.hip).

The strategy fits a trainer whose step is one HIP graph and whose optimiser counts on the device:

  * dead Gaussians (opacity <= min_opacity) are RELOCATED onto live ones drawn in proportion to their opacity, so a
    refinement does not change the count by itself;
  * growth is n <- min(cap_max, floor(grow_factor n)): host arithmetic (`n_after`), never a device read-back.  The
    parameters and the optimiser's moments live in storage of cap_max rows from `initialize` on; the leaves are views
    [:n] of it, and growing takes new views of the same storage;
  * the per-step part, position noise scaled by the covariance and by the means' current learning rate, has a fixed
    shape: one launch that reads GaussianAdam's device counter, capturable with the rest of the step.

The three operations are also exposed as functions (mcmc_weights, mcmc_relocate, mcmc_noise).  There is no fallback: they
run in the library or raise.  No call here synchronises."""
from __future__ import annotations

from typing import Dict, Optional, Sequence, Tuple

import torch

from . import _lib
from ._lib import MgsError

KEYS = ("means", "quats", "scales", "opacities", "colors")          # Trainer.KEYS


def _f32(t: torch.Tensor, what: str) -> torch.Tensor:
    _lib.require_device(t)
    if t.dtype != torch.float32 or not t.is_contiguous():
        raise MgsError(f"{what} must be a contiguous fp32 tensor, got {t.dtype} {tuple(t.shape)}")
    return t


class _Scratch:
    """The caller-owned outputs of the weights pass for up to `rows` Gaussians."""

    def __init__(self, rows: int, device):
        self.rows = rows
        self.w = torch.empty(max(rows, 1), dtype=torch.float32, device=device)
        self.dead = torch.empty(max(rows, 1), dtype=torch.int32, device=device)
        self.sources = torch.empty(max(rows, 1), dtype=torch.int32, device=device)
        self.stats = torch.zeros(2, dtype=torch.float64, device=device)      # mgs_mcmc_stats: { double, int32, int32 }

    def counts(self) -> Tuple[float, int, int]:
        """(T, n_dead, n_live) -- reads the device: for tests and logs, not for the training loop."""
        total = float(self.stats[0])
        n_dead, n_live = self.stats[1:].view(torch.int32).tolist()
        return total, n_dead, n_live


@torch.no_grad()
def mcmc_weights(opacities: torch.Tensor, min_opacity: float, mode: int = _lib.MCMC_RELOCATE,
                 scratch: Optional[_Scratch] = None) -> _Scratch:
    """Operation (a) of include/mgs_refine.h on opacity logits [n]: scratch.w, scratch.dead, scratch.stats."""
    _f32(opacities, "opacities")
    n = opacities.shape[0]
    s = scratch if scratch is not None and scratch.rows >= n else _Scratch(n, opacities.device)
    _lib.sized_call(_lib.lib().mgs_mcmc_weights,
                    (n, opacities.data_ptr(), float(min_opacity), int(mode), s.w.data_ptr(), s.dead.data_ptr(),
                     s.stats.data_ptr()), opacities.device, cached=True)
    return s


@torch.no_grad()
def mcmc_relocate(mode: int, n: int, n_new: int, storage: Dict[str, torch.Tensor],
                  moments: Optional[Dict[str, Tuple[torch.Tensor, torch.Tensor]]], min_opacity: float, u: torch.Tensor,
                  scratch: Optional[_Scratch] = None, keys: Sequence[str] = KEYS) -> _Scratch:
    """Operations (a) + (b) on the first n rows of storage[k] ([capacity, ...] each, raw form): relocate the dead rows
    (mode MCMC_RELOCATE) or fill the rows [n, n + n_new) (MCMC_ADD) from sources drawn with the uniforms u.
    moments[k] = (exp_avg, exp_avg_sq) shaped like storage[k]; None (or a missing key): no optimiser state.
    Returns the scratch: w, dead, stats and the source of each target."""
    capacity = storage["opacities"].shape[0]
    entries = []
    for k in keys:
        t = _f32(storage[k], k)
        if t.shape[0] != capacity:
            raise MgsError(f"storage[{k!r}] has {t.shape[0]} rows, storage['opacities'] {capacity}")
        m = v = None
        if moments is not None and moments.get(k) is not None:
            m, v = (_f32(x, f"a moment of {k}") for x in moments[k])
            if m.shape != t.shape or v.shape != t.shape:
                raise MgsError(f"the moments of {k} are not shaped like it")
        entries.append(_lib.RefineGroup(t.data_ptr(), _lib.ptr(m), _lib.ptr(v), t.numel() // capacity if capacity else 1))
    if len(entries) > _lib.REFINE_MAX_GROUPS:
        raise MgsError(f"{len(entries)} parameter groups: one refinement moves at most {_lib.REFINE_MAX_GROUPS}")
    targets = n if mode == _lib.MCMC_RELOCATE else n_new
    _f32(u, "u")
    if u.numel() < targets:
        raise MgsError(f"{targets} targets need as many uniforms, got {u.numel()}")
    device = storage["opacities"].device
    s = scratch if scratch is not None and scratch.rows >= max(n, targets) else _Scratch(max(n, targets), device)
    table = (_lib.RefineGroup * len(entries))(*entries)
    _lib.sized_call(_lib.lib().mgs_mcmc_relocate,
                    (int(mode), n, n_new, capacity, storage["opacities"].data_ptr(), storage["scales"].data_ptr(),
                     len(entries), table, float(min_opacity), u.data_ptr(), s.w.data_ptr(), s.dead.data_ptr(),
                     s.stats.data_ptr(), s.sources.data_ptr()), device, cached=True)
    return s


@torch.no_grad()
def mcmc_noise(means: torch.Tensor, quats: torch.Tensor, scales: torch.Tensor, opacities: torch.Tensor, z: torch.Tensor,
               noise_lr: float, lr: float, lr_final: Optional[float] = None, decay_steps: int = 0,
               step_state: Optional[torch.Tensor] = None) -> None:
    """Operation (c): means += Sigma (z gate lambda) in place, lambda = noise_lr * (the rate of the next update, from
    step_state = GaussianAdam.step_state; None: lr itself)."""
    n = means.shape[0]
    for t, shape, what in ((means, (n, 3), "means"), (quats, (n, 4), "quats"), (scales, (n, 3), "scales"),
                           (opacities, (n,), "opacities"), (z, (n, 3), "z")):
        if tuple(_f32(t, what).shape) != shape:
            raise MgsError(f"{what} must be {shape}, got {tuple(t.shape)}")
    if step_state is not None:
        _lib.require_device(step_state)
        if step_state.dtype != torch.int32:
            raise MgsError(f"step_state must be int32, got {step_state.dtype}")
    _lib.check(_lib.lib().mgs_mcmc_noise(n, means.data_ptr(), quats.data_ptr(), scales.data_ptr(), opacities.data_ptr(),
                                         z.data_ptr(), float(noise_lr), float(lr),
                                         float(lr if lr_final is None else lr_final), int(decay_steps),
                                         _lib.ptr(step_state), _lib.stream_handle()), "mgs_mcmc_noise")


class MCMCStrategy:
    """gsplat's MCMCStrategy for a `Trainer` with raw parameters (log-scales, opacity logits):

        strategy = MCMCStrategy(cap_max=1_000_000)
        params = strategy.initialize(params, optimizer)            # storage of cap_max rows, leaves are views [:n]
        tr = Trainer(params, optimizer, W, H, raw_params=True, strategy=strategy, ...)
        for it in range(iters):
            colors, alphas, meta = tr.render(viewmats, Ks)
            tr.step(loss(colors))                                  # ... optimiser step, then strategy.step(tr)

    Step number s (0-based) is a refinement step when refine_start_iter < s < refine_stop_iter and s % refine_every == 0
    (gsplat's rule): the dead Gaussians are relocated, then min(cap_max, floor(grow_factor n)) - n new ones are added,
    both by sampling live Gaussians in proportion to their opacity; the trainer is rebound to views [:n'] of the same
    storage.  Every step adds the noise.  `n_after(k)` is the count after k steps, computed on the host.

    Under graph capture `step` records the noise only: a refinement runs eagerly, between replays."""

    def __init__(self, cap_max: int, refine_every: int = 100, refine_start_iter: int = 500, refine_stop_iter: int = 25000,
                 min_opacity: float = 0.005, noise_lr: float = 5e5, grow_factor: float = 1.05):
        if cap_max < 1 or refine_every < 1:
            raise ValueError(f"cap_max {cap_max} and refine_every {refine_every} must be positive")
        if not 0.0 < min_opacity < 1.0:
            raise ValueError(f"min_opacity {min_opacity} not in (0, 1)")
        if grow_factor < 1.0 or noise_lr < 0.0:
            raise ValueError(f"grow_factor {grow_factor} < 1 or noise_lr {noise_lr} < 0")
        self.cap_max, self.refine_every = int(cap_max), int(refine_every)
        self.refine_start_iter, self.refine_stop_iter = int(refine_start_iter), int(refine_stop_iter)
        self.min_opacity, self.noise_lr, self.grow_factor = float(min_opacity), float(noise_lr), float(grow_factor)
        self.n0: Optional[int] = None
        self.n: Optional[int] = None
        self.storage: Dict[str, torch.Tensor] = {}
        self.moments: Dict[str, Tuple[torch.Tensor, torch.Tensor]] = {}
        self.refinements = 0
        self.last_z: Optional[torch.Tensor] = None       # the normals of the last inject_noise (a replay's, under a graph)
        self._scratch: Optional[_Scratch] = None

    # ---- host arithmetic -----------------------------------------------------------------------------------------
    def due(self, step: int) -> bool:
        """Is 0-based step number `step` a refinement step?"""
        return self.refine_start_iter < step < self.refine_stop_iter and step % self.refine_every == 0

    def grown(self, n: int) -> int:
        """The count a refinement grows n to: min(cap_max, floor(grow_factor n)), never below n."""
        return max(n, min(self.cap_max, int(self.grow_factor * n)))

    def n_after(self, steps: int, n0: Optional[int] = None) -> int:
        """The Gaussian count after `steps` steps from n0 (default: the count `initialize` saw)."""
        n = self.n0 if n0 is None else int(n0)
        if n is None:
            raise MgsError("n_after needs n0 before initialize()")
        for s in range(0, min(int(steps), self.refine_stop_iter), self.refine_every):
            if n >= self.cap_max:
                break
            if s > self.refine_start_iter:
                n = self.grown(n)
        return n

    # ---- storage -------------------------------------------------------------------------------------------------
    def initialize(self, params: Dict[str, torch.Tensor], optimizer: Optional[torch.optim.Optimizer],
                   raw_params: bool = True) -> Dict[str, torch.Tensor]:
        """Move the five Trainer.KEYS tensors and the optimiser's moments into storage of cap_max rows; returns the
        params dict with leaf views [:n] in their place (other keys as they were), the optimiser re-keyed to them."""
        if not raw_params:
            raise MgsError("MCMCStrategy works on raw parameters (log-scales, opacity logits: Trainer(raw_params=True)); "
                           "the activated form is refused")
        missing = [k for k in KEYS if k not in params]
        if missing:
            raise KeyError(f"params lacks {missing} (needs {KEYS})")
        n = params["means"].shape[0]
        for k in KEYS:
            _f32(params[k].detach(), k)
            if params[k].shape[0] != n:
                raise MgsError(f"params[{k!r}] has {params[k].shape[0]} rows, params['means'] {n}")
        if n > self.cap_max:
            raise MgsError(f"{n} Gaussians exceed cap_max {self.cap_max}")
        self.n0 = self.n = n
        with torch.no_grad():
            for k in KEYS:
                p = params[k]
                store = torch.zeros((self.cap_max, *p.shape[1:]), dtype=torch.float32, device=p.device)
                store[:n].copy_(p.detach())
                self.storage[k] = store
                m, v = torch.zeros_like(store), torch.zeros_like(store)
                st = optimizer.state.get(p, {}) if optimizer is not None else {}
                if "exp_avg" in st:
                    m[:n].copy_(st["exp_avg"])
                    v[:n].copy_(st["exp_avg_sq"])
                self.moments[k] = (m, v)
        self._scratch = _Scratch(self.cap_max, params["means"].device)
        return self._views(params, optimizer, n)

    def _views(self, params, optimizer, n: int) -> Dict[str, torch.Tensor]:
        """Leaf views [:n] of the storage in a copy of `params`; the optimiser's groups and state follow them."""
        out = dict(params)
        for k in KEYS:
            old = params[k]
            new = self.storage[k][:n].detach().requires_grad_(True)
            out[k] = new
            if optimizer is None:
                continue
            for group in optimizer.param_groups:
                group["params"] = [new if q is old else q for q in group["params"]]
            st = optimizer.state.pop(old, None)
            st = dict(st) if st else {}
            st["exp_avg"], st["exp_avg_sq"] = self.moments[k][0][:n], self.moments[k][1][:n]
            optimizer.state[new] = st
        return out

    # ---- the per-step part ---------------------------------------------------------------------------------------
    def _means_rate(self, trainer):
        """(lr, lr_final, decay_steps, step_state) of the group that trains the means."""
        opt, means = trainer.optimizer, trainer.params["means"]
        if opt is None:
            raise MgsError("MCMCStrategy scales its noise by the means' learning rate: the trainer has no optimiser")
        for group in opt.param_groups:
            if any(q is means for q in group["params"]):
                lr = float(group["lr"])
                state = getattr(opt, "step_state", None)
                if state is None and hasattr(opt, "_counter"):
                    state = opt._counter(means.device)
                return lr, group.get("lr_final"), int(group.get("decay_steps") or 0), state
        raise MgsError("the optimiser has no group with params['means']")

    def inject_noise(self, trainer) -> None:
        """One launch: means += Sigma (z gate noise_lr lr_next), z ~ N(0, 1) from torch's generator (capturable)."""
        p = trainer.params
        lr, lr_final, decay_steps, state = self._means_rate(trainer)
        z = self.last_z = torch.randn(p["means"].shape, dtype=torch.float32, device=p["means"].device)
        mcmc_noise(p["means"].detach(), p["quats"].detach(), p["scales"].detach(), p["opacities"].detach(), z,
                   self.noise_lr, lr, lr_final, decay_steps, state)

    def refine(self, trainer) -> int:
        """Relocate the dead, grow to `grown(n)`, rebind the trainer to views [:n'] of the same storage.  Returns n'."""
        if self.n is None:
            raise MgsError("MCMCStrategy.initialize(params, optimizer) has not been called")
        n, device = self.n, self.storage["means"].device
        if trainer.params["means"].data_ptr() != self.storage["means"].data_ptr() or trainer.params["means"].shape[0] != n:
            raise MgsError("the trainer's parameters are not the views MCMCStrategy.initialize handed back")
        mcmc_relocate(_lib.MCMC_RELOCATE, n, 0, self.storage, self.moments, self.min_opacity,
                      torch.rand(n, dtype=torch.float32, device=device), self._scratch)
        n_to = self.grown(n)
        if n_to > n:
            mcmc_relocate(_lib.MCMC_ADD, n, n_to - n, self.storage, self.moments, self.min_opacity,
                          torch.rand(n_to - n, dtype=torch.float32, device=device), self._scratch)
        self.n = n_to
        self.refinements += 1
        trainer.rebind(self._views(trainer.params, trainer.optimizer, n_to), trainer.optimizer, trainer.extra_state
                       if n_to == n else ())
        return n_to

    def step(self, trainer) -> None:
        """After the optimiser step of trainer step number trainer.it - 1: refine when due (never while capturing),
        then the noise."""
        if not trainer.raw_params:
            raise MgsError("MCMCStrategy works on raw parameters: build the Trainer with raw_params=True")
        _lib.require_device(trainer.params["means"])
        if self.due(trainer.it - 1) and not torch.cuda.is_current_stream_capturing():
            self.refine(trainer)
        self.inject_noise(trainer)
