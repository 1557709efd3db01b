"""GaussianAdam: torch.optim.Adam's update for the Gaussian parameters as ONE launch of libmgs.so's mgs_adam_step
(include/mgs_optim.h, csrc/optim.hip), with the three things a captured splatfacto step needs from its optimiser:

  * per-part learning rates inside one tensor: a group's `head_floats` / `rest_lr_scale` train the first floats of every
    row (features_dc of the [N, K, 3] SH tensor) at lr and the rest (features_rest) at lr * rest_lr_scale;
  * a learning-rate schedule that a replayed HIP graph follows: the step counter is a device tensor the launch itself
    advances, and lr_t = lr (lr_final / lr)^(min(t - 1, decay_steps) / decay_steps) is evaluated on the device
    (nerfstudio's ExponentialDecayScheduler without warm-up);
  * visibility-masked updates (gsplat's SelectiveAdam): `step(visibility=meta["radii"])` leaves the parameters and the
    moments of every Gaussian no camera saw untouched, and does not move their bytes.

There is no fallback: the update runs in the library or raises.
"""
from __future__ import annotations

from typing import Dict, Iterable, List, Optional, Tuple

import torch

from . import _lib
from ._lib import MgsError


class GaussianAdam(torch.optim.Optimizer):
    """Adam (amsgrad=False, weight_decay=0, maximize=False) over per-Gaussian fp32 CUDA tensors whose first dimension
    is the Gaussian count.

    params: tensors or ordinary param groups.  Per-group options: lr; lr_final and decay_steps (decay_steps 0 = constant
    lr); head_floats and rest_lr_scale (head_floats 0 = one rate for the whole row).  Global options: betas, eps,
    selective.  selective=True makes `step` demand a visibility argument.

    The moments are `state[p]["exp_avg"]` / `["exp_avg_sq"]`, shaped like p, so reorder_parameters / Trainer.reorder
    permute them with the parameters.  The update number is one device counter per optimiser (`step_state`, int32
    { steps taken, ticket }), advanced by every launch -- also for a parameter that had no gradient in some step.  At most
    eight parameters can have a gradient in one step (one launch updates them all)."""

    def __init__(self, params, lr: float = 1e-3, betas: Tuple[float, float] = (0.9, 0.999), eps: float = 1e-8, *,
                 lr_final: Optional[float] = None, decay_steps: int = 0, head_floats: int = 0,
                 rest_lr_scale: float = 1.0, selective: bool = False):
        if not (0.0 <= betas[0] < 1.0 and 0.0 <= betas[1] < 1.0):
            raise ValueError(f"betas {betas} not in [0, 1)")
        if eps < 0.0:
            raise ValueError(f"eps {eps} is negative")
        self.betas = (float(betas[0]), float(betas[1]))
        self.eps = float(eps)
        self.selective = bool(selective)
        self.step_state: Optional[torch.Tensor] = None
        super().__init__(params, dict(lr=lr, lr_final=lr_final, decay_steps=decay_steps, head_floats=head_floats,
                                      rest_lr_scale=rest_lr_scale))

    # ---- the counter -------------------------------------------------------------------------------------------------
    def _counter(self, device) -> torch.Tensor:
        if self.step_state is None:
            self.step_state = torch.zeros(2, dtype=torch.int32, device=device)
        return self.step_state

    def steps_taken(self) -> int:
        """The number of updates made so far (reads the device counter: synchronises)."""
        return 0 if self.step_state is None else int(self.step_state[0])

    def state_dict(self):
        sd = super().state_dict()
        sd["step_state"] = None if self.step_state is None else self.step_state.clone()
        return sd

    def load_state_dict(self, state_dict) -> None:
        state_dict = dict(state_dict)
        saved = state_dict.pop("step_state", None)
        super().load_state_dict(state_dict)
        if saved is None:
            if self.step_state is not None:
                self.step_state.zero_()
        elif self.step_state is None:
            device = next((p.device for g in self.param_groups for p in g["params"]), saved.device)
            self.step_state = saved.to(device=device, dtype=torch.int32).clone()
        else:
            self.step_state.copy_(saved)             # in place: a captured graph keeps its pointer

    # ---- the step ----------------------------------------------------------------------------------------------------
    @staticmethod
    def _visibility(vis: torch.Tensor, n: int):
        """-> (radii, radii_y, n_cams, cam_stride, mask, keep-alive) of mgs_adam_step."""
        _lib.require_device(vis)
        if vis.dtype in (torch.bool, torch.uint8):
            if vis.dim() != 1 or vis.shape[0] != n:
                raise MgsError(f"a visibility mask must be [N] = [{n}], got {tuple(vis.shape)}")
            vis = vis.contiguous()
            mask = vis.view(torch.uint8) if vis.dtype == torch.bool else vis
            return None, None, 0, 0, mask.data_ptr(), mask
        if vis.dtype != torch.int32:
            raise MgsError(f"visibility must be int32 radii ([C,N] or [C,N,2]) or a bool [N] mask, got {vis.dtype}")
        if vis.dim() == 1:
            vis = vis[None]
        if vis.dim() == 2 and vis.shape[1] == n:
            if vis.stride(1) != 1:
                vis = vis.contiguous()
            return vis.data_ptr(), None, vis.shape[0], (vis.stride(0) if vis.shape[0] > 1 else n), None, vis
        if vis.dim() == 3 and vis.shape[1] == n and vis.shape[2] == 2:
            if vis.stride(1) != 1 or (vis.shape[0] > 1 and vis.stride(0) < n):      # interleaved pairs: make them planar
                vis = vis.permute(0, 2, 1).contiguous().permute(0, 2, 1)
            stride = vis.stride(0) if vis.shape[0] > 1 else n
            return vis.data_ptr(), vis.data_ptr() + 4 * vis.stride(2), vis.shape[0], stride, None, vis
        raise MgsError(f"visibility radii must be [C,{n}] or [C,{n},2], got {tuple(vis.shape)}")

    @torch.no_grad()
    def step(self, visibility: Optional[torch.Tensor] = None, closure=None):
        """One update of every parameter that has a gradient (a parameter whose .grad is None is left out of the launch).
        visibility: meta["radii"] of the render that produced the gradients ([C,N], or [C,N,2] under the opacity-aware
        radius rule), or a bool [N] mask; None updates every Gaussian."""
        loss = None
        if closure is not None:
            with torch.enable_grad():
                loss = closure()
        if self.selective and visibility is None:
            raise MgsError("GaussianAdam(selective=True).step() needs visibility= (meta['radii'] or a bool [N] mask)")
        entries, keep = [], []
        for group in self.param_groups:
            for p in group["params"]:
                if p.grad is None:
                    continue
                _lib.require_device(p, p.grad)
                if p.grad.is_sparse:
                    raise MgsError("GaussianAdam does not take sparse gradients")
                if p.dtype != torch.float32 or p.grad.dtype != torch.float32 or p.dim() < 1 or not p.is_contiguous():
                    raise MgsError(f"GaussianAdam updates contiguous fp32 tensors with a leading Gaussian dimension, got "
                                   f"{p.dtype} {tuple(p.shape)}")
                grad = p.grad if p.grad.is_contiguous() else p.grad.contiguous()
                st = self.state[p]
                if "exp_avg" not in st:
                    st["exp_avg"] = torch.zeros_like(p, memory_format=torch.contiguous_format)
                    st["exp_avg_sq"] = torch.zeros_like(p, memory_format=torch.contiguous_format)
                n = p.shape[0]
                lr = float(group["lr"])
                entries.append(_lib.AdamGroup(
                    p.data_ptr(), grad.data_ptr(), st["exp_avg"].data_ptr(), st["exp_avg_sq"].data_ptr(), n,
                    p.numel() // n if n else 1, int(group["head_floats"]), lr,
                    lr if group["lr_final"] is None else float(group["lr_final"]), int(group["decay_steps"]),
                    float(group["rest_lr_scale"])))
                keep.append(grad)
        if not entries:
            return loss
        if len(entries) > _lib.ADAM_MAX_GROUPS:
            raise MgsError(f"{len(entries)} parameters have a gradient: one step updates at most {_lib.ADAM_MAX_GROUPS}")
        radii = radii_y = mask = None
        n_cams = cam_stride = 0
        if visibility is not None:
            rows = {int(e.n) for e in entries}
            if len(rows) != 1:
                raise MgsError(f"a visibility mask needs one Gaussian count, the parameters have {sorted(rows)} rows")
            radii, radii_y, n_cams, cam_stride, mask, alive = self._visibility(visibility, rows.pop())
            keep.append(alive)
        device = next(p.device for g in self.param_groups for p in g["params"] if p.grad is not None)
        table = (_lib.AdamGroup * len(entries))(*entries)
        _lib.check(_lib.lib().mgs_adam_step(len(entries), table, self.betas[0], self.betas[1], self.eps,
                                            self._counter(device).data_ptr(), radii, radii_y, n_cams, cam_stride, mask,
                                            _lib.stream_handle()), "mgs_adam_step")
        return loss


def splatfacto_groups(params: Dict[str, torch.Tensor], means_lr: float = 1.6e-4, means_lr_final: float = 1.6e-6,
                      decay_steps: int = 30000, quats_lr: float = 1e-3, scales_lr: float = 5e-3,
                      opacities_lr: float = 5e-2, features_dc_lr: float = 2.5e-3,
                      features_rest_lr: Optional[float] = None) -> List[dict]:
    """The five param groups of Trainer.KEYS with splatfacto's default rates: means 1.6e-4 decaying exponentially to
    1.6e-6 over 30 000 steps, quats 1e-3, scales 5e-3, opacities 5e-2, and the SH tensor params["colors"] [N, K, 3] split
    after its first 3 floats into features_dc at 2.5e-3 and features_rest at features_dc_lr / 20.  (Splatfacto's Adam
    eps is 1e-15: pass eps=1e-15 to GaussianAdam for its exact update.)"""
    if features_rest_lr is None:
        features_rest_lr = features_dc_lr / 20.0
    colors = params["colors"]
    split = colors.dim() == 3 and colors.shape[1] > 1
    return [
        dict(name="means", params=[params["means"]], lr=means_lr, lr_final=means_lr_final, decay_steps=int(decay_steps)),
        dict(name="quats", params=[params["quats"]], lr=quats_lr),
        dict(name="scales", params=[params["scales"]], lr=scales_lr),
        dict(name="opacities", params=[params["opacities"]], lr=opacities_lr),
        dict(name="colors", params=[colors], lr=features_dc_lr, head_floats=3 if split else 0,
             rest_lr_scale=features_rest_lr / features_dc_lr if split else 1.0),
    ]
