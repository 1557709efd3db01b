"""Register one point set onto another (include/mgs_register.h, csrc/register.hip): ICP for world-frame alignment.

    reg = register_points(tensors["means"], target_points, max_distance=0.05, with_scale=True, init=(R0, t0, s0))
    aligned = reg.apply(tensors)                           # transform_gaussians with the estimated similarity
    R, t, s = reg.pose()

The source is typically the Gaussian means (or the points of a labelled part), the target a depth camera's cloud, samples
of a scanned mesh (`Mesh.sample_points`) or the vertices of a TSDFVolume mesh.  Each iteration matches every transformed
source point to its nearest target within `max_distance` (a uniform grid over the target, built once per call on the
GPU; the answer is the brute-force one), then solves the similarity of the matched pairs in closed form (fp64 moments about
a pivot, fixed summation order, Kabsch / Umeyama on the device).  Nothing is read back until a field of the returned
`Registration` is used, and the same inputs give the same bytes in every run.  ICP is local: `init` must bring the sets
within `max_distance` of each other where they overlap.
"""
from __future__ import annotations

from typing import Optional

import numpy as np
import torch
from torch import Tensor

from . import _lib
from ._lib import aligned_workspace, check, check_tensor, ptr, require_device, stream_handle
from .ops import _f32c

RESULT_DOUBLES = 32      # include/mgs_register.h: R 0..8 | t 9..11 | s | rmse | fitness | n_inliers | iterations | converged | flags | h | dims
INIT_DOUBLES = 13        # R | t | s
MAX_ITERATIONS = 256
FLAG_UNDETERMINED, FLAG_NONFINITE = 1, 2


def workspace_bytes(n_s: int, n_t: int, iterations: int) -> int:
    """mgs_register_workspace_bytes: what a call on n_s source and n_t target points needs."""
    return int(_lib.lib().mgs_register_workspace_bytes(int(n_s), int(n_t), int(iterations)))


def register_workspace(n_s: int, n_t: int, iterations: int, device) -> Tensor:
    """A workspace for register_icp_raw(workspace=...): the bytes the library asks for plus room to align to 256."""
    return torch.empty(workspace_bytes(n_s, n_t, iterations) + 256, dtype=torch.uint8, device=device)


def pack_init(init) -> np.ndarray:
    """`init` as the 13 doubles R | t | s: (R, t), (R, t, s) or a 4x4 matrix whose upper-left block is s R."""
    if isinstance(init, (tuple, list)) and len(init) in (2, 3):
        R, t = np.asarray(init[0], np.float64).reshape(3, 3), np.asarray(init[1], np.float64).reshape(3)
        s = float(init[2]) if len(init) == 3 else 1.0
    else:
        M = np.asarray(init, np.float64)
        if M.shape != (4, 4):
            raise ValueError("init must be (R, t), (R, t, s) or a 4x4 matrix")
        s = float(np.cbrt(np.linalg.det(M[:3, :3])))
        if not s > 0:
            raise ValueError("init: the 4x4 matrix is not a similarity (its determinant is not positive)")
        R, t = M[:3, :3] / s, M[:3, 3].copy()
    if not (np.isfinite(R).all() and np.isfinite(t).all() and np.isfinite(s) and s > 0):
        raise ValueError("init must be finite with a positive scale")
    if abs(np.linalg.det(R) - 1.0) > 1e-4 or np.abs(R @ R.T - np.eye(3)).max() > 1e-4:
        raise ValueError("init: not a proper rotation (pass the scale separately, or a 4x4 similarity)")
    return np.concatenate([R.reshape(9), t, [s]])


def _points(x: Tensor, what: str) -> Tensor:
    if x.dim() != 2 or x.shape[1] != 3:
        raise ValueError(f"{what} must be [n,3], got {tuple(x.shape)}")
    if x.shape[0] == 0:
        raise ValueError(f"{what} is empty")
    return _f32c(x.detach())


def register_icp_raw(source: Tensor, target: Tensor, max_distance: float, iterations: int = 30, with_scale: bool = False,
                     tol: float = 1e-6, init: Optional[Tensor] = None, correspondence: Optional[Tensor] = None,
                     distance2: Optional[Tensor] = None, history: Optional[Tensor] = None, result: Optional[Tensor] = None,
                     workspace: Optional[Tensor] = None) -> Tensor:
    """mgs_register_icp on torch's current stream: no synchronisation, capturable.  source / target float32 [n,3] on the
    GPU; init (optional) float64 [13] on the GPU; correspondence int32 [n_s], distance2 float32 [n_s] and history float64
    [iterations,4] (all optional) receive what their names say; result (optional) float64 [32] receives the record and is
    returned.  workspace: a uint8 tensor from register_workspace() (a caller that captures a graph keeps its own);
    otherwise one is allocated for the call."""
    require_device(source, target, init, correspondence, distance2, history, result, workspace)
    a, b = _points(source, "source"), _points(target, "target")
    n_s, n_t, dev = a.shape[0], b.shape[0], a.device
    iterations = int(iterations)
    if init is not None:
        check_tensor("init", init, torch.float64, (INIT_DOUBLES,), dev)
    if correspondence is not None:
        check_tensor("correspondence", correspondence, torch.int32, (n_s,), dev)
    if distance2 is not None:
        check_tensor("distance2", distance2, torch.float32, (n_s,), dev)
    if history is not None:
        check_tensor("history", history, torch.float64, (iterations, 4), dev)
    if result is None:
        result = torch.empty(RESULT_DOUBLES, dtype=torch.float64, device=dev)
    else:
        check_tensor("result", result, torch.float64, (RESULT_DOUBLES,), dev)
    L = _lib.lib()
    workspace, pad = aligned_workspace(workspace, int(L.mgs_register_workspace_bytes(n_s, n_t, iterations)), dev)
    check(L.mgs_register_icp(n_s, ptr(a), n_t, ptr(b), float(max_distance), iterations, int(bool(with_scale)), float(tol),
                             ptr(init), workspace.data_ptr() + pad, max(0, workspace.numel() - pad), ptr(correspondence),
                             ptr(distance2), ptr(history), ptr(result), stream_handle()), "mgs_register_icp")
    return result


class Registration:
    """An estimated similarity x -> s R x + t.  `result` is the 32-double record of mgs_register_icp and `history_rows` the
    [iterations,4] rows [n_inliers, rmse, scale, 0], both still on the device; the first read of .rotation, .translation,
    .scale, .rmse, .fitness, .n_inliers, .iterations, .converged, .flags or .history copies them to the host once (which
    waits for the call).  correspondence (int32 [n_s], -1: no target within max_distance) and distance2 (float32 [n_s], +inf
    there) are device tensors where the call was asked for them."""

    def __init__(self, result, history_rows=None, correspondence: Optional[Tensor] = None,
                 distance2: Optional[Tensor] = None):
        self.result, self.history_rows = result, history_rows
        self.correspondence, self.distance2 = correspondence, distance2
        self._record = self._history = None

    def _host(self) -> np.ndarray:
        if self._record is None:
            r = self.result
            r = r.detach().cpu().numpy() if torch.is_tensor(r) else np.asarray(r)
            self._record = np.array(r, dtype=np.float64).reshape(RESULT_DOUBLES)
        return self._record

    rotation = property(lambda self: self._host()[0:9].reshape(3, 3).copy())
    translation = property(lambda self: self._host()[9:12].copy())
    scale = property(lambda self: float(self._host()[12]))
    rmse = property(lambda self: float(self._host()[13]))
    fitness = property(lambda self: float(self._host()[14]))
    n_inliers = property(lambda self: int(self._host()[15]))
    iterations = property(lambda self: int(self._host()[16]))
    converged = property(lambda self: bool(self._host()[17]))
    flags = property(lambda self: int(self._host()[18]))
    cell_edge = property(lambda self: float(self._host()[19]))
    grid_dims = property(lambda self: tuple(int(d) for d in self._host()[20:23]))

    @property
    def history(self) -> np.ndarray:
        """float64 [iterations executed, 4]: n_inliers, rmse and scale each iteration was matched under."""
        if self._history is None:
            h = self.history_rows
            if h is None:
                h = np.zeros((0, 4))
            h = h.detach().cpu().numpy() if torch.is_tensor(h) else np.asarray(h)
            self._history = np.array(h, dtype=np.float64).reshape(-1, 4)[:self.iterations]
        return self._history

    def matrix(self) -> np.ndarray:
        """The 4x4 matrix [[s R, t], [0, 1]], float64."""
        M = np.eye(4)
        M[:3, :3], M[:3, 3] = self.scale * self.rotation, self.translation
        return M

    def pose(self):
        """(R [3,3], t [3], s): what transform_gaussians(rotations=[R], translations=[t], scales=[s]) takes."""
        return self.rotation, self.translation, self.scale

    def apply(self, tensors, **kw):
        """transform_gaussians(tensors, [R], [t], [s], **kw): the scene in the target's frame."""
        from .transform import transform_gaussians
        R, t, s = self.pose()
        return transform_gaussians(tensors, [R], [t], [s], **kw)

    def __repr__(self):
        return (f"Registration(scale={self.scale:.6g}, rmse={self.rmse:.4g}, fitness={self.fitness:.4f}, "
                f"n_inliers={self.n_inliers}, iterations={self.iterations}, converged={self.converged}, flags={self.flags})")


@torch.no_grad()
def register_points(source: Tensor, target: Tensor, max_distance: float, *, init=None, with_scale: bool = False,
                    iterations: int = 30, tol: float = 1e-6, return_correspondence: bool = False) -> Registration:
    """ICP of source [n_s,3] onto target [n_t,3], both on the GPU: the similarity (a rigid motion unless with_scale) that
    brings the source onto the target, starting from `init` ((R, t), (R, t, s) or a 4x4 matrix; the identity if absent).  A
    source point counts only while a target lies within max_distance of it; a point with a non-finite coordinate takes no
    part.  The loop ends after `iterations` rounds, or once the rmse changes by at most tol of itself, or when the matched
    pairs no longer determine a rotation (fewer than 3, or collinear: flags bit 0).  iterations=0 is a radius-bounded
    nearest-neighbour query under `init`.  No synchronisation: the returned Registration reads the record on first use.
    return_correspondence: also keep, per source point, the index of its target (-1: none) and the squared distance."""
    require_device(source, target)
    if not (np.isfinite(max_distance) and max_distance > 0):
        raise ValueError(f"max_distance {max_distance} is not a finite positive number")
    if not (np.isfinite(tol) and tol >= 0):
        raise ValueError(f"tol {tol} is not a finite non-negative number")
    iterations = int(iterations)
    if not 0 <= iterations <= MAX_ITERATIONS:
        raise ValueError(f"iterations {iterations} outside 0..{MAX_ITERATIONS}")
    dev, n_s = source.device, source.shape[0]
    init_d = None if init is None else torch.from_numpy(pack_init(init)).to(dev)
    c = d2 = None
    if return_correspondence:
        c = torch.empty(n_s, dtype=torch.int32, device=dev)
        d2 = torch.empty(n_s, dtype=torch.float32, device=dev)
    history = torch.zeros((iterations, 4), dtype=torch.float64, device=dev)
    result = register_icp_raw(source, target, max_distance, iterations, with_scale, tol, init_d, c, d2, history)
    return Registration(result, history, c, d2)


__all__ = ["Registration", "register_points", "register_icp_raw", "register_workspace", "workspace_bytes", "pack_init",
           "RESULT_DOUBLES", "INIT_DOUBLES", "MAX_ITERATIONS"]
