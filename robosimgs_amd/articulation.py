"""The joint a labelled part moves about (include/mgs_hinge.h, csrc/hinge.hip): contact set and hinge axis of two point sets.

    ids = lift_labels(...).class_ids                       # or any int32 [N] of part labels
    hinge = fit_hinge(tensors["means"], ids, part=LID, base=BODY)
    R, t = hinge.pose(0.6)                                 # what FrameRenderer.submit(rotations=[R], translations=[t]) takes

The two sets' nearest-neighbour distances are found by brute force on the GPU (fp32 difference form, bit-identical under
any tiling), the points within `threshold` of the closest approach form the contact set, the hinge position is the mean
of the two sets' contact centroids and its axis the principal direction of all contact points (fp64 moments about a
pivot, fixed summation order, a Jacobi eigen solve on the device).  Nothing is read back until a field of the returned
`Hinge` is used.
"""
from __future__ import annotations

from typing import Optional

import numpy as np
import torch
from torch import Tensor

from . import _lib
from ._lib import aligned_workspace, check, check_tensor, ptr, require_device, sized_call, stream_handle
from .ops import _f32c

JOINT_DOUBLES = 16       # include/mgs_hinge.h: position 0..2, axis 3..5, confidence, min_distance, counts, eigenvalues, flags
FLAG_FALLBACK_AXIS, FLAG_NONFINITE = 1, 2


def workspace_bytes(n_a: int, n_b: int) -> int:
    """mgs_hinge_workspace_bytes: what a fit of n_a against n_b points needs."""
    return int(_lib.lib().mgs_hinge_workspace_bytes(int(n_a), int(n_b)))


def hinge_workspace(n_a: int, n_b: int, device) -> Tensor:
    """A workspace for hinge_fit_raw(workspace=...): the bytes the library asks for plus room to align to 256."""
    return torch.empty(workspace_bytes(n_a, n_b) + 256, dtype=torch.uint8, device=device)


def _sized_entry(L):
    """mgs_hinge_fit in the shape _lib.sized_call drives -- (..., workspace, byref(bytes), stream, contact_a, contact_b,
    joint) -- with mgs_hinge_workspace_bytes as its size query."""
    def mgs_hinge_fit(n_a, pts_a, n_b, pts_b, threshold, workspace, nbytes, stream, contact_a, contact_b, joint):
        if workspace is None:
            nbytes._obj.value = L.mgs_hinge_workspace_bytes(n_a, n_b)
            return 0
        return L.mgs_hinge_fit(n_a, pts_a, n_b, pts_b, threshold, workspace, nbytes._obj.value, contact_a, contact_b, joint,
                               stream)
    return mgs_hinge_fit


def _points(x: Tensor, what: str) -> Tensor:
    if x.dim() != 2 or x.shape[1] != 3:
        raise ValueError(f"{what} must be [n,3], got {tuple(x.shape)}")
    if x.shape[0] == 0:
        raise ValueError(f"{what} is empty")
    return _f32c(x.detach())


def hinge_fit_raw(points_a: Tensor, points_b: Tensor, threshold: float = 0.01, contact_a: Optional[Tensor] = None,
                  contact_b: Optional[Tensor] = None, joint: Optional[Tensor] = None,
                  workspace: Optional[Tensor] = None) -> Tensor:
    """mgs_hinge_fit on torch's current stream: no synchronisation, capturable.  points_* float32 [n,3] on the GPU (A is
    the moving part); contact_* (optional) uint8 [n] receive the contact masks; joint (optional) float64 [16] receives the
    record and is returned.  workspace: a uint8 tensor from hinge_workspace() (a caller that captures a graph keeps its
    own); otherwise the stream's cached scratch is used."""
    require_device(points_a, points_b, contact_a, contact_b, joint, workspace)
    a, b = _points(points_a, "points_a"), _points(points_b, "points_b")
    n_a, n_b, dev = a.shape[0], b.shape[0], a.device
    for c, n, what in ((contact_a, n_a, "contact_a"), (contact_b, n_b, "contact_b")):
        if c is not None:
            check_tensor(what, c, torch.uint8, (n,))
    if joint is None:
        joint = torch.empty(JOINT_DOUBLES, dtype=torch.float64, device=dev)
    else:
        check_tensor("joint", joint, torch.float64, (JOINT_DOUBLES,))
    L = _lib.lib()
    args = [n_a, ptr(a), n_b, ptr(b), float(threshold)]
    if workspace is None:
        sized_call(_sized_entry(L), args, dev, cached=True, trailing=(ptr(contact_a), ptr(contact_b), ptr(joint)))
    else:
        workspace, pad = aligned_workspace(workspace, 0, dev)
        check(L.mgs_hinge_fit(*args, workspace.data_ptr() + pad, max(0, workspace.numel() - pad), ptr(contact_a),
                              ptr(contact_b), ptr(joint), stream_handle()), "mgs_hinge_fit")
    return joint


class Hinge:
    """A fitted revolute joint.  `joint` is the 16-double record of mgs_hinge_fit, still on the device; the first read of
    .position, .axis, .axis_confidence, .min_distance, .n_contact, .eigenvalues, .fallback or .nonfinite copies it to the
    host once (one device-to-host copy, which waits for the fit).  contact_a / contact_b: bool device tensors where the
    fit was asked for them."""

    def __init__(self, joint, contact_a: Optional[Tensor] = None, contact_b: Optional[Tensor] = None,
                 threshold: float = 0.01):
        self.joint, self.contact_a, self.contact_b, self.threshold = joint, contact_a, contact_b, float(threshold)
        self._record = None
        self._torch_consts = {}

    def _host(self) -> np.ndarray:
        if self._record is None:
            j = self.joint
            j = j.detach().cpu().numpy() if torch.is_tensor(j) else np.asarray(j)
            self._record = np.array(j, dtype=np.float64).reshape(JOINT_DOUBLES)
        return self._record

    position = property(lambda self: self._host()[0:3].copy())
    axis = property(lambda self: self._host()[3:6].copy())
    axis_confidence = property(lambda self: float(self._host()[6]))
    min_distance = property(lambda self: float(self._host()[7]))
    n_contact = property(lambda self: (int(self._host()[8]), int(self._host()[9])))
    eigenvalues = property(lambda self: self._host()[10:13].copy())
    fallback = property(lambda self: bool(int(self._host()[13]) & FLAG_FALLBACK_AXIS))
    nonfinite = property(lambda self: bool(int(self._host()[13]) & FLAG_NONFINITE))

    def to_origin(self) -> np.ndarray:
        """The translation that moves the hinge to the origin: -position."""
        return -self.position

    def pose(self, angle):
        """(R, t) of the rotation by `angle` (radians, right-handed about `axis`) about the line through `position`:
        x -> R x + t with t = position - R position.  float64 NumPy; a scalar angle gives R [3,3] and t [3], an array of
        K angles R [K,3,3] and t [K,3] -- what pack_transforms / transform_gaussians / FrameRenderer.submit(rotations=,
        translations=) take for the part's group."""
        ang = np.asarray(angle, dtype=np.float64)
        k, p = self.axis, self.position
        k = k / np.linalg.norm(k)
        K = np.array([[0.0, -k[2], k[1]], [k[2], 0.0, -k[0]], [-k[1], k[0], 0.0]])
        c, s = np.cos(ang)[..., None, None], np.sin(ang)[..., None, None]
        R = c * np.eye(3) + s * K + (1.0 - c) * np.outer(k, k)            # Rodrigues
        return R, p - R @ p

    def pose_torch(self, angle: Tensor):
        """`pose` in torch, differentiable in `angle`: Rodrigues on the angle's device and in its dtype, t = position -
        R position; the values are those of `pose`.  A scalar angle gives R [3,3] and t [3], K angles R [K,3,3] and t [K,3]
        -- what pose_gaussians(rotations=, translations=) takes for the part's group (R[None], t[None] for one angle)."""
        key = (angle.device, angle.dtype)
        consts = self._torch_consts.get(key)
        if consts is None:                       # [k]x, k k^T, I and the position, uploaded once per device and dtype
            k, p = self.axis, self.position
            k = k / np.linalg.norm(k)
            kw = dict(dtype=angle.dtype, device=angle.device)
            consts = self._torch_consts[key] = (
                torch.tensor([[0.0, -k[2], k[1]], [k[2], 0.0, -k[0]], [-k[1], k[0], 0.0]], **kw),
                torch.tensor(np.outer(k, k), **kw), torch.eye(3, **kw), torch.tensor(p, **kw))
        K, kk, eye, pt = consts
        c, s = torch.cos(angle)[..., None, None], torch.sin(angle)[..., None, None]
        R = c * eye + s * K + (1.0 - c) * kk                              # Rodrigues
        return R, pt - R @ pt

    def __repr__(self):
        return (f"Hinge(position={self.position.tolist()}, axis={self.axis.tolist()}, axis_confidence={self.axis_confidence:.4f}, "
                f"min_distance={self.min_distance:.3g}, n_contact={self.n_contact}, fallback={self.fallback})")


@torch.no_grad()
def fit_hinge_points(points_a: Tensor, points_b: Tensor, threshold: float = 0.01, return_contacts: bool = False) -> Hinge:
    """The hinge between two point sets of the caller's own (mesh vertices, say): points_a [n_a,3] is the moving part,
    points_b [n_b,3] the base, both on the GPU.  A point with a non-finite coordinate takes no part.  No synchronisation:
    the returned Hinge reads the record on first use.  return_contacts: also keep the contact masks (bool [n])."""
    require_device(points_a, points_b)
    if not (np.isfinite(threshold) and threshold > 0):
        raise ValueError(f"threshold {threshold} is not a finite positive number")
    ca = cb = None
    if return_contacts:
        ca = torch.empty(points_a.shape[0], dtype=torch.uint8, device=points_a.device)
        cb = torch.empty(points_b.shape[0], dtype=torch.uint8, device=points_b.device)
    joint = hinge_fit_raw(points_a, points_b, threshold, ca, cb)
    return Hinge(joint, ca.bool() if return_contacts else None, cb.bool() if return_contacts else None, threshold)


@torch.no_grad()
def fit_hinge(means: Tensor, class_ids: Tensor, part: int, base: int, threshold: float = 0.01,
              return_contacts: bool = False) -> Hinge:
    """The hinge of the Gaussians labelled `part` (the moving part) against those labelled `base`: means [N,3] and
    class_ids int [N] (the form lift_labels returns) on the GPU.  Selecting means[class_ids == part] is boolean indexing,
    which synchronises with the device: fine for a call made once per scene, not for a per-frame loop (keep the two
    selections and call fit_hinge_points, or hinge_fit_raw, there).  With return_contacts the masks index the selected
    rows, in the order of the scene.  Raises ValueError naming a class that has no Gaussian."""
    require_device(means, class_ids)
    if means.dim() != 2 or means.shape[1] != 3 or class_ids.shape != (means.shape[0],):
        raise ValueError("expected means [N,3] and class_ids [N]")
    sets = []
    for name, cls in (("part", part), ("base", base)):
        rows = means[class_ids == int(cls)]
        if rows.shape[0] == 0:
            raise ValueError(f"class {int(cls)} ({name}) has no Gaussian")
        sets.append(rows)
    return fit_hinge_points(sets[0], sets[1], threshold, return_contacts)


__all__ = ["Hinge", "fit_hinge", "fit_hinge_points", "hinge_fit_raw", "hinge_workspace", "workspace_bytes", "JOINT_DOUBLES"]
