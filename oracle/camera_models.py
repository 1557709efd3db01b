"""The camera models of the oracle's projection (include/mgs.h MGS_CAMERA_*): the one place that knows how a model
forms the projected mean and the 2 x 3 Jacobian J of A.2 step 3 (TEST INFRASTRUCTURE ONLY).  Written once for NumPy
and torch (the `xp` argument); gs_oracle_np.project and gs_oracle_torch.project call it for "ortho" and "fisheye" and
keep pinhole, with its frustum clamp, in their own step 3.  See the header of gs_oracle_np.py for the maps.
"""
from __future__ import annotations

import numpy as np

CAMERA_MODELS = ("pinhole", "ortho", "fisheye")
# below t = rho^2 / z^2 = 1e-3 the fisheye terms come from their series (fp64: 8 terms are exact to rounding)
_SERIES_T = 1e-3


def _fisheye_s_a(q, z, xp):
    """s = theta / rho and a = (z / r2 - s) / q as functions of q = rho^2 and z, with the series near the axis
    (xp = numpy or torch; the torch form keeps both branches finite so that autograd through `where` stays finite)."""
    where = xp.where
    z2 = z * z
    small = q < _SERIES_T * z2
    t = where(small, q / z2, xp.zeros_like(q))
    s_ser = sum(((-t) ** n) / (2 * n + 1) for n in range(8)) / z
    a_ser = sum(((-1) ** (n + 1)) * 2.0 * (n + 1) / (2 * n + 3) * t ** n for n in range(8)) / (z2 * z)
    qs = where(small, xp.ones_like(q), q)           # the closed form, away from the axis
    rho = xp.sqrt(qs)
    atan2 = np.arctan2 if xp is np else xp.atan2
    s_dir = atan2(rho, z) / rho
    a_dir = (z / (qs + z2) - s_dir) / qs
    return where(small, s_ser, s_dir), where(small, a_ser, a_dir)


def mean_and_J(x, y, z, fx, fy, cx, cy, camera_model, xp):
    """Camera-space x, y, z [N] (z already made safe where it is culled) -> ((mu_x, mu_y), the six entries of J row by
    row), each [N], under "ortho" or "fisheye".  No frustum clamp; the arithmetic stays in the dtype of x, y, z."""
    zero = xp.zeros_like(x)
    if camera_model == "ortho":
        mu = (fx * x + cx, fy * y + cy)
        J = (fx + zero, zero, zero, zero, fy + zero, zero)
    elif camera_model == "fisheye":
        q = x * x + y * y
        s, a = _fisheye_s_a(q, z, xp)
        ir2 = 1.0 / (q + z * z)
        mu = (fx * s * x + cx, fy * s * y + cy)
        J = (fx * (s + x * x * a), fx * x * y * a, -fx * x * ir2, fy * x * y * a, fy * (s + y * y * a), -fy * y * ir2)
    else:
        raise ValueError(camera_model)
    return mu, J
