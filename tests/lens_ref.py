"""The fp64 reference of the distorted fisheye (include/mgs.h MGS_CAMERA_FISHEYE_KB; TEST INFRASTRUCTURE ONLY).

OpenCV's fisheye / nerfstudio's OPENCV_FISHEYE model on top of the oracle's equidistant lens: with q = x^2 + y^2,
r2 = q + z^2, theta = atan2(sqrt(q), z), s = theta / sqrt(q), a = (z / r2 - s) / q (oracle/camera_models.py, series near
the axis) and u = theta^2 = s^2 q,

    P(u) = 1 + k1 u + k2 u^2 + k3 u^3 + k4 u^4          theta_d = theta P(theta^2)
    S = s P     A = a P + 2 s^2 z P' / r2     D = P + 2 u P'  (= d theta_d / d theta)
    mean = (fx S x + cx, fy S y + cy)
    J    = [[fx (S + x^2 A), fx x y A, -fx x D / r2], [fy x y A, fy (S + y^2 A), -fy y D / r2]]

`lens(k)` substitutes this for `mean_and_J` in oracle.gs_oracle_np and oracle.gs_oracle_torch (both import the name), so
the unchanged oracle `project` / `render`, called with camera_model="fisheye", project, cull, rasterise and differentiate
under the lens.

The cull.  The lens is valid up to theta_max, the smallest positive root of D (where theta_d stops growing), or pi/2.  A
point with u >= u_max = theta_max^2 is culled here by MASKING THE RADII through the oracle's own screen test: its mean is
reported 1e30 pixels off screen (a constant: no gradient) and its J is the finite J of the ideal lens, so the oracle's
`mean + radius <= 0` test drops it like any off-screen Gaussian and every masked output is zero.  z is left alone.
"""
from __future__ import annotations

import contextlib
import math

import numpy as np

from oracle import camera_models as CM
from oracle import gs_oracle_np as O
from oracle import gs_oracle_torch as OT

MILD = (-0.04, 0.012, -0.006, 0.0015)      # no fold below pi/2
FOLDING = (-0.2, 0.0, 0.0, 0.0)            # theta_max = sqrt(1 / 0.6) = 1.2909944...
_OFF_SCREEN = -1e30


def _D(k, u):
    return 1.0 + u * (3.0 * k[0] + u * (5.0 * k[1] + u * (7.0 * k[2] + u * 9.0 * k[3])))


def theta_max(k) -> float:
    """Smallest positive root of D(theta^2) = 1 + 3 k1 theta^2 + 5 k2 theta^4 + 7 k3 theta^6 + 9 k4 theta^8 below pi/2, or
    pi/2: a scan of (0, pi/2] in 2^16 steps for the first sign change, then bisection to the last bit."""
    k = [float(v) for v in k]
    n = 1 << 16
    lo = 0.0
    for i in range(1, n + 1):
        hi = 0.5 * math.pi * i / n
        if _D(k, hi * hi) <= 0.0:
            for _ in range(200):
                mid = 0.5 * (lo + hi)
                if mid == lo or mid == hi:
                    break
                if _D(k, mid * mid) > 0.0:
                    lo = mid
                else:
                    hi = mid
            return hi
        lo = hi
    return 0.5 * math.pi


def u_of(x, y, z, xp=np):
    """theta^2 of camera points, as the cull sees it."""
    q = x * x + y * y
    s, _ = CM._fisheye_s_a(q, z, xp)
    return s * s * q


def mean_and_J(x, y, z, fx, fy, cx, cy, k, xp, u_max=None):
    """((mu_x, mu_y), the six entries of J row by row) of the distorted fisheye at camera points x, y, z [N], xp = numpy
    or torch, in the dtype of the inputs.  u_max given: points with u >= u_max get the off-screen mean (see the header)."""
    k1, k2, k3, k4 = (float(v) for v in k)
    q = x * x + y * y
    s, a = CM._fisheye_s_a(q, z, xp)
    ir2 = 1.0 / (q + z * z)
    u = s * s * q
    P = 1.0 + u * (k1 + u * (k2 + u * (k3 + u * k4)))
    P1 = k1 + u * (2.0 * k2 + u * (3.0 * k3 + u * 4.0 * k4))
    S = s * P
    A = a * P + 2.0 * s * s * z * P1 * ir2
    D = P + 2.0 * u * P1
    mu = (fx * S * x + cx, fy * S * y + cy)
    J = (fx * (S + x * x * A), fx * x * y * A, -fx * x * D * ir2, fy * x * y * A, fy * (S + y * y * A), -fy * y * D * ir2)
    if u_max is not None:
        out = u >= u_max
        off = xp.zeros_like(x) + _OFF_SCREEN
        ideal = (fx * (s + x * x * a), fx * x * y * a, -fx * x * ir2, fy * x * y * a, fy * (s + y * y * a), -fy * y * ir2)
        mu = tuple(xp.where(out, off, m) for m in mu)
        J = tuple(xp.where(out, i, j) for i, j in zip(ideal, J))
    return mu, J


@contextlib.contextmanager
def lens(k):
    """Inside: oracle.gs_oracle_np / gs_oracle_torch `project` and `render` with camera_model="fisheye" see the lens k
    (k1..k4), cull included.  The other models are passed through."""
    u_max = theta_max(k) ** 2
    orig = CM.mean_and_J

    def patched(x, y, z, fx, fy, cx, cy, camera_model, xp):
        if camera_model != "fisheye":
            return orig(x, y, z, fx, fy, cx, cy, camera_model, xp)
        return mean_and_J(x, y, z, fx, fy, cx, cy, k, xp, u_max=u_max)
    saved = (O.mean_and_J, OT.mean_and_J)
    O.mean_and_J = OT.mean_and_J = patched
    try:
        yield u_max
    finally:
        O.mean_and_J, OT.mean_and_J = saved


def lens_row(K, k):
    """The 16-float camera row of include/mgs.h for one camera: K row-major, k1..k4, u_max, two zeros (float64)."""
    return np.concatenate([np.asarray(K, dtype=np.float64).reshape(9), np.asarray(k, dtype=np.float64),
                           [theta_max(k) ** 2, 0.0, 0.0]])
