"""The fp64 reference of the pinhole lens (include/mgs_lens_pinhole.h MGS_CAMERA_PINHOLE_BC; TEST INFRASTRUCTURE ONLY).

OpenCV's radial / tangential (Brown-Conrady) model, cv2.calibrateCamera's distCoeffs (k1, k2, p1, p2, k3) and nerfstudio's
camera_model "OPENCV".  For a camera point (x, y, z):

    x' = x/z   y' = y/z   u = x'^2 + y'^2
    Rad = 1 + k1 u + k2 u^2 + k3 u^3          Rad1 = dRad/du
    xd = x' Rad + 2 p1 x' y' + p2 (u + 2 x'^2)
    yd = y' Rad + p1 (u + 2 y'^2) + 2 p2 x' y'
    mean = (fx xd + cx, fy yd + cy)
    Jd = d(xd,yd)/d(x',y') = [[Rad + 2x'^2 Rad1 + 2 p1 y' + 6 p2 x',  2x'y' Rad1 + 2 p1 x' + 2 p2 y'],
                              [ same off-diagonal,                    Rad + 2y'^2 Rad1 + 6 p1 y' + 2 p2 x']]
    J  = diag(fx, fy) Jd [[1/z, 0, -x/z^2], [0, 1/z, -y/z^2]]

`lens(k, W, H)` substitutes this for `mean_and_J` in oracle.gs_oracle_np and oracle.gs_oracle_torch (both import the name)
under the model name "fisheye" -- the oracle's generic path for a dense J without a clamp -- so the unchanged oracle
`project` / `render`, called with camera_model="fisheye", project, cull, rasterise and differentiate under the lens.

The culls.  A point is culled when (1) u >= u_max, the smallest positive root of 1 + 3 k1 u + 5 k2 u^2 + 7 k3 u^3 (inf
without one), (2) det Jd <= 0, or (3) (xd, yd) lies outside [-lim_xn, lim_xp] x [-lim_yn, lim_yp], the plain pinhole's clamp
box (frame plus 0.3 of the half field).  All three are applied by MASKING THE RADII through the oracle's own screen test:
the mean of a culled point is reported 1e30 pixels off screen (a constant: no gradient) and its J is the finite J of the
ideal pinhole, so the oracle's `mean + radius <= 0` test drops it like any off-screen Gaussian.  z is left alone.
"""
from __future__ import annotations

import contextlib
import math

import numpy as np

from oracle import camera_models as CM
from oracle import gs_oracle_np as O
from oracle import gs_oracle_torch as OT

MILD = (-0.12, 0.03, 0.002, -0.0015, -0.004)     # radial fold at u = 4.2989, far outside the box at f = 90, 112 x 80
FOLDING = (-0.35, 0.0, 0.003, -0.002, 0.0)       # radial fold at u = 0.95238: inside the frame at f = 50
_OFF_SCREEN = -1e30
_U_SCAN_END = 64.0      # |x'| = 8: 83 degrees off the axis; a fold further out is no fold of a pinhole camera's field


def _dradial(k, u):
    return 1.0 + u * (3.0 * k[0] + u * (5.0 * k[1] + u * 7.0 * k[4]))


def u_max(k) -> float:
    """Smallest positive root of 1 + 3 k1 u + 5 k2 u^2 + 7 k3 u^3, or inf: a scan of (0, 64] in 2^18 steps for the first
    sign change, then bisection to the last bit.  (Independent of the product's polynomial root finder.)"""
    k = full(k)
    n = 1 << 18
    lo = 0.0
    for i in range(1, n + 1):
        hi = _U_SCAN_END * i / n
        if _dradial(k, hi) <= 0.0:
            for _ in range(200):
                mid = 0.5 * (lo + hi)
                if mid == lo or mid == hi:
                    break
                if _dradial(k, mid) > 0.0:
                    lo = mid
                else:
                    hi = mid
            return hi
        lo = hi
    return math.inf


def full(k):
    """(k1, k2, p1, p2, k3) as floats; four values mean k3 = 0."""
    k = [float(v) for v in k]
    return k + [0.0] if len(k) == 4 else k


def box(fx, fy, cx, cy, W, H):
    """(lim_xn, lim_xp, lim_yn, lim_yp) of the pinhole clamp: the frame plus 0.3 of the half field, in normalised units."""
    tanx, tany = 0.5 * W / fx, 0.5 * H / fy
    return cx / fx + 0.3 * tanx, (W - cx) / fx + 0.3 * tanx, cy / fy + 0.3 * tany, (H - cy) / fy + 0.3 * tany


def distort(a, b, k):
    """(xd, yd, (d00, d01, d11), u) at normalised points a = x/z, b = y/z (numpy arrays or torch tensors)."""
    k1, k2, p1, p2, k3 = full(k)
    u = a * a + b * b
    rad = 1.0 + u * (k1 + u * (k2 + u * k3))
    rad1 = k1 + u * (2.0 * k2 + u * 3.0 * k3)
    xd = a * rad + 2.0 * p1 * a * b + p2 * (u + 2.0 * a * a)
    yd = b * rad + p1 * (u + 2.0 * b * b) + 2.0 * p2 * a * b
    d00 = rad + 2.0 * a * a * rad1 + 2.0 * p1 * b + 6.0 * p2 * a
    d01 = 2.0 * a * b * rad1 + 2.0 * p1 * a + 2.0 * p2 * b
    d11 = rad + 2.0 * b * b * rad1 + 6.0 * p1 * b + 2.0 * p2 * a
    return xd, yd, (d00, d01, d11), u


def cull_margins(x, y, z, fx, fy, cx, cy, k, W, H, umax=None):
    """How far camera points are from flipping each cull, as (culled [N] bool, margin [N]): margin is the smallest of
    |u / u_max - 1|, |det Jd| and the relative distances of (xd, yd) to the four box borders.  numpy, fp64."""
    umax = u_max(k) if umax is None else umax
    a, b = x / z, y / z
    xd, yd, (d00, d01, d11), u = distort(a, b, k)
    det = d00 * d11 - d01 * d01
    lxn, lxp, lyn, lyp = box(fx, fy, cx, cy, W, H)
    culled = (u >= umax) | (det <= 0.0) | (xd > lxp) | (xd < -lxn) | (yd > lyp) | (yd < -lyn)
    margin = np.minimum.reduce([np.abs(u / umax - 1.0) if math.isfinite(umax) else np.full_like(u, np.inf), np.abs(det),
                                np.abs(xd / lxp - 1.0), np.abs(xd / lxn + 1.0), np.abs(yd / lyp - 1.0), np.abs(yd / lyn + 1.0)])
    return culled, margin


def mean_and_J(x, y, z, fx, fy, cx, cy, k, xp, W=None, H=None, umax=None):
    """((mu_x, mu_y), the six entries of J row by row) of the pinhole lens at camera points x, y, z [N], xp = numpy or
    torch, in the dtype of the inputs.  W, H and umax given: culled points get the off-screen mean (see the header)."""
    zs = xp.where(z > 0.0, z, xp.ones_like(z))      # (behind the camera: culled below, on finite numbers)
    rz = 1.0 / zs
    a, b = x / zs, y / zs
    xd, yd, (d00, d01, d11), u = distort(a, b, k)
    mu = (fx * xd + cx, fy * yd + cy)
    J = (fx * d00 * rz, fx * d01 * rz, -fx * rz * (d00 * a + d01 * b),
         fy * d01 * rz, fy * d11 * rz, -fy * rz * (d01 * a + d11 * b))
    if umax is not None:
        lxn, lxp, lyn, lyp = box(fx, fy, cx, cy, W, H)
        det = d00 * d11 - d01 * d01
        out = (u >= umax) | (det <= 0.0) | (xd > lxp) | (xd < -lxn) | (yd > lyp) | (yd < -lyn) | (z <= 0.0)
        off = xp.zeros_like(x) + _OFF_SCREEN
        zero = xp.zeros_like(x)
        ideal = (fx * rz, zero, -fx * a * rz, zero, fy * rz, -fy * b * rz)
        mu = tuple(xp.where(out, off, m) for m in mu)
        J = tuple(xp.where(out, i, j) for i, j in zip(ideal, J))
    return mu, J


@contextlib.contextmanager
def lens(k, W, H):
    """Inside: oracle.gs_oracle_np / gs_oracle_torch `project` and `render` with camera_model="fisheye" see the pinhole
    lens k (k1, k2, p1, p2, k3) of a W x H frame, culls included.  The other models are passed through."""
    umax = u_max(k)
    orig = CM.mean_and_J

    def patched(x, y, z, fx, fy, cx, cy, camera_model, xp):
        if camera_model != "fisheye":
            return orig(x, y, z, fx, fy, cx, cy, camera_model, xp)
        return mean_and_J(x, y, z, fx, fy, cx, cy, k, xp, W=W, H=H, umax=umax)
    saved = (O.mean_and_J, OT.mean_and_J)
    O.mean_and_J = OT.mean_and_J = patched
    try:
        yield umax
    finally:
        O.mean_and_J, OT.mean_and_J = saved


def lens_row(K, k):
    """The 16-float camera row of include/mgs_lens_pinhole.h for one camera: K row-major, k1 k2 p1 p2 k3, u_max (FLT_MAX
    without a fold), zero (float64)."""
    um = u_max(k)
    return np.concatenate([np.asarray(K, dtype=np.float64).reshape(9), np.asarray(full(k), dtype=np.float64),
                           [um if math.isfinite(um) else float(np.finfo(np.float32).max), 0.0]])


# ---- the test scenes (shared by tests/test_pinhole_lens_host.py and tests/test_gpu_pinhole_lens.py) ---------------------
W, H, CX, CY = 112, 80, 57.5, 39.0
LENSES = {"mild": MILD, "folding": FOLDING}
FOCAL = {"mild": 90.0, "folding": 50.0}
NEAR = 0.05
FLIP_MARGIN = 1e-4        # a centre closer than this (relative) to flipping a cull is not a kernel error: kept out of scenes
FLIP_CAP = 0.02           # ... which may cost a scene at most this share of its Gaussians
# the culls that Gaussians are planted around under each lens: MILD's folds lie far outside its box, and inside FOLDING's
# radial fold the distorted point never reaches the box
PLANTED_CULLS = {"mild": ("box",), "folding": ("fold", "det")}


def intrinsics(lens, w=W, h=H):
    """K of a lens's camera, scaled with the frame from the 112 x 80 one the lenses were checked at."""
    f = FOCAL[lens] * w / W
    return np.array([[f, 0.0, CX * w / W], [0.0, f, CY * h / H], [0.0, 0.0, 1.0]])


def camera_points(means, vm):
    """fp64 camera points of the fp32 means and view matrix the GPU is handed."""
    f = lambda a: np.asarray(a, dtype=np.float32).astype(np.float64)
    return f(means) @ f(vm)[:3, :3].T + f(vm)[:3, 3]


def first_cull(k, K, w, h, phi, r_end=3.0, steps=3000):
    """Along the ray (x', y') = r (cos phi, sin phi): (r*, kind) of the first cull met -- "fold" (u >= u_max), "det"
    (det Jd <= 0) or "box" -- by a scan in r and bisection; kind is read just past r*."""
    fx, fy, cx, cy = K[0, 0], K[1, 1], K[0, 2], K[1, 2]
    umax = u_max(k)
    c, s_ = math.cos(phi), math.sin(phi)

    def culled(r):
        return bool(cull_margins(np.array([r * c]), np.array([r * s_]), np.ones(1), fx, fy, cx, cy, k, w, h, umax)[0][0])
    lo = 0.0
    for i in range(1, steps + 1):
        hi = r_end * i / steps
        if culled(hi):
            break
        lo = hi
    else:
        raise AssertionError(f"no cull along phi = {phi}")
    for _ in range(60):
        mid = 0.5 * (lo + hi)
        lo, hi = (lo, mid) if culled(mid) else (mid, hi)
    a, b = np.array([hi * 1.0001 * c]), np.array([hi * 1.0001 * s_])
    xd, yd, (d00, d01, d11), u = distort(a, b, k)
    kind = "fold" if u[0] >= umax else ("det" if (d00 * d11 - d01 * d01)[0] <= 0.0 else "box")
    return hi, kind


def plant(g, vm, lens, K, w, h, count=8):
    """Move the first Gaussians of g: `count` onto the optical axis and `count` just off it, and for every cull of
    PLANTED_CULLS[lens] `count` to 0.97 .. 0.995 of the cull's border (inside: visible) and `count` to 1.005 .. 1.03 of it
    (outside: culled; around the box both are 0.12 x depth wide, so that only the box cull keeps the outer ones off the
    frame), along `count` azimuths spread over the directions in which that cull is the first one met -- for the
    box, that is every side of it.  Depths 1.5 .. 3.  Returns (number planted, {cull: (inside indices, outside indices)})."""
    k = LENSES[lens]
    rays = [(phi,) + first_cull(k, K, w, h, phi) for phi in np.linspace(0.0, 2.0 * math.pi, 96, endpoint=False) + 0.01]
    pts, where = [], {}
    for i in range(count):
        d, phi = 1.5 + 1.5 * i / count, 0.8 * i
        pts.append((0.0, 0.0, d))
        pts.append((1e-4 * d * math.cos(phi), 1e-4 * d * math.sin(phi), d))
    for cull in PLANTED_CULLS[lens]:
        mine = [r for r in rays if r[2] == cull]
        assert len(mine) >= count, f"{lens}: the {cull} cull is the first one met along {len(mine)} of {len(rays)} rays only"
        picks = [mine[(j * len(mine)) // count] for j in range(count)]
        inside, outside = [], []
        for i, (phi, r, _) in enumerate(picks):
            d = 1.5 + 1.5 * i / count
            for rel, idx in ((0.97 + 0.025 * i / (count - 1), inside), (1.005 + 0.025 * i / (count - 1), outside)):
                idx.append(len(pts))
                pts.append((d * r * rel * math.cos(phi), d * r * rel * math.sin(phi), d))
                if cull == "box":      # the box's border lies 0.3 of the half field outside the frame: wide enough to reach in
                    g.log_scales[idx[-1]] = math.log(0.12 * d)
        where[cull] = (np.array(inside), np.array(outside))
    pc = np.array(pts)
    R, tvec = np.asarray(vm)[:3, :3], np.asarray(vm)[:3, 3]
    g.means[:len(pc)] = ((pc - tvec) @ R).astype(g.means.dtype)          # world = R^T (p - t)
    return len(pc), where


def scene(lens, n, deg, mu=0.07, w=W, h=H, seed=0, planted=True, radius=3.0, theta=0.7):
    """(Gaussians, viewmat, K, info) of a lens's test scene: robosimgs_amd.synthetic_scene seen from a ring camera close
    enough that Gaussians lie on both sides of every cull (uniformly: past the box under MILD, past the radial fold under
    FOLDING), the planted Gaussians of plant() first, and every Gaussian within FLIP_MARGIN of flipping a cull removed --
    at most FLIP_CAP of the scene, asserted here.  info: planted (count), where (plant's index map), removed (count)."""
    from robosimgs_amd import camera_ring, synthetic_scene
    g = synthetic_scene(n, math.log(mu), deg, seed)
    vm = camera_ring(1, w, h, thetas=[theta], radius=radius)[0].viewmat()
    K = intrinsics(lens, w, h)
    n_planted, where = plant(g, vm, lens, K, w, h) if planted else (0, {})
    pc = camera_points(g.means, vm)
    front = pc[:, 2] > 0.0
    z = np.where(front, pc[:, 2], 1.0)
    _, margin = cull_margins(pc[:, 0], pc[:, 1], z, K[0, 0], K[1, 1], K[0, 2], K[1, 2], LENSES[lens], w, h)
    near = front & (np.abs(pc[:, 2] / NEAR - 1.0) < FLIP_MARGIN)          # (the near plane is a cull like the others)
    drop = (front & (margin < FLIP_MARGIN)) | near
    assert not drop[:n_planted].any(), "a planted Gaussian is a near-flip"
    assert drop.sum() <= FLIP_CAP * n, f"the near-flip filter removes {int(drop.sum())} of {n} Gaussians"
    g = g.permuted(np.flatnonzero(~drop))
    return g, vm, K, {"planted": n_planted, "where": where, "removed": int(drop.sum())}
