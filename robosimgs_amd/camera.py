"""Cameras in the conventions RoboSimGS uses (pinhole, orthographic or equidistant fisheye, ideal or with OpenCV's k1..k4).

The reference stores cameras as OpenGL camera-to-world matrices (+X right, +Y up, camera
looks down -Z) plus a 3x3 intrinsic matrix:
  * nerfstudio `transforms.json` frames (`transform_matrix`, `fl_x`, `fl_y`, `cx`, `cy`)
    -- /root/reference/Articulation/utils/nerf2physic_utils.py:26-52
  * `camera_params.json` written by the segmenter (`intrinsics`, `c2w`, `resolution`)
    -- /root/reference/Articulation/segmentation/interactive_segmenter.py:279-320
The renderer consumes OpenCV world-to-camera view matrices (+Z forward, +Y down).  The
conversion is the one `project_3d_to_2d` applies (nerf2physic_utils.py:14-16): invert
c2w, negate camera Y and Z.
"""
from __future__ import annotations

import json
import math
from dataclasses import dataclass, field
from typing import Dict, List, Optional, Sequence, Tuple

import numpy as np

_FLIP_YZ = np.diag([1.0, -1.0, -1.0, 1.0])
CAMERA_MODELS = ("pinhole", "ortho", "fisheye")      # rasterization(camera_model=...); include/mgs.h MGS_CAMERA_*


def lens_theta_max(k) -> float:
    """Where the fisheye polynomial theta_d = theta (1 + k1 theta^2 + k2 theta^4 + k3 theta^6 + k4 theta^8) stops being
    monotonic: the smallest positive root of d theta_d / d theta = 1 + 3 k1 u + 5 k2 u^2 + 7 k3 u^3 + 9 k4 u^4, u = theta^2,
    or pi/2 (the near plane's limit) when there is none below it.  fp64; the renderer culls theta >= theta_max."""
    k1, k2, k3, k4 = (float(v) for v in k)
    coeffs = np.trim_zeros(np.array([9.0 * k4, 7.0 * k3, 5.0 * k2, 3.0 * k1, 1.0]), "f")
    best = 0.5 * math.pi
    if len(coeffs) > 1:
        for r in np.roots(coeffs):
            if abs(r.imag) <= 1e-12 * max(1.0, abs(r.real)) and r.real > 0.0:
                best = min(best, math.sqrt(r.real))
    return best


def pinhole_lens_u_max(k) -> float:
    """Where the radial map r Rad(r^2) of the pinhole lens (OpenCV k1 k2 p1 p2 k3; Rad(u) = 1 + k1 u + k2 u^2 + k3 u^3, u =
    x'^2 + y'^2 in normalised coordinates) stops growing: the smallest positive real root of d(r Rad)/dr =
    1 + 3 k1 u + 5 k2 u^2 + 7 k3 u^3, or inf when there is none.  fp64; the renderer culls u >= u_max."""
    k = [float(v) for v in k]
    k1, k2, k3 = k[0], k[1], (k[4] if len(k) > 4 else 0.0)
    coeffs = np.trim_zeros(np.array([7.0 * k3, 5.0 * k2, 3.0 * k1, 1.0]), "f")
    best = math.inf
    if len(coeffs) > 1:
        for r in np.roots(coeffs):
            if abs(r.imag) <= 1e-12 * max(1.0, abs(r.real)) and r.real > 0.0:
                best = min(best, float(r.real))
    return best


def pinhole_lens_distort(a, b, k):
    """OpenCV's radial / tangential lens at normalised points a = x/z, b = y/z (fp64 ndarrays), k = (k1, k2, p1, p2, k3):
    (xd, yd, det Jd), Jd the 2 x 2 Jacobian of (xd, yd) in (a, b) (include/mgs_lens_pinhole.h)."""
    k1, k2, p1, p2, k3 = (float(v) for v in k)
    u = a * a + b * b
    rad = 1.0 + u * (k1 + u * (k2 + u * k3))
    rad1 = k1 + u * (2.0 * k2 + u * 3.0 * k3)
    xd = a * rad + 2.0 * p1 * a * b + p2 * (u + 2.0 * a * a)
    yd = b * rad + p1 * (u + 2.0 * b * b) + 2.0 * p2 * a * b
    d00 = rad + 2.0 * a * a * rad1 + 2.0 * p1 * b + 6.0 * p2 * a
    d01 = 2.0 * a * b * rad1 + 2.0 * p1 * a + 2.0 * p2 * b
    d11 = rad + 2.0 * b * b * rad1 + 6.0 * p1 * b + 2.0 * p2 * a
    return xd, yd, d00 * d11 - d01 * d01


@dataclass
class Camera:
    """One camera.  `c2w` is OpenGL camera-to-world (4x4, float64).  `model`: "pinhole", "ortho" (pixel =
    (fx x + cx, fy y + cy) in camera space: fx is pixels per world unit) or "fisheye" (ideal equidistant lens,
    pixel radius = f theta, theta the angle off the optical axis).  `distortion` (meaningful for "fisheye"): OpenCV fisheye
    coefficients (k1, k2, k3, k4), pixel radius = f theta (1 + k1 theta^2 + k2 theta^4 + k3 theta^6 + k4 theta^8) -- what
    cv2.fisheye.calibrate and nerfstudio's OPENCV_FISHEYE store; None: the ideal lens.  `pinhole_distortion` (needs
    "pinhole"): OpenCV's distCoeffs (k1, k2, p1, p2, k3) of cv2.calibrateCamera / nerfstudio's OPENCV -- four values mean
    k3 = 0; None: no lens."""

    c2w: np.ndarray
    fx: float
    fy: float
    cx: float
    cy: float
    width: int
    height: int
    near: float = 0.01
    far: float = 1e10
    # keyword-only (Camera(..., distortion=(k1, k2, k3, k4))), so that `model` stays the last positional field
    distortion: Optional[Tuple[float, float, float, float]] = field(default=None, kw_only=True)
    pinhole_distortion: Optional[Tuple[float, float, float, float, float]] = field(default=None, kw_only=True)
    model: str = "pinhole"

    def __post_init__(self):
        if self.model not in CAMERA_MODELS:
            raise ValueError(f"camera model {self.model!r} not in {CAMERA_MODELS}")
        if self.pinhole_distortion is not None:
            if self.model != "pinhole":
                raise ValueError(f"pinhole_distortion (k1, k2, p1, p2, k3) needs model='pinhole', got {self.model!r}")
            self.pinhole_distortion = tuple(float(v) for v in self.pinhole_distortion)
            if len(self.pinhole_distortion) == 4:
                self.pinhole_distortion += (0.0,)
            if len(self.pinhole_distortion) != 5 or not all(math.isfinite(v) for v in self.pinhole_distortion):
                raise ValueError("pinhole_distortion must be finite (k1, k2, p1, p2, k3), or (k1, k2, p1, p2) for k3 = 0")
        if self.distortion is not None:
            if self.model != "fisheye":
                raise ValueError(f"distortion (fisheye k1..k4) needs model='fisheye', got {self.model!r}")
            self.distortion = tuple(float(v) for v in self.distortion)
            if len(self.distortion) != 4:
                raise ValueError("distortion must be (k1, k2, k3, k4)")
        self.c2w = np.asarray(self.c2w, dtype=np.float64).reshape(4, 4)
        self.width = int(self.width)
        self.height = int(self.height)

    # -- constructors --------------------------------------------------------------
    @classmethod
    def from_c2w_opengl(cls, c2w, K, width, height, **kw) -> "Camera":
        K = np.asarray(K, dtype=np.float64)
        return cls(c2w, K[0, 0], K[1, 1], K[0, 2], K[1, 2], width, height, **kw)

    @classmethod
    def from_w2c_opencv(cls, viewmat, K, width, height, **kw) -> "Camera":
        """Inverse of :meth:`viewmat`."""
        c2w = np.linalg.inv(_FLIP_YZ @ np.asarray(viewmat, dtype=np.float64))
        return cls.from_c2w_opengl(c2w, K, width, height, **kw)

    @classmethod
    def from_camera_params(cls, entry: Dict, **kw) -> "Camera":
        """One entry of the segmenter's `camera_params.json`
        (interactive_segmenter.py:313-320: keys intrinsics / c2w / resolution)."""
        w, h = entry["resolution"]
        return cls.from_c2w_opengl(entry["c2w"], entry["intrinsics"], w, h, **kw)

    @classmethod
    def look_at(cls, position, target, up, width, height, fov_x_deg, **kw) -> "Camera":
        """Look-at construction with the reference's column layout
        (interactive_segmenter.py:291-311: columns right / up / -forward / position)
        and its fov -> focal rule (:280-281, applied to the image width)."""
        position = np.asarray(position, dtype=np.float64)
        forward = np.asarray(target, dtype=np.float64) - position
        forward /= np.linalg.norm(forward)
        right = np.cross(forward, np.asarray(up, dtype=np.float64))
        right /= np.linalg.norm(right)
        true_up = np.cross(right, forward)
        true_up /= np.linalg.norm(true_up)
        c2w = np.eye(4)
        c2w[:3, 0], c2w[:3, 1], c2w[:3, 2], c2w[:3, 3] = right, true_up, -forward, position
        f = (width / 2.0) / math.tan(math.radians(fov_x_deg / 2.0))
        return cls(c2w, f, f, width / 2.0, height / 2.0, width, height, **kw)

    # -- derived quantities --------------------------------------------------------
    @property
    def K(self) -> np.ndarray:
        return np.array([[self.fx, 0.0, self.cx], [0.0, self.fy, self.cy],
                         [0.0, 0.0, 1.0]])

    def viewmat(self) -> np.ndarray:
        """OpenCV world-to-camera 4x4: diag(1,-1,-1,1) @ inv(c2w)."""
        return _FLIP_YZ @ np.linalg.inv(self.c2w)

    @property
    def position(self) -> np.ndarray:
        return self.c2w[:3, 3].copy()

    def project(self, pts: np.ndarray, return_dists: bool = False):
        """Pixel coordinates of world points; same contract as the reference's
        `project_3d_to_2d(pts, w2c, K, return_dists)` (nerf2physic_utils.py:10-23) for a pinhole camera, and the
        camera model's map otherwise (the one the renderer projects Gaussian means with)."""
        pts = np.asarray(pts, dtype=np.float64)
        pc = pts @ self.viewmat()[:3, :3].T + self.viewmat()[:3, 3]
        if self.model == "pinhole":
            uvw = pc @ self.K.T
            uv = uvw[:, :2] / uvw[:, 2:]
            if self.pinhole_distortion is not None and any(self.pinhole_distortion):
                # the lens, and NaN where the renderer culls: past the radial fold, where the map folds, outside the box
                with np.errstate(all="ignore"):
                    xd, yd, det = pinhole_lens_distort(pc[:, 0] / pc[:, 2], pc[:, 1] / pc[:, 2], self.pinhole_distortion)
                    u = (pc[:, 0] / pc[:, 2]) ** 2 + (pc[:, 1] / pc[:, 2]) ** 2
                tanx, tany = 0.5 * self.width / self.fx, 0.5 * self.height / self.fy
                keep = ((pc[:, 2] > 0.0) & (u < pinhole_lens_u_max(self.pinhole_distortion)) & (det > 0.0)
                        & (xd <= (self.width - self.cx) / self.fx + 0.3 * tanx) & (xd >= -(self.cx / self.fx + 0.3 * tanx))
                        & (yd <= (self.height - self.cy) / self.fy + 0.3 * tany) & (yd >= -(self.cy / self.fy + 0.3 * tany)))
                uv = np.where(keep[:, None], np.stack([self.fx * xd + self.cx, self.fy * yd + self.cy], axis=-1), np.nan)
        else:
            xy = pc[:, :2]
            if self.model == "fisheye":       # r = f theta: scale the camera-plane offset by theta / rho
                rho = np.linalg.norm(xy, axis=-1)
                theta = np.arctan2(rho, pc[:, 2])
                safe = np.where(rho > 0, rho, 1.0)
                theta_d = theta
                if self.distortion is not None and any(self.distortion):
                    k1, k2, k3, k4 = self.distortion
                    u = theta * theta
                    theta_d = theta * (1.0 + u * (k1 + u * (k2 + u * (k3 + u * k4))))
                    theta_d = np.where(theta < lens_theta_max(self.distortion), theta_d, np.nan)   # past the fold
                xy = xy * np.where(rho > 0, theta_d / safe, 0.0 * theta_d)[:, None]
            uv = xy * np.array([self.fx, self.fy]) + np.array([self.cx, self.cy])
        if return_dists:
            return uv, np.linalg.norm(pc, axis=-1)
        return uv

    def scaled(self, factor: float) -> "Camera":
        """Same view at a different resolution."""
        return Camera(self.c2w.copy(), self.fx * factor, self.fy * factor,
                      self.cx * factor, self.cy * factor,
                      int(round(self.width * factor)), int(round(self.height * factor)),
                      self.near, self.far, self.model, distortion=self.distortion,
                      pinhole_distortion=self.pinhole_distortion)


def cameras_from_transforms_json(path: str, width: int | None = None,
                                 height: int | None = None, lens_distortion: bool = False,
                                 pinhole_distortion: bool = False) -> List[Camera]:
    """nerfstudio `transforms.json` -> cameras.  Accepts global or per-frame intrinsics,
    the two layouts `parse_transforms_json` reads (nerf2physic_utils.py:30-45).

    nerfstudio's `camera_model` key (top level or per frame): "OPENCV_FISHEYE" is read as the ideal equidistant
    fisheye when its distortion coefficients k1..k4 are absent or zero; non-zero coefficients raise ValueError unless
    lens_distortion=True, which loads them into Camera.distortion (the renderer then applies the lens).  Every other value
    loads as a pinhole camera; the radial / tangential terms k1, k2, k3, p1, p2 of an "OPENCV" frame (per-frame keys over
    top-level ones) are dropped unless pinhole_distortion=True, which loads them into Camera.pinhole_distortion (the
    renderer then applies the lens).  A non-zero k4 under "OPENCV" then raises: the rational model is not built."""
    with open(path, "rb") as f:
        t = json.load(f)
    cams = []
    for fr in t["frames"]:
        src = fr if "fl_x" in fr else t
        w = int(src.get("w", t.get("w", width or round(2 * src["cx"]))))
        h = int(src.get("h", t.get("h", height or round(2 * src["cy"]))))
        model, dist = _transforms_camera_model(fr, t, lens_distortion)
        pdist = _transforms_pinhole_lens(fr, t) if pinhole_distortion and model == "pinhole" else None
        cams.append(Camera(fr["transform_matrix"], src["fl_x"], src["fl_y"], src["cx"],
                           src["cy"], w, h, model=model, distortion=dist, pinhole_distortion=pdist))
    return cams


def _transforms_camera_model(frame: Dict, top: Dict, lens_distortion: bool = False):
    """(Camera.model, Camera.distortion) of one transforms.json frame (per-frame keys override top-level ones)."""
    name = frame.get("camera_model", top.get("camera_model", "OPENCV"))
    if name != "OPENCV_FISHEYE":
        return "pinhole", None
    ks = {k: float(frame.get(k, top.get(k, 0.0))) for k in ("k1", "k2", "k3", "k4")}
    nonzero = {k: v for k, v in ks.items() if v != 0.0}
    if nonzero and not lens_distortion:
        raise ValueError(f"OPENCV_FISHEYE with distortion coefficients {nonzero}: fisheye lens distortion (k1..k4) is "
                         "not supported by default; pass lens_distortion=True to load it into Camera.distortion (without "
                         "it only the ideal equidistant fisheye, all k zero, is read)")
    return "fisheye", (tuple(ks.values()) if nonzero else None)


def _transforms_pinhole_lens(frame: Dict, top: Dict):
    """Camera.pinhole_distortion of one transforms.json frame whose camera_model is "OPENCV" (nerfstudio's default when
    the key is absent): (k1, k2, p1, p2, k3), or None when all are zero or the frame names another pinhole-like model."""
    if frame.get("camera_model", top.get("camera_model", "OPENCV")) != "OPENCV":
        return None
    ks = {k: float(frame.get(k, top.get(k, 0.0))) for k in ("k1", "k2", "p1", "p2", "k3", "k4")}
    if ks.pop("k4") != 0.0:
        raise ValueError("OPENCV with a non-zero k4: the rational model's k4..k6 are not supported (only k1, k2, k3, p1, p2)")
    return tuple(ks.values()) if any(ks.values()) else None


def cameras_from_camera_params_json(path: str) -> Dict[str, Camera]:
    with open(path, "r") as f:
        d = json.load(f)
    return {k: Camera.from_camera_params(v) for k, v in d.items()}


def camera_ring(n: int, width: int, height: int, radius: float = 7.0,
                height_z: float = 1.5, fov_x_deg: float = 60.0,
                thetas: Sequence[float] | None = None) -> List[Camera]:
    """Look-at ring used by every benchmark config: position
    (r cos t, r sin t, h), target origin, world up +Z."""
    if thetas is None:
        thetas = [2.0 * math.pi * k / n for k in range(n)]
    return [Camera.look_at((radius * math.cos(t), radius * math.sin(t), height_z),
                           (0.0, 0.0, 0.0), (0.0, 0.0, 1.0), width, height, fov_x_deg)
            for t in thetas]


def depth_to_distance(depth: np.ndarray, K: np.ndarray) -> np.ndarray:
    """z-depth map -> ray distance, |K^-1 [u,v,1]| * depth at integer pixel (u,v)
    (same contract as nerf2physic_utils.py:120-132)."""
    h, w = depth.shape
    return depth * _ray_norm(h, w, K)


def distance_to_depth(dists: np.ndarray, K: np.ndarray) -> np.ndarray:
    """Inverse of :func:`depth_to_distance` (nerf2physic_utils.py:135-146)."""
    h, w = dists.shape
    return dists / _ray_norm(h, w, K)


def _ray_norm(h: int, w: int, K: np.ndarray) -> np.ndarray:
    Kinv = np.linalg.inv(np.asarray(K, dtype=np.float64))
    u, v = np.meshgrid(np.arange(w, dtype=np.float64), np.arange(h, dtype=np.float64))
    rays = np.stack([u, v, np.ones_like(u)], axis=-1) @ Kinv.T
    return np.linalg.norm(rays, axis=-1)


def unproject_point(pt_2d, depth: np.ndarray, c2w: np.ndarray, K: np.ndarray):
    """Pixel + z-depth map -> world point in the OpenGL camera convention
    (nerf2physic_utils.py:172-185: camera-space ray [x, -y, -1] * depth)."""
    K = np.asarray(K, dtype=np.float64)
    x = (pt_2d[0] - K[0, 2]) / K[0, 0]
    y = (pt_2d[1] - K[1, 2]) / K[1, 1]
    p = np.array([x, -y, -1.0]) * depth[pt_2d[1], pt_2d[0]]
    return (np.asarray(c2w, dtype=np.float64) @ np.append(p, 1.0))[:3]
