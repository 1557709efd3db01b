"""fp64 restatement of the SSIM term of robosimgs_amd.losses (ssim / l1_ssim_loss), in NumPy and in torch.

A helper module of the SSIM tests (not a conftest).  Images are [..., H, W, ch] channel-last, as the renderer returns
them.  Per channel, with the 2D window w(i, j) = g(i) g(j), g(k) = exp(-(k - 5)^2 / 4.5) / sum, taken as a direct 11 x 11
windowed sum (not the separable form the kernel uses):
  mu_x = w * x, sigma_x^2 = w * x^2 - mu_x^2, sigma_xy = w * (x y) - mu_x mu_y,
  S = (2 mu_x mu_y + C1)(2 sigma_xy + C2) / ((mu_x^2 + mu_y^2 + C1)(sigma_x^2 + sigma_y^2 + C2)),  C1 = 0.01^2, C2 = 0.03^2;
padding "valid": S where the window lies inside the image ((H - 10) x (W - 10) positions); "same": the image zero-padded
by 5, S at every pixel.  SSIM = the mean of S over positions, channels and leading dimensions.
"""
from __future__ import annotations

import numpy as np
import torch

R = 5
C1, C2 = 0.01 ** 2, 0.03 ** 2


def window() -> np.ndarray:
    k = np.arange(2 * R + 1, dtype=np.float64) - R
    g = np.exp(-(k * k) / (2 * 1.5 ** 2))
    return g / g.sum()


def _planes(x) -> np.ndarray:
    """[..., H, W, ch] -> [P, H, W] fp64 (P = leading dims x ch)."""
    x = np.asarray(x, dtype=np.float64)
    h, w, ch = x.shape[-3:]
    return np.moveaxis(x.reshape(-1, h, w, ch), -1, 1).reshape(-1, h, w)


def _filter_np(p: np.ndarray, padding: str) -> np.ndarray:
    w2 = np.outer(window(), window())
    if padding == "same":
        p = np.pad(p, ((0, 0), (R, R), (R, R)))
    win = np.lib.stride_tricks.sliding_window_view(p, (2 * R + 1, 2 * R + 1), axis=(1, 2))
    return np.einsum("phwij,ij->phw", win, w2, optimize=True)


def ssim_map_np(x, y, padding: str = "valid") -> np.ndarray:
    """S at every position, [P, H', W'] (P = planes: leading dims x channels)."""
    px, py = _planes(x), _planes(y)
    mx, my = _filter_np(px, padding), _filter_np(py, padding)
    exx, eyy, exy = _filter_np(px * px, padding), _filter_np(py * py, padding), _filter_np(px * py, padding)
    vxx, vyy, vxy = exx - mx * mx, eyy - my * my, exy - mx * my
    return (2 * mx * my + C1) * (2 * vxy + C2) / ((mx * mx + my * my + C1) * (vxx + vyy + C2))


def ssim_np(x, y, padding: str = "valid") -> float:
    return float(ssim_map_np(x, y, padding).mean())


def l1_ssim_np(x, y, ssim_lambda: float = 0.2, padding: str = "valid") -> float:
    l1 = float(np.abs(np.asarray(x, np.float64) - np.asarray(y, np.float64)).mean())
    return (1 - ssim_lambda) * l1 + ssim_lambda * (1 - ssim_np(x, y, padding))


def _planes_torch(x: torch.Tensor) -> torch.Tensor:
    h, w, ch = x.shape[-3:]
    return x.reshape(-1, h, w, ch).permute(0, 3, 1, 2).reshape(-1, 1, h, w)


def ssim_torch(x: torch.Tensor, y: torch.Tensor, padding: str = "valid") -> torch.Tensor:
    """The same in torch at x's dtype (fp64 for the gradient oracle): a direct 11 x 11 conv2d per plane."""
    w2 = torch.from_numpy(np.outer(window(), window())).to(x.device, x.dtype)[None, None]
    pad = R if padding == "same" else 0
    f = lambda t: torch.nn.functional.conv2d(t, w2, padding=pad)
    px, py = _planes_torch(x), _planes_torch(y)
    mx, my = f(px), f(py)
    vxx, vyy, vxy = f(px * px) - mx * mx, f(py * py) - my * my, f(px * py) - mx * my
    s = (2 * mx * my + C1) * (2 * vxy + C2) / ((mx * mx + my * my + C1) * (vxx + vyy + C2))
    return s.mean()


def l1_ssim_torch(x: torch.Tensor, y: torch.Tensor, ssim_lambda: float = 0.2, padding: str = "valid") -> torch.Tensor:
    return (1 - ssim_lambda) * (x - y).abs().mean() + ssim_lambda * (1 - ssim_torch(x, y, padding))
