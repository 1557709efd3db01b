"""Why a masked tile does not use the unmasked arithmetic of ssim_kernel (loss.hip): how much of the 1e-5 loss gate fp32
rounding alone uses up with it on a frame of one SSIM window (11 x 11, "valid").  That arithmetic restated in NumPy
float32 -- pixels shifted by the value at the tile's centre pixel (the corner (10, 10) of so small a frame), the window
along rows then columns, variances as differences of moments -- against tests/ssim_ref.py in fp64, on near-constant
images (0.5 + 0.01 u) with no mask and under a binary 4 x 4 blob mask with 30 % zeros.  No GPU.  Prints the distribution
of |loss - loss_fp64| / (1e-5 |loss_fp64|) (profiles/rgbd_loss/README.md, section 4).

    python scripts/rgbd_loss_fp32_rounding.py [frames]
"""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tests"))
import ssim_ref as S  # noqa: E402

G = S.window().astype(np.float32)
C1, C2 = np.float32(S.C1), np.float32(S.C2)


def ssim_fp32(x, y, sx, sy):
    """S of the single window of an 11 x 11 plane, every operation rounded to float32."""
    x, y = x.astype(np.float32) - np.float32(sx), y.astype(np.float32) - np.float32(sy)

    def win(a):
        rows = np.zeros(11, np.float32)
        for k in range(11):
            rows = rows + G[k] * a[:, k]
        s = np.float32(0)
        for k in range(11):
            s = s + G[k] * rows[k]
        return s

    mx, my = win(x), win(y)
    vxx, vyy, vxy = win(x * x) - mx * mx, win(y * y) - my * my, win(x * y) - mx * my
    mux, muy = np.float32(sx) + mx, np.float32(sy) + my
    return (2 * mux * muy + C1) * (2 * vxy + C2) / ((mux * mux + muy * muy + C1) * (vxx + vyy + C2))


def main():
    frames = int(sys.argv[1]) if len(sys.argv) > 1 else 300
    rng = np.random.default_rng(1)
    masks = {"binary mask": lambda: (rng.random((3, 3)) >= 0.3).repeat(4, 0).repeat(4, 1)[:11, :11].astype(float),
             "no mask": lambda: np.ones((11, 11))}
    for name, make in masks.items():
        ratios = []
        for _ in range(frames):
            m = make()[..., None]
            if not m.any():
                continue
            c, t = 0.5 + 0.01 * rng.random((11, 11, 3)), 0.5 + 0.01 * rng.random((11, 11, 3))
            x, y = (m * c).astype(np.float32).astype(np.float64), (m * t).astype(np.float32).astype(np.float64)
            ref = S.l1_ssim_np(x, y, 0.2)
            s32 = np.mean([float(ssim_fp32(x[..., k], y[..., k], x[10, 10, k], y[10, 10, k])) for k in range(3)])
            got = 0.8 * np.abs(x - y).mean() + 0.2 * (1 - s32)
            ratios.append(abs(got - ref) / (1e-5 * abs(ref)))
        r = np.array(ratios)
        print(f"{name}: loss error / gate  median {np.median(r):.2f}  90th percentile {np.quantile(r, 0.9):.2f}  "
              f"max {r.max():.2f}  share over the gate {np.mean(r > 1):.2f}")


if __name__ == "__main__":
    main()
