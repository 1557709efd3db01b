"""SSIM / L1 + D-SSIM without a GPU: the fp64 oracle (tests/ssim_ref.py) against independent restatements of
pytorch_msssim ("valid") and the original 3DGS ssim() ("same"), its gradient against finite differences, and the C ABI's
image-loss descriptor (include/mgs.h mgs_image_loss): header, ctypes table and library agree, the size query answers
and every malformed descriptor is refused before anything touches a device."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import ssim_ref as S

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "mgs.h")


def _images(shape, seed):
    return np.random.default_rng(seed).random(shape)


def _msssim_style(x, y):
    """pytorch_msssim._ssim (size_average, data_range 1, K = (0.01, 0.03)): NCHW, the 1D window along H then W as two
    grouped conv2d without padding, per-channel means of the map, then their mean."""
    x = torch.from_numpy(np.moveaxis(x, -1, -3).reshape(-1, x.shape[-1], *x.shape[-3:-1]).copy())
    y = torch.from_numpy(np.moveaxis(y, -1, -3).reshape(-1, y.shape[-1], *y.shape[-3:-1]).copy())
    c = x.shape[1]
    g = torch.from_numpy(S.window())
    wh, ww = g.view(1, 1, -1, 1).repeat(c, 1, 1, 1), g.view(1, 1, 1, -1).repeat(c, 1, 1, 1)
    filt = lambda t: F.conv2d(F.conv2d(t, wh, groups=c), ww, groups=c)
    mu1, mu2 = filt(x), filt(y)
    s1, s2, s12 = filt(x * x) - mu1 ** 2, filt(y * y) - mu2 ** 2, filt(x * y) - mu1 * mu2
    cs = (2 * s12 + S.C2) / (s1 + s2 + S.C2)
    m = (2 * mu1 * mu2 + S.C1) / (mu1 ** 2 + mu2 ** 2 + S.C1) * cs
    return float(m.flatten(2).mean(-1).mean())


def _inria_style(x, y):
    """The original 3DGS utils/loss_utils.ssim: the 2D window (outer product of the 1D one), grouped conv2d with padding
    window_size // 2 (zeros), ssim_map.mean()."""
    x = torch.from_numpy(np.moveaxis(x, -1, -3).reshape(-1, x.shape[-1], *x.shape[-3:-1]).copy())
    y = torch.from_numpy(np.moveaxis(y, -1, -3).reshape(-1, y.shape[-1], *y.shape[-3:-1]).copy())
    c = x.shape[1]
    g = torch.from_numpy(S.window())[:, None]
    win = (g @ g.t())[None, None].expand(c, 1, 11, 11).contiguous()
    filt = lambda t: F.conv2d(t, win, padding=5, groups=c)
    mu1, mu2 = filt(x), filt(y)
    s1, s2, s12 = filt(x * x) - mu1 ** 2, filt(y * y) - mu2 ** 2, filt(x * y) - mu1 * mu2
    m = ((2 * mu1 * mu2 + S.C1) * (2 * s12 + S.C2)) / ((mu1 ** 2 + mu2 ** 2 + S.C1) * (s1 + s2 + S.C2))
    return float(m.mean())


@pytest.mark.parametrize("shape", [(11, 11, 3), (13, 17, 1), (37, 29, 4), (2, 24, 31, 3)])
def test_oracle_matches_pytorch_msssim_and_inria(shape):
    x, y = _images(shape, 1), _images(shape, 2)
    y = 0.6 * x + 0.4 * y                          # correlated, so that S is far from 0
    assert S.ssim_np(x, y, "valid") == pytest.approx(_msssim_style(x, y), rel=1e-12, abs=1e-14)
    assert S.ssim_np(x, y, "same") == pytest.approx(_inria_style(x, y), rel=1e-12, abs=1e-14)
    assert S.ssim_map_np(x, y, "valid").shape[-2:] == (shape[-3] - 10, shape[-2] - 10)
    assert S.ssim_map_np(x, y, "same").shape[-2:] == shape[-3:-1]
    xt, yt = torch.from_numpy(x), torch.from_numpy(y)
    for pad in ("valid", "same"):
        assert float(S.ssim_torch(xt, yt, pad)) == pytest.approx(S.ssim_np(x, y, pad), rel=1e-12)


def test_ssim_of_an_image_with_itself_is_one_exactly():
    for shape in [(11, 11, 1), (20, 33, 3)]:
        x = _images(shape, 3)
        for pad in ("valid", "same"):
            assert np.all(S.ssim_map_np(x, x, pad) == 1.0)
            assert S.ssim_np(x, x, pad) == 1.0
            assert S.l1_ssim_np(x, x, 0.2, pad) == 0.0


@pytest.mark.parametrize("padding", ["valid", "same"])
def test_oracle_gradient_matches_finite_differences(padding):
    x = torch.from_numpy(_images((13, 14, 2), 4)).requires_grad_(True)
    y = torch.from_numpy(0.5 * x.detach().numpy() + 0.5 * _images((13, 14, 2), 5))
    S.l1_ssim_torch(x, y, 0.2, padding).backward()
    g = x.grad.numpy()
    rng = np.random.default_rng(6)
    h = 1e-6
    for idx in [tuple(rng.integers(0, d) for d in x.shape) for _ in range(12)] + [(0, 0, 0), (12, 13, 1), (6, 7, 0)]:
        xp, xm = x.detach().numpy().copy(), x.detach().numpy().copy()
        xp[idx] += h
        xm[idx] -= h
        yy = y.numpy()
        fd = (S.l1_ssim_np(xp, yy, 0.2, padding) - S.l1_ssim_np(xm, yy, 0.2, padding)) / (2 * h)
        assert abs(fd - g[idx]) <= 1e-7 + 1e-5 * abs(g[idx]), (idx, fd, g[idx])


def _decl_args(name):
    src = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    m = re.search(r"\bint\s+" + name + r"\s*\(([^;]*?)\)\s*;", src, flags=re.S)
    return [a.strip() for a in m.group(1).split(",")]


def test_header_table_and_library_agree_on_the_descriptor():
    from robosimgs_amd import _lib
    header = open(HEADER).read()
    assert int(re.search(r"#define\s+MGS_VERSION\s+(\d+)", header).group(1)) == 450 == _lib.MGS_VERSION
    L = _lib.lib()
    assert L.mgs_version() == 450
    for name, nargs in (("mgs_l1_loss_fwd", 8), ("mgs_l1_loss_bwd", 7), ("mgs_l1_loss_fwd_grad", 9)):
        args = _decl_args(name)
        assert len(args) == nargs and args[-1] == "const mgs_image_loss *image", (name, args)
        assert getattr(L, name).argtypes[-1] == ctypes.POINTER(_lib.ImageLoss), name
    assert _decl_args("mgs_l1_loss_bwd_scale") == ["size_t n", "const float *v_loss", "float *v_a", "mgs_stream_t stream"]
    assert int(re.search(r"#define\s+MGS_SSIM_VALID\s+(\d+)", header).group(1)) == _lib.MGS_SSIM_VALID == 0
    assert int(re.search(r"#define\s+MGS_SSIM_SAME\s+(\d+)", header).group(1)) == _lib.MGS_SSIM_SAME == 1
    body = re.search(r"typedef struct mgs_image_loss \{(.*?)\} mgs_image_loss;", header, flags=re.S).group(1)
    fields = re.findall(r"(\w+)\s*[,;]", re.sub(r"/\*.*?\*/", "", body, flags=re.S))
    assert fields == [f for f, _ in _lib.ImageLoss._fields_]
    assert ctypes.sizeof(_lib.ImageLoss) == 24


def _desc(images=1, h=1080, w=1920, ch=3, lam=0.2, padding=0):
    from robosimgs_amd import _lib
    return _lib.ImageLoss(images, h, w, ch, lam, padding)


def test_size_queries_with_a_descriptor_need_no_gpu():
    from robosimgs_amd import _lib
    L = _lib.lib()
    nb = ctypes.c_size_t(0)
    for (images, h, w, ch, pad), tiles in [((1, 1080, 1920, 3, 0), 34 * 60), ((3, 64, 96, 3, 1), 3 * 2 * 3),
                                           ((1, 11, 11, 1, 0), 1), ((2, 5, 7, 4, 1), 2)]:
        n = images * h * w * ch
        d = _desc(images, h, w, ch, 0.2, pad)
        nb.value = 0
        assert L.mgs_l1_loss_fwd(n, None, None, None, None, ctypes.byref(nb), None, ctypes.byref(d)) == 0
        assert nb.value == 2 * 4 * tiles, (images, h, w, ch, nb.value)
        nb.value = 0
        assert L.mgs_l1_loss_fwd_grad(n, None, None, None, None, None, ctypes.byref(nb), None, ctypes.byref(d)) == 0
        assert nb.value == 2 * 4 * tiles
    nb.value = 0                                      # NULL: the plain L1, as before
    assert L.mgs_l1_loss_fwd(100, None, None, None, None, ctypes.byref(nb), None, None) == 0 and nb.value == 4096


@pytest.mark.parametrize("kw,n_delta,msg", [
    (dict(ch=0), 0, b"channels"), (dict(ch=5), 0, b"channels"),
    (dict(h=10, w=20), 0, b"height and width >= 11"), (dict(h=20, w=10), 0, b"height and width >= 11"),
    (dict(lam=-0.1), 0, b"ssim_weight"), (dict(lam=1.5), 0, b"ssim_weight"), (dict(lam=float("nan")), 0, b"ssim_weight"),
    (dict(padding=2), 0, b"padding"), (dict(padding=-1), 0, b"padding"),
    (dict(images=0), 0, b"positive"), (dict(h=0, padding=1), 0, b"positive"),
    (dict(), 1, b"images x height x width x channels"), (dict(), -3, b"images x height x width x channels"),
])
def test_malformed_descriptors_are_refused_without_a_gpu(kw, n_delta, msg):
    from robosimgs_amd import _lib
    L = _lib.lib()
    base = dict(images=2, h=16, w=24, ch=3, lam=0.2, padding=0)
    base.update(kw)
    d = _desc(**base)
    n = max(base["images"], 0) * base["h"] * base["w"] * base["ch"] + n_delta
    nb = ctypes.c_size_t(12345)
    assert L.mgs_l1_loss_fwd(n, None, None, None, None, ctypes.byref(nb), None, ctypes.byref(d)) == -1
    assert msg in L.mgs_last_error_string() and nb.value == 12345
    assert L.mgs_l1_loss_fwd_grad(n, None, None, None, None, None, ctypes.byref(nb), None, ctypes.byref(d)) == -1
    assert msg in L.mgs_last_error_string()
    assert L.mgs_l1_loss_bwd(n, None, None, None, None, None, ctypes.byref(d)) == -1
    assert msg in L.mgs_last_error_string()


def test_python_argument_checks_need_no_gpu():
    from robosimgs_amd import l1_ssim_loss, ssim
    a = torch.rand(16, 16, 3)
    with pytest.raises(ValueError, match="shape mismatch"):
        l1_ssim_loss(a, torch.rand(16, 16, 4))
    with pytest.raises(ValueError, match=">= 11"):
        ssim(torch.rand(10, 16, 3), torch.rand(10, 16, 3))
    with pytest.raises(ValueError, match="padding"):
        ssim(a, a, padding="reflect")
    with pytest.raises(ValueError, match="ssim_lambda"):
        l1_ssim_loss(a, a, ssim_lambda=1.2)
    with pytest.raises(ValueError, match="1 to 4 channels"):
        ssim(torch.rand(16, 16, 5), torch.rand(16, 16, 5))
    from robosimgs_amd._lib import MgsError
    with pytest.raises(MgsError, match="GPU only"):      # a CPU tensor: no fallback
        l1_ssim_loss(a, a)
