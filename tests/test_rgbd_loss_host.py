"""rgbd_loss without a GPU: the fp64 reference (tests/rgbd_loss_ref.py) against ssim_ref where the two coincide, its
gradient against finite differences, its select semantics, and the C ABI of include/mgs_loss_rgbd.h: header, ctypes
table and library agree, the size queries answer and every malformed call is refused before anything touches a device."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

import rgbd_loss_ref as R
import ssim_ref as S

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "mgs_loss_rgbd.h")
ENTRY_POINTS = ("mgs_rgbd_loss_fwd", "mgs_rgbd_loss_fwd_grad", "mgs_rgbd_loss_bwd")


def _scene(shape=(13, 14), seed=0):
    """render [.., 4], target_rgb, target_depth (a NaN and a 0 in it), a soft mask with zeros."""
    rng = np.random.default_rng(seed)
    render = rng.random(shape + (4,))
    render[..., 3] = 1.0 + 2.0 * render[..., 3]
    target = 0.5 * render[..., :3] + 0.5 * rng.random(shape + (3,))
    depth = 1.0 + 2.0 * rng.random(shape)
    depth[..., 2, 3] = np.nan
    depth[..., 4, 5] = 0.0
    mask = rng.random(shape)
    mask[mask < 0.3] = 0.0
    return render, target, depth, mask


@pytest.mark.parametrize("padding", ["valid", "same"])
def test_reference_is_ssim_ref_at_trivial_inputs(padding):
    render, target, _, _ = _scene((2, 15, 16), 1)
    want = S.l1_ssim_np(render[..., :3], target, 0.2, padding)
    for m in (None, np.ones(render.shape[:-1])):
        got, terms = R.rgbd_loss_np(render[..., :3], target, None, m, 0.2, 0.0, padding)
        assert got == pytest.approx(want, rel=1e-12)
        assert terms[1] == pytest.approx(S.ssim_np(render[..., :3], target, padding), rel=1e-12) and terms[2:] == (0.0, 0.0)
        t = R.rgbd_loss_torch(torch.from_numpy(render[..., :3].copy()), torch.from_numpy(target), None,
                              None if m is None else torch.from_numpy(m), 0.2, 0.0, padding)[0]
        assert float(t) == pytest.approx(want, rel=1e-12)


@pytest.mark.parametrize("padding", ["valid", "same"])
def test_reference_gradient_matches_finite_differences(padding):
    render, target, depth, mask = _scene()
    x = torch.from_numpy(render.copy()).requires_grad_(True)
    loss, terms = R.rgbd_loss_torch(x, torch.from_numpy(target), torch.from_numpy(depth), torch.from_numpy(mask), 0.2, 0.5, padding)
    loss.backward()
    g = x.grad.numpy()
    l_np, t_np = R.rgbd_loss_np(render, target, depth, mask, 0.2, 0.5, padding)
    assert float(loss.detach()) == pytest.approx(l_np, rel=1e-12)
    assert [float(v) for v in terms] == pytest.approx(list(t_np), rel=1e-12)
    rng = np.random.default_rng(6)
    h = 1e-6
    picks = [tuple(rng.integers(0, d) for d in render.shape) for _ in range(16)]
    picks += [(0, 0, 0), (12, 13, 3), (6, 7, 1), (2, 3, 3), (4, 5, 3), (5, 5, 3)]
    picks += [tuple(np.argwhere(mask == 0)[0]) + (c,) for c in (0, 3)]
    for idx in picks:
        rp, rm = render.copy(), render.copy()
        rp[idx] += h
        rm[idx] -= h
        fd = (R.rgbd_loss_np(rp, target, depth, mask, 0.2, 0.5, padding)[0]
              - R.rgbd_loss_np(rm, target, depth, mask, 0.2, 0.5, padding)[0]) / (2 * h)
        assert abs(fd - g[idx]) <= 1e-7 + 1e-5 * abs(g[idx]), (idx, fd, g[idx])
    assert g[2, 3, 3] == 0 and g[4, 5, 3] == 0                       # d* NaN, d* 0: no weight
    assert not g[mask == 0].any()


def test_select_semantics_keep_non_finite_values_out():
    render, target, depth, mask = _scene()
    base, base_terms = R.rgbd_loss_np(render, target, depth, mask, 0.2, 0.5)
    x0 = torch.from_numpy(render.copy()).requires_grad_(True)
    R.rgbd_loss_torch(x0, torch.from_numpy(target), torch.from_numpy(depth), torch.from_numpy(mask), 0.2, 0.5)[0].backward()
    off = mask == 0
    render[off] = np.inf
    render[off, 1] = np.nan
    target[off] = -np.inf
    depth[off] = np.nan
    got, terms = R.rgbd_loss_np(render, target, depth, mask, 0.2, 0.5)
    assert np.isfinite(got) and got == base and terms == base_terms
    x = torch.from_numpy(render.copy()).requires_grad_(True)
    loss, _ = R.rgbd_loss_torch(x, torch.from_numpy(target), torch.from_numpy(depth), torch.from_numpy(mask), 0.2, 0.5)
    loss.backward()
    assert float(loss.detach()) == pytest.approx(base, rel=1e-12)
    assert torch.isfinite(x.grad).all() and not x.grad.numpy()[off].any()
    assert torch.equal(x.grad, x0.grad)


def test_no_weight_means_no_depth_term():
    render, target, depth, mask = _scene()
    colour = R.rgbd_loss_np(render, target, None, mask, 0.2, 0.0)[0]
    for dt, m in ((np.full_like(depth, np.nan), mask), (np.zeros_like(depth), None), (depth, np.zeros_like(mask))):
        want = colour if m is mask else R.rgbd_loss_np(render, target, None, m, 0.2, 0.0)[0]
        got, terms = R.rgbd_loss_np(render, target, dt, m, 0.2, 0.5)
        assert got == want and terms[2:] == (0.0, 0.0)
        x = torch.from_numpy(render.copy()).requires_grad_(True)
        loss, tt = R.rgbd_loss_torch(x, torch.from_numpy(target), torch.from_numpy(dt), None if m is None else torch.from_numpy(m),
                                     0.2, 0.5)
        loss.backward()
        assert float(tt[2]) == 0.0 and float(tt[3]) == 0.0 and not x.grad[..., 3].any()


# ---- header, ctypes and library ---------------------------------------------------------------------------------------
def _decl_args(name):
    src = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    m = re.search(r"\bint\s+" + name + r"\s*\(([^;]*?)\)\s*;", src, flags=re.S)
    return [" ".join(a.split()) for a in m.group(1).split(",")]


def _ctype_of(arg):
    from robosimgs_amd import _lib
    if arg.startswith("const mgs_rgbd_loss *"):
        return ctypes.POINTER(_lib.RgbdLoss)
    if arg.startswith("size_t *"):
        return ctypes.POINTER(ctypes.c_size_t)
    assert "*" in arg or arg.startswith("mgs_stream_t "), arg
    return ctypes.c_void_p


def test_header_table_and_library_agree():
    from robosimgs_amd import _lib
    L = _lib.lib()
    assert L.mgs_version() == 450 == _lib.MGS_VERSION
    header = open(HEADER).read()
    body = re.search(r"typedef struct mgs_rgbd_loss \{(.*?)\} mgs_rgbd_loss;", header, flags=re.S).group(1)
    decls = re.findall(r"(int|float)\s+([\w\s,]+);", re.sub(r"/\*.*?\*/", "", body, flags=re.S))
    fields = [(n.strip(), ctypes.c_int if t == "int" else ctypes.c_float) for t, names in decls for n in names.split(",")]
    assert fields == list(_lib.RgbdLoss._fields_)
    assert ctypes.sizeof(_lib.RgbdLoss) == 28
    assert list(_lib.RGBD_LOSS_EXPORTS) == list(ENTRY_POINTS)
    common = ["const mgs_rgbd_loss *desc", "const float *render", "const float *target_rgb", "const float *target_depth",
              "const float *mask"]
    tail = ["void *workspace", "size_t *workspace_bytes", "mgs_stream_t stream"]
    want = {"mgs_rgbd_loss_fwd": common + ["float *loss", "float *terms"] + tail,
            "mgs_rgbd_loss_fwd_grad": common + ["float *loss", "float *terms", "float *v_render"] + tail,
            "mgs_rgbd_loss_bwd": common + ["const float *v_loss", "float *v_render"] + tail}
    for name in ENTRY_POINTS:
        args = _decl_args(name)
        assert args == want[name], (name, args)
        fn = getattr(L, name)
        assert fn.argtypes == [_ctype_of(a) for a in args] and fn.restype == ctypes.c_int, name


def _desc(images=2, h=16, w=24, cr=4, lam=0.2, padding=0, lam_d=0.0):
    from robosimgs_amd import _lib
    return _lib.RgbdLoss(images, h, w, cr, lam, padding, lam_d)


def _calls(L, d, nb, render=None, target=None, depth=None, mask=None, out=None, ws=None):
    """The three entry points on the same arguments (`out` stands for loss, v_render and v_loss)."""
    dp, nbp = (ctypes.byref(d) if d is not None else None), (ctypes.byref(nb) if nb is not None else None)
    yield "fwd", L.mgs_rgbd_loss_fwd(dp, render, target, depth, mask, out, None, ws, nbp, None)
    yield "fwd_grad", L.mgs_rgbd_loss_fwd_grad(dp, render, target, depth, mask, out, None, out, ws, nbp, None)
    yield "bwd", L.mgs_rgbd_loss_bwd(dp, render, target, depth, mask, out, out, ws, nbp, None)


def test_size_queries_need_no_gpu():
    from robosimgs_amd import _lib
    L = _lib.lib()
    for (images, h, w, cr, pad, lam_d), tiles in [((1, 1080, 1920, 4, 0, 0.5), 34 * 60), ((3, 64, 96, 3, 1, 0.0), 3 * 2 * 3),
                                                   ((1, 11, 11, 4, 0, 0.0), 1), ((2, 5, 7, 4, 1, 2.0), 2)]:
        nb = ctypes.c_size_t(0)
        for what, rc in _calls(L, _desc(images, h, w, cr, 0.2, pad, lam_d), nb):
            assert rc == 0 and nb.value == 4 * (5 * tiles + 256), (what, rc, nb.value)
            nb.value = 0


@pytest.mark.parametrize("kw,msg", [
    (dict(cr=2), b"render_channels"), (dict(cr=5), b"render_channels"), (dict(cr=0), b"render_channels"),
    (dict(lam_d=-0.5), b"depth_weight"), (dict(lam_d=float("nan")), b"depth_weight"), (dict(lam_d=float("inf")), b"depth_weight"),
    (dict(cr=3, lam_d=0.5), b"needs render_channels == 4"),
    # what ssim_plan refuses
    (dict(h=10, w=20), b"height and width >= 11"), (dict(h=20, w=10), b"height and width >= 11"),
    (dict(lam=-0.1), b"ssim_weight"), (dict(lam=1.5), b"ssim_weight"), (dict(lam=float("nan")), b"ssim_weight"),
    (dict(padding=2), b"padding"), (dict(padding=-1), b"padding"),
    (dict(images=0), b"positive"), (dict(h=0, padding=1), b"positive"), (dict(w=-3, padding=1), b"positive"),
])
def test_malformed_descriptors_are_refused_without_a_gpu(kw, msg):
    from robosimgs_amd import _lib
    L = _lib.lib()
    nb = ctypes.c_size_t(12345)
    for what, rc in _calls(L, _desc(**kw), nb):
        assert rc == -1 and msg in L.mgs_last_error_string() and nb.value == 12345, (what, rc, L.mgs_last_error_string())


def test_null_pointers_and_small_workspaces_are_refused_without_a_gpu():
    """Past the size query: the pointers below are never followed, every call ends before a launch."""
    from robosimgs_amd import _lib
    L = _lib.lib()
    fake = ctypes.c_void_p(4096)                       # stands for a device buffer
    for what, rc in _calls(L, None, ctypes.c_size_t(0)):
        assert rc == -1 and b"desc is null" in L.mgs_last_error_string(), what
    for what, rc in _calls(L, _desc(), None):
        assert rc == -1 and b"workspace_bytes is null" in L.mgs_last_error_string(), what
    need = 4 * (5 * 2 + 256)
    for what, rc in _calls(L, _desc(), ctypes.c_size_t(need - 1), fake, fake, None, None, fake, fake):
        assert rc == -2 and b"workspace" in L.mgs_last_error_string(), what
    for missing in ("render", "target", "out"):
        a = dict(render=fake, target=fake, out=fake)
        a[missing] = None
        for what, rc in _calls(L, _desc(), ctypes.c_size_t(need), depth=None, mask=None, ws=fake, **a):
            assert rc == -1 and b"null pointer" in L.mgs_last_error_string(), (missing, what)
    for what, rc in _calls(L, _desc(lam_d=0.5), ctypes.c_size_t(need), fake, fake, None, fake, fake, fake):
        assert rc == -1 and b"needs target_depth" in L.mgs_last_error_string(), what


def test_python_argument_checks_need_no_gpu():
    from robosimgs_amd import rgbd_loss
    from robosimgs_amd._lib import MgsError
    r4, t3 = torch.rand(16, 16, 4), torch.rand(16, 16, 3)
    with pytest.raises(ValueError, match="shape mismatch"):
        rgbd_loss(r4, torch.rand(16, 16, 4))
    with pytest.raises(ValueError, match="shape mismatch"):
        rgbd_loss(r4, t3, target_depth=torch.rand(16, 15), depth_lambda=0.5)
    with pytest.raises(ValueError, match="shape mismatch: mask"):
        rgbd_loss(r4, t3, mask=torch.rand(16, 16, 1))
    with pytest.raises(ValueError, match="four-channel"):
        rgbd_loss(r4[..., :3], t3, target_depth=torch.rand(16, 16), depth_lambda=0.5)
    with pytest.raises(ValueError, match="needs target_depth"):
        rgbd_loss(r4, t3, depth_lambda=0.5)
    with pytest.raises(ValueError, match="depth_lambda"):
        rgbd_loss(r4, t3, target_depth=torch.rand(16, 16), depth_lambda=-1.0)
    with pytest.raises(ValueError, match=">= 11"):
        rgbd_loss(r4[:10], t3[:10])
    with pytest.raises(ValueError, match="render must be"):
        rgbd_loss(torch.rand(16, 16, 2), torch.rand(16, 16, 2))
    with pytest.raises(MgsError, match="GPU only"):
        rgbd_loss(r4, t3)
