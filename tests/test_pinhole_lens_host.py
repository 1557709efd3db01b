"""Pinhole lens distortion (OpenCV k1 k2 p1 p2 k3; include/mgs_lens_pinhole.h MGS_CAMERA_PINHOLE_BC) on the host: the fp64
reference (tests/pinhole_lens_ref.py) against autograd of its own mean map and against hand-computed values, the radial
fold, Camera / loader / keyword handling and every refusal, the C ABI's argument checks, and the per-Gaussian DEVICE math
(robosimgs_amd/csrc/mgs_math.h, project_gaussian<MGS_CAMERA_PINHOLE_BC> and its backward, compiled with g++:
tests/host_harness/pinhole_lens.cpp) against that reference through the unchanged oracle -- forward rows, backward against
fp64 autograd, on the optical axis, at the box's border and up to the folds -- plus an address / undefined-behaviour
sanitizer build of the stand-alone harness."""
import ctypes
import dataclasses
import json
import math
import os
import re
import subprocess

import numpy as np
import pytest
import torch

import pinhole_lens_ref as PR
from oracle import camera_models as CM
from oracle import gs_oracle_np as O
from oracle import gs_oracle_torch as OT
from robosimgs_amd import Camera, cameras_from_transforms_json
from test_host_camera_models import _check_forward, _close, _f, _p

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
LENSES = dict(PR.LENSES, zero=(0.0, 0.0, 0.0, 0.0, 0.0))
FX, FY, CX, CY = 81.5, 84.0, 58.25, 38.6
W, H = PR.W, PR.H


# ---- the reference itself ------------------------------------------------------------------------------------------
def _points():
    """Random camera points out to |(x', y')| = 1.2, in front of the camera, and the optical axis."""
    rng = np.random.default_rng(0)
    r, phi, z = rng.uniform(0.0, 1.2, 200), rng.uniform(0, 2 * math.pi, 200), rng.uniform(0.3, 9.0, 200)
    pts = [np.stack([z * r * np.cos(phi), z * r * np.sin(phi), z], axis=-1)]
    for zz in (0.4, 1.0, 6.0):
        pts.append(np.array([[0.0, 0.0, zz]]))
    return np.concatenate(pts)


@pytest.mark.parametrize("lens", list(LENSES))
def test_reference_jacobian_is_autograd_of_its_mean_map(lens):
    k = LENSES[lens]
    pts = torch.tensor(_points())
    _, J = PR.mean_and_J(pts[:, 0], pts[:, 1], pts[:, 2], FX, FY, CX, CY, k, torch)
    J = torch.stack(J, dim=-1).reshape(-1, 2, 3)

    def mean_map(p):
        mu, _ = PR.mean_and_J(p[0:1], p[1:2], p[2:3], FX, FY, CX, CY, k, torch)
        return torch.cat(mu)
    worst = 0.0
    for i in range(len(pts)):
        Ja = torch.autograd.functional.jacobian(mean_map, pts[i])
        worst = max(worst, float((J[i] - Ja).abs().max() / Ja.abs().max()))
    print(f"\n{lens}: worst relative error of the closed-form J against autograd over {len(pts)} points: {worst:.2e}")
    assert worst <= 1e-12


def test_hand_computed_values():
    """(x', y') = (0.5, -0.25) under (k1, k2, p1, p2, k3) = (-0.2, 0.05, 0.01, -0.02, 0.001), by hand:
    u = 0.3125, Rad = 1 - 0.0625 + 0.0048828125 + 0.000030517578125 = 0.942413330078125,
    xd = 0.5 Rad + 2 (0.01)(-0.125) - 0.02 (0.3125 + 0.5) = 0.4712066650390625 - 0.0025 - 0.01625,
    yd = -0.25 Rad + 0.01 (0.3125 + 0.125) + 2 (-0.02)(-0.125) = -0.23560333251953125 + 0.004375 + 0.005."""
    k = (-0.2, 0.05, 0.01, -0.02, 0.001)
    xd, yd, (d00, d01, d11), u = PR.distort(np.array([0.5]), np.array([-0.25]), k)
    assert u[0] == 0.3125
    assert abs(xd[0] - 0.4524566650390625) < 1e-15 and abs(yd[0] - (-0.22622833251953125)) < 1e-15
    # Rad1 = -0.2 + 2 (0.05)(0.3125) + 3 (0.001)(0.09765625) = -0.16845703125
    rad, rad1 = 0.942413330078125, -0.16845703125
    assert abs(d00[0] - (rad + 0.5 * rad1 + 2 * 0.01 * -0.25 + 6 * -0.02 * 0.5)) < 1e-15
    assert abs(d01[0] - (2 * 0.5 * -0.25 * rad1 + 2 * 0.01 * 0.5 + 2 * -0.02 * -0.25)) < 1e-15
    assert abs(d11[0] - (rad + 2 * 0.0625 * rad1 + 6 * 0.01 * -0.25 + 2 * -0.02 * 0.5)) < 1e-15
    # purely radial, on the x axis: xd = r (1 + k1 r^2), d00 = 1 + 3 k1 r^2 (zero at the fold), d11 = 1 + k1 r^2
    r = math.sqrt(1.0 / 1.05)
    xd, yd, (d00, d01, d11), _ = PR.distort(np.array([r]), np.array([0.0]), (-0.35, 0, 0, 0, 0))
    assert abs(xd[0] - r * (1 - 0.35 / 1.05)) < 1e-15 and yd[0] == 0 and abs(d00[0]) < 1e-15 and abs(d11[0] - 2.0 / 3.0) < 1e-15
    mu, J = PR.mean_and_J(np.array([1.0]), np.array([-0.5]), np.array([2.0]), 100.0, 50.0, 7.0, 9.0, k, np)
    assert abs(mu[0][0] - (100 * 0.4524566650390625 + 7)) < 1e-12 and abs(mu[1][0] - (50 * -0.22622833251953125 + 9)) < 1e-12


def test_zero_coefficients_are_the_pinhole_map_exactly():
    p = _points()
    mu, J = PR.mean_and_J(p[:, 0], p[:, 1], p[:, 2], FX, FY, CX, CY, (0, 0, 0, 0, 0), np)
    assert np.array_equal(mu[0], FX * (p[:, 0] / p[:, 2]) + CX) and np.array_equal(mu[1], FY * (p[:, 1] / p[:, 2]) + CY)
    xd, yd, (d00, d01, d11), _ = PR.distort(p[:, 0] / p[:, 2], p[:, 1] / p[:, 2], (0, 0, 0, 0))
    assert np.array_equal(xd, p[:, 0] / p[:, 2]) and np.array_equal(yd, p[:, 1] / p[:, 2])
    assert np.all(d00 == 1) and np.all(d01 == 0) and np.all(d11 == 1)
    np.testing.assert_allclose(J[2], -FX * p[:, 0] / p[:, 2] ** 2, rtol=1e-15)
    with PR.lens((0, 0, 0, 0, 0), W, H) as umax:       # and through the patch: other models pass through, nothing folds
        assert umax == math.inf
        assert O.mean_and_J(p[:, 0], p[:, 1], p[:, 2], FX, FY, CX, CY, "ortho", np)[0][0][0] == FX * p[0, 0] + CX
    assert O.mean_and_J is CM.mean_and_J and OT.mean_and_J is CM.mean_and_J


def test_u_max():
    """The product's radial fold (polynomial roots) is the reference's (scan and bisection), for lenses whose
    1 + 3 k1 u + 5 k2 u^2 + 7 k3 u^3 has zero, one and two positive roots."""
    from robosimgs_amd.camera import pinhole_lens_u_max
    assert abs(PR.u_max(PR.FOLDING) - 1.0 / 1.05) < 1e-15 and abs(PR.u_max(PR.MILD) - 4.2989) < 1e-4
    none = [(0, 0, 0, 0, 0), (0.1, 0.02, 0.01, 0.01, 0.003), (0.0, 0.0, 0.3, -0.2, 0.0), (-0.1, 0.2, 0, 0, 0)]
    one = [PR.FOLDING, (-0.35, 0, 0, 0), (0.1, 0.0, 0.0, 0.0, -0.01), PR.MILD]
    two = [(-0.5, 0.1, 0.0, 0.0, 0.0), (-0.5, 0.1, 0.004, -0.003, 0.0)]   # 1 - 1.5 u + 0.5 u^2 = 0 at u = 1 and u = 2
    assert abs(PR.u_max(two[0]) - 1.0) < 1e-14
    none.append((-0.4, 0.1, 0.0, 0.0, 0.0))                               # 1 - 1.2 u + 0.5 u^2: no real root
    for k in none:
        assert PR.u_max(k) == math.inf and pinhole_lens_u_max(PR.full(k)) == math.inf, k
    for k in one + two:
        ref = PR.u_max(k)
        assert math.isfinite(ref) and abs(pinhole_lens_u_max(PR.full(k)) - ref) <= 1e-12 * ref, k
    roots = np.roots([0.5, -1.5, 1.0])
    assert (np.abs(roots.imag) < 1e-12).all() and (roots.real > 0).all()          # `two` has two positive roots indeed
    assert sum(1 for r in np.roots([7 * -0.004, 5 * 0.03, 3 * -0.12, 1.0]) if abs(r.imag) < 1e-12 and r.real > 0) == 1


def test_uniform_scenes_stay_under_the_near_flip_cap():
    """The fp64 reference alone: the scenes the GPU tests use lose at most 2 % to the near-flip filter, keep Gaussians on
    both sides of every cull and hold the planted ones where they were planted."""
    for lens in PR.LENSES:
        for n, deg in ((2000, 0), (1500, 3), (600, 0)):
            g, vm, K, info = PR.scene(lens, n, deg)
            assert info["removed"] <= PR.FLIP_CAP * n and len(g) == n - info["removed"]
            pc = PR.camera_points(g.means, vm)
            front = pc[:, 2] > PR.NEAR
            culled, margin = PR.cull_margins(pc[front, 0], pc[front, 1], pc[front, 2], K[0, 0], K[1, 1], K[0, 2], K[1, 2],
                                             PR.LENSES[lens], W, H)
            assert margin.min() >= PR.FLIP_MARGIN
            assert culled.sum() > n // 10 and (~culled).sum() > n // 4
            full = np.zeros(len(g), bool)
            full[np.flatnonzero(front)] = culled
            for cull, (inside, outside) in info["where"].items():
                assert len(inside) >= 8 and len(outside) >= 8
                assert not full[inside].any() and full[outside].all(), (lens, cull)
    assert set(PR.PLANTED_CULLS["mild"]) | set(PR.PLANTED_CULLS["folding"]) == {"fold", "det", "box"}
    # the tangential fold is live before the radial one under FOLDING: a share of the disc u < u_max has det Jd <= 0
    rng = np.random.default_rng(1)
    r, phi = np.sqrt(rng.uniform(0, PR.u_max(PR.FOLDING), 200_000)), rng.uniform(0, 2 * math.pi, 200_000)
    _, _, (d00, d01, d11), _ = PR.distort(r * np.cos(phi), r * np.sin(phi), PR.FOLDING)
    share = float((d00 * d11 - d01 * d01 <= 0).mean())
    assert 0.004 < share < 0.009, share


# ---- Camera, loader, keywords --------------------------------------------------------------------------------------
def _camera(pinhole_distortion, model="pinhole", f=50.0):
    c2w = np.eye(4)
    c2w[:3, :3] = np.array([[0.8, -0.6, 0.0], [0.6, 0.8, 0.0], [0.0, 0.0, 1.0]])
    c2w[:3, 3] = (0.3, -0.2, 0.5)
    return Camera(c2w, f, f, PR.CX, PR.CY, W, H, model=model, pinhole_distortion=pinhole_distortion)


def test_camera_project_applies_the_lens():
    rng = np.random.default_rng(3)
    pts = rng.uniform(-3, 3, size=(600, 3))
    for name, k in PR.LENSES.items():
        cam = _camera(k, f=PR.FOCAL[name])
        vm = cam.viewmat()
        pc = pts @ vm[:3, :3].T + vm[:3, 3]
        front = pc[:, 2] > 0.01
        culled = np.ones(len(pts), bool)
        culled[front], _ = PR.cull_margins(pc[front, 0], pc[front, 1], pc[front, 2], cam.fx, cam.fy, cam.cx, cam.cy, k, W, H)
        inside = front & ~culled
        assert inside.sum() > 30 and (front & culled).sum() > 30
        uv = cam.project(pts)
        mu, _ = PR.mean_and_J(pc[inside, 0], pc[inside, 1], pc[inside, 2], cam.fx, cam.fy, cam.cx, cam.cy, k, np)
        np.testing.assert_allclose(uv[inside], np.stack(mu, axis=-1), rtol=1e-12, atol=1e-10)
        assert np.isnan(uv[front & culled]).all()
        assert cam.scaled(0.5).pinhole_distortion == tuple(k) and cam.scaled(0.5).model == "pinhole"
    plain = _camera(None).project(pts)
    assert np.array_equal(_camera((0, 0, 0, 0, 0)).project(pts), plain)
    cam = _camera(PR.FOLDING)
    assert dataclasses.replace(cam, cx=1.0).pinhole_distortion == PR.FOLDING and dataclasses.replace(cam, cx=1.0).cx == 1.0
    assert "pinhole_distortion" in [f.name for f in dataclasses.fields(Camera)] and "pinhole_distortion=(-0.35" in repr(cam)
    assert list(Camera.__dataclass_fields__)[-1] == "model"
    assert _camera((0.1, 0.02, 0.001, 0.002)).pinhole_distortion == (0.1, 0.02, 0.001, 0.002, 0.0)      # [4]: k3 = 0
    for model in ("fisheye", "ortho"):
        with pytest.raises(ValueError, match="pinhole"):
            _camera(PR.MILD, model=model)
    with pytest.raises(ValueError):
        _camera((0.1, 0.2))
    with pytest.raises(ValueError):
        _camera((0.1, 0.2, 0.0, 0.0, float("nan")))
    with pytest.raises(TypeError):            # keyword-only
        Camera(np.eye(4), 1, 1, 0, 0, 4, 4, 0.01, 1e10, "pinhole", PR.MILD)


def _write(tmp_path, top, frame_extra=None):
    frame = dict({"file_path": "a.png", "transform_matrix": np.eye(4).tolist()}, **(frame_extra or {}))
    doc = dict({"fl_x": 300.0, "fl_y": 301.0, "cx": 160.0, "cy": 120.0, "w": 320, "h": 240, "frames": [frame]}, **top)
    path = tmp_path / "transforms.json"
    path.write_text(json.dumps(doc))
    return str(path)


def test_loader_reads_the_lens_only_when_asked(tmp_path):
    cal = {"camera_model": "OPENCV", "k1": -0.12, "k2": 0.03, "k3": -0.004, "p1": 0.002, "p2": -0.0015}
    path = _write(tmp_path, cal)
    for kw in ({}, {"lens_distortion": True}, {"pinhole_distortion": False}):
        cams = cameras_from_transforms_json(path, **kw)
        assert cams[0].model == "pinhole" and cams[0].pinhole_distortion is None and cams[0].distortion is None
    cams = cameras_from_transforms_json(path, pinhole_distortion=True)
    assert cams[0].model == "pinhole" and cams[0].pinhole_distortion == PR.MILD
    del cal["camera_model"]                                  # nerfstudio's default camera_model is OPENCV
    assert cameras_from_transforms_json(_write(tmp_path, cal), pinhole_distortion=True)[0].pinhole_distortion == PR.MILD
    cams = cameras_from_transforms_json(_write(tmp_path, cal, {"k1": -0.35, "k3": 0.0}), pinhole_distortion=True)
    assert cams[0].pinhole_distortion == (-0.35, 0.03, 0.002, -0.0015, 0.0)          # per-frame keys over top-level ones
    cams = cameras_from_transforms_json(_write(tmp_path, {"camera_model": "OPENCV"}), pinhole_distortion=True)
    assert cams[0].pinhole_distortion is None
    with pytest.raises(ValueError, match="k4"):
        cameras_from_transforms_json(_write(tmp_path, {"camera_model": "OPENCV", "k1": 0.1, "k4": 0.01}), pinhole_distortion=True)
    assert cameras_from_transforms_json(_write(tmp_path, {"camera_model": "OPENCV", "k1": 0.1, "k4": 0.01}))[0].model == "pinhole"
    fish = {"camera_model": "OPENCV_FISHEYE", "k1": -0.04, "k2": 0.012, "k3": -0.006, "k4": 0.0015}
    cams = cameras_from_transforms_json(_write(tmp_path, fish), lens_distortion=True, pinhole_distortion=True)
    assert cams[0].model == "fisheye" and cams[0].pinhole_distortion is None and cams[0].distortion is not None


def test_keyword_handling_and_refusals():
    from robosimgs_amd import FrameRenderer, ops, rasterization
    assert ops.camera_model_id("pinhole") == ops.camera_model_id("pinhole", None, None) == 0
    assert ops.camera_model_id("pinhole", None, (0, 0, 0, 0, 0)) == ops.camera_model_id("pinhole", None, np.zeros((3, 5))) == 0
    assert ops.camera_model_id("pinhole", None, PR.MILD) == ops.camera_model_id("pinhole", None, [PR.MILD, (0,) * 5]) == 4
    assert ops.camera_model_id("pinhole", None, (0.1, 0.0, 0.0, 0.0)) == 4                       # [4]: k3 = 0
    k = ops.pinhole_lens_coefficients((0.1, 0.2, 0.3, 0.4))
    assert k.shape == (1, 5) and k[0, 4] == 0.0 and ops.pinhole_lens_coefficients(np.zeros(5)) is None
    for model in ("fisheye", "ortho"):
        for lens in (PR.MILD, (0, 0, 0, 0, 0)):
            with pytest.raises(ValueError, match="pinhole"):
                ops.camera_model_id(model, None, lens)
    with pytest.raises(ValueError, match="one of them"):
        ops.camera_model_id("pinhole", (0.1, 0, 0, 0), PR.MILD)
    with pytest.raises(ValueError, match="one of them"):
        ops.camera_model_id("fisheye", (0.1, 0, 0, 0), PR.MILD)
    with pytest.raises(ValueError, match="fisheye"):           # distortion= keeps its meaning and its error
        ops.camera_model_id("pinhole", (0.1, 0, 0, 0))
    with pytest.raises(ValueError, match=r"\[5\] or \[C,5\]"):
        ops.camera_model_id("pinhole", None, (0.1, 0.2, 0.3))
    with pytest.raises(ValueError, match=r"\[5\] or \[C,5\]"):
        ops.pinhole_lens_coefficients(np.zeros((2, 5)), 3)
    with pytest.raises(ValueError, match="finite"):
        ops.camera_model_id("pinhole", None, (0.1, float("inf"), 0, 0, 0))
    z = torch.zeros(4, 3)
    args = (z, torch.zeros(4, 4), z, torch.zeros(4), torch.zeros(4, 1, 3), torch.eye(4)[None], torch.eye(3)[None], 32, 32)
    with pytest.raises(ValueError, match="pinhole"):           # checked before anything touches a device
        rasterization(*args, sh_degree=0, camera_model="fisheye", pinhole_distortion=PR.MILD)
    with pytest.raises(ValueError, match="one of them"):
        rasterization(*args, sh_degree=0, distortion=(0.1, 0, 0, 0), pinhole_distortion=PR.MILD)
    with pytest.raises(ValueError, match="dataset"):
        rasterization(*args, sh_degree=0, render_mode="RGB+ED", dataset_out=(None, None, np.eye(3), False), pinhole_distortion=PR.MILD)
    t = dict(means=z, quats=torch.zeros(4, 4), scales=z, opacities=torch.zeros(4), colors=torch.zeros(4, 1, 3), sh_degree=0)
    with pytest.raises(ValueError, match="pinhole"):
        FrameRenderer(t, 32, 32, isect_capacity=1000, camera_model="fisheye", pinhole_distortion=PR.MILD)
    with pytest.raises(ValueError, match="one of them"):
        FrameRenderer(t, 32, 32, isect_capacity=1000, distortion=(0.1, 0, 0, 0), pinhole_distortion=PR.MILD)
    with pytest.raises(ValueError, match="dataset"):
        FrameRenderer(t, 32, 32, render_mode="RGB+ED", isect_capacity=1000, dataset_output=torch.float32, dataset_K=np.eye(3),
                      pinhole_distortion=PR.MILD)


def test_flag_bits_and_argument_checks_without_a_gpu():
    """include/mgs_lens_pinhole.h's values are ops' and its bits are free bits of both flag words; the C ABI refuses two
    camera bits and an unknown camera_model, and admits MGS_CAMERA_PINHOLE_BC, before anything is launched."""
    from robosimgs_amd import _lib, ops
    defs = {}
    for header in ("mgs.h", "mgs_lens.h", "mgs_lens_pinhole.h"):
        text = open(os.path.join(ROOT, "include", header)).read()
        defs.update({m.group(1): int(m.group(2)) for m in re.finditer(r"^#define\s+MGS_(\w+)\s+(\d+)\b", text, flags=re.M)})
    assert ops.CAMERA_PINHOLE_BC == defs["CAMERA_PINHOLE_BC"] == 4 and defs["VERSION"] == 450
    assert ops.BIN_CAMERA_PINHOLE_BC == defs["BIN_CAMERA_PINHOLE_BC"] == 512
    assert ops.FRAMES_CAMERA_PINHOLE_BC == defs["FRAMES_CAMERA_PINHOLE_BC"] == 512
    assert defs["LENS_PINHOLE_ROW_K1"] == 9 and defs["LENS_PINHOLE_ROW_UMAX"] == 14 and ops.LENS_ROW_FLOATS == defs["LENS_ROW_FLOATS"]
    bin_bits = [v for n, v in defs.items() if n.startswith("BIN_") and n != "BIN_CAMERA_PINHOLE_BC"] + [defs["PARAMS_RAW"], defs["PARAMS_OPAC_PLAIN"]]
    frame_bits = [v for n, v in defs.items() if re.match(r"(FRAMES|RASTER)_(?!BWD)", n) and n != "FRAMES_CAMERA_PINHOLE_BC"] + [defs["PARAMS_RAW"]]
    assert all(b & 512 == 0 for b in bin_bits), bin_bits
    assert all(b & 512 == 0 for b in frame_bits), frame_bits
    assert 512 == 2 * max(bin_bits) == 2 * max(frame_bits), "the next free bit of both words"
    assert ops.camera_bin_flags(4) == 512 and ops.frames_flags(False, False, True, False, 4) == 512
    assert ops.frames_flags(False, False, True, False, 4, raw=True) == 512 | defs["PARAMS_RAW"]
    assert "PINHOLE_BC" not in open(os.path.join(ROOT, "include", "mgs.h")).read()      # (tests/test_abi.py counts mgs.h's defines)
    L = _lib.lib()
    f = ctypes.c_float

    def fwd(bin_flags):
        return L.mgs_project_color_fwd(0, None, None, None, None, 0, 1, None, None, None, 16, 16, f(0.3), f(0.01), f(1e10),
                                       f(0.0), None, None, None, None, None, 3, None, None, bin_flags, None, None, None, None)
    assert fwd(512) == 0 and fwd(512 | defs["PARAMS_RAW"]) in (0, -1)       # (raw needs opacities: not this check's subject)
    for other in ("BIN_CAMERA_ORTHO", "BIN_CAMERA_FISHEYE", "BIN_CAMERA_FISHEYE_KB"):
        assert fwd(512 | defs[other]) == -1 and b"more than one MGS_BIN_CAMERA_" in L.mgs_last_error_string()
    assert fwd(defs["BIN_CAMERA_ORTHO"] | defs["BIN_CAMERA_FISHEYE"]) == -1
    assert b"MGS_BIN_CAMERA_ORTHO and MGS_BIN_CAMERA_FISHEYE" in L.mgs_last_error_string()         # the error it was

    row = (ctypes.c_float * 16)()          # an empty call never reads it: only its presence is checked

    def proj(camera_model, K=None):
        return L.mgs_projection_fwd(0, None, None, None, None, K, 16, 16, f(0.3), f(0.01), f(1e10), f(0.0), None, None,
                                    None, None, None, None, 0, None, camera_model, None)
    assert proj(4, row) == 0 and proj(3) == 0 and proj(0) == 0
    # where camera_model names the model, MGS_CAMERA_PINHOLE_BC is taken only together with its row, for n = 0 too
    assert proj(4) == -1 and b"MGS_CAMERA_PINHOLE_BC needs K" in L.mgs_last_error_string()
    bwd = lambda cm, K: L.mgs_projection_bwd(0, None, None, None, None, K, 16, 16, f(0.3), *([None] * 11), cm, None)
    assert bwd(4, row) == 0 and bwd(4, None) == -1 and b"MGS_CAMERA_PINHOLE_BC needs K" in L.mgs_last_error_string()
    assert bwd(3, None) == 0
    assert proj(7) == -1 and b"camera_model 7" in L.mgs_last_error_string()
    assert proj(5) == -1 and proj(-1) == -1
    ws = ctypes.c_size_t(0)

    def frames(flags, channels=3, ds=None):
        return L.mgs_render_frames(1, None, None, None, None, 0, 1, None, 1, None, None, 16, 16, f(0.3), f(0.01), f(1e10),
                                   f(0.0), 0, channels, flags, None, 1000, None, None, None, None, ds, None, 0, None, None,
                                   ctypes.byref(ws), None)
    for other in ("FRAMES_CAMERA_ORTHO", "FRAMES_CAMERA_FISHEYE", "FRAMES_CAMERA_FISHEYE_KB"):
        assert frames(512 | defs[other]) == -1 and b"more than one MGS_FRAMES_CAMERA_" in L.mgs_last_error_string()
    # the workspace query under the bit succeeds and equals the plain pinhole's (no parameter list or layout changed)
    assert frames(512) == 0
    under_lens = ws.value
    assert frames(0) == 0 and ws.value == under_lens and under_lens > 0
    # dataset output stays plain-pinhole-only: MGS_ERR_UNSUPPORTED
    assert frames(512, channels=4, ds=ctypes.c_void_p(256)) == -3 and b"pinhole lens" in L.mgs_last_error_string()


# ---- the device math on the host ------------------------------------------------------------------------------------
SRC = os.path.join(HERE, "host_harness", "pinhole_lens.cpp")


@pytest.fixture(scope="module")
def hh(tmp_path_factory):
    so = tmp_path_factory.mktemp("hh_pinhole_lens") / "libpinholelens.so"
    subprocess.run(["g++", "-O2", "-std=c++17", "-shared", "-fPIC", SRC, "-o", str(so)], check=True)
    return ctypes.CDLL(str(so))


def test_harness_is_clean_under_address_and_undefined_sanitizers(tmp_path):
    """The stand-alone program of tests/host_harness/pinhole_lens.cpp (its own main; host code only), built with
    -fsanitize=address,undefined and run as it is: any report aborts it."""
    exe = tmp_path / "pinhole_lens_sanitized"
    subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-DPINHOLE_LENS_MAIN", "-fsanitize=address,undefined",
                    "-fno-sanitize-recover=all", SRC, "-o", str(exe)], check=True)
    r = subprocess.run([str(exe)], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    assert re.search(r"pinhole lens harness: \d+ visible, 0 bad", r.stdout), r.stdout


RULE_ID = {"classic": 0, "opacity_aware": 1}


def project(L, k, means, quats, scales, vm, K, w, h, rule="classic", opacities=None, aa=False, near=PR.NEAR):
    n = len(means)
    out = (np.zeros(n, np.int32), np.zeros(n, np.int32), np.zeros((n, 2), np.float32), np.zeros(n, np.float32),
           np.zeros((n, 3), np.float32), np.zeros(n, np.float32))
    rc = L.hh_pinhole_lens_project(n, _p(_f(means)), _p(_f(quats)), _p(_f(scales)), _p(_f(vm)), _p(_f(PR.lens_row(K, k))), w, h,
                                   ctypes.c_float(0.3), ctypes.c_float(near), ctypes.c_float(1e10), ctypes.c_float(0.0),
                                   RULE_ID[rule], _p(_f(opacities)) if opacities is not None else None, int(aa),
                                   *[_p(a) for a in out])
    assert rc == 0
    return dict(zip(("radii", "radii_y", "means2d", "depths", "conics", "compensations"), out))


def vjp(L, k, means, quats, scales, vm, K, w, h, fw, cot):
    n = len(means)
    out = (np.zeros((n, 3), np.float32), np.zeros((n, 4), np.float32), np.zeros((n, 3), np.float32),
           np.zeros((n, 9), np.float32), np.zeros((n, 3), np.float32))
    rc = L.hh_pinhole_lens_vjp(n, _p(_f(means)), _p(_f(quats)), _p(_f(scales)), _p(_f(vm)), _p(_f(PR.lens_row(K, k))), w, h,
                               ctypes.c_float(0.3), _p(fw["radii"]), _p(fw["conics"]), _p(fw["compensations"]),
                               *[_p(_f(c)) for c in cot], *[_p(a) for a in out])
    assert rc == 0
    return dict(zip(("v_means", "v_quats", "v_scales", "v_R", "v_t"), out))


f64 = lambda a: _f(a).astype(np.float64)          # what the device is given


@pytest.mark.parametrize("lens", list(PR.LENSES))
@pytest.mark.parametrize("rule", ["classic", "opacity_aware"])
@pytest.mark.parametrize("aa", [False, True])
def test_device_forward_matches_fp64_reference(hh, lens, rule, aa):
    k, n = PR.LENSES[lens], 4000
    g, vm, K, info = PR.scene(lens, n, 0)
    n = len(g)
    op = _f(g.opacities) if rule == "opacity_aware" else None
    got = project(hh, k, g.means, g.quats, g.scales, vm, K, W, H, rule, op, aa)
    with PR.lens(k, W, H):
        ref = O.project(f64(g.means), f64(g.quats), f64(g.scales), f64(vm), f64(K), W, H, near_plane=PR.NEAR, radius_rule=rule,
                        opacities=None if op is None else op.astype(np.float64), antialiased=aa, camera_model="fisheye")
    for cull, (inside, outside) in info["where"].items():
        assert (got["radii"][inside] > 0).all() and not (got["radii"][outside] > 0).any(), cull
        assert not (ref["radii"].reshape(n, -1)[outside] > 0).any(), cull
    _check_forward(got, {a: b for a, b in ref.items() if a in ("radii", "means2d", "depths", "conics", "compensations")},
                   rule, min_vis=600)
    culled = got["radii"] == 0
    assert culled.sum() > n // 10
    for name in ("means2d", "depths", "conics", "compensations"):
        assert not got[name][culled].any(), name
    # the lens is not the plain pinhole: the same Gaussians land elsewhere
    with PR.lens((0, 0, 0, 0, 0), W, H):
        plain = O.project(f64(g.means), f64(g.quats), f64(g.scales), f64(vm), f64(K), W, H, near_plane=PR.NEAR, camera_model="fisheye")
    both = (plain["radii"] > 0) & (ref["radii"].reshape(n, -1)[:, 0] > 0)
    assert np.abs(plain["means2d"][both] - ref["means2d"][both]).max() > 1.0


def _border_scene(lens):
    """Identity camera; points exactly on the optical axis and just off it, across the frame, and -- along 12 azimuths --
    at 0.9, 0.99 and 0.999 of the first cull met (the box's border under MILD, the radial or tangential fold under
    FOLDING)."""
    rng = np.random.default_rng(5)
    k, K = PR.LENSES[lens], PR.intrinsics(lens)
    pts = []
    for z in (0.5, 2.0, 7.0):
        pts.append((0.0, 0.0, z))
        for r in (1e-6, 1e-3, 0.1, 0.3):
            for phi in (0.3, 2.0, 4.4):
                pts.append((r * z * math.cos(phi), r * z * math.sin(phi), z))
    kinds, wide = set(), []
    for phi in np.linspace(0, 2 * math.pi, 12, endpoint=False) + 0.05:
        r, kind = PR.first_cull(k, K, W, H, phi)
        kinds.add(kind)
        for rel in (0.9, 0.99, 0.999):
            if kind == "box":          # the box's border lies outside the frame: wide enough to reach into it
                wide.append(len(pts))
            pts.append((3.0 * rel * r * math.cos(phi), 3.0 * rel * r * math.sin(phi), 3.0))
    assert kinds == set(PR.PLANTED_CULLS[lens])
    means = np.array(pts)
    n = len(means)
    scales = np.exp(rng.uniform(math.log(0.02), math.log(0.1), size=(n, 3)))
    scales[wide] = rng.uniform(0.3, 0.45, size=(len(wide), 3))
    return means, rng.normal(size=(n, 4)), scales, np.eye(4), K, n


def _autograd(k, means, quats, scales, vm, K, w, h, vis, cot, near=PR.NEAR):
    t = lambda a: torch.tensor(_f(a).astype(np.float64), requires_grad=True)
    tm, tq, ts, tv = t(means), t(quats), t(scales), t(vm)
    with PR.lens(k, w, h):
        p = OT.project(tm, tq, ts, tv, torch.tensor(_f(K).astype(np.float64)), w, h, near_plane=near, camera_model="fisheye")
    mask = torch.tensor(vis.astype(np.float64))
    v_m2d, v_dep, v_con, v_comp = (torch.tensor(c.astype(np.float64)) for c in cot)
    loss = (((p["means2d"] * v_m2d).sum(-1) + p["depths"] * v_dep + (p["conics"] * v_con).sum(-1)
             + p["compensations"] * v_comp) * mask).sum()
    loss.backward()
    return tm.grad.numpy(), tq.grad.numpy(), ts.grad.numpy(), tv.grad.numpy(), p


@pytest.mark.parametrize("lens", list(PR.LENSES))
def test_device_math_from_the_axis_to_the_culls(hh, lens):
    k = PR.LENSES[lens]
    means, quats, scales, vm, K, n = _border_scene(lens)
    fw = project(hh, k, means, quats, scales, vm, K, W, H)
    assert (fw["radii"] > 0).all(), "every test point is inside every cull"
    with PR.lens(k, W, H):
        ref = O.project(f64(means), f64(quats), f64(scales), vm, f64(K), W, H, near_plane=PR.NEAR, camera_model="fisheye")
    _check_forward(fw, ref, "classic", min_vis=n)
    rng = np.random.default_rng(2)
    cot = [rng.normal(size=(n, 2)), rng.normal(size=n), rng.normal(size=(n, 3)), rng.normal(size=n)]
    # As under the fisheye lens (tests/test_lens_host.py): the compensation's cotangent is left out where the REFERENCE's
    # compensation is below 1/255 -- a splat squashed flat by a fold blends nowhere when anti-aliased.
    weak = ref["compensations"] < 1.0 / 255.0
    assert weak.sum() <= 12 and not (lens == "mild" and weak.any())
    cot[3] = np.where(weak, 0.0, cot[3])
    got = vjp(hh, k, means, quats, scales, vm, K, W, H, fw, cot)
    for name, v in got.items():
        assert np.isfinite(v).all(), name
    gm, gq, gs, gv, _ = _autograd(k, means, quats, scales, vm, K, W, H, np.ones(n, bool), cot)
    _close(got["v_means"], gm, "v_means")
    _close(got["v_quats"], gq, "v_quats")
    _close(got["v_scales"], gs, "v_scales")
    _close(got["v_R"].sum(0).reshape(1, 9), gv[:3, :3].reshape(1, 9), "v_viewmat R")
    _close(got["v_t"].sum(0).reshape(1, 3), gv[:3, 3].reshape(1, 3), "v_viewmat t")


@pytest.mark.parametrize("lens", list(PR.LENSES))
@pytest.mark.parametrize("aa", [False, True])
def test_device_backward_matches_fp64_autograd(hh, lens, aa):
    k = PR.LENSES[lens]
    g, vm, K, info = PR.scene(lens, 2500, 0)
    n = len(g)
    fw = project(hh, k, g.means, g.quats, g.scales, vm, K, W, H)
    rng = np.random.default_rng(1)
    cot = [rng.normal(size=(n, 2)), rng.normal(size=n), rng.normal(size=(n, 3)), rng.normal(size=n) if aa else np.zeros(n)]
    gm, gq, gs, gv, p = _autograd(k, g.means, g.quats, g.scales, vm, K, W, H, np.ones(n, bool), cot)
    vis = (p["radii"].numpy() > 0) & (fw["radii"] > 0)
    assert vis.sum() > 500 and int(((p["radii"].numpy() > 0) != (fw["radii"] > 0)).sum()) <= 1
    for cull, (inside, _) in info["where"].items():
        assert vis[inside].all(), cull
    # the loss of both sides over the same Gaussians
    gm, gq, gs, gv, _ = _autograd(k, g.means, g.quats, g.scales, vm, K, W, H, vis, cot)
    fw["radii"] = np.where(vis, fw["radii"], 0).astype(np.int32)
    got = vjp(hh, k, g.means, g.quats, g.scales, vm, K, W, H, fw, cot)
    _close(got["v_means"][vis], gm[vis], "v_means")
    _close(got["v_quats"][vis], gq[vis], "v_quats")
    _close(got["v_scales"][vis], gs[vis], "v_scales")
    _close(got["v_R"].sum(0).reshape(1, 9), gv[:3, :3].reshape(1, 9), "v_viewmat R")
    _close(got["v_t"].sum(0).reshape(1, 3), gv[:3, 3].reshape(1, 3), "v_viewmat t")


def test_zero_lens_row_is_the_pinhole_instantiation_inside_the_box(hh, tmp_path):
    """project_gaussian<MGS_CAMERA_PINHOLE_BC> on a row with all coefficients zero computes what <MGS_CAMERA_PINHOLE> computes
    for every Gaussian centred inside the clamp box, to fp32 rounding of the (then trivial) lens; outside the box it drops
    what the pinhole keeps with a clamped J -- the documented difference.  (Callers never take this path: zero coefficients
    select the pinhole instantiation itself.)"""
    so = tmp_path / "libcam.so"
    subprocess.run(["g++", "-O2", "-std=c++17", "-shared", "-fPIC", os.path.join(HERE, "host_harness", "camera_models.cpp"),
                    "-o", str(so)], check=True)
    import test_host_camera_models as T
    g, vm, K, _ = PR.scene("mild", 2000, 0, planted=False)
    zero = (0.0,) * 5
    a = project(hh, zero, g.means, g.quats, g.scales, vm, K, W, H)
    b = T.project(ctypes.CDLL(str(so)), "pinhole", g.means, g.quats, g.scales, vm, K, W, H, near=PR.NEAR)
    pc = PR.camera_points(g.means, vm)
    front = pc[:, 2] > PR.NEAR
    culled = np.ones(len(g), bool)
    culled[front], _ = PR.cull_margins(pc[front, 0], pc[front, 1], pc[front, 2], K[0, 0], K[1, 1], K[0, 2], K[1, 2], zero, W, H)
    inside = ~culled
    assert (a["radii"][inside] > 0).sum() > 400 and not (a["radii"][culled] > 0).any()
    assert (b["radii"][culled] > 0).sum() > 0, "the plain pinhole keeps Gaussians centred outside the box"
    for name in a:
        np.testing.assert_allclose(a[name][inside], b[name][inside], rtol=2e-5, atol=2e-5, err_msg=name)
