"""Fisheye lens distortion (OpenCV k1..k4; include/mgs.h MGS_CAMERA_FISHEYE_KB) on the host: the fp64 reference
(tests/lens_ref.py) against autograd of its own mean map, the end of the lens's range, Camera / loader / keyword handling,
the C ABI's argument checks, and the per-Gaussian DEVICE math (robosimgs_amd/csrc/mgs_math.h,
project_gaussian<MGS_CAMERA_FISHEYE_KB> and its backward, compiled with g++: tests/host_harness/lens.cpp) against that
reference through the unchanged oracle -- forward values, backward against fp64 autograd, on the optical axis, around the
series switch and up to theta_max -- plus an address / undefined-behaviour sanitizer build of the stand-alone harness."""
import ctypes
import json
import math
import os
import re
import subprocess

import numpy as np
import pytest
import torch

import lens_ref as LR
from oracle import camera_models as CM
from oracle import gs_oracle_np as O
from oracle import gs_oracle_torch as OT
from robosimgs_amd import Camera, cameras_from_transforms_json, synthetic_scene
from test_host_camera_models import _check_forward, _close, _f, _p

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
LENSES = {"mild": LR.MILD, "folding": LR.FOLDING, "zero": (0.0, 0.0, 0.0, 0.0)}
FX, FY, CX, CY = 81.5, 84.0, 128.25, 95.6


# ---- the reference itself ------------------------------------------------------------------------------------------
def _points():
    """Random camera points out to 85 degrees, the optical axis, and q / z^2 just either side of the oracle's series
    switch (oracle/camera_models.py _SERIES_T)."""
    rng = np.random.default_rng(0)
    th, phi, d = rng.uniform(0.0, math.radians(85), 200), rng.uniform(0, 2 * math.pi, 200), rng.uniform(0.3, 9.0, 200)
    pts = [np.stack([d * np.sin(th) * np.cos(phi), d * np.sin(th) * np.sin(phi), d * np.cos(th)], axis=-1)]
    for z in (0.4, 1.0, 6.0):
        pts.append(np.array([[0.0, 0.0, z]]))
        for rel in (-1e-6, -1e-12, 1e-12, 1e-6):
            rho = z * math.sqrt(CM._SERIES_T * (1.0 + rel))
            for a in (0.3, 2.2, 4.9):
                pts.append(np.array([[rho * math.cos(a), rho * math.sin(a), z]]))
    return np.concatenate(pts)


@pytest.mark.parametrize("lens", list(LENSES))
def test_reference_jacobian_is_autograd_of_its_mean_map(lens):
    k = LENSES[lens]
    pts = torch.tensor(_points())
    q_over_z2 = (pts[:, 0] ** 2 + pts[:, 1] ** 2) / pts[:, 2] ** 2
    assert (q_over_z2 == 0).sum() == 3 and (q_over_z2 < CM._SERIES_T).sum() > 20 and (q_over_z2 >= CM._SERIES_T).sum() > 200
    _, J = LR.mean_and_J(pts[:, 0], pts[:, 1], pts[:, 2], FX, FY, CX, CY, k, torch)
    J = torch.stack(J, dim=-1).reshape(-1, 2, 3)

    def mean_map(p):
        mu, _ = LR.mean_and_J(p[0:1], p[1:2], p[2:3], FX, FY, CX, CY, k, torch)
        return torch.cat(mu)
    worst = 0.0
    for i in range(len(pts)):
        Ja = torch.autograd.functional.jacobian(mean_map, pts[i])
        worst = max(worst, float((J[i] - Ja).abs().max() / Ja.abs().max()))
    print(f"\n{lens}: worst relative error of the closed-form J against autograd over {len(pts)} points: {worst:.2e}")
    assert worst <= 1e-12


def test_zero_coefficients_are_the_oracles_ideal_fisheye_exactly():
    p = _points()
    mu, J = LR.mean_and_J(p[:, 0], p[:, 1], p[:, 2], FX, FY, CX, CY, (0, 0, 0, 0), np)
    mu0, J0 = CM.mean_and_J(p[:, 0], p[:, 1], p[:, 2], FX, FY, CX, CY, "fisheye", np)
    for a, b in zip(mu + J, mu0 + J0):
        assert np.array_equal(a, b)
    with LR.lens((0, 0, 0, 0)) as u_max:       # and through the patch: nothing below pi/2 is culled
        assert u_max == (0.5 * math.pi) ** 2
        mu1, _ = O.mean_and_J(p[:, 0], p[:, 1], p[:, 2], FX, FY, CX, CY, "fisheye", np)
        assert np.array_equal(mu1[0], mu0[0])
        assert O.mean_and_J(p[:, 0], p[:, 1], p[:, 2], FX, FY, CX, CY, "ortho", np)[0][0][0] == FX * p[0, 0] + CX
    assert O.mean_and_J is CM.mean_and_J and OT.mean_and_J is CM.mean_and_J


def test_theta_max():
    from robosimgs_amd.camera import lens_theta_max
    assert abs(LR.theta_max(LR.FOLDING) - 1.2909944) < 1e-7
    assert abs(LR.theta_max(LR.FOLDING) - math.sqrt(1.0 / 0.6)) < 1e-14
    assert LR.theta_max(LR.MILD) == 0.5 * math.pi and LR.theta_max((0, 0, 0, 0)) == 0.5 * math.pi
    # 1 + 0.3 u - 1.5 u^2 = 0 at u = (0.3 + sqrt(6.09)) / 3; a root beyond pi/2 does not count
    two = (0.1, -0.3, 0.0, 0.0)
    assert abs(LR.theta_max(two) - math.sqrt((0.3 + math.sqrt(6.09)) / 3.0)) < 1e-14
    assert LR.theta_max((-0.1, 0, 0, 0)) == 0.5 * math.pi           # root at theta = 1.826
    for k in (LR.FOLDING, LR.MILD, two, (-0.1, 0, 0, 0), (0, 0, 0, 0), (0.02, -0.01, 0.004, -0.002), (0, 0, 0, -0.01)):
        assert abs(lens_theta_max(k) - LR.theta_max(k)) < 1e-12, k   # the product's (polynomial roots) = the reference's (bisection)


# ---- Camera, loader, keywords --------------------------------------------------------------------------------------
def _camera(distortion, model="fisheye"):
    c2w = np.eye(4)
    c2w[:3, :3] = np.array([[0.8, -0.6, 0.0], [0.6, 0.8, 0.0], [0.0, 0.0, 1.0]])
    c2w[:3, 3] = (0.3, -0.2, 0.5)
    return Camera(c2w, FX, FY, CX, CY, 256, 192, model=model, distortion=distortion)


def test_camera_project_applies_the_lens():
    rng = np.random.default_rng(3)
    pts = rng.uniform(-3, 3, size=(400, 3))
    for k in (LR.MILD, LR.FOLDING):
        cam = _camera(k)
        vm = cam.viewmat()
        pc = pts @ vm[:3, :3].T + vm[:3, 3]
        front = pc[:, 2] > 0.01
        inside = front & (LR.u_of(pc[:, 0], pc[:, 1], np.where(front, pc[:, 2], 1.0)) < LR.theta_max(k) ** 2)
        assert inside.sum() > 100
        uv = cam.project(pts)
        mu, _ = LR.mean_and_J(pc[inside, 0], pc[inside, 1], pc[inside, 2], FX, FY, CX, CY, k, np)
        np.testing.assert_allclose(uv[inside], np.stack(mu, axis=-1), rtol=1e-12, atol=1e-10)
        past = front & ~inside
        if k == LR.FOLDING:
            assert past.sum() > 20 and np.isnan(uv[past]).all()       # theta >= theta_max
        assert cam.scaled(0.5).distortion == tuple(k) and cam.scaled(0.5).model == "fisheye"
    ideal = _camera(None).project(pts)
    assert np.array_equal(_camera((0, 0, 0, 0)).project(pts), ideal)
    mild = _camera(LR.MILD).project(pts)            # the mild lens reaches pi/2: finite wherever the ideal lens is in front
    vm = _camera(None).viewmat()
    front = (pts @ vm[:3, :3].T + vm[:3, 3])[:, 2] > 0.01
    assert front.sum() > 100 and np.isfinite(mild[front]).all() and np.abs(mild[front] - ideal[front]).max() > 1.0
    # a real dataclass field: copies keep the lens, equality and repr see it, and `model` is still the last field
    import dataclasses
    cam = _camera(LR.FOLDING)
    assert dataclasses.replace(cam, cx=1.0).distortion == LR.FOLDING and dataclasses.replace(cam, cx=1.0).cx == 1.0
    assert "distortion" in [f.name for f in dataclasses.fields(Camera)] and "distortion=(-0.2" in repr(cam)
    assert list(Camera.__dataclass_fields__)[-1] == "model"
    assert Camera(np.eye(4), FX, FY, CX, CY, 256, 192, 0.01, 1e10, "fisheye").model == "fisheye"      # positional, as before
    with pytest.raises(ValueError, match="fisheye"):
        _camera(LR.MILD, model="pinhole")
    with pytest.raises(ValueError):
        _camera((0.1, 0.2))


def _write(tmp_path, top):
    frame = {"file_path": "a.png", "transform_matrix": np.eye(4).tolist()}
    doc = dict({"fl_x": 300.0, "fl_y": 301.0, "cx": 160.0, "cy": 120.0, "w": 320, "h": 240, "frames": [frame]}, **top)
    path = tmp_path / "transforms.json"
    path.write_text(json.dumps(doc))
    return str(path)


def test_loader_reads_the_lens_only_when_asked(tmp_path):
    cal = {"camera_model": "OPENCV_FISHEYE", "k1": -0.04, "k2": 0.012, "k3": -0.006, "k4": 0.0015}
    path = _write(tmp_path, cal)
    with pytest.raises(ValueError, match="k1"):
        cameras_from_transforms_json(path)
    cams = cameras_from_transforms_json(path, lens_distortion=True)
    assert cams[0].model == "fisheye" and cams[0].distortion == LR.MILD
    cams = cameras_from_transforms_json(_write(tmp_path, {"camera_model": "OPENCV_FISHEYE"}), lens_distortion=True)
    assert cams[0].model == "fisheye" and cams[0].distortion is None
    cams = cameras_from_transforms_json(_write(tmp_path, {"camera_model": "OPENCV", "k1": 0.1, "p1": 0.01}), lens_distortion=True)
    assert cams[0].model == "pinhole" and cams[0].distortion is None


def test_distortion_needs_the_fisheye_model():
    from robosimgs_amd import ops, rasterization
    assert ops.camera_model_id("fisheye") == ops.camera_model_id("fisheye", None) == 2
    assert ops.camera_model_id("fisheye", (0, 0, 0, 0)) == ops.camera_model_id("fisheye", np.zeros((3, 4))) == 2
    assert ops.camera_model_id("fisheye", LR.MILD) == ops.camera_model_id("fisheye", [LR.MILD, (0,) * 4]) == 3
    for model in ("pinhole", "ortho"):
        with pytest.raises(ValueError, match="fisheye"):
            ops.camera_model_id(model, LR.MILD)
        with pytest.raises(ValueError, match="fisheye"):
            ops.camera_model_id(model, (0, 0, 0, 0))
    with pytest.raises(ValueError, match=r"\[4\] or \[C,4\]"):
        ops.camera_model_id("fisheye", (0.1, 0.2, 0.3))
    z = torch.zeros(4, 3)
    with pytest.raises(ValueError, match="fisheye"):        # checked before anything touches a device
        rasterization(z, torch.zeros(4, 4), z, torch.zeros(4), torch.zeros(4, 1, 3), torch.eye(4)[None], torch.eye(3)[None],
                      32, 32, sh_degree=0, camera_model="pinhole", distortion=LR.MILD)


def test_flag_bits_and_argument_checks_without_a_gpu():
    """include/mgs_lens.h's bits are ops' and are free bits of both flag words; the C ABI refuses two camera bits and an
    unknown camera_model, and admits MGS_CAMERA_FISHEYE_KB, before anything is launched."""
    from robosimgs_amd import _lib, ops
    defs = {}
    for header in ("mgs.h", "mgs_lens.h"):
        text = open(os.path.join(ROOT, "include", header)).read()
        defs.update({m.group(1): int(m.group(2)) for m in re.finditer(r"^#define\s+MGS_(\w+)\s+(\d+)\b", text, flags=re.M)})
    assert ops.CAMERA_FISHEYE_KB == defs["CAMERA_FISHEYE_KB"] == 3 and ops.LENS_ROW_FLOATS == defs["LENS_ROW_FLOATS"] == 16
    assert ops.BIN_CAMERA_FISHEYE_KB == defs["BIN_CAMERA_FISHEYE_KB"] and ops.FRAMES_CAMERA_FISHEYE_KB == defs["FRAMES_CAMERA_FISHEYE_KB"]
    bin_bits = [v for n, v in defs.items() if n.startswith("BIN_") and n != "BIN_CAMERA_FISHEYE_KB"] + [defs["PARAMS_RAW"], defs["PARAMS_OPAC_PLAIN"]]
    frame_bits = [v for n, v in defs.items() if re.match(r"(FRAMES|RASTER)_(?!BWD)", n) and n != "FRAMES_CAMERA_FISHEYE_KB"] + [defs["PARAMS_RAW"]]
    assert all(b & defs["BIN_CAMERA_FISHEYE_KB"] == 0 for b in bin_bits), bin_bits
    assert all(b & defs["FRAMES_CAMERA_FISHEYE_KB"] == 0 for b in frame_bits), frame_bits
    assert ops.camera_bin_flags(3) == defs["BIN_CAMERA_FISHEYE_KB"] and ops.camera_bin_flags(2) == defs["BIN_CAMERA_FISHEYE"]
    assert ops.frames_flags(False, False, True, False, 3) == defs["FRAMES_CAMERA_FISHEYE_KB"]
    L = _lib.lib()
    f = ctypes.c_float

    def fwd(bin_flags):
        return L.mgs_project_color_fwd(0, None, None, None, None, 0, 1, None, None, None, 16, 16, f(0.3), f(0.01), f(1e10),
                                       f(0.0), None, None, None, None, None, 3, None, None, bin_flags, None, None, None, None)
    assert fwd(defs["BIN_CAMERA_FISHEYE_KB"]) == 0
    for other in ("BIN_CAMERA_ORTHO", "BIN_CAMERA_FISHEYE"):
        assert fwd(defs["BIN_CAMERA_FISHEYE_KB"] | defs[other]) == -1 and b"MGS_BIN_CAMERA_" in L.mgs_last_error_string()
    assert fwd(defs["BIN_CAMERA_ORTHO"] | defs["BIN_CAMERA_FISHEYE"]) == -1
    assert b"MGS_BIN_CAMERA_ORTHO and MGS_BIN_CAMERA_FISHEYE" in L.mgs_last_error_string()

    def proj(camera_model):
        return L.mgs_projection_fwd(0, None, None, None, None, None, 16, 16, f(0.3), f(0.01), f(1e10), f(0.0), None, None,
                                    None, None, None, None, 0, None, camera_model, None)
    assert proj(3) == 0 and proj(2) == 0
    assert proj(7) == -1 and b"camera_model 7" in L.mgs_last_error_string()
    assert proj(4) == -1 and proj(-1) == -1
    ws = ctypes.c_size_t(0)
    for other in ("FRAMES_CAMERA_ORTHO", "FRAMES_CAMERA_FISHEYE"):
        rc = L.mgs_render_frames(1, None, None, None, None, 0, 1, None, 1, None, None, 16, 16, f(0.3), f(0.01), f(1e10), f(0.0),
                                 0, 3, defs["FRAMES_CAMERA_FISHEYE_KB"] | defs[other], None, 1000, None, None, None, None,
                                 None, None, 0, None, None, ctypes.byref(ws), None)
        assert rc == -1 and b"MGS_FRAMES_CAMERA_" in L.mgs_last_error_string()
    # dataset output stays pinhole-only under the lens: MGS_ERR_UNSUPPORTED
    rc = L.mgs_render_frames(1, None, None, None, None, 0, 1, None, 1, None, None, 16, 16, f(0.3), f(0.01), f(1e10), f(0.0),
                             0, 4, defs["FRAMES_CAMERA_FISHEYE_KB"], None, 1000, None, None, None, None,
                             ctypes.c_void_p(256), None, 0, None, None, ctypes.byref(ws), None)
    assert rc == -3 and b"pinhole" in L.mgs_last_error_string()


# ---- the device math on the host ------------------------------------------------------------------------------------
SRC = os.path.join(HERE, "host_harness", "lens.cpp")


@pytest.fixture(scope="module")
def hh(tmp_path_factory):
    so = tmp_path_factory.mktemp("hh_lens") / "liblens.so"
    subprocess.run(["g++", "-O2", "-std=c++17", "-shared", "-fPIC", SRC, "-o", str(so)], check=True)
    return ctypes.CDLL(str(so))


def test_harness_is_clean_under_address_and_undefined_sanitizers(tmp_path):
    """The stand-alone program of tests/host_harness/lens.cpp (its own main; host code only), built with
    -fsanitize=address,undefined and run as it is: any report aborts it."""
    exe = tmp_path / "lens_sanitized"
    subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-DLENS_MAIN", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                    SRC, "-o", str(exe)], check=True)
    r = subprocess.run([str(exe)], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    assert re.search(r"lens harness: \d+ visible, 0 bad", r.stdout), r.stdout


RULE_ID = {"classic": 0, "opacity_aware": 1}


def project(L, k, means, quats, scales, vm, K, w, h, rule="classic", opacities=None, aa=False, near=0.01):
    n = len(means)
    out = (np.zeros(n, np.int32), np.zeros(n, np.int32), np.zeros((n, 2), np.float32), np.zeros(n, np.float32),
           np.zeros((n, 3), np.float32), np.zeros(n, np.float32))
    rc = L.hh_lens_project(n, _p(_f(means)), _p(_f(quats)), _p(_f(scales)), _p(_f(vm)), _p(_f(LR.lens_row(K, k))), w, h,
                           ctypes.c_float(0.3), ctypes.c_float(near), ctypes.c_float(1e10), ctypes.c_float(0.0),
                           RULE_ID[rule], _p(_f(opacities)) if opacities is not None else None, int(aa), *[_p(a) for a in out])
    assert rc == 0
    return dict(zip(("radii", "radii_y", "means2d", "depths", "conics", "compensations"), out))


def vjp(L, k, means, quats, scales, vm, K, w, h, fw, cot):
    n = len(means)
    out = (np.zeros((n, 3), np.float32), np.zeros((n, 4), np.float32), np.zeros((n, 3), np.float32),
           np.zeros((n, 9), np.float32), np.zeros((n, 3), np.float32))
    rc = L.hh_lens_vjp(n, _p(_f(means)), _p(_f(quats)), _p(_f(scales)), _p(_f(vm)), _p(_f(LR.lens_row(K, k))), w, h,
                       ctypes.c_float(0.3), _p(fw["radii"]), _p(fw["conics"]), _p(fw["compensations"]),
                       *[_p(_f(c)) for c in cot], *[_p(a) for a in out])
    assert rc == 0
    return dict(zip(("v_means", "v_quats", "v_scales", "v_R", "v_t"), out))


def _inside_scene(n, w, h, seed=4):
    """A 180-degree f = w / pi camera standing inside the scene: Gaussians all around it, from the axis to behind it."""
    g = synthetic_scene(n, math.log(0.05), 0, seed)
    c2w = np.eye(4)
    c2w[:3, 3] = (0.2, -0.1, 0.3)
    vm = Camera(c2w, 1, 1, 0, 0, w, h).viewmat()
    K = np.array([[w / math.pi, 0, w / 2 + 0.3], [0, 1.05 * w / math.pi, h / 2 - 0.2], [0, 0, 1]])
    return g, vm, K


def _band(means, vm, k, rel=1e-5):
    """Gaussians whose own fp64 u lies within rel u_max of u_max: the only ones whose visibility fp32 rounding of u
    (about 1e-6) may decide differently."""
    pc = _f(means).astype(np.float64) @ _f(vm).astype(np.float64)[:3, :3].T + _f(vm).astype(np.float64)[:3, 3]
    front = pc[:, 2] > 0
    u = LR.u_of(pc[:, 0], pc[:, 1], np.where(front, pc[:, 2], 1.0))
    u_max = LR.theta_max(k) ** 2
    return front & (np.abs(u - u_max) <= rel * u_max), front & (u > u_max), pc


@pytest.mark.parametrize("lens", ["mild", "folding"])
@pytest.mark.parametrize("rule", ["classic", "opacity_aware"])
@pytest.mark.parametrize("aa", [False, True])
def test_device_forward_matches_fp64_reference(hh, lens, rule, aa):
    k, n, w, h = LENSES[lens], 4000, 256, 192
    g, vm, K = _inside_scene(n, w, h)
    op = _f(g.opacities) if rule == "opacity_aware" else None
    got = project(hh, k, g.means, g.quats, g.scales, vm, K, w, h, rule, op, aa, near=0.2)
    f64 = lambda a: _f(a).astype(np.float64)          # what the device is given
    with LR.lens(k):
        ref = O.project(f64(g.means), f64(g.quats), f64(g.scales), f64(vm), f64(K), w, h, near_plane=0.2, radius_rule=rule,
                        opacities=None if op is None else op.astype(np.float64), antialiased=aa, camera_model="fisheye")
    band, past, pc = _band(g.means, vm, k)
    assert band.sum() <= n // 1000
    if lens == "folding":
        beyond = past & (pc[:, 2] > 0.2) & ~band
        assert beyond.sum() > 200
        assert not (got["radii"][beyond] > 0).any() and not (ref["radii"].reshape(n, -1)[beyond] > 0).any()
    keep = ~band
    _check_forward({a: b[keep] for a, b in got.items()},
                   {a: b[keep] for a, b in ref.items() if a in ("radii", "means2d", "depths", "conics", "compensations")},
                   rule, min_vis=600)
    # the lens is not the ideal one: the same Gaussians land elsewhere
    with LR.lens((0, 0, 0, 0)):
        ideal = O.project(f64(g.means), f64(g.quats), f64(g.scales), f64(vm), f64(K), w, h, near_plane=0.2, camera_model="fisheye")
    both = (ideal["radii"] > 0) & (ref["radii"].reshape(n, -1)[:, 0] > 0)
    assert np.abs(ideal["means2d"][both] - ref["means2d"][both]).max() > 1.0


def _axis_scene(k):
    """Identity camera; points exactly on the optical axis, rho / z = 1e-6 and 1e-3, either side of the device's series
    switch (rho^2 / z^2 = 0.1), and from 5 degrees up to just inside theta_max (or 85 degrees) in several azimuths."""
    rng = np.random.default_rng(5)
    top = min(math.degrees(LR.theta_max(k)) * (1 - 1e-4), 85.0)
    pts = []
    for z in (0.5, 2.0, 7.0):
        pts.append((0.0, 0.0, z))
        for r in (1e-6, 1e-3, math.sqrt(0.1) * (1 - 1e-4), math.sqrt(0.1) * (1 + 1e-4)):
            for phi in (0.3, 2.0, 4.4):
                pts.append((r * z * math.cos(phi), r * z * math.sin(phi), z))
    for deg in (5, 20, 45, 60, 0.9 * top, 0.99 * top, top):
        for phi in np.linspace(0, 2 * math.pi, 7, endpoint=False):
            th = math.radians(deg)
            pts.append((3.0 * math.sin(th) * math.cos(phi), 3.0 * math.sin(th) * math.sin(phi), 3.0 * math.cos(th)))
    means = np.array(pts)
    n = len(means)
    return means, rng.normal(size=(n, 4)), np.exp(rng.uniform(math.log(0.02), math.log(0.1), size=(n, 3))), np.eye(4), n


def _autograd(k, means, quats, scales, vm, K, w, h, vis, cot, near=0.01):
    t = lambda a: torch.tensor(_f(a).astype(np.float64), requires_grad=True)
    tm, tq, ts, tv = t(means), t(quats), t(scales), t(vm)
    with LR.lens(k):
        p = OT.project(tm, tq, ts, tv, torch.tensor(_f(K).astype(np.float64)), w, h, near_plane=near, camera_model="fisheye")
    mask = torch.tensor(vis.astype(np.float64))
    v_m2d, v_dep, v_con, v_comp = (torch.tensor(c.astype(np.float64)) for c in cot)
    loss = (((p["means2d"] * v_m2d).sum(-1) + p["depths"] * v_dep + (p["conics"] * v_con).sum(-1)
             + p["compensations"] * v_comp) * mask).sum()
    loss.backward()
    return tm.grad.numpy(), tq.grad.numpy(), ts.grad.numpy(), tv.grad.numpy(), p


@pytest.mark.parametrize("lens", ["mild", "folding"])
def test_device_math_from_the_axis_to_theta_max(hh, lens):
    k = LENSES[lens]
    means, quats, scales, vm, n = _axis_scene(k)
    w = h = 512
    K = np.array([[w / math.pi, 0, w / 2], [0, w / math.pi, h / 2], [0, 0, 1]])
    fw = project(hh, k, means, quats, scales, vm, K, w, h)
    assert (fw["radii"] > 0).all(), "every test point is inside the lens's range and on the image"
    with LR.lens(k):
        ref = O.project(_f(means).astype(np.float64), _f(quats).astype(np.float64), _f(scales).astype(np.float64), vm,
                        _f(K).astype(np.float64), w, h, camera_model="fisheye")
    _check_forward(fw, ref, "classic", min_vis=n)
    rng = np.random.default_rng(2)
    cot = [rng.normal(size=(n, 2)), rng.normal(size=n), rng.normal(size=(n, 3)), rng.normal(size=n)]
    # The compensation's cotangent is left out where the REFERENCE's compensation is below 1/255 (the last ring of the
    # folding lens, squashed radially by D = 2e-4): d sqrt(det0 / det) is 1 / (2 compensation) times a difference that
    # cancels as det0 -> 0, which the shared fp32 VJP does not resolve -- and such a Gaussian blends nowhere when
    # anti-aliased (alpha <= opacity x compensation < 1/255), so that cotangent is zero in every frame.
    weak = ref["compensations"] < 1.0 / 255.0
    assert weak.sum() <= 7 and (lens == "folding") == bool(weak.any())
    cot[3] = np.where(weak, 0.0, cot[3])
    got = vjp(hh, k, means, quats, scales, vm, K, w, h, fw, cot)
    for name, v in got.items():
        assert np.isfinite(v).all(), name
    gm, gq, gs, gv, _ = _autograd(k, means, quats, scales, vm, K, w, h, np.ones(n, bool), cot)
    _close(got["v_means"], gm, "v_means")
    _close(got["v_quats"], gq, "v_quats")
    _close(got["v_scales"], gs, "v_scales")
    _close(got["v_R"].sum(0).reshape(1, 9), gv[:3, :3].reshape(1, 9), "v_viewmat R")
    _close(got["v_t"].sum(0).reshape(1, 3), gv[:3, 3].reshape(1, 3), "v_viewmat t")


@pytest.mark.parametrize("lens", ["mild", "folding"])
@pytest.mark.parametrize("aa", [False, True])
def test_device_backward_matches_fp64_autograd(hh, lens, aa):
    k, n, w, h = LENSES[lens], 2500, 256, 192
    g, vm, K = _inside_scene(n, w, h)
    fw = project(hh, k, g.means, g.quats, g.scales, vm, K, w, h, near=0.2)
    rng = np.random.default_rng(1)
    cot = [rng.normal(size=(n, 2)), rng.normal(size=n), rng.normal(size=(n, 3)), rng.normal(size=n) if aa else np.zeros(n)]
    gm, gq, gs, gv, p = _autograd(k, g.means, g.quats, g.scales, vm, K, w, h, np.ones(n, bool), cot, near=0.2)
    vis = (p["radii"].numpy() > 0) & (fw["radii"] > 0)
    assert vis.sum() > 500
    # the loss of both sides over the same Gaussians
    gm, gq, gs, gv, _ = _autograd(k, g.means, g.quats, g.scales, vm, K, w, h, vis, cot, near=0.2)
    fw["radii"] = np.where(vis, fw["radii"], 0).astype(np.int32)
    got = vjp(hh, k, g.means, g.quats, g.scales, vm, K, w, h, fw, cot)
    _close(got["v_means"][vis], gm[vis], "v_means")
    _close(got["v_quats"][vis], gq[vis], "v_quats")
    _close(got["v_scales"][vis], gs[vis], "v_scales")
    _close(got["v_R"].sum(0).reshape(1, 9), gv[:3, :3].reshape(1, 9), "v_viewmat R")
    _close(got["v_t"].sum(0).reshape(1, 3), gv[:3, 3].reshape(1, 3), "v_viewmat t")


def test_zero_lens_row_is_the_ideal_fisheye_instantiation(hh, tmp_path):
    """project_gaussian<MGS_CAMERA_FISHEYE_KB> on a row with k = 0 computes what <MGS_CAMERA_FISHEYE> computes, to fp32
    rounding of the (then trivial) polynomial; and the untouched camera-model harness still builds against the header."""
    so = tmp_path / "libcam.so"
    subprocess.run(["g++", "-O2", "-std=c++17", "-shared", "-fPIC", os.path.join(HERE, "host_harness", "camera_models.cpp"),
                    "-o", str(so)], check=True)
    import test_host_camera_models as T
    n, w, h = 2000, 256, 192
    g, vm, K = _inside_scene(n, w, h)
    a = project(hh, (0, 0, 0, 0), g.means, g.quats, g.scales, vm, K, w, h, near=0.2)
    b = T.project(ctypes.CDLL(str(so)), "fisheye", g.means, g.quats, g.scales, vm, K, w, h, near=0.2)
    assert (a["radii"] > 0).sum() > 600
    for name in a:
        np.testing.assert_allclose(a[name], b[name], rtol=1e-6, atol=1e-6, err_msg=name)
