"""Camera.model on the host: project() under each model, scaled() keeps it, and transforms.json's camera_model key
(OPENCV_FISHEYE without distortion is the ideal fisheye; with distortion it is refused; everything else loads as it
always has)."""
import json
import math

import numpy as np
import pytest

from oracle import gs_oracle_np as O
from robosimgs_amd import Camera
from robosimgs_amd.camera import cameras_from_transforms_json


def _cam(model, **kw):
    return Camera.look_at((2.0, -3.0, 1.5), (0.0, 0.0, 0.2), (0.0, 0.0, 1.0), 320, 240, 70.0, model=model, **kw)


def _pts(n=200, seed=0):
    return np.random.default_rng(seed).uniform(-1, 1, size=(n, 3))


def test_model_field_defaults_to_pinhole_and_is_checked():
    c = _cam("pinhole")
    assert Camera(np.eye(4), 100.0, 100.0, 50.0, 40.0, 100, 80).model == "pinhole"
    assert _cam("fisheye").model == "fisheye"
    with pytest.raises(ValueError):
        Camera(np.eye(4), 100.0, 100.0, 50.0, 40.0, 100, 80, model="equirect")
    assert list(Camera.__dataclass_fields__)[-1] == "model"
    assert c.scaled(0.5).model == "pinhole"


@pytest.mark.parametrize("model", ["pinhole", "ortho", "fisheye"])
def test_project_follows_the_model(model):
    c = _cam(model)
    pts = _pts()
    uv = c.project(pts)
    vm = c.viewmat()
    pc = pts @ vm[:3, :3].T + vm[:3, 3]
    x, y, z = pc.T
    if model == "pinhole":
        want = np.stack([c.fx * x / z + c.cx, c.fy * y / z + c.cy], -1)
    elif model == "ortho":
        want = np.stack([c.fx * x + c.cx, c.fy * y + c.cy], -1)
    else:
        rho = np.hypot(x, y)
        s = np.arctan2(rho, z) / rho
        want = np.stack([c.fx * s * x + c.cx, c.fy * s * y + c.cy], -1)
    np.testing.assert_allclose(uv, want, rtol=1e-12, atol=1e-9)
    # the renderer's projected means are the same map
    ref = O.project(pts, np.tile([1.0, 0, 0, 0], (len(pts), 1)), np.full((len(pts), 3), 1e-3), vm, c.K, c.width,
                    c.height, camera_model=model)
    np.testing.assert_allclose(ref["mu"], want, rtol=1e-12, atol=1e-9)
    uv2, d = c.project(pts, return_dists=True)
    np.testing.assert_allclose(d, np.linalg.norm(pc, axis=-1))


def test_fisheye_project_on_the_optical_axis():
    c = Camera(np.eye(4), 100.0, 110.0, 64.0, 48.0, 128, 96, model="fisheye")
    p = c.position - 2.0 * c.c2w[:3, 2]           # straight ahead (OpenGL: the camera looks down -Z)
    np.testing.assert_allclose(c.project(p[None]), [[64.0, 48.0]])
    # 90 degrees off axis lands at radius f pi / 2
    side = c.position + c.c2w[:3, 0]
    np.testing.assert_allclose(c.project(side[None]), [[64.0 + 100.0 * math.pi / 2, 48.0]], atol=1e-9)


@pytest.mark.parametrize("model", ["pinhole", "ortho", "fisheye"])
def test_scaled_keeps_the_model(model):
    c = _cam(model, near=0.1, far=50.0)
    s = c.scaled(2.0)
    assert s.model == model and s.near == 0.1 and s.far == 50.0
    assert (s.fx, s.cx, s.width) == (2 * c.fx, 2 * c.cx, 2 * c.width)


def _frames(extra_top=None, extra_frame=None):
    fr = {"transform_matrix": np.eye(4).tolist(), **(extra_frame or {})}
    return {"fl_x": 300.0, "fl_y": 310.0, "cx": 160.0, "cy": 120.0, "w": 320, "h": 240, "frames": [fr, dict(fr)],
            **(extra_top or {})}


def _load(tmp_path, t):
    p = tmp_path / "transforms.json"
    p.write_text(json.dumps(t))
    return cameras_from_transforms_json(str(p))


def test_transforms_fisheye_without_distortion_loads_as_fisheye(tmp_path):
    cams = _load(tmp_path, _frames({"camera_model": "OPENCV_FISHEYE"}))
    assert [c.model for c in cams] == ["fisheye", "fisheye"]
    cams = _load(tmp_path, _frames({"camera_model": "OPENCV_FISHEYE", "k1": 0.0, "k2": 0, "k3": 0.0, "k4": 0.0}))
    assert [c.model for c in cams] == ["fisheye", "fisheye"]
    # per frame
    cams = _load(tmp_path, _frames(extra_frame={"camera_model": "OPENCV_FISHEYE"}))
    assert [c.model for c in cams] == ["fisheye", "fisheye"]
    assert (cams[0].fx, cams[0].fy, cams[0].cx, cams[0].cy, cams[0].width, cams[0].height) == (300.0, 310.0, 160.0, 120.0,
                                                                                                 320, 240)


@pytest.mark.parametrize("k", ["k1", "k2", "k3", "k4"])
def test_transforms_fisheye_with_distortion_raises(tmp_path, k):
    with pytest.raises(ValueError, match=k):
        _load(tmp_path, _frames({"camera_model": "OPENCV_FISHEYE", k: 0.01}))


@pytest.mark.parametrize("top", [None, {"camera_model": "OPENCV"}, {"camera_model": "PINHOLE"},
                                 {"camera_model": "OPENCV", "k1": 0.1, "p1": 0.01}])
def test_pinhole_and_opencv_files_load_as_before(tmp_path, top):
    cams = _load(tmp_path, _frames(top))
    plain = Camera(np.eye(4), 300.0, 310.0, 160.0, 120.0, 320, 240)
    for c in cams:
        assert c.model == "pinhole"
        assert np.array_equal(c.c2w, plain.c2w)
        assert (c.fx, c.fy, c.cx, c.cy, c.width, c.height, c.near, c.far) == \
            (plain.fx, plain.fy, plain.cx, plain.cy, plain.width, plain.height, plain.near, plain.far)
