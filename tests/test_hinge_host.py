"""The hinge fit without a GPU: include/mgs_hinge.h <-> libmgs.so / libmgs_debug.so <-> the sixth ctypes table
(_lib.HINGE_EXPORTS), the argument checks of mgs_hinge_fit, the workspace size, the fp64 reference of tests/hinge_ref.py
against what the reference project recorded for its open box (tests/golden/hinge_openbox.npz), and Hinge.pose.
"""
import ctypes
import os
import re
import subprocess

import numpy as np
import pytest

import hinge_ref as HR

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "mgs_hinge.h")
GOLDEN = os.path.join(ROOT, "tests", "golden", "hinge_openbox.npz")


def _code(path=HEADER):
    return re.sub(r"/\*.*?\*/", "", open(path).read(), flags=re.S)


def _declared(path=HEADER):
    decls = re.findall(r"\b(?:int|void|size_t|const char \*)\s*\*?\s*(mgs_\w+)\s*\(([^;]*?)\)\s*;", _code(path), flags=re.S)
    return {name: 0 if args.strip() == "void" else len([a for a in args.split(",") if a.strip()]) for name, args in decls}


def test_hinge_header_symbols_are_exported_and_bound_in_both_libraries():
    from robosimgs_amd import _lib
    decl = _declared()
    assert sorted(decl) == sorted(_lib.HINGE_EXPORTS) == ["mgs_hinge_fit", "mgs_hinge_workspace_bytes"]
    others = (_lib.EXPORTS, _lib.OPTIM_EXPORTS, _lib.REFINE_EXPORTS, _lib.LABEL_EXPORTS, _lib.LIFT_EXPORTS)
    assert not set(_lib.HINGE_EXPORTS) & set().union(*map(set, others))
    assert len(_lib.EXPORTS) == 29                                        # include/mgs.h's table is untouched
    assert decl == {"mgs_hinge_workspace_bytes": 2, "mgs_hinge_fit": 11}
    for L in (_lib.lib(), _lib.debug_lib()):
        for name, nargs in decl.items():
            assert len(getattr(L, name).argtypes) == nargs, name
        assert L.mgs_hinge_fit.argtypes[4] is ctypes.c_float and L.mgs_hinge_fit.argtypes[6] is ctypes.c_size_t
        assert L.mgs_hinge_workspace_bytes.restype is ctypes.c_size_t
    nm = lambda path: subprocess.run(["nm", "-D", "--defined-only", path], capture_output=True, text=True).stdout
    for path in (_lib.LIB_PATH, _lib.DEBUG_LIB_PATH):
        assert all(name in nm(path) for name in decl), path
    code = _code()
    assert "MGS_VERSION" not in code and "#define" not in code.replace("#define MGS_HINGE_H_", "")
    assert '#include "mgs.h"' in code


@pytest.mark.parametrize("kw,word", [
    (dict(n_a=0), b"a part is empty"),
    (dict(n_b=0), b"a part is empty"),
    (dict(n_a=-3), b"a part is empty"),
    (dict(pts_a=None), b"pts_a or pts_b is null"),
    (dict(pts_b=None), b"pts_a or pts_b is null"),
    (dict(joint=None), b"joint is null"),
    (dict(workspace=None), b"workspace is null"),
    (dict(workspace_bytes=0), b"workspace of 0 bytes"),
    (dict(workspace_bytes=-1), b"needed"),              # one byte short of what the size function reports
    (dict(threshold=0.0), b"threshold"),
    (dict(threshold=-0.01), b"threshold"),
    (dict(threshold=float("nan")), b"threshold"),
    (dict(threshold=float("inf")), b"threshold"),
])
def test_hinge_fit_argument_errors_are_reported_without_a_gpu(kw, word):
    """mgs_hinge_fit on made-up addresses: every case must be refused before anything is launched."""
    from robosimgs_amd import _lib
    L = _lib.lib()
    a = dict(n_a=100, pts_a=0x1000, n_b=200, pts_b=0x2000, threshold=0.01, workspace=0x10000, workspace_bytes=None,
             joint=0x3000)
    a.update(kw)
    need = L.mgs_hinge_workspace_bytes(100, 200)
    if a["workspace_bytes"] is None:
        a["workspace_bytes"] = need
    elif a["workspace_bytes"] == -1:
        a["workspace_bytes"] = need - 1
    rc = L.mgs_hinge_fit(a["n_a"], a["pts_a"], a["n_b"], a["pts_b"], a["threshold"], a["workspace"], a["workspace_bytes"],
                         None, None, a["joint"], None)
    msg = L.mgs_last_error_string()
    assert rc == -1 and word in msg and msg.startswith(b"hinge_fit:"), (rc, msg)


def test_workspace_bytes_is_monotone_and_is_what_the_wrapper_allocates():
    from robosimgs_amd import _lib, articulation
    L = _lib.lib()
    size = L.mgs_hinge_workspace_bytes
    assert size(0, 5) == size(5, 0) == size(-1, -1) == 0
    ns = [1, 2, 63, 64, 65, 255, 256, 257, 1000, 4410, 8416, 100_000, 800_000, 2**31 - 1]
    for fixed in (1, 4099):
        a = [size(n, fixed) for n in ns]
        b = [size(fixed, n) for n in ns]
        assert a == sorted(a) and b == sorted(b) and a[0] > 0
        assert a[-1] > 4 * (2**31 - 1)                                       # no 32-bit wrap in the layout
    assert all(size(n, m) % 256 == 0 and size(n, m) >= 4 * (n + m) for n in ns[:-1] for m in (1, 777))
    for n, m in ((1, 1), (4410, 8416), (1000, 4099)):
        assert articulation.workspace_bytes(n, m) == size(n, m)
        assert articulation.hinge_workspace(n, m, "cpu").numel() == size(n, m) + 256     # room to align to 256 bytes


@pytest.fixture(scope="module")
def golden():
    g = np.load(GOLDEN)
    return g, HR.fit(g["lid"], g["body"], float(g["threshold"]))


def test_fp64_reference_reproduces_the_recorded_hinge(golden):
    g, ref = golden
    assert g["lid"].shape == (4410, 3) and g["body"].shape == (8416, 3) and g["lid"].dtype == np.float32
    print(f"\nposition error {np.abs(ref.position - g['position']).max():.2e}, 1 - |axis . axis_ref| "
          f"{abs(1 - abs(ref.axis @ g['axis'])):.2e}, confidence error {abs(ref.axis_confidence - g['axis_confidence']):.2e}, "
          f"gap {ref.gap:.3e}")
    assert np.abs(ref.position - g["position"]).max() <= 1e-12
    assert abs(1.0 - abs(ref.axis @ g["axis"])) <= 1e-12
    assert abs(ref.axis_confidence - float(g["axis_confidence"])) <= 1e-12
    assert np.abs(-ref.position - g["translation_applied"]).max() <= 1e-12
    assert ref.n_contact == (212, 208) and ref.min_distance == 0.0 and ref.gap > 1e-4
    assert not ref.fallback and not ref.nonfinite
    k = int(np.argmax(np.abs(ref.axis)))
    assert ref.axis[k] > 0 and k == 2                  # the sign rule: the file's axis is the other sign
    assert np.all(np.diff(ref.eigenvalues) >= 0)


def test_reference_rules():
    """The rules the restatement adds to the reference: non-finite rows, the sign rule's tie, the fallback."""
    rng = np.random.default_rng(3)
    a = rng.random((40, 3)).astype(np.float32)
    b = (rng.random((50, 3)) + [1.0, 0, 0]).astype(np.float32)
    clean = HR.fit(a, b, 0.05)
    a2, b2 = np.vstack([a, [[np.nan, 0, 0]], [[0.99, 0.5, np.inf]]]).astype(np.float32), np.vstack([[[1.0, -np.inf, 0.5]], b]).astype(np.float32)
    dirty = HR.fit(a2, b2, 0.05)
    assert dirty.nonfinite and not clean.nonfinite
    assert not dirty.contact_a[40:].any() and not dirty.contact_b[0]
    assert np.array_equal(dirty.contact_a[:40], clean.contact_a) and np.array_equal(dirty.contact_b[1:], clean.contact_b)
    assert np.array_equal(dirty.position, clean.position) and dirty.min2 == clean.min2
    assert HR.sign_rule(np.array([-0.5, 0.5, 0.1])).tolist() == [0.5, -0.5, -0.1]           # a tie: the lowest index decides
    assert HR.sign_rule(np.array([0.1, -0.9, 0.2])).tolist() == [-0.1, 0.9, -0.2]
    blob = rng.normal(size=(400, 3)).astype(np.float32) * 0.001
    iso = HR.fit(blob[:200], blob[200:], 1.0)
    assert iso.fallback and iso.axis.tolist() == [1.0, 0.0, 0.0] and iso.axis_confidence < 0.5


def _hinge(position, axis):
    from robosimgs_amd.articulation import Hinge
    joint = np.zeros(16)
    joint[0:3], joint[3:6] = position, axis
    joint[6], joint[8], joint[9] = 0.9, 7, 9
    return Hinge(joint)


def test_hinge_pose():
    from robosimgs_amd.transform import pack_transforms
    rng = np.random.default_rng(5)
    axis = rng.normal(size=3)
    axis /= np.linalg.norm(axis)
    pos = rng.normal(size=3) * 3
    h = _hinge(pos, axis)
    assert h.n_contact == (7, 9) and not h.fallback and h.axis_confidence == 0.9
    assert np.array_equal(h.to_origin(), -pos)
    R0, t0 = h.pose(0.0)
    assert np.array_equal(R0, np.eye(3)) and np.abs(t0).max() <= 1e-15
    a, b = 0.7, -1.9
    (Ra, ta), (Rb, tb), (Rab, tab) = h.pose(a), h.pose(b), h.pose(a + b)
    assert Ra.shape == (3, 3) and ta.shape == (3,) and Ra.dtype == np.float64
    on_axis = pos + np.linspace(-4, 4, 9)[:, None] * axis
    assert np.abs(on_axis @ Ra.T + ta - on_axis).max() <= 1e-12              # points on the axis are fixed
    assert np.abs(Ra @ Rb - Rab).max() <= 1e-12 and np.abs(Ra @ tb + ta - tab).max() <= 1e-12
    # a right-handed rotation by the angle: a point off the axis turns by `a` about it
    off = pos + np.cross(axis, [0.3, -0.2, 0.9])
    v0, v1 = off - pos, Ra @ off + ta - pos
    assert abs(np.dot(v0, v1) / np.dot(v0, v0) - np.cos(a)) <= 1e-12 and np.dot(np.cross(v0, v1), axis) > 0
    # vectorised over angles, and accepted by pack_transforms' own rotation check
    angles = np.array([0.0, a, b, a + b, 3.0])
    R, t = h.pose(angles)
    assert R.shape == (5, 3, 3) and t.shape == (5, 3)
    for k, (Rk, tk) in enumerate(((R0, t0), (Ra, ta), (Rb, tb), (Rab, tab))):
        assert np.array_equal(R[k], Rk) and np.array_equal(t[k], tk)
    x, rot = pack_transforms(R, t, sh_degree=1)
    assert x.shape == (5, 20) and rot.shape == (5, 84)
    assert np.allclose(x[:, :9].reshape(5, 3, 3), R, atol=1e-7) and np.allclose(x[:, 9:12], t, atol=1e-6)
