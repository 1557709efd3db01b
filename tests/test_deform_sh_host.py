"""SH rotation in the particle-driven deformation without a GPU: include/mgs_deform_sh.h <-> libmgs.so / libmgs_debug.so <->
the ninth ctypes table (_lib.DEFORM_SH_EXPORTS), the argument checks of mgs_deform_apply_sh, the fp64 reference of
tests/deform_sh_ref.py against closed forms, its bounds against a NumPy emulation of the kernel's fp32 arithmetic, and the
Python wrappers' own errors.

Ratios recorded here (error / bound, worst over the cases of `test_bounds_hold_for_an_fp32_emulation_of_the_kernel`, whose R
is the emulated apply's own): band 1 0.075, band 2 0.030, band 3 0.022, the norm check 0.363; bound_R at most 8.9e-6.
"""
import ctypes
import os
import re
import subprocess

import numpy as np
import pytest

import deform_ref as DR
import deform_sh_ref as SR
from test_deform_host import APPLY, _code, _declared

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "mgs_deform_sh.h")


def test_deform_sh_header_symbol_is_exported_and_bound_in_both_libraries():
    from robosimgs_amd import _lib
    decl = _declared(HEADER)
    assert decl == {"mgs_deform_apply_sh": 22} and _lib.DEFORM_SH_EXPORTS == ["mgs_deform_apply_sh"]
    others = (_lib.EXPORTS, _lib.OPTIM_EXPORTS, _lib.REFINE_EXPORTS, _lib.LABEL_EXPORTS, _lib.LIFT_EXPORTS, _lib.HINGE_EXPORTS,
              _lib.POSE_EXPORTS, _lib.DEFORM_EXPORTS)
    assert not set(_lib.DEFORM_SH_EXPORTS) & set().union(*map(set, others))
    assert len(_lib.EXPORTS) == 29 and len(_lib.DEFORM_EXPORTS) == 3           # the other tables are untouched
    for L in (_lib.lib(), _lib.debug_lib()):
        at = L.mgs_deform_apply_sh.argtypes
        assert len(at) == 22 and list(at[:16]) == list(L.mgs_deform_apply.argtypes[:16])
        assert [at[k] for k in (16, 17, 20)] == [ctypes.c_int] * 3 and [at[k] for k in (18, 19, 21)] == [ctypes.c_void_p] * 3
        assert L.mgs_deform_apply_sh.restype is ctypes.c_int
    nm = lambda path: subprocess.run(["nm", "-D", "--defined-only", path], capture_output=True, text=True).stdout
    for path in (_lib.LIB_PATH, _lib.DEBUG_LIB_PATH):
        assert "mgs_deform_apply_sh" in nm(path), path
    code = _code(HEADER)
    assert "MGS_VERSION" not in code and re.findall(r"#define\s+(\w+)", code) == ["MGS_DEFORM_SH_H_"]
    assert '#include "mgs_deform.h"' in code
    # the first sixteen parameters are mgs_deform_apply's, name by name
    params = lambda path, fn: [a.split()[-1].lstrip("*") for a in
                               re.search(r"\b%s\s*\(([^;]*?)\)\s*;" % fn, _code(path), flags=re.S).group(1).split(",")]
    mine = params(HEADER, "mgs_deform_apply_sh")
    assert mine[:16] == params(os.path.join(ROOT, "include", "mgs_deform.h"), "mgs_deform_apply")[:16]
    assert mine[16:] == ["sh_degree", "coeff_stride", "sh_coeffs", "out_sh", "copy_unbound", "stream"]
    # the tables the kernel multiplies by are the reference's, to the last bit
    tab = SR.header_tables()
    for l in (2, 3):
        B, W = SR.tables(l)
        assert np.array_equal(tab[("kDir", l)], SR.DIRS[l]) and np.array_equal(tab[("kInv", l)], W.astype(np.float32))
        assert abs(np.linalg.norm(SR.DIRS[l].astype(np.float64), axis=1) - 1).max() <= 2e-7
        assert np.linalg.cond(B) < 1.8


SH = dict(APPLY, sh_degree=3, coeff_stride=16, sh_coeffs=0x9000, out_sh=0xA000, copy_unbound=1)


@pytest.mark.parametrize("kw,word", [
    (dict(n=-1), b"n -1 is negative"),
    (dict(m=7), b"m 7 particles"),
    (dict(mode=2), b"mode 2"),
    (dict(mode=-1), b"mode -1"),
    (dict(means=None), b"means, quats or scales is null"),
    (dict(quats=None), b"means, quats or scales is null"),
    (dict(scales=None), b"means, quats or scales is null"),
    (dict(idx=None), b"a binding array"),
    (dict(w=None), b"a binding array"),
    (dict(p=None), b"a binding array"),
    (dict(rest=None), b"a binding array"),
    (dict(flags=None), b"a binding array"),
    (dict(particles_now=None), b"particles_now is null"),
    (dict(out_means=None), b"an output is null"),
    (dict(out_quats=None), b"an output is null"),
    (dict(out_scales=None), b"an output is null"),
    (dict(sh_degree=-1), b"sh_degree -1 is outside 0..3"),
    (dict(sh_degree=4), b"sh_degree 4 is outside 0..3"),
    (dict(coeff_stride=15), b"rows of 15 coefficients cannot hold the 16 of degree 3"),
    (dict(sh_degree=2, coeff_stride=8), b"rows of 8 coefficients"),
    (dict(sh_degree=1, coeff_stride=3), b"rows of 3 coefficients"),
    (dict(sh_degree=0, coeff_stride=0), b"rows of 0 coefficients"),
    (dict(coeff_stride=-16), b"rows of -16 coefficients"),
    (dict(sh_coeffs=None), b"sh_coeffs or out_sh is null"),
    (dict(out_sh=None), b"sh_coeffs or out_sh is null"),
    (dict(out_sh=0x9000), b"out_sh is sh_coeffs"),
])
def test_deform_apply_sh_argument_errors_are_reported_without_a_gpu(kw, word):
    """mgs_deform_apply_sh on made-up addresses: every case must be refused before anything is launched."""
    from robosimgs_amd import _lib
    L = _lib.lib()
    a = dict(SH)
    a.update(kw)
    rc = L.mgs_deform_apply_sh(*[a[k] for k in SH], None)
    msg = L.mgs_last_error_string()
    assert rc == -1 and word in msg and msg.startswith(b"deform_apply_sh:"), (rc, msg)


def test_an_empty_call_enqueues_nothing_and_succeeds():
    from robosimgs_amd import _lib
    L = _lib.lib()
    for deg, stride in ((0, 1), (3, 16), (1, 4)):
        assert L.mgs_deform_apply_sh(0, *([None] * 8), 1, 50, *([None] * 5), deg, stride, None, None, 0, None) == 0
    # a refused scalar is refused at n = 0 too, as in mgs_deform_apply
    assert L.mgs_deform_apply_sh(0, *([None] * 8), 1, 50, *([None] * 5), 4, 16, None, None, 0, None) == -1


# ---- the fp64 reference against closed forms -------------------------------------------------------------------------------
def _rotations(n, seed):
    rng = np.random.default_rng(seed)
    return np.stack([DR.random_rotation(rng) for _ in range(n)])


def _axis(axis, ang):
    c, s = np.cos(ang), np.sin(ang)
    a, b = [(1, 2), (2, 0), (0, 1)][axis]
    R = np.eye(3)
    R[a, a], R[a, b], R[b, a], R[b, b] = c, -s, s, c
    return R


def test_reference_matrices_are_the_functions_own_and_have_the_defining_property():
    from robosimgs_amd.gaussians import _sh_basis_np, sh_rotation_matrices
    R = _rotations(20, 0)
    M = SR.sh_matrices(R, 3)
    rng = np.random.default_rng(1)
    d = rng.normal(size=(200, 3))
    d /= np.linalg.norm(d, axis=1, keepdims=True)
    Y = _sh_basis_np(3, d)
    for k in range(len(R)):
        own = sh_rotation_matrices(R[k], 3)
        Yr = _sh_basis_np(3, d @ R[k])                                       # rows (R^T d)^T
        for l in (1, 2, 3):
            sl = slice(l * l, (l + 1) * (l + 1))
            assert np.abs(M[l][k] - own[l]).max() <= 1e-14
            assert np.abs(Y[:, sl] @ M[l][k] - Yr[:, sl]).max() <= 1e-13      # sum_k Y_k(d) M_kj = Y_j(R^T d)
            assert np.abs(M[l][k] @ M[l][k].T - np.eye(2 * l + 1)).max() <= 1e-13
    # the homogeneous forms the kernel evaluates are the renderer's basis on the unit sphere, band by band
    for l in (1, 2, 3):
        assert np.abs(SR.band_basis(l, d) - Y[:, l * l:(l + 1) * (l + 1)]).max() <= 1e-15
        assert np.abs(SR.band_basis(l, 1.7 * d) - 1.7 ** l * SR.band_basis(l, d)).max() <= 1e-13


def test_reference_band_1_is_the_permuted_rotation_and_products_compose():
    R = _rotations(12, 2)
    M = SR.sh_matrices(R, 3)
    Pi = np.array([[0, -1, 0], [0, 0, 1], [-1, 0, 0]], np.float64)          # (x, y, z) -> (-y, z, -x)
    assert np.abs(M[1] - Pi @ R @ Pi.T).max() <= 1e-14
    R12 = R[:6] @ R[6:]
    M12 = SR.sh_matrices(R12, 3)
    for l in (1, 2, 3):
        assert np.abs(M12[l] - M[l][:6] @ M[l][6:]).max() <= 1e-13
    # ||M_l(R1) - M_l(R2)||_2 <= l theta, and ||R1 - R2||_F = 2 sqrt 2 sin(theta / 2)
    for ang in (1e-3, 0.1, 1.0):
        R2 = R[:6] @ np.stack([_axis(k % 3, ang) for k in range(6)])
        assert np.abs(np.linalg.norm(R2 - R[:6], axis=(1, 2)) - 2 * np.sqrt(2) * np.sin(ang / 2)).max() <= 1e-14
        M2 = SR.sh_matrices(R2, 3)
        for l in (1, 2, 3):
            assert (np.linalg.norm(M2[l] - M[l][:6], 2, axis=(1, 2)) <= l * ang * (1 + 1e-12)).all()


def test_reference_quarter_turns_are_signed_permutations():
    # band 1 about every axis; about z, the basis' own axis, every band (about x and y the higher bands mix: z^2 -> y^2)
    for axis in range(3):
        for turns in (1, 2, 3):
            M = SR.sh_matrices(_axis(axis, turns * np.pi / 2)[None], 3)
            for l in ((1, 2, 3) if axis == 2 else (1,)):
                m = M[l][0]
                r = np.round(m)
                assert np.abs(m - r).max() <= 1e-13 and (np.abs(r).sum(0) == 1).all() and (np.abs(r).sum(1) == 1).all(), (axis, l)
    # a turn about z by phi turns the pair (m, -m) of a band by m phi: check l = 2, m = 2 (coefficients 4 and 8)
    phi = 0.3
    m2 = SR.sh_matrices(_axis(2, phi)[None], 2)[2][0]
    blk = m2[np.ix_([0, 4], [0, 4])]
    assert np.abs(np.diag(blk) - np.cos(2 * phi)).max() <= 1e-13 and np.abs(np.abs(blk[[0, 1], [1, 0]]) - np.sin(2 * phi)).max() <= 1e-13
    assert abs(blk[0, 1] + blk[1, 0]) <= 1e-13
    assert abs(m2[2, 2] - 1) <= 1e-13


def test_counted_constants_of_the_bound():
    """N_l, the tangential derivative and YBAR, the three facts a_l rests on, against dense sampling."""
    rng = np.random.default_rng(3)
    d = rng.normal(size=(20000, 3))
    d /= np.linalg.norm(d, axis=1, keepdims=True)
    tau = np.cross(d, rng.normal(size=d.shape))
    tau /= np.linalg.norm(tau, axis=1, keepdims=True)
    h = 1e-6
    for l in (2, 3):
        N = np.sqrt((2 * l + 1) / (4 * np.pi))
        y = SR.band_basis(l, d)
        assert np.abs(np.linalg.norm(y, axis=1) - N).max() <= 1e-12
        dy = (SR.band_basis(l, d + h * tau) - SR.band_basis(l, d - h * tau)) / (2 * h)
        assert np.abs(np.linalg.norm(dy, axis=1) - N * np.sqrt(l * (l + 1) / 2)).max() <= 1e-6
        assert np.abs((y * dy).sum(1)).max() <= 1e-6                           # orthogonal to the radial derivative l y
    x, y, z = np.abs(d).T
    ybar2 = np.stack([SR.K1 * x * y, SR.K1 * y * z, SR.K2 * (2 * z * z + x * x + y * y), SR.K1 * x * z, SR.K3 * (x * x + y * y)], 1)
    q = 4 * z * z + x * x + y * y
    ybar3 = np.stack([SR.K4 * y * (3 * x * x + y * y), SR.K5 * x * y * z, SR.K6 * y * q, SR.K7 * z * (2 * z * z + 3 * (x * x + y * y)),
                      SR.K6 * x * q, SR.K8 * z * (x * x + y * y), SR.K4 * x * (x * x + 3 * y * y)], 1)
    assert np.linalg.norm(ybar2, axis=1).max() <= SR.YBAR[2] <= 1.27 and np.linalg.norm(ybar3, axis=1).max() <= SR.YBAR[3] <= 3.32
    assert 4.2e-7 <= SR.A[1] <= 4.3e-7 and 7.5e-6 <= SR.A[2] <= 7.7e-6 and 1.5e-5 <= SR.A[3] <= 1.6e-5


def test_emulation_turns_exactly_where_the_arithmetic_is_exact():
    """R = I and the quarter turns about z have entries 0 and +-1: band 1 is then exact, bit for bit."""
    c = SR.random_colors(40, 16, 4)
    same = lambda a, b: a.view(np.uint32).tolist() == b.view(np.uint32).tolist()
    out = SR.emulate_rotate(np.tile(np.eye(3), (40, 1, 1)), c, 3)
    assert same(out[:, :1], c[:, :1]) and np.array_equal(out[:, 1:4], c[:, 1:4])
    for l in (2, 3):
        sl = slice(l * l, (l + 1) * (l + 1))
        err = np.linalg.norm(out[:, sl].astype(np.float64) - c[:, sl], axis=1)
        assert (err <= SR.A[l] * np.linalg.norm(c[:, sl].astype(np.float64), axis=1)).all()
    Rz = np.tile(_axis(2, np.pi / 2).round(), (40, 1, 1))
    out = SR.emulate_rotate(Rz, c, 1)
    want = np.einsum("kj,njc->nkc", SR.sh_matrices(Rz[:1], 1)[1][0].round(), c[:, 1:4].astype(np.float64))
    assert np.array_equal(out[:, 1:4], want.astype(np.float32)) and same(out[:, 4:], c[:, 4:])


# ---- bounds against the emulation ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", [0, 1])
@pytest.mark.parametrize("motion", ["rigid", "bend", "stretch"])
@pytest.mark.parametrize("kind", ["cloud", "sheet"])
def test_bounds_hold_for_an_fp32_emulation_of_the_kernel(kind, motion, mode):
    """The apply in NumPy as tests/deform_ref.py emulates it; the kernel's R is the fp64 polar factor of the P it accumulated
    in fp32 (Kabsch by SVD here, within bound_R of R_ref), the SH rows turn in the kernel's fp32 order.  Every ratio error / bound is at most 1, and is printed (the module docstring records the worst)."""
    mu, q, s, X = DR.cloud(200, 400, 11, kind)
    idx, w, p, rest, flags = DR.emulate_bind(mu, X)
    Y = DR.move(X, motion)
    om, oq, osc, st = DR.emulate_apply(mu, q, s, idx, w, p, rest, flags, mode, Y)
    ref = DR.apply_ref(mu, q, s, idx, w, p, rest, flags, mode, Y, status_seen=st)
    rows = SR.rotated_rows(ref)
    assert rows.all() and (ref["branch"] == (3 if (mode == 1 and kind == "cloud") else 2)).sum() > 150
    # the emulated kernel's own R: the fp64 polar factor of the fp32-accumulated P
    now = Y[idx]                                                             # [8,n,3]
    e = now[1:] - now[0]
    P = np.zeros((len(mu), 3, 3), np.float32)
    for k in range(1, DR.K):
        term = e[k - 1][:, :, None] * p[k].T[:, None, :]
        P = term.astype(np.float32) if k == 1 else DR.fma32(e[k - 1][:, :, None], p[k].T[:, None, :], P)
    Rk, _, _ = DR.kabsch(P)
    colors = SR.random_colors(len(mu), 16, 7)
    for degree in (1, 2, 3):
        out = colors.copy()
        out[rows] = SR.emulate_rotate(Rk[rows], colors[rows], degree)
        res = SR.check_sh(ref, q, colors, out, degree)
        print(f"\n{kind} / {motion} / mode {mode} / degree {degree}: {res}")
        assert res["rotated"] == len(mu) and all(res[f"band{l}"] <= 1.0 for l in range(1, degree + 1)) and res["norm"] <= 1.0, res
        assert np.isfinite(res["bound_R"])                                   # no rotated row is exempt (check_sh asserts it row by row)


# ---- the Python wrappers' own errors -----------------------------------------------------------------------------------------
def test_wrapper_errors_raise_without_a_device():
    import torch
    import robosimgs_amd
    from robosimgs_amd import _lib, deform
    assert robosimgs_amd.deform_apply_sh_raw is deform.deform_apply_sh_raw and "deform_apply_sh_raw" in deform.__all__
    n, m, K = 10, 20, DR.K
    b = deform.ParticleBinding(torch.zeros(K, n, dtype=torch.int32), torch.zeros(K, n), torch.zeros(K, 3, n),
                               torch.zeros(12, n), torch.zeros(n, dtype=torch.uint8), n, m)
    parts = torch.zeros(m, 3)
    t = dict(means=torch.zeros(n, 3), quats=torch.zeros(n, 4), scales=torch.ones(n, 3), opacities=torch.ones(n),
             colors=torch.zeros(n, 16, 3), sh_degree=3)
    for kw in (dict(rotate_sh=True), dict(rotate_sh=True, copy_unbound=False), dict(rotate_sh=False)):
        with pytest.raises(_lib.MgsError, match="GPU only"):
            deform.deform_gaussians(t, b, parts, **kw)
    with pytest.raises(ValueError, match="out is tensors"):
        deform.deform_gaussians(t, b, parts, out=t, rotate_sh=True)
    with pytest.raises(ValueError, match=r"colors must be \[10,K,3\]"):
        deform.deform_gaussians(dict(t, colors=torch.zeros(n - 1, 16, 3)), b, parts, rotate_sh=True)
    o = [torch.zeros(n, 3), torch.zeros(n, 4), torch.zeros(n, 3)]
    with pytest.raises(_lib.MgsError, match="GPU only"):
        deform.deform_apply_sh_raw(t["means"], t["quats"], t["scales"], b, 0, parts, *o, 3, t["colors"], torch.zeros(n, 16, 3))
    import inspect
    sig = inspect.signature(deform.deform_gaussians).parameters
    assert sig["rotate_sh"].default is False and sig["copy_unbound"].default is True
    from robosimgs_amd.pipeline import FrameRenderer
    assert inspect.signature(FrameRenderer.__init__).parameters["deform_rotate_sh"].default is False
