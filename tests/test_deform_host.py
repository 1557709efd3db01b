"""Particle-driven deformation without a GPU: include/mgs_deform.h <-> libmgs.so / libmgs_debug.so <-> the eighth ctypes
table (_lib.DEFORM_EXPORTS), the argument checks of mgs_deform_bind and mgs_deform_apply, the workspace size, the fp64
reference of tests/deform_ref.py against closed forms, its bounds against a NumPy emulation of the kernels' fp32 arithmetic,
and the Python wrappers' own errors.

Ratios recorded here (error / bound, worst over the cases of `test_bounds_hold_for_an_fp32_emulation_of_the_kernels`; the
emulation accumulates c, P, A in fp32 as the kernel does and is held to fp64 Kabsch by SVD): rotation 0.086 on a random
cloud and 0.081 on a coplanar sheet, affine covariance 0.159, means 0.793 (the colinear strand: a translation), bind stage
0.473 (a Q^-1 row).
"""
import ctypes
import os
import re
import subprocess

import numpy as np
import pytest

import deform_ref as DR

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "mgs_deform.h")


def _code(path=HEADER):
    return re.sub(r"/\*.*?\*/", "", open(path).read(), flags=re.S)


def _declared(path=HEADER):
    decls = re.findall(r"\b(?:int|void|size_t|const char \*)\s*\*?\s*(mgs_\w+)\s*\(([^;]*?)\)\s*;", _code(path), flags=re.S)
    return {name: 0 if args.strip() == "void" else len([a for a in args.split(",") if a.strip()]) for name, args in decls}


def test_deform_header_symbols_are_exported_and_bound_in_both_libraries():
    from robosimgs_amd import _lib
    decl = _declared()
    assert sorted(decl) == sorted(_lib.DEFORM_EXPORTS) == ["mgs_deform_apply", "mgs_deform_bind", "mgs_deform_bind_workspace_bytes"]
    others = (_lib.EXPORTS, _lib.OPTIM_EXPORTS, _lib.REFINE_EXPORTS, _lib.LABEL_EXPORTS, _lib.LIFT_EXPORTS, _lib.HINGE_EXPORTS,
              _lib.POSE_EXPORTS)
    assert not set(_lib.DEFORM_EXPORTS) & set().union(*map(set, others))
    assert len(_lib.EXPORTS) == 29                                        # include/mgs.h's table is untouched
    assert decl == {"mgs_deform_bind_workspace_bytes": 2, "mgs_deform_bind": 14, "mgs_deform_apply": 17}
    for L in (_lib.lib(), _lib.debug_lib()):
        for name, nargs in decl.items():
            assert len(getattr(L, name).argtypes) == nargs, name
        assert L.mgs_deform_bind.argtypes[5] is ctypes.c_float and L.mgs_deform_bind.argtypes[7] is ctypes.c_size_t
        assert L.mgs_deform_bind_workspace_bytes.restype is ctypes.c_size_t
    nm = lambda path: subprocess.run(["nm", "-D", "--defined-only", path], capture_output=True, text=True).stdout
    for path in (_lib.LIB_PATH, _lib.DEBUG_LIB_PATH):
        assert all(name in nm(path) for name in decl), path
    code = _code()
    defines = re.findall(r"#define\s+(\w+)", code)
    assert "MGS_VERSION" not in code and sorted(defines) == ["MGS_DEFORM_H_", "MGS_DEFORM_K"]
    assert re.search(r"#define\s+MGS_DEFORM_K\s+8\b", code) and _lib.DEFORM_K == DR.K == 8
    assert '#include "mgs.h"' in code
    # the Jacobi solve is one header that both translation units include
    csrc = os.path.join(ROOT, "robosimgs_amd", "csrc")
    for src in ("hinge.hip", "deform.hip"):
        text = open(os.path.join(csrc, src)).read()
        assert '#include "jacobi3.h"' in text and "void jacobi_rotate" not in text, src
    assert "void jacobi_rotate" in open(os.path.join(csrc, "jacobi3.h")).read()
    from robosimgs_amd.csrc import build
    assert "deform.hip" in build.SOURCES


BIND = dict(n=100, means=0x1000, select=None, m=50, particles_rest=0x2000, max_distance=float("inf"), workspace=0x10000,
            workspace_bytes=None, idx=0x3000, w=0x4000, p=0x5000, rest=0x6000, flags=0x7000)


@pytest.mark.parametrize("kw,word", [
    (dict(n=-1), b"n -1 is negative"),
    (dict(m=7), b"m 7 particles"),
    (dict(m=0), b"particles"),
    (dict(m=-5), b"particles"),
    (dict(means=None), b"means or particles_rest is null"),
    (dict(particles_rest=None), b"means or particles_rest is null"),
    (dict(idx=None), b"an output"),
    (dict(w=None), b"an output"),
    (dict(p=None), b"an output"),
    (dict(rest=None), b"an output"),
    (dict(flags=None), b"an output"),
    (dict(workspace=None), b"workspace is null"),
    (dict(workspace_bytes=0), b"workspace of 0 bytes"),
    (dict(workspace_bytes=-1), b"needed"),              # one byte short of what the size function reports
    (dict(max_distance=0.0), b"max_distance"),
    (dict(max_distance=-0.5), b"max_distance"),
    (dict(max_distance=float("nan")), b"max_distance"),
    (dict(max_distance=float("-inf")), b"max_distance"),
])
def test_deform_bind_argument_errors_are_reported_without_a_gpu(kw, word):
    """mgs_deform_bind on made-up addresses: every case must be refused before anything is launched."""
    from robosimgs_amd import _lib
    L = _lib.lib()
    a = dict(BIND)
    a.update(kw)
    need = L.mgs_deform_bind_workspace_bytes(100, 50)
    assert need > 0
    if a["workspace_bytes"] is None:
        a["workspace_bytes"] = need
    elif a["workspace_bytes"] == -1:
        a["workspace_bytes"] = need - 1
    rc = L.mgs_deform_bind(a["n"], a["means"], a["select"], a["m"], a["particles_rest"], a["max_distance"], a["workspace"],
                           a["workspace_bytes"], a["idx"], a["w"], a["p"], a["rest"], a["flags"], None)
    msg = L.mgs_last_error_string()
    assert rc == -1 and word in msg and msg.startswith(b"deform_bind:"), (rc, msg)


APPLY = dict(n=100, means=0x1000, quats=0x1100, scales=0x1200, idx=0x3000, w=0x4000, p=0x5000, rest=0x6000, flags=0x7000,
             mode=0, m=50, particles_now=0x2000, out_means=0x8000, out_quats=0x8100, out_scales=0x8200, status=None)


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
])
def test_deform_apply_argument_errors_are_reported_without_a_gpu(kw, word):
    from robosimgs_amd import _lib
    L = _lib.lib()
    a = dict(APPLY)
    a.update(kw)
    rc = L.mgs_deform_apply(*[a[k] for k in APPLY], None)
    msg = L.mgs_last_error_string()
    assert rc == -1 and word in msg and msg.startswith(b"deform_apply:"), (rc, msg)


def test_empty_calls_enqueue_nothing_and_succeed():
    from robosimgs_amd import _lib
    L = _lib.lib()
    a = dict(BIND, n=0, workspace=None, workspace_bytes=0)
    assert L.mgs_deform_bind(a["n"], None, None, a["m"], None, a["max_distance"], None, 0, None, None, None, None, None, None) == 0
    assert L.mgs_deform_apply(0, *([None] * 8), 1, 50, *([None] * 5), None) == 0


def test_bind_workspace_bytes_is_monotone_and_a_multiple_of_256():
    from robosimgs_amd import _lib, deform
    size = _lib.lib().mgs_deform_bind_workspace_bytes
    assert size(0, 50) == size(-1, 50) == size(100, 7) == size(100, 0) == 0
    ns = [1, 2, 63, 64, 65, 255, 256, 257, 1000, 4097, 200_000, 1_000_000, 2**31 - 1]
    ms = [8, 9, 1023, 1024, 1025, 50_000, 2**31 - 1]
    for m in ms:
        a = [size(n, m) for n in ns]
        assert a == sorted(a) and a[0] > 0 and all(v % 256 == 0 for v in a)
        assert a[-1] > 4 * 8 * (2**31 - 2)                                   # no 32-bit wrap in the layout
    for n in ns:
        b = [size(n, m) for m in ms]
        assert b == sorted(b)
    assert deform.bind_workspace_bytes(1000, 50) == size(1000, 50)


# ---- the fp64 reference against closed forms ---------------------------------------------------------------------------------
def _bound_cloud(n=60, m=200, seed=0, kind="cloud"):
    mu, q, s, X = DR.cloud(n, m, seed, kind)
    idx, _ = DR.knn_ref(DR.d2_exact(mu, X))
    ref = DR.bind_ref(mu, X, idx)
    f32 = lambda k: ref[k][0].astype(np.float32)
    return mu, q, s, X, idx, f32("w"), f32("p"), f32("rest"), ref["flags"]


def test_reference_weights_and_moments_are_consistent():
    mu, q, s, X, idx, w, p, rest, flags = _bound_cloud()
    ref = DR.bind_ref(mu, X, idx)
    wv, pv, rv = ref["w"][0], ref["p"][0], ref["rest"][0]
    assert not flags.any() and not ref["flags_free"].any()
    assert np.abs(wv.sum(0) - 1).max() <= 1e-14 and np.abs(pv.sum(0)).max() <= 1e-14      # sum w = 1, sum w r = 0
    assert (np.diff(wv, axis=0) <= 1e-15).all()                                            # nearer weighs more
    assert np.allclose(wv[7] / wv[0], np.exp(-1.0 + DR.d2_exact(mu, X)[np.arange(60), idx[0]] / rv[9]), rtol=1e-12)
    Xn = X.astype(np.float64)[idx]                                                          # [8,n,3]
    Xbar = (wv[..., None] * Xn).sum(0)
    assert np.abs(mu - rv[0:3].T - Xbar).max() <= 1e-14
    assert (rv[11] <= rv[10]).all() and (rv[10] <= 1).all() and (rv[11] > 1e-3).all()
    Q = np.einsum("kn,kna,knb->nab", wv, Xn - Xbar, Xn - Xbar)
    assert np.abs(DR._qinv_matrix(rv) @ Q - np.eye(3)).max() <= 1e-9


def test_an_exact_rigid_motion_gives_that_rotation_and_the_means_follow():
    mu, q, s, X, idx, w, p, rest, flags = _bound_cloud(seed=1)
    rng = np.random.default_rng(5)
    R0, t0 = DR.random_rotation(rng), rng.normal(size=3)
    Y = X.astype(np.float64) @ R0.T + t0                              # fp64 particles: the closed form itself
    for mode in (0, 1):
        ref = DR.apply_ref(mu, q, s, idx, w, p, rest, flags, mode, Y)
        assert (ref["branch"] == (2 if mode == 0 else 3)).all() and not ref["status"].any()
        # w, p, d0 are the fp32-rounded binding, so the closed form holds to their rounding: the means to 4 U of the
        # neighbourhood's extent, the map to 4 U cond(Q)
        assert np.abs(ref["means"][0] - (mu.astype(np.float64) @ R0.T + t0)).max() <= 2e-6
        if mode == 0:
            assert np.abs(ref["rot"][0] - R0 @ DR.quat_to_rot(q)).max() <= 2e-6
        else:
            assert np.abs(ref["A"][0] - R0).max() <= 1e-4
            Sig = np.einsum("nab,nb,ncb->nac", DR.quat_to_rot(q), s.astype(np.float64) ** 2, DR.quat_to_rot(q))
            want = R0 @ Sig @ R0.T
            assert np.abs(ref["cov"][0] - want).max() <= 1e-3 * np.abs(want).max()


def test_an_exact_affine_map_gives_A_equal_F_to_the_rounding_of_the_fp32_inputs():
    mu, q, s, X, idx, w, p, rest, flags = _bound_cloud(seed=2)
    F = np.array([[1.4, 0.2, 0.0], [0.0, 0.8, 0.1], [0.1, 0.0, 1.1]])
    Y = X.astype(np.float64) @ F.T + [0.3, -0.2, 0.1]
    ref = DR.apply_ref(mu, q, s, idx, w, p, rest, flags, 1, Y)
    A = ref["A"][0]
    # P = F Q exactly for the exact binding; the stored p and Q^-1 are rounded to fp32, each to U, and the inverse
    # amplifies p's rounding by cond(Q) <= 1 / (lambda_min / lambda_max)
    cond = 1.0 / rest[11].astype(np.float64)
    tol = 16 * DR.U * cond * np.abs(F).max()
    err = np.abs(A - F).max(axis=(1, 2))
    print(f"\n|A - F| worst {err.max():.2e}, worst error / (16 U cond |F|) {float((err / tol).max()):.3f}")
    assert (err <= tol).all()
    assert np.abs(ref["means"][0] - (mu.astype(np.float64) @ F.T + [0.3, -0.2, 0.1])).max() <= 1e-4
    # shape matching fits the rotation to P = F Q, not to F: the rigid mode gives the SO(3) polar factor of F Q
    Q = np.linalg.inv(DR._qinv_matrix(rest))
    Rk, _, _ = DR.kabsch(F @ Q)
    rig = DR.apply_ref(mu, q, s, idx, w, p, rest, flags, 0, Y)
    assert np.abs(rig["rot"][0] - Rk @ DR.quat_to_rot(q)).max() <= 1e-4


def test_a_coplanar_neighbourhood_is_flat_and_still_gives_the_rotation():
    mu, q, s, X, idx, w, p, rest, flags = _bound_cloud(seed=3, kind="sheet")
    assert (flags == DR.FLAG_FLAT).all() and not rest[3:9].any() and (rest[11] == 0).all() and (rest[10] > 1e-3).all()
    rng = np.random.default_rng(6)
    R0, t0 = DR.random_rotation(rng), rng.normal(size=3)
    Y = X.astype(np.float64) @ R0.T + t0
    for mode in (0, 1):
        ref = DR.apply_ref(mu, q, s, idx, w, p, rest, flags, mode, Y)
        assert (ref["branch"] == 2).all() and (ref["status"] == (0 if mode == 0 else DR.ST_FALLBACK)).all()
        assert np.abs(ref["rot"][0] - R0 @ DR.quat_to_rot(q)).max() <= 2e-6
        assert np.abs(ref["means"][0] - (mu.astype(np.float64) @ R0.T + t0)).max() <= 2e-6


def test_a_colinear_neighbourhood_is_thin_and_is_translated():
    mu, q, s, X, idx, w, p, rest, flags = _bound_cloud(seed=4, kind="strand")
    assert ((flags & DR.FLAG_THIN) != 0).all() and ((flags & DR.FLAG_FLAT) != 0).all()
    Y = X.astype(np.float64) + [0.5, -1.0, 2.0]
    ref = DR.apply_ref(mu, q, s, idx, w, p, rest, flags, 0, Y)
    assert (ref["branch"] == 1).all() and (ref["status"] == DR.ST_THIN).all()
    assert np.abs(ref["means"][0] - (mu.astype(np.float64) + [0.5, -1.0, 2.0])).max() <= 1e-6
    # a healthy neighbourhood whose particles collapse to one point at frame time is thin for that frame
    mu, q, s, X, idx, w, p, rest, flags = _bound_cloud(seed=5)
    ref = DR.apply_ref(mu, q, s, idx, w, p, rest, flags, 1, np.tile([[1.0, 2.0, 3.0]], (len(X), 1)))
    assert (ref["status"] == DR.ST_THIN).all()
    assert np.abs(ref["means"][0] - ([1.0, 2.0, 3.0] + rest[0:3].T.astype(np.float64))).max() <= 1e-15


def test_reference_rules_of_the_bind():
    """Ties go to the lower index, non-finite points take no part, fewer than 8 finite particles bind nobody."""
    X = np.array([[i, j, k] for i in range(3) for j in range(3) for k in range(3)], np.float32)
    mu = np.array([[1, 1, 1], [0.5, 0.5, 0.5], [np.nan, 0, 0], [2, 2, 2]], np.float32)
    idx, d = DR.knn_ref(DR.d2_exact(mu, X))
    assert idx[:, 0].tolist() == [13, 4, 10, 12, 14, 16, 22, 1]          # the centre, its 6 face neighbours, then the lowest edge
    assert idx[:, 1].tolist() == [0, 1, 3, 4, 9, 10, 12, 13] and (d[:, 1] == 0.75).all()
    assert (idx[:, 2] == -1).all()
    X2 = X.copy()
    X2[13] = np.inf
    assert 13 not in DR.knn_ref(DR.d2_exact(mu, X2))[0][:, 0].tolist()
    X3 = np.full((27, 3), np.nan, np.float32)
    X3[:7] = X[:7]
    assert (DR.knn_ref(DR.d2_exact(mu, X3))[0] == -1).all()
    sel = np.array([1, 0, 1, 1])
    idx, _ = DR.knn_ref(DR.d2_exact(mu, X), sel, max_distance=0.5)
    assert (idx[:, 1] == -1).all() and (idx[:, 0] >= 0).all() and (idx[:, 3] >= 0).all()
    assert np.array_equal(DR.d2_exact(mu[[0, 1, 3]], X), DR.d2_fp32(mu[[0, 1, 3]], X))        # a lattice is exact in fp32


CASES = [("cloud", "rigid"), ("cloud", "bend"), ("cloud", "stretch"), ("sheet", "rigid"), ("sheet", "bend"),
         ("strand", "bend")]


@pytest.mark.parametrize("kind,motion", CASES)
def test_bounds_hold_for_an_fp32_emulation_of_the_kernels(kind, motion):
    """The kernels' arithmetic in NumPy (fp32 d2, fp32 fma chains for c, P, A; eigh in place of Jacobi) against the fp64
    statement with Kabsch by SVD: every ratio error / bound is at most 1, and is printed (the module docstring records them)."""
    mu, q, s, X = DR.cloud(200, 400, 11, kind)
    idx, w, p, rest, flags = DR.emulate_bind(mu, X)
    assert DR.check_neighbours(mu, X, idx) <= 1.0
    bref = DR.bind_ref(mu, X, idx)
    rb = DR.check_bind(bref, w, p, rest, flags)
    Y = DR.move(X, motion)
    out = {}
    for mode in (0, 1):
        om, oq, osc, st = DR.emulate_apply(mu, q, s, idx, w, p, rest, flags, mode, Y)
        ref = DR.apply_ref(mu, q, s, idx, w, p, rest, flags, mode, Y, status_seen=st)
        out[mode] = DR.check_apply(ref, mu, q, s, om, oq, osc, st)
    print(f"\n{kind} / {motion}: bind {rb}, rigid {out[0]}, affine {out[1]}")
    for r in (rb, out[0], out[1]):
        assert all(v <= 1.0 for v in r.values()), r
    if kind == "cloud":
        assert "rot" in out[0] and "cov" in out[1]
    if kind == "sheet":
        assert "rot" in out[1] and "cov" not in out[1]                   # the affine mode fell back


# ---- the Python wrappers' own errors -------------------------------------------------------------------------------------------
def test_wrapper_errors_raise_without_a_device():
    import torch
    from robosimgs_amd import _lib, deform
    import robosimgs_amd
    assert robosimgs_amd.bind_particles is deform.bind_particles and robosimgs_amd.deform_gaussians is deform.deform_gaussians
    assert robosimgs_amd.ParticleBinding is deform.ParticleBinding
    n, m = 10, 20
    means, parts = torch.zeros(n, 3), torch.zeros(m, 3)
    with pytest.raises(ValueError, match=r"means must be a tensor \[n,3\]"):
        deform.bind_particles(torch.zeros(n, 4), parts)
    with pytest.raises(ValueError, match="floating-point"):
        deform.bind_particles(means.to(torch.int32), parts)
    with pytest.raises(ValueError, match="at least 8"):
        deform.bind_particles(means, torch.zeros(7, 3))
    with pytest.raises(ValueError, match="select"):
        deform.bind_particles(means, parts, select=torch.ones(n + 1, dtype=torch.bool))
    with pytest.raises(ValueError, match="select"):
        deform.bind_particles(means, parts, select=torch.ones(n))
    for bad in (0.0, -1.0, float("nan")):
        with pytest.raises(ValueError, match="max_distance"):
            deform.bind_particles(means, parts, max_distance=bad)
    with pytest.raises(_lib.MgsError, match="GPU only"):
        deform.bind_particles(means, parts)

    K = DR.K
    b = deform.ParticleBinding(torch.zeros(K, n, dtype=torch.int32), torch.zeros(K, n), torch.zeros(K, 3, n),
                               torch.zeros(12, n), torch.zeros(n, dtype=torch.uint8), n, m)
    assert (b.n, b.m, b.n_bound()) == (n, m, n)
    with pytest.raises(ValueError, match="binding.p"):
        deform.ParticleBinding(b.idx, b.w, torch.zeros(K, n, 3), b.rest, b.flags, n, m)
    with pytest.raises(ValueError, match="binding.idx"):
        deform.ParticleBinding(b.idx.long(), b.w, b.p, b.rest, b.flags, n, m)
    # reordered: an index_select on the last dimension of every array
    b.idx[:] = torch.arange(n, dtype=torch.int32)[None, :]
    b.flags[:] = torch.arange(n, dtype=torch.uint8)
    b.p[:] = torch.arange(n, dtype=torch.float32)[None, None, :]
    order = torch.tensor([3, 1, 7, 7])
    r = b.reordered(order)
    assert (r.n, r.m) == (4, m) and r.idx[5].tolist() == [3, 1, 7, 7] and r.flags.tolist() == [3, 1, 7, 7]
    assert r.p.shape == (K, 3, 4) and r.p[2, 1].tolist() == [3.0, 1.0, 7.0, 7.0] and r.rest.shape == (12, 4) and r.p.is_contiguous()

    t = dict(means=means, quats=torch.zeros(n, 4), scales=torch.ones(n, 3), opacities=torch.ones(n), colors=torch.zeros(n, 1, 3),
             sh_degree=0)
    with pytest.raises(ValueError, match="out is tensors"):
        deform.deform_gaussians(t, b, parts, out=t)
    with pytest.raises(ValueError, match="mode"):
        deform.deform_gaussians(t, b, parts, mode="elastic")
    with pytest.raises(ValueError, match=r"particles must be \[20,3\]"):
        deform.deform_gaussians(t, b, torch.zeros(m + 1, 3))
    with pytest.raises(ValueError, match="9 rows"):
        deform.deform_gaussians(dict(t, means=torch.zeros(n - 1, 3)), b, parts)
    with pytest.raises(ValueError, match="status"):
        deform.deform_gaussians(t, b, parts, status=torch.zeros(n))
    with pytest.raises(_lib.MgsError, match="GPU only"):
        deform.deform_gaussians(t, b, parts)
    assert deform.MODES == {"rigid": 0, "affine": 1}
    assert (deform.FLAG_UNBOUND, deform.FLAG_FLAT, deform.FLAG_THIN) == (DR.FLAG_UNBOUND, DR.FLAG_FLAT, DR.FLAG_THIN)
    assert (deform.STATUS_UNBOUND, deform.STATUS_FALLBACK, deform.STATUS_THIN, deform.STATUS_NONFINITE) == (1, 2, 4, 8)
