"""The backward of the particle-driven deformation without a GPU: include/mgs_deform_bwd.h <-> libmgs.so / libmgs_debug.so
<-> the ctypes table _lib.DEFORM_BWD_EXPORTS, the argument checks of mgs_deform_apply_bwd, the workspace size, the fp64
statement of tests/deform_bwd_ref.py against central differences of deform_ref's forward, its bounds against a NumPy
emulation of the kernels' arithmetic, the transposed binding's torch recipe against a plain loop, and the wrappers' own
errors.

Recorded here: central differences at h = 1e-6 agree with the statement to 8.8e-10 (proper) and 1.0e-9 (mirrored
neighbourhoods) of the largest gradient entry.  Worst error / bound of the emulation over the cases of
`test_bounds_hold_for_an_emulation_of_the_kernels`: v_means 0.037, v_quats 0.027, contributions 0.98 (a thin row's single
rounding), v_particles 0.26 (thin rows again); rows that turn: contributions 0.009, v_particles 0.005.
"""
import ctypes
import os
import re
import subprocess

import numpy as np
import pytest

import deform_ref as DR
import deform_bwd_ref as BR

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "mgs_deform_bwd.h")
NAMES = ["mgs_deform_apply_bwd", "mgs_deform_apply_bwd_workspace_bytes"]


def _code(path=HEADER):
    return re.sub(r"/\*.*?\*/", "", open(path).read(), flags=re.S)


def _declared(path=HEADER):
    decls = re.findall(r"\b(?:int|void|size_t|const char \*)\s*\*?\s*(mgs_\w+)\s*\(([^;]*?)\)\s*;", _code(path), flags=re.S)
    return {name: 0 if args.strip() == "void" else len([a for a in args.split(",") if a.strip()]) for name, args in decls}


def test_deform_bwd_header_symbols_are_exported_and_bound_in_both_libraries():
    from robosimgs_amd import _lib
    decl = _declared()
    assert sorted(decl) == sorted(_lib.DEFORM_BWD_EXPORTS) == NAMES
    assert decl == {"mgs_deform_apply_bwd_workspace_bytes": 1, "mgs_deform_apply_bwd": 23}
    assert len(_lib.EXPORTS) == 29 and len(_lib.DEFORM_EXPORTS) == 3              # the older tables are untouched
    assert not set(_lib.DEFORM_BWD_EXPORTS) & (set(_lib.EXPORTS) | set(_lib.DEFORM_EXPORTS) | set(_lib.DEFORM_SH_EXPORTS))
    for L in (_lib.lib(), _lib.debug_lib()):
        for name, nargs in decl.items():
            assert len(getattr(L, name).argtypes) == nargs, name
        assert L.mgs_deform_apply_bwd.argtypes[21] is ctypes.c_size_t and L.mgs_deform_apply_bwd.argtypes[7] is ctypes.c_int
        assert L.mgs_deform_apply_bwd_workspace_bytes.restype is ctypes.c_size_t
    nm = lambda path: subprocess.run(["nm", "-D", "--defined-only", path], capture_output=True, text=True).stdout
    for path in (_lib.LIB_PATH, _lib.DEBUG_LIB_PATH):
        assert all(name in nm(path) for name in decl), path
    code = _code()
    assert "MGS_VERSION" not in code and re.findall(r"#define\s+(\w+)", code) == ["MGS_DEFORM_BWD_H_"]
    assert '#include "mgs_deform.h"' in code
    text = open(HEADER).read()
    for word in ("v_means of a bound row is\n * DEFINED as v_d0", "d = 32, 16, 8, 4, 2, 1", "Guard.", "t_start int32 [m + 1]"):
        assert word in text, word


BWD = dict(n=100, quats=0x1100, idx=0x3000, w=0x4000, p=0x5000, rest=0x6000, flags=0x7000, m=50, particles_now=0x2000,
           status=0x7100, ct_means=None, ct_quats=None, ct_scales=None, t_start=0x9000, t_entry=0xA000, v_means=0x8000,
           v_quats=0x8100, v_scales=0x8200, v_particles=0x8300, bwd_status=None, workspace=0x10000, workspace_bytes=None)


@pytest.mark.parametrize("kw,word", [
    (dict(n=-1), b"n -1 is negative"),
    (dict(n=2**28), b"t_entry is int32"),
    (dict(m=7), b"m 7 particles"),
    (dict(quats=None), b"quats is null"),
    (dict(idx=None), b"a binding array"),
    (dict(w=None), b"a binding array"),
    (dict(p=None), b"a binding array"),
    (dict(rest=None), b"a binding array"),
    (dict(flags=None), b"a binding array"),
    (dict(particles_now=None), b"particles_now is null"),
    (dict(status=None), b"status is null"),
    (dict(t_start=None), b"transposed binding"),
    (dict(t_entry=None), b"transposed binding"),
    (dict(v_particles=None), b"v_particles is null"),
    (dict(v_means=None), b"only in part"),
    (dict(v_quats=None), b"only in part"),
    (dict(v_scales=None), b"only in part"),
    (dict(workspace=None), b"workspace is null"),
    (dict(workspace_bytes=0), b"workspace of 0 bytes"),
    (dict(workspace_bytes=-1), b"needed"),              # one byte short of what the size function reports
])
def test_deform_apply_bwd_argument_errors_are_reported_without_a_gpu(kw, word):
    """mgs_deform_apply_bwd on made-up addresses: every case must be refused before anything is launched."""
    from robosimgs_amd import _lib
    L = _lib.lib()
    a = dict(BWD)
    a.update(kw)
    need = L.mgs_deform_apply_bwd_workspace_bytes(100)
    assert need > 0
    if a["workspace_bytes"] is None:
        a["workspace_bytes"] = need
    elif a["workspace_bytes"] == -1:
        a["workspace_bytes"] = need - 1
    rc = L.mgs_deform_apply_bwd(*[a[k] for k in BWD], None)
    msg = L.mgs_last_error_string()
    assert rc == -1 and word in msg and msg.startswith(b"deform_apply_bwd:"), (rc, msg)


def test_apply_bwd_workspace_bytes_is_the_contribution_array():
    from robosimgs_amd import _lib, deform
    size = _lib.lib().mgs_deform_apply_bwd_workspace_bytes
    assert size(0) == size(-1) == 0
    ns = [1, 2, 63, 64, 65, 255, 256, 257, 1000, 4097, 200_000, 1_000_000, 2**28 - 1]
    a = [size(n) for n in ns]
    assert a == sorted(a) and all(v % 256 == 0 for v in a)
    assert all(96 * n <= v < 96 * n + 256 for n, v in zip(ns, a))             # float [8][3][n], no 32-bit wrap
    assert deform.apply_bwd_workspace_bytes(1000) == size(1000)


# ---- the statement against central differences ----------------------------------------------------------------------------
def _bound_cloud(n, m, seed):
    mu, q, s, X = DR.cloud(n, m, seed, "cloud")
    idx, _ = DR.knn_ref(DR.d2_exact(mu, X))
    ref = DR.bind_ref(mu, X, idx)
    f32 = lambda k: ref[k][0].astype(np.float32)
    return q, s, X, idx, f32("w"), f32("p"), f32("rest"), ref["flags"]


@pytest.mark.parametrize("mirrored", [False, True])
def test_statement_agrees_with_central_differences_of_the_forward(mirrored):
    """All gradients of the bare closed form (no guard) against fp64 central differences of deform_ref's rigid forward,
    h = 1e-6, 1e-6 of the largest entry of each gradient.  Mirrored: det P < 0 everywhere; rows whose sigma_2 - sigma_3 is
    below 5 % of sigma_1 get zero cotangents (the differences' own truncation error grows with the inverse cube of it)."""
    n, m, h = 24, 40, 1e-6
    q, s, X, idx, w, p, rest, flags = _bound_cloud(n, m, 21)
    Y = DR.move(X, "bend").astype(np.float64)
    if mirrored:
        Y = BR.mirror(Y).astype(np.float64)
    q, s = q.astype(np.float64), s.astype(np.float64)
    w, p, rest = w.astype(np.float64), p.astype(np.float64), rest.astype(np.float64)
    status = np.zeros(n, np.uint8)
    ct_m, ct_q, ct_s = (a.astype(np.float64) for a in BR.cotangents(n, 3))
    probe = BR.bwd_ref(q, idx, w, p, rest, flags, Y, status, ct_m, ct_q, ct_s, use_guard=False)
    assert (probe["kind"] == 2).all()
    weak = probe["ratio"] < 0.05
    assert weak.sum() < n // 2 and (mirrored or not weak.any())
    if mirrored:
        assert (probe["ratio"] < 1.0).all()                                   # (sigma_2 - sigma_3) / sigma_1
        e = Y[idx][1:] - Y[idx][0]
        P = np.einsum("kna,knb->nab", e, np.transpose(p, (0, 2, 1))[1:])
        assert (np.linalg.det(P) < 0).all()
    ct_m[weak], ct_q[weak], ct_s[weak] = 0, 0, 0
    ref = BR.bwd_ref(q, idx, w, p, rest, flags, Y, status, ct_m, ct_q, ct_s, use_guard=False)
    (vp, _), _ = BR.scatter_ref(ref["contrib"], idx, m)
    loss = lambda q_=q, rest_=rest, Y_=Y, s_=s: BR.forward_loss(q_, idx, w, p, rest_, flags, Y_, ct_m, ct_q, ct_s, s_)
    worst = {}
    fd = np.zeros((m, 3))
    for j in range(m):
        for c in range(3):
            Yp, Ym = Y.copy(), Y.copy()
            Yp[j, c] += h
            Ym[j, c] -= h
            fd[j, c] = (loss(Y_=Yp).sum() - loss(Y_=Ym).sum()) / (2 * h)
    worst["v_particles"] = np.abs(fd - vp).max() / np.abs(vp).max()
    fd = np.zeros((n, 3))
    for c in range(3):
        rp, rm = rest.copy(), rest.copy()
        rp[c] += h
        rm[c] -= h
        fd[:, c] = (loss(rest_=rp) - loss(rest_=rm)) / (2 * h)
    worst["v_means"] = np.abs(fd - ref["v_means"][0]).max() / np.abs(ref["v_means"][0]).max()
    fd = np.zeros((n, 4))
    for c in range(4):
        qp, qm = q.copy(), q.copy()
        qp[:, c] += h
        qm[:, c] -= h
        fd[:, c] = (loss(q_=qp) - loss(q_=qm)) / (2 * h)
    worst["v_quats"] = np.abs(fd - ref["v_quats"][0]).max() / np.abs(ref["v_quats"][0]).max()
    fd = np.zeros((n, 3))
    for c in range(3):
        sp, sm = s.copy(), s.copy()
        sp[:, c] += h
        sm[:, c] -= h
        fd[:, c] = (loss(s_=sp) - loss(s_=sm)) / (2 * h)
    worst["v_scales"] = np.abs(fd - ref["v_scales"][0]).max() / np.abs(ct_s).max()
    print(f"\ncentral differences, mirrored={mirrored}: {({k: float(f'{v:.2e}') for k, v in worst.items()})}")
    assert all(v <= 1e-6 for v in worst.values()), worst
    assert np.abs(vp).max() > 0.1 and np.abs(vp.sum(0) - ct_m.sum(0)).max() <= 1e-12     # a translation moves every mean


# ---- the bounds against an emulation of the kernels ---------------------------------------------------------------------
def host_scene(kind, motion, mirrored, n=200, m=400, seed=11):
    mu, q, s, X = DR.cloud(n, m, seed, kind)
    select = (np.arange(n) % 7 != 3).astype(np.uint8)                         # unbound rows
    idx, w, p, rest, flags = DR.emulate_bind(mu, X, select)
    Y = DR.move(X, "rigid" if motion == "collapse" else motion)
    if mirrored:
        Y = BR.mirror(Y)
    if motion == "collapse":
        Y[:] = np.float32([1.0, 2.0, 3.0])
    Y[idx[0, np.flatnonzero(idx[0] >= 0)[2]]] = np.nan                        # a non-finite particle somebody is bound to
    _, _, _, status = DR.emulate_apply(mu, q, s, idx, w, p, rest, flags, 0, Y)
    return q, idx, w, p, rest, flags, Y, status


CASES = [("cloud", "rigid", False), ("cloud", "bend", False), ("cloud", "stretch", False), ("sheet", "rigid", False),
         ("sheet", "bend", False), ("strand", "bend", False), ("cloud", "collapse", False), ("cloud", "bend", True),
         ("cloud", "rigid", True)]


@pytest.mark.parametrize("kind,motion,mirrored", CASES)
def test_bounds_hold_for_an_emulation_of_the_kernels(kind, motion, mirrored):
    q, idx, w, p, rest, flags, Y, status = host_scene(kind, motion, mirrored)
    n, m = idx.shape[1], len(Y)
    ct = BR.cotangents(n, 1)
    # the reference alone has no free row in these scenes (nothing of the kernel's is followed)
    alone = BR.bwd_ref(q, idx, w, p, rest, flags, Y, status, *ct)
    assert not alone["free"].any()
    assert ((status & DR.ST_UNBOUND) != 0).sum() >= n // 8 and ((status & DR.ST_NONFINITE) != 0).any()
    got = BR.emulate_bwd(q, idx, w, p, rest, flags, Y, status, *ct)
    ref = BR.bwd_ref(q, idx, w, p, rest, flags, Y, status, *ct, guard_seen=got["bwd_status"])
    vp_ref, cnt = BR.scatter_ref(ref["contrib"], idx, m)
    ratios = BR.check_bwd(ref, vp_ref, got, *ct)
    kinds = np.bincount(ref["kind"], minlength=3)
    print(f"\n{kind} / {motion} / mirrored={mirrored}: rows pass-through, thin, turned {kinds.tolist()}, guarded "
          f"{int(ref['guard'].sum())}, {({k: round(v, 3) for k, v in ratios.items()})}")
    assert all(v <= 1.0 for v in ratios.values()), ratios
    if kind == "strand" or motion == "collapse":
        assert kinds[2] == 0 and kinds[1] > 0
    else:
        assert kinds[1] == 0 and kinds[2] > 0
    if mirrored:
        assert not ref["guard"].all() and (ref["ratio"][ref["kind"] == 2] < 1).all()
    else:
        assert not ref["guard"].any()
    # null cotangents are zeros
    got0 = BR.emulate_bwd(q, idx, w, p, rest, flags, Y, status, ct[0], None, None)
    ref0 = BR.bwd_ref(q, idx, w, p, rest, flags, Y, status, ct[0], None, None, guard_seen=got0["bwd_status"])
    r0 = BR.check_bwd(ref0, BR.scatter_ref(ref0["contrib"], idx, m)[0], got0, ct[0], None, None)
    assert all(v <= 1.0 for v in r0.values()), r0


def test_long_segments_and_unreferenced_particles_in_the_emulated_scatter():
    """m = 8 makes every particle the neighbour of all n = 300 Gaussians (a lane's chain of 5); m = 64 with one Gaussian
    leaves 56 particles with exact zeros."""
    for n, m in ((300, 8), (1, 64)):
        mu, q, s, X = DR.cloud(n, m, 5, "cloud")
        idx, w, p, rest, flags = DR.emulate_bind(mu, X)
        Y = DR.move(X, "bend")
        _, _, _, status = DR.emulate_apply(mu, q, s, idx, w, p, rest, flags, 0, Y)
        ct = BR.cotangents(n, 2)
        got = BR.emulate_bwd(q, idx, w, p, rest, flags, Y, status, *ct)
        ref = BR.bwd_ref(q, idx, w, p, rest, flags, Y, status, *ct, guard_seen=got["bwd_status"])
        vp_ref, cnt = BR.scatter_ref(ref["contrib"], idx, m)
        ratios = BR.check_bwd(ref, vp_ref, got, *ct)
        assert all(v <= 1.0 for v in ratios.values()), ratios
        if m == 8:
            assert (cnt == n).all()
        else:
            assert (cnt == 0).sum() == 56 and not got["v_particles"][cnt == 0].any()


def test_a_mirrored_lattice_is_guarded_in_every_row():
    """sigma_2 = sigma_3 and det P < 0: G is singular, the guard drops the rotation's gradient and says so."""
    mu, q, s, X = BR.lattice()
    n, m = len(mu), len(X)
    idx, w, p, rest, flags = DR.emulate_bind(mu, X)
    assert not flags.any()
    for mirrored in (False, True):
        Y = DR.move(X, "rigid")
        if mirrored:
            Y = BR.mirror(Y)
        _, _, _, status = DR.emulate_apply(mu, q, s, idx, w, p, rest, flags, 0, Y)
        assert not status.any()
        ct = BR.cotangents(n, 7)
        alone = BR.bwd_ref(q, idx, w, p, rest, flags, Y, status, *ct)
        assert not alone["free"].any() and alone["guard"].all() == mirrored and alone["guard"].any() == mirrored
        got = BR.emulate_bwd(q, idx, w, p, rest, flags, Y, status, *ct)
        assert (got["bwd_status"] != 0).all() == mirrored
        ref = BR.bwd_ref(q, idx, w, p, rest, flags, Y, status, *ct, guard_seen=got["bwd_status"])
        ratios = BR.check_bwd(ref, BR.scatter_ref(ref["contrib"], idx, m)[0], got, *ct)
        assert all(v <= 1.0 for v in ratios.values()), ratios
        if mirrored:
            assert got["v_quats"].tobytes() == ct[1].tobytes() and np.abs(ref["ratio"]).max() < 1e-6


# ---- the transposed binding ----------------------------------------------------------------------------------------------
def test_transposed_binding_of_the_torch_recipe_equals_a_plain_loop():
    import torch
    from robosimgs_amd import deform
    rng = np.random.default_rng(0)
    for n, m in ((1, 8), (37, 11), (200, 64)):
        idx = rng.integers(0, m, (DR.K, n)).astype(np.int32)
        idx[:, rng.random(n) < 0.2] = -1                                       # unbound Gaussians
        b = deform.ParticleBinding(torch.from_numpy(idx), torch.zeros(DR.K, n), torch.zeros(DR.K, 3, n),
                                   torch.zeros(12, n), torch.from_numpy((idx[0] < 0).astype(np.uint8)), n, m)
        t_start, t_entry = b.transposed()
        assert b.transposed()[0] is t_start                                    # cached
        assert t_start.dtype == torch.int32 and t_entry.dtype == torch.int32
        assert tuple(t_start.shape) == (m + 1,) and tuple(t_entry.shape) == (DR.K * n,)
        ws, we = BR.transpose_loop(idx, m)
        assert t_start.numpy().tolist() == ws.tolist() and t_entry.numpy().tolist() == we.tolist()
        assert int(t_start[0]) == DR.K * int((idx[0] < 0).sum()) and int(t_start[m]) == DR.K * n
        for j in range(m):
            seg = we[ws[j]:ws[j + 1]]
            assert (np.diff(seg) > 0).all() and (idx.reshape(-1)[seg] == j).all()
        order = torch.tensor([n - 1, 0, 0][:max(1, min(3, n))])
        r = b.reordered(order)
        rs, re_ = BR.transpose_loop(r.idx.numpy(), m)
        assert r.transposed()[0].numpy().tolist() == rs.tolist() and r.transposed()[1].numpy().tolist() == re_.tolist()


# ---- the wrappers' own errors -----------------------------------------------------------------------------------------------
def test_wrapper_errors_and_shift_offsets_without_a_device():
    import torch
    import robosimgs_amd
    from robosimgs_amd import _lib, deform
    assert robosimgs_amd.deform_gaussians_autograd is deform.deform_gaussians_autograd
    assert robosimgs_amd.deform_apply_bwd_raw is deform.deform_apply_bwd_raw
    assert {"deform_gaussians_autograd", "deform_apply_bwd_raw"} <= set(deform.__all__)
    n, m, K = 10, 20, DR.K
    flags = torch.zeros(n, dtype=torch.uint8)
    flags[4] = deform.FLAG_UNBOUND
    b = deform.ParticleBinding(torch.zeros(K, n, dtype=torch.int32), torch.zeros(K, n), torch.zeros(K, 3, n),
                               torch.zeros(12, n), flags, n, m)
    t = dict(means=torch.zeros(n, 3), quats=torch.zeros(n, 4), scales=torch.ones(n, 3), opacities=torch.ones(n),
             colors=torch.zeros(n, 4, 3), sh_degree=1)
    parts = torch.zeros(m, 3)
    with pytest.raises(NotImplementedError, match="affine"):
        deform.deform_gaussians_autograd(t, b, parts, mode="affine")
    with pytest.raises(NotImplementedError, match="rotate_sh"):
        deform.deform_gaussians_autograd(t, b, parts, rotate_sh=True)
    with pytest.raises(ValueError, match="mode"):
        deform.deform_gaussians_autograd(t, b, parts, mode="elastic")
    with pytest.raises(ValueError, match=r"particles must be \[20,3\]"):
        deform.deform_gaussians_autograd(t, b, torch.zeros(m + 1, 3))
    with pytest.raises(ValueError, match="status"):
        deform.deform_gaussians_autograd(t, b, parts, status=torch.zeros(n))
    with pytest.raises(_lib.MgsError, match="GPU only"):
        deform.deform_gaussians_autograd(t, b, parts)
    with pytest.raises(_lib.MgsError, match="GPU only"):
        deform.deform_apply_bwd_raw(t["quats"], b, parts, torch.zeros(n, dtype=torch.uint8))
    delta = torch.arange(n * 3, dtype=torch.float32).reshape(n, 3) + 1
    assert b.shift_offsets_(delta) is b
    want = delta.t().clone()
    want[:, 4] = 0                                                               # the unbound row stays zero
    assert torch.equal(b.rest[0:3], want) and not b.rest[3:].any()
    with pytest.raises(ValueError, match="delta"):
        b.shift_offsets_(torch.zeros(n + 1, 3))
