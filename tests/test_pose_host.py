"""Differentiable group poses without a GPU: include/mgs_pose.h <-> libmgs.so / libmgs_debug.so <-> the seventh ctypes table
(_lib.POSE_EXPORTS), the argument checks of mgs_pose_bwd, the workspace size, pack_transforms_torch against
pack_transforms, Hinge.pose_torch against Hinge.pose, and the fp64 reference of tests/pose_ref.py against central
differences of the forward's own reference (frame_helper_ref.transform_ref).
"""
import ctypes
import os
import re
import subprocess

import numpy as np
import pytest
import torch

import frame_helper_ref as FR
import pose_ref as PR

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "mgs_pose.h")


def _code(path=HEADER):
    return re.sub(r"/\*.*?\*/", "", open(path).read(), flags=re.S)


def _declared(path=HEADER):
    decls = re.findall(r"\b(?:int|void|size_t|const char \*)\s*\*?\s*(mgs_\w+)\s*\(([^;]*?)\)\s*;", _code(path), flags=re.S)
    return {name: 0 if args.strip() == "void" else len([a for a in args.split(",") if a.strip()]) for name, args in decls}


def test_pose_header_symbols_are_exported_and_bound_in_both_libraries():
    from robosimgs_amd import _lib
    decl = _declared()
    assert sorted(decl) == sorted(_lib.POSE_EXPORTS) == ["mgs_pose_bwd", "mgs_pose_bwd_workspace_bytes"]
    others = (_lib.EXPORTS, _lib.OPTIM_EXPORTS, _lib.REFINE_EXPORTS, _lib.LABEL_EXPORTS, _lib.LIFT_EXPORTS, _lib.HINGE_EXPORTS)
    assert not set(_lib.POSE_EXPORTS) & set().union(*map(set, others))
    assert len(_lib.EXPORTS) == 29                                        # include/mgs.h's table is untouched
    assert decl == {"mgs_pose_bwd_workspace_bytes": 2, "mgs_pose_bwd": 23}
    for L in (_lib.lib(), _lib.debug_lib()):
        for name, nargs in decl.items():
            assert len(getattr(L, name).argtypes) == nargs, name
        assert L.mgs_pose_bwd.argtypes[21] is ctypes.c_size_t
        assert L.mgs_pose_bwd_workspace_bytes.restype is ctypes.c_size_t
    nm = lambda path: subprocess.run(["nm", "-D", "--defined-only", path], capture_output=True, text=True).stdout
    for path in (_lib.LIB_PATH, _lib.DEBUG_LIB_PATH):
        assert all(name in nm(path) for name in decl), path
    code = _code()
    assert "MGS_VERSION" not in code and "#define" not in code.replace("#define MGS_POSE_H_", "")
    assert '#include "mgs.h"' in code


_ADDR = dict(means=0x1000, quats=0x2000, scales=0x3000, sh=0x4000, gids=0x5000, xforms=0x6000, sh_rot=0x7000,
             ct_means=0x8000, ct_quats=0x9000, ct_scales=0xA000, ct_sh=0xB000, v_means=0xC000, v_quats=0xD000,
             v_scales=0xE000, v_sh=0xF000, v_pose=0x10000, workspace=0x20000)


@pytest.mark.parametrize("kw,word", [
    (dict(means=None), b"posed array"),
    (dict(quats=None), b"posed array"),
    (dict(scales=None), b"posed array"),
    (dict(xforms=None), b"xforms is null"),
    (dict(v_pose=None), b"v_pose is null"),
    (dict(n=-1), b"n is negative"),
    (dict(n_groups=0), b"n_groups"),
    (dict(n_groups=-2), b"n_groups"),
    (dict(sh_degree=-1), b"sh_degree"),
    (dict(sh_degree=4), b"sh_degree"),
    (dict(sh_degree=3, coeff_stride=15), b"coeff_stride"),
    (dict(sh_degree=1, coeff_stride=3), b"coeff_stride"),
    (dict(sh_rot=None), b"needs sh_rot"),
    (dict(sh=None), b"without posed SH rows"),                       # ct_sh and v_sh are still given
    (dict(workspace=None), b"workspace is null"),
    (dict(workspace_bytes=0), b"workspace of 0 bytes"),
    (dict(workspace_bytes=-1), b"needed"),                           # one byte short of what the size function reports
    (dict(v_means=None), b"only in part"),
    (dict(v_quats=None), b"only in part"),
    (dict(v_scales=None), b"only in part"),
    (dict(v_sh=None), b"only in part"),
    (dict(v_means=None, v_quats=None, v_scales=None), b"only in part"),     # v_sh alone
])
def test_pose_bwd_argument_errors_are_reported_without_a_gpu(kw, word):
    """mgs_pose_bwd on made-up addresses: every case must be refused before anything is launched."""
    from robosimgs_amd import _lib
    L = _lib.lib()
    a = dict(_ADDR, n=1000, n_groups=3, sh_degree=2, coeff_stride=16, workspace_bytes=None)
    a.update(kw)
    need = L.mgs_pose_bwd_workspace_bytes(1000, 3)
    assert need > 0
    if a["workspace_bytes"] is None:
        a["workspace_bytes"] = need
    elif a["workspace_bytes"] == -1:
        a["workspace_bytes"] = need - 1
    rc = L.mgs_pose_bwd(a["n"], a["means"], a["quats"], a["scales"], a["sh_degree"], a["coeff_stride"], a["sh"], a["gids"],
                        a["n_groups"], a["xforms"], a["sh_rot"], a["ct_means"], a["ct_quats"], a["ct_scales"], a["ct_sh"],
                        a["v_means"], a["v_quats"], a["v_scales"], a["v_sh"], a["v_pose"], a["workspace"],
                        a["workspace_bytes"], None)
    msg = L.mgs_last_error_string()
    assert rc == -1 and word in msg and msg.startswith(b"pose_bwd:"), (rc, msg)


def test_workspace_bytes_is_monotone_in_both_arguments():
    from robosimgs_amd import _lib, pose
    size = _lib.lib().mgs_pose_bwd_workspace_bytes
    assert size(-1, 3) == size(10, 0) == size(10, -1) == 0
    ns = [0, 1, 63, 64, 65, 4097, 300_001, 1_000_000, 2**31 - 1]
    gs = [1, 2, 3, 8, 63, 64, 65, 70, 1000, 2**31 - 1]
    for g in gs:
        col = [size(n, g) for n in ns]
        assert col == sorted(col) and col[0] > 0 and all(v % 256 == 0 for v in col)
    for n in ns:
        row = [size(n, g) for g in gs]
        assert row == sorted(row)
    assert size(2**31 - 1, 64) > 2**32                                   # no 32-bit wrap in the layout
    up = lambda b: max(256, -(-b // 256) * 256)
    for n, g in ((1, 1), (4097, 3), (4097, 70), (300_001, 3), (1_000_000, 8)):
        waves = (n + 63) // 64
        chunks = (waves + 63) // 64
        # a count per wave; a row of 32 bytes per wave and group id it can hold (at most 64); 64 bytes per group and chunk
        assert size(n, g) == up(4 * waves) + up(32 * waves * min(g, 64)) + up(64 * chunks * g), (n, g)
    assert pose.workspace_bytes(4097, 3) == size(4097, 3)


# ---- pack_transforms_torch ----------------------------------------------------------------------------------
def _branch_rotations():
    """Proper rotations that take each branch of _rotmat_to_quat: trace > 0, and a half turn (and more) about an axis
    near x, y and z, whose trace is negative and whose largest diagonal entry is R[0,0], R[1,1], R[2,2]."""
    out = [np.eye(3), PR.expm_so3([0.3, -0.2, 0.5])]
    for axis in ([1.0, 0.1, -0.05], [0.08, 1.0, 0.1], [-0.1, 0.07, 1.0]):
        a = np.array(axis) / np.linalg.norm(axis)
        out += [PR.expm_so3(a * 3.0), PR.expm_so3(a * np.pi), PR.expm_so3(a * 3.5)]
    rng = np.random.default_rng(11)
    for _ in range(4):
        q, _r = np.linalg.qr(rng.normal(size=(3, 3)))
        if np.linalg.det(q) < 0:
            q[:, 0] = -q[:, 0]
        out.append(q)
    return np.stack(out)


def _ulps(a, b):
    a, b = np.asarray(a, np.float32), np.asarray(b, np.float32)
    return np.abs(a.astype(np.float64) - b.astype(np.float64)) / np.maximum(np.spacing(np.maximum(np.abs(a), np.abs(b))), 2.0 ** -149)


@pytest.mark.parametrize("degree", [0, 1, 2, 3])
@pytest.mark.parametrize("dtype", [torch.float64, torch.float32])
def test_pack_transforms_torch_matches_pack_transforms(degree, dtype):
    from robosimgs_amd.pose import pack_transforms_torch
    from robosimgs_amd.transform import pack_transforms
    R = _branch_rotations()
    tr, diag = np.trace(R, axis1=1, axis2=2), np.diagonal(R, axis1=1, axis2=2)
    assert (tr > 0).any() and all(((tr <= 0) & (np.argmax(diag, axis=1) == i)).any() for i in range(3))
    rng = np.random.default_rng(2)
    t, s = rng.normal(size=(len(R), 3)) * 2, rng.uniform(0.5, 2.0, len(R))
    Rt, tt, st = (torch.tensor(a, dtype=dtype) for a in (R, t, s))
    for scales_np, scales_t in ((s, st), (None, None)):
        x, rot = pack_transforms_torch(Rt, tt, scales_t, degree)
        # the host packing is handed what the torch one sees (the same dtype's values), so only the arithmetic differs
        xr, rotr = pack_transforms(Rt.double().numpy(), tt.double().numpy(),
                                   None if scales_np is None else st.double().numpy(), degree)
        assert x.dtype == torch.float32 and tuple(x.shape) == xr.shape == (len(R), 20) and not x.requires_grad
        worst = float(_ulps(x.numpy(), xr).max())
        print(f"\ndegree {degree} {dtype}: xforms worst {worst:.2f} ulp", end="")
        assert worst <= 2.0
        assert np.array_equal(x.numpy()[:, 17:], np.zeros((len(R), 3), np.float32))
        if degree == 0:
            assert rot is None and rotr is None
        else:
            assert rot.dtype == torch.float32 and tuple(rot.shape) == rotr.shape == (len(R), 84)
            err = float(np.abs(rot.numpy().astype(np.float64) - rotr).max())
            print(f", sh_rot worst {err:.2e}", end="")
            assert err <= 1e-6 and np.abs(rotr).max() <= 1.0 + 1e-6
            used = sum((2 * l + 1) ** 2 for l in range(1, degree + 1))
            assert not rot.numpy()[:, used:].any()


def test_pack_transforms_torch_takes_no_gradient():
    from robosimgs_amd.pose import pack_transforms_torch
    R = torch.tensor(_branch_rotations()[:3], requires_grad=True)
    x, rot = pack_transforms_torch(R, torch.zeros(3, 3, dtype=torch.float64, requires_grad=True), None, 2)
    assert not x.requires_grad and not rot.requires_grad


# ---- Hinge.pose_torch ---------------------------------------------------------------------------------------
def _hinge(position, axis):
    from robosimgs_amd.articulation import Hinge
    joint = np.zeros(16)
    joint[0:3], joint[3:6] = position, axis
    joint[6], joint[8], joint[9] = 0.9, 7, 9
    return Hinge(joint)


def test_hinge_pose_torch_matches_pose_and_gradcheck():
    rng = np.random.default_rng(5)
    axis = rng.normal(size=3)
    pos = rng.normal(size=3) * 3
    h = _hinge(pos, axis)                                               # an unnormalised axis: both normalise it
    for ang in (0.0, 0.7, -1.9, 3.0):
        R, t = h.pose_torch(torch.tensor(ang, dtype=torch.float64))
        Rn, tn = h.pose(ang)
        assert R.shape == (3, 3) and t.shape == (3,) and R.dtype == torch.float64
        assert np.abs(R.numpy() - Rn).max() <= 1e-12 and np.abs(t.numpy() - tn).max() <= 1e-12
    angles = np.array([0.0, 0.7, -1.9, 3.0])
    R, t = h.pose_torch(torch.tensor(angles))
    Rn, tn = h.pose(angles)
    assert R.shape == (4, 3, 3) and t.shape == (4, 3)
    assert np.abs(R.numpy() - Rn).max() <= 1e-12 and np.abs(t.numpy() - tn).max() <= 1e-12
    assert h.pose_torch(torch.tensor(0.3))[0].dtype == torch.float32
    w = torch.tensor(rng.normal(size=(12,)))
    scalar = lambda a: torch.cat([x.reshape(-1) for x in h.pose_torch(a)]) @ w
    assert torch.autograd.gradcheck(scalar, (torch.tensor(0.4, dtype=torch.float64, requires_grad=True),))
    vec = lambda a: torch.cat([x.reshape(-1) for x in h.pose_torch(a)])
    assert torch.autograd.gradcheck(vec, (torch.tensor([0.4, -2.0], dtype=torch.float64, requires_grad=True),))


# ---- the reference against itself ---------------------------------------------------------------------------
def test_generator_tables_match_central_differences_and_are_antisymmetric():
    from robosimgs_amd import pose
    fd, table = PR.generators_fd(3), pose.sh_generator_matrices(3)
    magnitudes = set()
    for k in range(3):
        for l in (1, 2, 3):
            L = table[k][l]
            assert L.shape == (2 * l + 1, 2 * l + 1) and np.array_equal(L, -L.T)
            assert np.abs(fd[k][l] + fd[k][l].T).max() <= 1e-8
            assert np.abs(L - fd[k][l]).max() <= 1e-8, (k, l)
            magnitudes |= {round(abs(v), 12) for v in L[np.nonzero(L)]}
        nz = [int(np.count_nonzero(table[k][l])) for l in (1, 2, 3)]
        assert nz == ([2, 6, 10] if k < 2 else [2, 4, 6])
    assert magnitudes == {round(v, 12) for v in (1, 3 ** .5, 2, 1.5 ** .5, 2.5 ** .5, 6 ** .5, 3)}
    # the source's table is the Python constant: every pair of csrc/pose.hip's kShGen, in order
    src = open(os.path.join(ROOT, "robosimgs_amd", "csrc", "pose.hip")).read()
    body = src[src.index("kShGen[3][kGenPairs] = {"):src.index("};", src.index("kShGen[3][kGenPairs] = {"))]
    body = re.sub(r"//[^\n]*", "", body)
    const = {"kSqrt3": 3 ** .5, "kSqrt6": 6 ** .5, "kSqrt3_2": 1.5 ** .5, "kSqrt5_2": 2.5 ** .5}
    for name, val in const.items():
        lit = re.search(r"constexpr float %s = ([0-9.]+)f;" % name, src).group(1)
        assert np.float32(lit) == np.float32(val)
    pairs = re.findall(r"\{(\d+), (\d+), (-?)(\w[\w.]*)\}", body)
    got = [(int(a), int(b), (-1 if sg else 1) * (const[v] if v in const else float(v.rstrip("f")))) for a, b, sg, v in pairs]
    got = [e for e in got if e[2] != 0]
    want = [e for axis in pose.SH_GENERATORS for e in axis]
    assert len(got) == len(want) == 24 and all(g[:2] == w[:2] and abs(g[2] - w[2]) < 1e-15 for g, w in zip(got, want))


def _posed_fp64(inp, K, degree, R, t, s):
    """The forward in fp64: transform_ref for means, scales and colours, and q_R (x) q for the quaternions."""
    from robosimgs_amd.gaussians import _quat_mul, _rotmat_to_quat
    ref = FR.transform_ref(inp["means"], inp["quats"], inp["scales"], inp["colors"], degree, inp["gids"], len(R), R, t, s)
    q = inp["quats"].astype(np.float64).copy()
    for g in range(len(R)):
        sel = inp["gids"] == g
        q[sel] = _quat_mul(_rotmat_to_quat(R[g])[None], q[sel])
    return ref["means"][0], q, ref["scales"][0], ref["colors"][0]


@pytest.mark.parametrize("K,degree", [(16, 3), (9, 2), (4, 1)])
def test_reference_matches_central_differences_of_the_forward(K, degree):
    from robosimgs_amd.gaussians import _rotmat_to_quat
    n, G = 200, 3
    inp = FR.transform_inputs(n, K)
    R, t, s = np.stack(inp["rotations"]), np.stack(inp["translations"]), np.array(inp["group_scales"])
    ct = [a.astype(np.float64) for a in PR.cotangents(n, K)]

    def loss(R_, t_, s_):
        m, q, sc, c = _posed_fp64(inp, K, degree, R_, t_, s_)
        return (ct[0] * m).sum() + (ct[1] * q).sum() + (ct[2] * sc).sum() + (ct[3] * c).sum()

    def xforms(R_, t_, s_):
        x = np.zeros((G, 20))
        for g in range(G):
            x[g, :9], x[g, 9:12], x[g, 12:16], x[g, 16] = (s_[g] * R_[g]).reshape(9), t_[g], _rotmat_to_quat(R_[g]), s_[g]
        return x
    from robosimgs_amd.gaussians import sh_rotation_matrices
    rot = np.zeros((G, 84))
    for g in range(G):
        rot[g, :sum((2 * l + 1) ** 2 for l in range(1, degree + 1))] = np.concatenate(
            [M.reshape(-1) for M in sh_rotation_matrices(R[g], degree)[1:]])
    m, q, sc, c = _posed_fp64(inp, K, degree, R, t, s)
    ref = PR.pose_ref(m, q, sc, c, degree, inp["gids"], G, xforms(R, t, s), rot, *ct)
    v = ref["v_pose"][0]
    # the same formulas fed the closed-form table the kernel uses (pose.SH_GENERATORS): the two agree far inside 1e-7
    from robosimgs_amd import pose
    closed = PR.pose_ref(m, q, sc, c, degree, inp["gids"], G, xforms(R, t, s), rot, *ct,
                         generators=pose.sh_generator_matrices(degree))["v_pose"][0]
    assert np.abs(closed - v).max() <= 1e-8 * np.abs(v).max()
    eps, worst = 1e-5, 0.0
    for g in range(G):
        for k in range(7):
            Rp, Rm, tp, tm, sp, sm = R.copy(), R.copy(), t.copy(), t.copy(), s.copy(), s.copy()
            e = np.zeros(3)
            e[k % 3] = eps
            if k < 3:
                Rp[g], Rm[g] = PR.expm_so3(e) @ R[g], PR.expm_so3(-e) @ R[g]
            elif k < 6:
                tp[g], tm[g] = t[g] + e, t[g] - e
            else:
                sp[g], sm[g] = s[g] * np.exp(eps), s[g] * np.exp(-eps)
            fd = (loss(Rp, tp, sp) - loss(Rm, tm, sm)) / (2 * eps)
            worst = max(worst, abs(fd - v[g, k]) / abs(v[g, k]))
    print(f"\nK {K} degree {degree}: worst relative difference to central differences {worst:.2e}")
    assert worst <= 1e-7
    assert not v[:, 7].any()
    # the rest-pose gradients are the transposed forward, which is affine in the rest pose: <v_x, dx> = <ct, F(dx) - F(0)>
    rng = np.random.default_rng(9)
    dirs = {k_: rng.normal(size=inp[k_].shape).astype(np.float32) for k_ in ("means", "quats", "scales", "colors")}

    def at(arrays):
        with np.errstate(invalid="ignore"):            # transform_ref also normalises the quaternions: 0 / 0 at the zero arrays
            m_, q_, s_, c_ = _posed_fp64(dict(inp, **arrays), K, degree, R, t, s)
        return (ct[0] * m_).sum() + (ct[1] * q_).sum() + (ct[2] * s_).sum() + (ct[3] * c_).sum()
    pair = sum((ref[name][0] * dirs[k_]).sum() for name, k_ in (("v_means", "means"), ("v_quats", "quats"),
                                                                ("v_scales", "scales"), ("v_sh", "colors")))
    assert abs(pair - (at(dirs) - at({k_: np.zeros_like(v_) for k_, v_ in dirs.items()}))) <= 1e-9 * abs(pair)


def test_tangent_to_ambient_rule():
    """<1/2 [v]x R, [d]x R> = v . d, and what pose.py's backward forms is that matrix."""
    from robosimgs_amd.pose import _skew_times
    rng = np.random.default_rng(4)
    skew = lambda w: np.array([[0, -w[2], w[1]], [w[2], 0, -w[0]], [-w[1], w[0], 0]])
    Rs, _t, _s = PR.random_poses(5, seed=3)
    for R in Rs:
        v = rng.normal(size=3)
        vR = PR.tangent_to_ambient(v, R)
        got = 0.5 * _skew_times(torch.tensor(v)[None], torch.tensor(R)[None])[0].numpy()
        assert np.abs(got - vR).max() <= 1e-15
        for _ in range(4):
            d = rng.normal(size=3)
            assert abs((vR * (skew(d) @ R)).sum() - v @ d) <= 1e-13
        assert np.abs(vR @ R.T + (vR @ R.T).T).max() <= 1e-15          # tangent: v_R R^T is antisymmetric, nothing normal
