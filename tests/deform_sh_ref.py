"""fp64 statement of the SH part of mgs_deform_apply_sh (include/mgs_deform_sh.h, csrc/deform.hip, csrc/sh_rotate.h) with the
bound each rotated band is held to.  A helper module, not a test file: tests/test_deform_sh_host.py checks it against closed
forms and against a NumPy emulation of the kernel's fp32 arithmetic without a GPU, tests/test_gpu_deform_sh.py holds the
kernel to it.  Geometry and status are not restated here: they are mgs_deform_apply's bytes (tests/deform_ref.py).

The rotation and its bound come from deform_ref.apply_ref on the GPU's own stored binding with status_seen=: `rot` holds
R_ref R(q) for every row past the thin test (affine rows included), so R_ref = rot R(q)^T, and its Frobenius bound is
rot_b - 3 GAMMA (the 3 GAMMA there belong to the rounding of the output quaternion, which the SH rows never see).
M_l(R_ref) is robosimgs_amd.gaussians.sh_rotation_matrices in fp64: a least-squares fit of the defining property
sum_k Y_k(d) c'_k = sum_k Y_k(R^T d) c_k on 64 directions, which shares nothing with what the kernel does.

The gate, per rotated row, band l and channel:   ||c'_gpu - M_l(R_ref) c_l||_2 <= (1.01 l bound_R / sqrt 2 + a_l) ||c_l||_2.
  first term   ||M_l(R1) - M_l(R2)||_2 <= l theta and ||R1 - R2||_F = 2 sqrt 2 sin(theta / 2): the kernel's fp64 R is within
               bound_R of R_ref, and M_l is orthogonal, so the error of R reaches c' as at most l bound_R / sqrt 2 (1.01
               for sin against its argument and second order).
  a_l          the counted rounding of the kernel's fp32 evaluation on its fp32-rounded R (below).
The norm check ||c'_l|| against ||c_l|| within a_l ||c_l|| holds whatever R the kernel found: M_l of any rotation is
orthogonal, and the kernel's fp32 R is a rotation to the rounding that a_l counts.

a_l.  U = 2^-24, GAMMA = 1.01 U; a chain of k roundings over a sum is within k GAMMA sum|terms|; an fma only removes roundings.
  band 1   c' = Pi u, u = R v, v = Pi^T c: signs are exact; u_a is a product and two fma (3) on entries of R rounded once (1):
           |du_a| <= 4 GAMMA sum_j |R_aj| |v_j|, so ||du||_2 <= 4 GAMMA || |R| ||_2 ||c||_2 <= 4 sqrt 3 GAMMA ||c||_2
           (|| |R| ||_2 <= ||R||_F).  a_1 = 1.01 * 4 sqrt 3 GAMMA.
  band l = 2, 3.  c' = W F, F_k = y(t_k) . c, t_k = R^T d_k, exactly B c' = F with B_kj = Y_j(d_k), W = B^-1, for the fp32
           directions d_k as they are, because y is evaluated in homogeneous form (both sides of the defining property are
           homogeneous polynomials of degree l in d, so it holds off the unit sphere too).
    t      a product and two fma (3) on entries of R rounded once (1): |dt_a| <= 4 GAMMA sum_b |R_ba| |d_b| <= 4 GAMMA |d_k|,
           so ||dt||_2 <= 4 sqrt 3 GAMMA 1.01 =: e_t (|d_k| = 1 to 1e-7).
    y(t)   moving t: on the unit sphere ||y||_2 = N_l = sqrt((2l+1) / 4 pi) and, from the addition theorem
           sum_m Y_lm(a) Y_lm(b) = N_l^2 P_l(a.b), the derivative along a unit tangent has norm N_l sqrt(l (l+1) / 2)
           (P_l'(1) = l (l+1) / 2), the radial one N_l l (homogeneity), and the two are orthogonal:
           ||dy||_2 <= 1.01 N_l sqrt(l^2 + l (l+1) / 2) e_t.
           rounding: every Y_j is evaluated with at most 7 roundings on any monomial's path (the longest, Y_12's y^2 z:
           y y, s, 3 s, the fma, z *, K7 *, and K7's own rounding): |dY_j| <= 7 GAMMA Ybar_j(t), Ybar_j the polynomial with
           every monomial in absolute value.  On the unit sphere |x y| <= 1/2, |x y z| <= 1 / (3 sqrt 3), x^2 |y| <=
           2 / (3 sqrt 3), z^2 + 1 <= 2, which gives ||Ybar||_2 <= 1.27 (band 2) and 3.32 (band 3) -- YBAR, recomputed from
           those four facts in `_ybar`.
    F_k    a product and 2l fma (2l + 1): (2l + 1) GAMMA sum_j |Y_j c_j| <= (2l + 1) GAMMA 1.01 N_l ||c||.
           So |dF_k| <= (||dy|| + 7 GAMMA 1.01 YBAR_l + (2l + 1) GAMMA 1.01 N_l) ||c|| =: f_l ||c||, ||dF||_2 <= sqrt(2l+1) f_l ||c||.
    c'     a product and 2l fma (2l + 1) on entries of W rounded once (1): |dc'_m| <= (2l + 2) GAMMA sum_k |W_mk| |F_k|, in
           norm (2l + 2) GAMMA ||W||_F ||F||_2 with ||F||_2 = ||B M_l c||_2 <= ||B||_2 ||c||_2; and W dF: ||W||_2 ||dF||_2.
    a_l = 1.01 (||W||_2 sqrt(2l+1) f_l + (2l + 2) GAMMA ||W||_F ||B||_2 1.01).
  With the tables of sh_rotate.h (cond B 1.55 and 1.74): a_1 = 4.2e-7, a_2 = 7.6e-6, a_3 = 1.6e-5.
"""
import os
import re

import numpy as np

import deform_ref as DR
from frame_helper_ref import GAMMA, U

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SH_ROTATE_H = os.path.join(ROOT, "robosimgs_amd", "csrc", "sh_rotate.h")

_f32, _f64 = DR._f32, DR._f64
fma32 = DR.fma32

K1, K2, K3 = 1.092548430592079, 0.31539156525252, 0.5462742152960395
K4, K5, K6, K7, K8 = 0.5900435899266435, 2.890611442640554, 0.4570457994644658, 0.3731763325901154, 1.445305721320277
EVAL_ROUNDINGS = 7

# the sample directions of sh_rotate.h, as the fp32 numbers they are
DIRS = {
    2: _f32([[-0.0929295272, -0.633738637, -0.767944932], [-0.774724364, -0.570928991, -0.271739185],
             [0.783877194, -0.222405255, 0.579717577], [-0.245348543, 0.967244864, 0.0651267916],
             [-0.87374717, 0.416757822, 0.250756472]]),
    3: _f32([[-0.417904168, 0.844621181, 0.334620893], [0.318835586, 0.669778705, -0.670626879],
             [-0.879883766, 0.450533539, 0.151076302], [0.718422353, -0.162688896, -0.676314771],
             [-0.839191675, -0.421071529, 0.344174534], [0.218622223, 0.964782119, -0.146286547],
             [-0.391046286, 0.853818178, -0.343623877]]),
}


def band_basis(l, t):
    """The band's 2l+1 basis functions in homogeneous form at t [...,3], fp64: gaussians._sh_basis_np on the unit sphere."""
    t = _f64(t)
    x, y, z = t[..., 0], t[..., 1], t[..., 2]
    xx, yy, zz = x * x, y * y, z * z
    if l == 1:
        c1 = 0.48860251190292
        return np.stack([-c1 * y, c1 * z, -c1 * x], -1)
    if l == 2:
        return np.stack([K1 * x * y, -K1 * y * z, K2 * (2 * zz - xx - yy), -K1 * x * z, K3 * (xx - yy)], -1)
    q = 4 * zz - xx - yy
    return np.stack([K4 * y * (yy - 3 * xx), K5 * x * y * z, -K6 * y * q, K7 * z * (2 * zz - 3 * (xx + yy)), -K6 * x * q,
                     K8 * z * (xx - yy), -K4 * x * (xx - 3 * yy)], -1)


def tables(l):
    """(B, W) in fp64 for band l = 2, 3: B_kj = Y_j(d_k) at the fp32 directions, W = B^-1."""
    B = band_basis(l, DIRS[l])
    return B, np.linalg.inv(B)


def header_tables():
    """{(name, l): fp32 array} of the kDir / kInv tables as csrc/sh_rotate.h spells them."""
    text = open(SH_ROTATE_H).read()
    out = {}
    for l in (2, 3):
        body = text[text.index("struct ShBandTables<%d>" % l):]
        body = body[:body.index("};\n};") + 5]
        for name in ("kDir", "kInv"):
            m = re.search(r"%s\[(\d+)\]\[(\d+)\]\s*=\s*\{(.*?)\};" % name, body, flags=re.S)
            vals = [np.float32(v) for v in re.findall(r"(-?\d+\.\d+(?:e-?\d+)?)f", m.group(3))]
            out[(name, l)] = np.array(vals, np.float32).reshape(int(m.group(1)), int(m.group(2)))
    return out


def _ybar(l):
    """||Ybar||_2 on the unit sphere from |x y| <= 1/2, |x y z| <= 1 / (3 sqrt 3), x^2 |y| <= 2 / (3 sqrt 3), 1 + z^2 <= 2."""
    h, t3, c = 0.5, 1 / (3 * np.sqrt(3)), 2 / (3 * np.sqrt(3))
    if l == 2:                                  # K1 |xy|, K1 |yz|, K2 (2 zz + xx + yy = 1 + zz), K1 |xz|, K3 (xx + yy)
        v = [K1 * h, K1 * h, K2 * 2, K1 * h, K3]
    else:                                       # |y| (3 xx + yy), |xyz|, |y| (4 zz + xx + yy), |z| (2 zz + 3 xx + 3 yy), ...
        v = [K4 * (3 * c + 1), K5 * t3, K6 * (4 * c + c + 1), K7 * (2 + 6 * c), K6 * (4 * c + c + 1), K8 * 2 * c, K4 * (3 * c + 1)]
    return float(np.linalg.norm(v))


YBAR = {2: _ybar(2), 3: _ybar(3)}


def a_l(l):
    """The counted rounding of band l (the module docstring), relative to ||c_l||_2."""
    if l == 1:
        return 1.01 * 4 * np.sqrt(3) * GAMMA
    B, W = tables(l)
    m = 2 * l + 1
    N = np.sqrt(m / (4 * np.pi))
    e_t = 4 * np.sqrt(3) * GAMMA * 1.01
    dy = 1.01 * N * np.sqrt(l * l + l * (l + 1) / 2) * e_t
    f = dy + EVAL_ROUNDINGS * GAMMA * 1.01 * YBAR[l] + m * GAMMA * 1.01 * N
    return float(1.01 * (np.linalg.norm(W, 2) * np.sqrt(m) * f + (m + 1) * GAMMA * np.linalg.norm(W) * np.linalg.norm(B, 2) * 1.01))


A = {l: a_l(l) for l in (1, 2, 3)}


# ---- M_l(R) in fp64: gaussians.sh_rotation_matrices, batched -----------------------------------------------------------------
def sh_matrices(R, degree):
    """[n,3,3] -> {l: [n,2l+1,2l+1]} for l = 1..degree: sh_rotation_matrices' own fit (the same sample directions, the same
    pseudo-inverses, the same basis) evaluated for all rows at once; the host test holds it to the function row by row."""
    from robosimgs_amd.gaussians import _sh_basis_np, _sh_fit_basis
    R = _f64(R)
    d, pinv = _sh_fit_basis(degree)
    t = np.einsum("ma,nab->nmb", d, R)                                    # rows are (R^T d)^T
    Y_old = _sh_basis_np(degree, t.reshape(-1, 3)).reshape(R.shape[0], d.shape[0], -1)
    return {l: np.einsum("km,nmj->nkj", pinv[l], Y_old[:, :, l * l:(l + 1) * (l + 1)]) for l in range(1, degree + 1)}


def rotation_of(ref, quats):
    """(R_ref [n,3,3], Frobenius bound [n]) from apply_ref's `rot` = R_ref R(q): rows past the thin test only are meaningful."""
    rot, rot_b = ref["rot"]
    return rot @ np.transpose(DR.quat_to_rot(quats), (0, 2, 1)), rot_b - 3 * GAMMA


def rotated_rows(ref):
    """The rows whose SH bands turn: past the thin test (branch 2 rigid, 3 affine)."""
    return ref["branch"] >= 2


def expected_rows(colors, R, degree, rows):
    """fp64 rows [n,K,3]: band l of `rows` is M_l(R) c_l, everything else the input."""
    out = _f64(colors).copy()
    if degree >= 1 and rows.any():
        M = sh_matrices(R[rows], degree)
        for l in range(1, degree + 1):
            out[rows, l * l:(l + 1) * (l + 1)] = np.einsum("nkj,njc->nkc", M[l], _f64(colors)[rows, l * l:(l + 1) * (l + 1)])
    return out


def check_sh(ref, quats, colors, out_colors, degree, written=None):
    """Hold out_colors [n,K,3] to the rule.  ref = apply_ref(..., status_seen=status).  written: bool [n], the rows the call
    writes (None: all); the others are not looked at.  Bit-identity where the header promises it, the gate elsewhere.
    Returns {"band1": worst error / bound, ..., "norm": worst | ||c'|| - ||c|| | / (a_l ||c||), "bound_R": max, "rotated": count}."""
    colors, out_colors = _f32(colors), _f32(out_colors)
    n, K = colors.shape[:2]
    rows = rotated_rows(ref) & (degree >= 1)
    written = np.ones(n, bool) if written is None else np.asarray(written, bool)
    same = lambda a, b: a.view(np.uint32).tolist() == b.view(np.uint32).tolist()
    keep = written & ~rows
    assert same(out_colors[keep], colors[keep]), "a row that does not rotate is not the input's bits"
    rows = rows & written
    assert same(out_colors[rows, 0], colors[rows, 0]), "coefficient 0 of a rotated row is not the input's bits"
    top = (degree + 1) ** 2
    assert same(out_colors[rows, top:], colors[rows, top:]), "a coefficient above the active degree is not the input's bits"
    res = {"rotated": int(rows.sum()), "norm": 0.0, "bound_R": 0.0}
    if not rows.any():
        return res
    R, bR = rotation_of(ref, quats)
    assert np.isfinite(bR[rows]).all(), "a rotated row has no bound on its rotation: it would be exempt"
    res["bound_R"] = float(bR[rows].max())
    want = expected_rows(colors, R, degree, rows)
    got = _f64(out_colors)
    for l in range(1, degree + 1):
        sl = slice(l * l, (l + 1) * (l + 1))
        cn = np.linalg.norm(_f64(colors)[rows, sl], axis=1)                       # [nr,3]: per channel
        err = np.linalg.norm(got[rows, sl] - want[rows, sl], axis=1)
        bound = (1.01 * l * bR[rows] / np.sqrt(2))[:, None] + A[l]
        tiny = np.finfo(np.float64).tiny
        res["band%d" % l] = float((err / np.maximum(bound * cn, tiny)).max())
        gn = np.linalg.norm(got[rows, sl], axis=1)
        res["norm"] = max(res["norm"], float((np.abs(gn - cn) / np.maximum(A[l] * cn, tiny)).max()))
    return res


# ---- the kernel's fp32 arithmetic in NumPy ----------------------------------------------------------------------------------
def _eval32(l, x, y, z):
    """sh_band_eval: the band at fp32 (x, y, z) [n], one rounding per operation, fma where the header writes one."""
    f = np.float32
    yy, zz = y * y, z * z
    s = fma32(x, x, yy)
    if l == 2:
        return [f(K1) * (x * y), f(-K1) * (y * z), f(K2) * fma32(f(2), zz, -s), f(-K1) * (x * z), f(K3) * fma32(x, x, -yy)]
    xx, q = x * x, fma32(f(4), zz, -s)
    return [f(K4) * (y * fma32(f(-3), xx, yy)), f(K5) * ((x * y) * z), f(-K6) * (y * q),
            f(K7) * (z * fma32(f(2), zz, -(f(3) * s))), f(-K6) * (x * q), f(K8) * (z * fma32(x, x, -yy)),
            f(-K4) * (x * fma32(f(-3), yy, xx))]


def emulate_rotate(R, colors, degree, W32=None):
    """Every row of colors [n,K,3] (fp32) turned by its R [n,3,3] (rounded to fp32 here, as the kernel does with its fp64 R)
    in the kernel's order of operations.  W32: {l: fp32 W} (default: W of `tables` rounded once)."""
    R = _f32(R)
    c = _f32(colors)
    out = c.copy()
    if degree >= 1:
        v = [-c[:, 3], -c[:, 1], c[:, 2]]                                        # [n,3] each: per channel
        u = [fma32(R[:, a, 2, None], v[2], fma32(R[:, a, 1, None], v[1], R[:, a, 0, None] * v[0])) for a in range(3)]
        out[:, 1], out[:, 2], out[:, 3] = -u[1], u[2], -u[0]
    for l in range(2, degree + 1):
        m = 2 * l + 1
        W = _f32(tables(l)[1]) if W32 is None else W32[l]
        cl = c[:, l * l:l * l + m]                                               # [n,m,3]
        F = []
        for k in range(m):
            d = DIRS[l][k]
            t = [fma32(R[:, 2, a], d[2], fma32(R[:, 1, a], d[1], R[:, 0, a] * d[0])) for a in range(3)]
            Y = _eval32(l, *t)
            acc = Y[0][:, None] * cl[:, 0]
            for j in range(1, m):
                acc = fma32(Y[j][:, None], cl[:, j], acc)
            F.append(acc)
        for r in range(m):
            acc = W[r, 0] * F[0]
            for k in range(1, m):
                acc = fma32(W[r, k], F[k], acc)
            out[:, l * l + r] = acc
    return out


def random_colors(n, K, seed):
    """[n,K,3] fp32 rows with every band populated, a few bands exactly zero and a few tiny."""
    rng = np.random.default_rng(seed)
    c = rng.normal(0.0, 0.3, (n, K, 3))
    if n > 8:
        c[5, 1:4] = 0.0
        c[6, 4:] *= 1e-20
    return _f32(c)
