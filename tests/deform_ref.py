"""fp64 statement of mgs_deform_bind and mgs_deform_apply (include/mgs_deform.h, csrc/deform.hip) with the error bound each
value is held to.  A helper module, not a test file: tests/test_deform_host.py checks it against closed forms and against a
NumPy emulation of the kernels' fp32 arithmetic without a GPU, tests/test_gpu_deform.py holds the kernels to it.

The formulas are the header's, evaluated in NumPy fp64 on the arrays the kernels read.  Each link is held on its own: the
bind stage is restated at the neighbour indices the GPU chose, the apply stage on the GPU's own stored fp32 idx, w, p and
rest.  U = 2^-24 is one fp32 rounding, GAMMA = 1.01 U (frame_helper_ref): a value formed by k chained roundings of a sum of
terms is within k GAMMA sum|terms| of the exact sum, and a fused multiply-add only removes roundings.  Factors 1.01 absorb
second-order terms (every relative error here is below 1e-2).

Bind stage.
  d2      the kernel's fp32 d2 = fma(dz, dz, fma(dy, dy, dx dx)): each difference is rounded once and enters squared (2),
          the product and the two fma round the running sum (3): |d2~ - d2| <= 5 GAMMA d2 (C_D2).  This is also the
          bound of rest row 9, h^2 = d2_7, and of the neighbour choice (`check_neighbours`): the GPU orders by d2~, so a
          chosen neighbour is at most d2_8th (1 + 10.1 GAMMA) away and a rejected one at least d2_8th (1 - 10.1 GAMMA).
  w       t_j = d2_j / h^2 carries both roundings, |dt_j| <= 10 GAMMA t_j =: a_j; through exp's derivative the raw weight
          moves by a_j relative; the normalising sum moves by abar = sum a_k w_k relative: |dw_j| <= 1.01 w_j (a_j + abar)
          =: ew_j, plus the one rounding of the stored value, GAMMA w_j.
  Xbar    the weights sum to 1 on both sides, so dXbar = sum dw_j (X_j - Xbar): ec = sum ew_j |r_j| per component, plus the
          fp64 summation of the eight terms on either side, 2 K eps64 sum w_j |X_j| (it is all there is where a component
          of every r_j vanishes: neighbours in a lattice plane).
  d0      ec + GAMMA |d0|.
  p_j     ew_j |r_j| + w_j ec + GAMMA |p_j|.
  Q       eQ = 1.01 sum (ew_j |r_j r_j^T| + w_j (ec |r_j|^T + |r_j| ec^T)), entrywise.
  Q^-1    dQ^-1 = -Q^-1 dQ Q^-1: 1.01 |Q^-1| eQ |Q^-1| + GAMMA |Q^-1| + FP64_INV max|Q^-1| (the fp64 inverse by cofactors at a
          condition number of at most 1e3, the flat threshold).
  ratios  Weyl: |d lambda_k| <= ||eQ||_F, so |d rho| <= 1.01 (1 + rho) ||eQ||_F / lambda_max + GAMMA rho + FP64_EIG.
  flags   flat / thin are compared where the ratio is farther from 1e-3 than its bound; nearer, either value stands (the
          test counts those rows).

Apply stage (on the stored binding, so no error of the bind enters).
  e_j     one rounding each.  c = sum_{1..7} w_j e_j and P = sum e_j p_j^T: seven terms, a product and six fma (7) and the
          rounding of e (1): (k + 1) GAMMA sum|terms| with k = 7 -- eC, eP.  xbar = x_0 + c adds GAMMA |xbar|.
  thin    mu' = xbar + d0: e_xbar + GAMMA |mu'|.  quats and scales are the input's bits.
  rigid   the rotation is the polar factor of P restricted to SO(3); first order (Kenney & Laub; Higham, Functions of
          Matrices, thm 8.9 adapted to the constrained factor):  ||R - R_ref||_F <= 2 ||dP||_F / (sigma_mid + s sigma_min),
          s = sign det P, with ||dP||_F <= ||eP||_F, times 1.01.  The kernel solves P^T P in fp64, which squares the
          condition: an error of 8 eps64 sigma_max^2 in P^T P acts like dP <= 8 eps64 sigma_max^2 / (2 sigma_mid), so the
          allowance for the fp64 solve is 8 eps64 sigma_max^2 / (sigma_mid (sigma_mid + s sigma_min)) (at most 2e-9 at the
          thin threshold).  mu' = xbar + R d0, rounded once: e_xbar + ||dR||_F ||d0|| + GAMMA |mu'|.  The output quaternion
          is compared as a matrix: R(q' / |q'|) against R_ref R(q / |q|); the four roundings of q' move it by at most
          2 sqrt(2) U in Frobenius norm (3 GAMMA).  scales are the input's bits.
  affine  |dA| <= |dP| |Q^-1| + 4 GAMMA |P| |Q^-1| (eA; three-term fma chains).  mu' = xbar + A d0 in fp32:
          e_xbar + eA |d0| + 3 GAMMA |A| |d0| + GAMMA |mu'|.  The covariance R(q') diag(s'^2) R(q')^T of the outputs is held
          against A Sigma A^T in fp64, entrywise: 1.01 (eA |Sigma A^T| + |A Sigma| eA^T) from dA, and for the roundings of
          s' (2 U of each eigenvalue) and q' (2 sqrt(2) U in Frobenius norm, twice) 8 GAMMA ||Sigma'||_F, plus FP64_EIG
          ||Sigma'||_F.  Quaternions and the order of scales are never compared directly.
  branch  sigma_mid(P) < 1e-3 sigma_max(P) and det A <= 0 are decided on P~ and A~ by the kernel; where the fp64 value is
          nearer to the threshold than its own bound the kernel's branch is followed (`free` bits of the status).
"""
import numpy as np

from frame_helper_ref import GAMMA, U

K = 8
REST_ROWS = 12
TH = 1e-3
C_D2 = 5
EPS64 = 2.0 ** -52
FP64_INV = 1e-11
FP64_EIG = 1e-13
FLAG_UNBOUND, FLAG_FLAT, FLAG_THIN = 1, 2, 4
ST_UNBOUND, ST_FALLBACK, ST_THIN, ST_NONFINITE = 1, 2, 4, 8
FLT_MIN = float(np.finfo(np.float32).tiny)

_f64 = lambda a: np.asarray(a, dtype=np.float64)
_f32 = lambda a: np.asarray(a, dtype=np.float32)


def fma32(a, b, c):
    """fp32 fused multiply-add: the product is exact in fp64, the sum is rounded to fp64 and then to fp32."""
    return (_f64(a) * _f64(b) + _f64(c)).astype(np.float32)


# ---- quaternions and rotations (wxyz) ------------------------------------------------------------------------------------
def quat_to_rot(q):
    """[n,4] wxyz -> [n,3,3] of q / |q|, fp64."""
    q = _f64(q)
    q = q / np.linalg.norm(q, axis=-1, keepdims=True)
    w, x, y, z = q[..., 0], q[..., 1], q[..., 2], q[..., 3]
    R = np.empty(q.shape[:-1] + (3, 3))
    R[..., 0, 0] = 1 - 2 * (y * y + z * z); R[..., 0, 1] = 2 * (x * y - w * z); R[..., 0, 2] = 2 * (x * z + w * y)
    R[..., 1, 0] = 2 * (x * y + w * z); R[..., 1, 1] = 1 - 2 * (x * x + z * z); R[..., 1, 2] = 2 * (y * z - w * x)
    R[..., 2, 0] = 2 * (x * z - w * y); R[..., 2, 1] = 2 * (y * z + w * x); R[..., 2, 2] = 1 - 2 * (x * x + y * y)
    return R


def rot_to_quat(R):
    """[n,3,3] proper rotations -> [n,4] wxyz unit quaternions, by the largest pivot (the kernel's rule)."""
    R = _f64(R)
    r = lambda a, b: R[..., a, b]
    tr = r(0, 0) + r(1, 1) + r(2, 2)
    piv = np.stack([tr, np.where(tr > 0, -np.inf, r(0, 0)), np.where(tr > 0, -np.inf, r(1, 1)),
                    np.where(tr > 0, -np.inf, r(2, 2))], -1)
    which = np.where(tr > 0, 0, 1 + np.argmax(piv[..., 1:], axis=-1))
    s = 2 * np.sqrt(np.maximum(1e-300, np.stack([tr + 1, 1 + r(0, 0) - r(1, 1) - r(2, 2), 1 + r(1, 1) - r(0, 0) - r(2, 2),
                                                 1 + r(2, 2) - r(0, 0) - r(1, 1)], -1)))
    cand = np.stack([
        np.stack([0.25 * s[..., 0], (r(2, 1) - r(1, 2)) / s[..., 0], (r(0, 2) - r(2, 0)) / s[..., 0], (r(1, 0) - r(0, 1)) / s[..., 0]], -1),
        np.stack([(r(2, 1) - r(1, 2)) / s[..., 1], 0.25 * s[..., 1], (r(0, 1) + r(1, 0)) / s[..., 1], (r(0, 2) + r(2, 0)) / s[..., 1]], -1),
        np.stack([(r(0, 2) - r(2, 0)) / s[..., 2], (r(0, 1) + r(1, 0)) / s[..., 2], 0.25 * s[..., 2], (r(1, 2) + r(2, 1)) / s[..., 2]], -1),
        np.stack([(r(1, 0) - r(0, 1)) / s[..., 3], (r(0, 2) + r(2, 0)) / s[..., 3], (r(1, 2) + r(2, 1)) / s[..., 3], 0.25 * s[..., 3]], -1)], -2)
    q = np.take_along_axis(cand, which[..., None, None], axis=-2)[..., 0, :]
    return q / np.linalg.norm(q, axis=-1, keepdims=True)


def quat_mul(a, b):
    a, b = _f64(a), _f64(b)
    aw, ax, ay, az = (a[..., k] for k in range(4))
    bw, bx, by, bz = (b[..., k] for k in range(4))
    return np.stack([aw * bw - ax * bx - ay * by - az * bz, aw * bx + ax * bw + ay * bz - az * by,
                     aw * by - ax * bz + ay * bw + az * bx, aw * bz + ax * by - ay * bx + az * bw], -1)


def kabsch(P):
    """argmax over SO(3) of tr(R^T P) by SVD, fp64: [n,3,3] -> (R [n,3,3], singular values descending [n,3], sign det P)."""
    Uu, S, Vt = np.linalg.svd(_f64(P))
    d = np.sign(np.linalg.det(Uu) * np.linalg.det(Vt))
    d = np.where(d == 0, 1.0, d)
    D = np.zeros_like(Uu)
    D[..., 0, 0] = D[..., 1, 1] = 1.0
    D[..., 2, 2] = d
    return Uu @ D @ Vt, S, d


# ---- the bind --------------------------------------------------------------------------------------------------------------
def d2_exact(means, parts):
    """fp64 squared distances of the fp32 inputs [n,m]; +inf where either point is non-finite."""
    mu, X = _f64(means), _f64(parts)
    with np.errstate(invalid="ignore", over="ignore"):
        D = ((mu[:, None, :] - X[None, :, :]) ** 2).sum(-1)
    bad = ~np.isfinite(mu).all(1)[:, None] | ~np.isfinite(X).all(1)[None, :]
    D[bad] = np.inf
    return D


def d2_fp32(means, parts):
    """The kernel's fp32 d2 [n,m] (difference form, two fma); +inf where either point is non-finite."""
    mu, X = _f32(means), _f32(parts)
    with np.errstate(invalid="ignore", over="ignore"):
        dx, dy, dz = (mu[:, None, k] - X[None, :, k] for k in range(3))
        D = fma32(dz, dz, fma32(dy, dy, dx * dx))
    bad = ~np.isfinite(mu).all(1)[:, None] | ~np.isfinite(X).all(1)[None, :]
    D[bad] = np.inf
    return D


def knn_ref(D, select=None, max_distance=np.inf):
    """The 8 smallest of every row of D [n,m] by the key (d2, j), ascending: idx int32 [8,n] (-1 in every row of an unbound
    Gaussian) and their d2 [8,n].  D must hold +inf for pairs that take no part."""
    n, m = D.shape
    order = np.argsort(D, axis=1, kind="stable")[:, :K]              # stable: a tie goes to the lower index
    d = np.take_along_axis(D, order, axis=1)
    ok = np.isfinite(d[:, K - 1]) if m >= K else np.zeros(n, bool)
    if select is not None:
        ok &= np.asarray(select) != 0
    with np.errstate(invalid="ignore"):
        ok &= ~(np.sqrt(d[:, 0].astype(np.float32)) > np.float32(max_distance))
    idx = np.where(ok[None, :], order.T, -1).astype(np.int32)
    return idx, np.where(ok[None, :], d.T, 0.0)


def check_neighbours(means, parts, idx):
    """Every chosen neighbour's fp64 d2 is at most the 8th smallest (1 + 10.1 GAMMA), every rejected one at least the 8th
    smallest (1 - 10.1 GAMMA), and the rows ascend to within the same rounding.  Returns the worst of the three as a
    multiple of the allowance (<= 1 passes), over the bound Gaussians."""
    D = d2_exact(means, parts)
    b = np.flatnonzero(idx[0] >= 0)
    if len(b) == 0:
        return 0.0
    Db = D[b]
    eighth = np.sort(Db, axis=1)[:, K - 1]
    chosen = np.take_along_axis(Db, idx[:, b].T.astype(np.int64), axis=1)          # [nb,8]
    tol = 2 * C_D2 * 1.01 * GAMMA * eighth
    tiny = np.finfo(np.float64).tiny
    over = (chosen.max(1) - eighth) / np.maximum(tol, tiny)
    rej = Db.copy()
    np.put_along_axis(rej, idx[:, b].T.astype(np.int64), np.inf, axis=1)
    under = (eighth - rej.min(1)) / np.maximum(tol, tiny) if Db.shape[1] > K else np.zeros(len(b))
    steps = (chosen[:, :-1] - chosen[:, 1:]).max(1) / np.maximum(tol, tiny)
    assert all(len(set(row)) == K for row in idx[:, b].T.tolist()), "a neighbour is listed twice"
    return float(max(over.max(), under.max(), steps.max(), 0.0))


def bind_ref(means, parts, idx):
    """The fp64 statement of the bind at the neighbour indices `idx` [8,n] (the GPU's): dict of (value, bound) for w [8,n],
    p [8,3,n], rest [12,n], plus "flags" (uint8 [n], the expected value) and "flags_free" (uint8 [n]: bits whose ratio is
    nearer to 1e-3 than its bound, where either value stands)."""
    idx = np.asarray(idx)
    n = idx.shape[1]
    out = {k: [np.zeros(s), np.zeros(s)] for k, s in (("w", (K, n)), ("p", (K, 3, n)), ("rest", (REST_ROWS, n)))}
    flags, free = np.zeros(n, np.uint8), np.zeros(n, np.uint8)
    b = np.flatnonzero(idx[0] >= 0)
    flags[idx[0] < 0] = FLAG_UNBOUND
    if len(b):
        mu, X = _f64(means)[b], _f64(parts)[idx[:, b]]                   # [nb,3], [8,nb,3]
        D = ((mu[None] - X) ** 2).sum(-1)
        h2 = D[K - 1]
        t = np.where(h2 > 0, D / np.where(h2 > 0, h2, 1.0), 0.0)
        wt = np.exp(-t)
        w = wt / wt.sum(0)
        a = 2 * C_D2 * GAMMA * t
        ew = 1.01 * w * (a + (a * w).sum(0))
        Xbar = (w[..., None] * X).sum(0)
        r = X - Xbar
        ar = np.abs(r)
        ec = (ew[..., None] * ar).sum(0) + 2 * K * EPS64 * (w[..., None] * np.abs(X)).sum(0)
        d0 = mu - Xbar
        p = w[..., None] * r
        Q = np.einsum("kn,kna,knb->nab", w, r, r)
        eQ = 1.01 * (np.einsum("kn,kna,knb->nab", ew, ar, ar) + np.einsum("kn,na,knb->nab", w, ec, ar)
                     + np.einsum("kn,kna,nb->nab", w, ar, ec))
        lam = np.linalg.eigvalsh(Q)                                      # ascending
        lmax = lam[:, 2]
        pos = lmax > 0
        lsafe = np.where(pos, lmax, 1.0)
        nF = np.linalg.norm(eQ, axis=(1, 2))
        rho = np.where(pos[:, None], lam[:, :2] / lsafe[:, None], 0.0)    # [nb,2]: min, mid
        brho = np.where(pos[:, None], 1.01 * (1 + rho) * (nF / lsafe)[:, None] + GAMMA * rho + FP64_EIG, 0.0)
        flat, thin = rho[:, 0] < TH, (rho[:, 1] < TH) | ~pos
        f_free = (np.abs(rho[:, 0] - TH) <= brho[:, 0]) & pos
        t_free = (np.abs(rho[:, 1] - TH) <= brho[:, 1]) & pos
        flags[b] = np.where(flat, FLAG_FLAT, 0) | np.where(thin, FLAG_THIN, 0)
        free[b] = np.where(f_free, FLAG_FLAT, 0) | np.where(t_free, FLAG_THIN, 0)
        inv_ok = ~flat & pos
        Qi = np.zeros_like(Q)
        Qi[inv_ok] = np.linalg.inv(Q[inv_ok])
        aQi = np.abs(Qi)
        bQi = 1.01 * (aQi @ eQ @ aQi) + GAMMA * aQi + FP64_INV * aQi.max(axis=(1, 2))[:, None, None]
        bQi[~inv_ok] = 0.0
        out["w"][0][:, b], out["w"][1][:, b] = w, ew + GAMMA * w
        out["p"][0][:, :, b] = np.transpose(p, (0, 2, 1))
        out["p"][1][:, :, b] = np.transpose(ew[..., None] * ar + w[..., None] * ec[None] + GAMMA * np.abs(p), (0, 2, 1))
        R, B = out["rest"]
        R[0:3, b], B[0:3, b] = d0.T, (ec + GAMMA * np.abs(d0)).T
        for row, (i, j) in enumerate(((0, 0), (0, 1), (0, 2), (1, 1), (1, 2), (2, 2))):
            R[3 + row, b], B[3 + row, b] = Qi[:, i, j], bQi[:, i, j]
        R[9, b], B[9, b] = h2, C_D2 * GAMMA * h2
        R[10, b], B[10, b] = rho[:, 1], brho[:, 1]
        R[11, b], B[11, b] = rho[:, 0], brho[:, 0]
    res = {k: tuple(v) for k, v in out.items()}
    res["flags"], res["flags_free"] = flags, free
    return res


def check_bind(ref, w, p, rest, flags):
    """Hold the GPU's (or the emulation's) binding arrays to `ref` = bind_ref(...) at its idx.  Where a free flat bit differs
    from the reference's choice the Q^-1 rows follow the flag that was stored.  Returns {name: worst error / bound}."""
    flags = np.asarray(flags)
    diff = (flags ^ ref["flags"]) & ~ref["flags_free"]
    assert not diff.any(), f"flags differ at {np.flatnonzero(diff)[:8]}: {flags[diff != 0][:8]} vs {ref['flags'][diff != 0][:8]}"
    ratios = {}
    flipped = ((flags ^ ref["flags"]) & FLAG_FLAT) != 0               # free rows only, by the assertion above
    for name, got in (("w", w), ("p", p), ("rest", rest)):
        val, bnd = ref[name]
        got = _f64(got)
        skip = np.zeros(val.shape, bool)
        if name == "rest":
            skip[3:9, flipped] = True                                  # (the caller counts these rows through flags_free)
        exact, held = (bnd == 0) & ~skip, (bnd > 0) & ~skip
        assert np.array_equal(got[exact], val[exact]), f"{name}: a value with bound 0 differs"
        ratios[name] = float((np.abs(got - val)[held] / bnd[held]).max()) if held.any() else 0.0
    return ratios


def emulate_bind(means, parts, select=None, max_distance=np.inf):
    """The kernels' arithmetic in NumPy: the fp32 d2 and the key order, then the fp64 moments rounded to fp32 once.
    Returns idx, w, p, rest, flags as the library stores them."""
    means, parts = _f32(means), _f32(parts)
    D32 = d2_fp32(means, parts)
    idx, d = knn_ref(D32, select, max_distance)
    n = idx.shape[1]
    w, p, rest = np.zeros((K, n), np.float32), np.zeros((K, 3, n), np.float32), np.zeros((REST_ROWS, n), np.float32)
    flags = np.where(idx[0] < 0, FLAG_UNBOUND, 0).astype(np.uint8)
    for i in np.flatnonzero(idx[0] >= 0):
        dd, X, mu = d[:, i].astype(np.float64), _f64(parts)[idx[:, i]], _f64(means)[i]
        h2 = dd[K - 1]
        wt = np.exp(-dd / h2) if h2 > 0 else np.ones(K)
        wi = wt / wt.sum()
        Xbar = (wi[:, None] * X).sum(0)
        r = X - Xbar
        Q = np.einsum("k,ka,kb->ab", wi, r, r)
        lam = np.linalg.eigvalsh(Q)
        flat, thin = lam[0] < TH * lam[2], lam[1] < TH * lam[2] or not lam[2] > 0
        Qi = np.linalg.inv(Q) if (not flat and lam[2] > 0) else np.zeros((3, 3))
        w[:, i], p[:, :, i] = wi, wi[:, None] * r
        rest[0:3, i] = mu - Xbar
        rest[3:9, i] = [Qi[0, 0], Qi[0, 1], Qi[0, 2], Qi[1, 1], Qi[1, 2], Qi[2, 2]]
        rest[9, i] = h2
        rest[10, i], rest[11, i] = (lam[1] / lam[2], lam[0] / lam[2]) if lam[2] > 0 else (0.0, 0.0)
        flags[i] = (FLAG_FLAT if flat else 0) | (FLAG_THIN if thin else 0)
    return idx, w, p, rest, flags


# ---- the apply -------------------------------------------------------------------------------------------------------------
def _qinv_matrix(rest):
    """rest rows 3..8 [6,n] -> symmetric [n,3,3]."""
    xx, xy, xz, yy, yz, zz = (_f64(rest[3 + k]) for k in range(6))
    return np.stack([np.stack([xx, xy, xz], -1), np.stack([xy, yy, yz], -1), np.stack([xz, yz, zz], -1)], -2)


def apply_ref(means, quats, scales, idx, w, p, rest, flags, mode, now, status_seen=None):
    """The fp64 statement of the apply on the stored binding.  mode 0 / 1.  status_seen: the status the kernel wrote; where
    a branch is nearer to its threshold than the bound, that status decides (otherwise the fp64 decision stands).  Returns
    a dict: status [n] and free [n] (status bits that may differ), branch [n] (0 pass-through, 1 thin, 2 rigid, 3 affine),
    means (value, bound) [n,3], rot (R_ref R(q) [n,3,3], Frobenius bound [n]) for branch 2, cov (A Sigma A^T [n,3,3], entrywise
    bound [n,3,3]) for branch 3, and the intermediate A (value, bound)."""
    means, quats, scales, now = _f64(means), _f64(quats), _f64(scales), _f64(now)
    idx, flags = np.asarray(idx), np.asarray(flags)
    n, m = means.shape[0], now.shape[0]
    status, free, branch = np.zeros(n, np.uint8), np.zeros(n, np.uint8), np.zeros(n, np.int64)
    mval, mbnd = means.copy(), np.zeros((n, 3))
    rot, rot_b = np.zeros((n, 3, 3)), np.zeros(n)
    cov, cov_b = np.zeros((n, 3, 3)), np.zeros((n, 3, 3))
    Aval, Abnd = np.zeros((n, 3, 3)), np.zeros((n, 3, 3))
    unbound = (flags & FLAG_UNBOUND) != 0
    status[unbound] = ST_UNBOUND
    safe = np.clip(idx, 0, m - 1)
    x = now[safe]                                                        # [8,n,3]
    okx = (np.isfinite(x).all(-1) & (idx >= 0) & (idx < m)).all(0)
    status[~unbound & ~okx] = ST_NONFINITE
    g = np.flatnonzero(~unbound & okx)
    res = {"status": status, "free": free, "branch": branch, "means": (mval, mbnd), "rot": (rot, rot_b),
           "cov": (cov, cov_b), "A": (Aval, Abnd)}
    if len(g) == 0:
        return res
    x, wg, pg = x[:, g], _f64(w)[:, g], np.transpose(_f64(p)[:, :, g], (0, 2, 1))     # [8,ng,3], [8,ng], [8,ng,3]
    e = x[1:] - x[0]
    c = (wg[1:, :, None] * e).sum(0)
    eC = (K * GAMMA) * (np.abs(wg[1:, :, None] * e)).sum(0)
    xbar = x[0] + c
    e_xbar = eC + GAMMA * np.abs(xbar)
    P = np.einsum("kna,knb->nab", e, pg[1:])
    eP = (K * GAMMA) * np.einsum("kna,knb->nab", np.abs(e), np.abs(pg[1:]))
    d0 = _f64(rest[0:3]).T[g]
    nP = np.linalg.norm(eP, axis=(1, 2))
    Rk, S, sdet = kabsch(P)
    smax, smid, smin = S[:, 0], S[:, 1], S[:, 2]
    fthin = (flags[g] & FLAG_THIN) != 0
    thin_now = ~(smax > 0) | (smid < TH * smax)
    thin_free = ~fthin & (np.abs(smid - TH * smax) <= 1.01 * (1 + TH) * nP + 1e-11 * smax) & (smax > 0)
    thin = fthin | thin_now
    if status_seen is not None:
        seen_thin = (np.asarray(status_seen)[g] & ST_THIN) != 0
        thin = np.where(thin_free, seen_thin, thin)
    # the affine map and its own decision
    Qi = _qinv_matrix(rest)[g]
    A = P @ Qi
    eA = eP @ np.abs(Qi) + 4 * GAMMA * (np.abs(P) @ np.abs(Qi))
    cof = np.stack([np.stack([A[:, (i + 1) % 3, (j + 1) % 3] * A[:, (i + 2) % 3, (j + 2) % 3]
                              - A[:, (i + 1) % 3, (j + 2) % 3] * A[:, (i + 2) % 3, (j + 1) % 3] for j in range(3)], -1)
                    for i in range(3)], -2)
    det = np.linalg.det(A)
    det_b = 1.01 * (eA * np.abs(cof)).sum((1, 2))
    fflat = (flags[g] & FLAG_FLAT) != 0
    fall = fflat | ~(det > 0)
    fall_free = ~fflat & (np.abs(det) <= det_b)
    if status_seen is not None:
        fall = np.where(fall_free, (np.asarray(status_seen)[g] & ST_FALLBACK) != 0, fall)
    if mode == 0:
        fall, fall_free = np.zeros(len(g), bool), np.zeros(len(g), bool)
    rigid = ~thin & ((mode == 0) | fall)
    affine = ~thin & ~rigid
    status[g] = np.where(thin, ST_THIN, np.where(rigid & (mode == 1), ST_FALLBACK, 0))
    free[g] = np.where(thin_free, ST_THIN | ST_FALLBACK, 0) | np.where(fall_free & ~thin, ST_FALLBACK, 0)
    branch[g] = np.where(thin, 1, np.where(rigid, 2, 3))
    # thin
    mu_thin = xbar + d0
    # rigid
    denom = smid + sdet * smin
    with np.errstate(divide="ignore", invalid="ignore"):
        dR = np.where(denom > 0, 1.01 * 2 * nP / denom + 8 * EPS64 * smax ** 2 / (smid * denom), np.inf)
    mu_rigid = xbar + np.einsum("nab,nb->na", Rk, d0)
    with np.errstate(invalid="ignore"):
        b_rigid = e_xbar + (dR * np.linalg.norm(d0, axis=1))[:, None] + GAMMA * np.abs(mu_rigid)
    # affine
    mu_aff = xbar + np.einsum("nab,nb->na", A, d0)
    b_aff = (e_xbar + np.einsum("nab,nb->na", eA, np.abs(d0)) + 3 * GAMMA * np.einsum("nab,nb->na", np.abs(A), np.abs(d0))
             + GAMMA * np.abs(mu_aff))
    Rq = quat_to_rot(quats[g])
    Sig = np.einsum("nab,nb,ncb->nac", Rq, scales[g] ** 2, Rq)
    Sp = A @ Sig @ np.transpose(A, (0, 2, 1))
    SAt, AS = np.abs(Sig @ np.transpose(A, (0, 2, 1))), np.abs(A @ Sig)
    bSp = (1.01 * (eA @ SAt + AS @ np.transpose(eA, (0, 2, 1)))
           + ((8 * GAMMA + FP64_EIG) * np.linalg.norm(Sp, axis=(1, 2)))[:, None, None])
    mval[g] = np.where(thin[:, None], mu_thin, np.where(rigid[:, None], mu_rigid, mu_aff))
    with np.errstate(invalid="ignore"):
        mbnd[g] = np.where(thin[:, None], e_xbar + GAMMA * np.abs(mu_thin), np.where(rigid[:, None], b_rigid, b_aff))
    rot[g], rot_b[g] = Rk @ Rq, dR + 3 * GAMMA
    cov[g], cov_b[g] = Sp, bSp
    Aval[g], Abnd[g] = A, eA
    return res


def check_apply(ref, means, quats, scales, out_means, out_quats, out_scales, status=None):
    """Hold the outputs to `ref` = apply_ref(..., status_seen=status).  Bit-identity where the header promises it, the bounds
    elsewhere.  Returns {name: worst error / bound}."""
    means, quats, scales = _f32(means), _f32(quats), _f32(scales)
    om, oq, osc = _f32(out_means), _f32(out_quats), _f32(out_scales)
    br = ref["branch"]
    if status is not None:
        status = np.asarray(status)
        diff = (status ^ ref["status"]) & ~ref["free"]
        assert not diff.any(), f"status differs at {np.flatnonzero(diff)[:8]}: {status[diff != 0][:8]} vs {ref['status'][diff != 0][:8]}"
    same = lambda a, b: a.view(np.uint32).tolist() == b.view(np.uint32).tolist()
    assert same(om[br == 0], means[br == 0]), "a passed-through mean is not the input's bits"
    assert same(oq[br <= 1], quats[br <= 1]), "a passed-through or thin quaternion is not the input's bits"
    assert same(osc[br <= 2], scales[br <= 2]), "a passed-through, thin or rigid scale is not the input's bits"
    assert np.isfinite(om).all() or not np.isfinite(means).all(), "a non-finite mean left the kernel"
    ratios = {}
    mv, mb = ref["means"]
    moved = br > 0
    if moved.any():
        err = np.abs(_f64(om)[moved] - mv[moved])
        ratios["means"] = float((err / mb[moved]).max())
    r = br == 2
    if r.any():
        Rv, Rb = ref["rot"]
        qn = np.linalg.norm(_f64(oq)[r], axis=1)
        assert np.abs(qn - 1).max() <= 4 * U, f"rigid quaternions off unit length by {np.abs(qn - 1).max():.2e}"
        err = np.linalg.norm(quat_to_rot(oq[r]) - Rv[r], axis=(1, 2))
        ratios["rot"] = float((err / Rb[r]).max())
    a = br == 3
    if a.any():
        Cv, Cb = ref["cov"]
        qn = np.linalg.norm(_f64(oq)[a], axis=1)
        assert np.abs(qn - 1).max() <= 4 * U, f"affine quaternions off unit length by {np.abs(qn - 1).max():.2e}"
        s = _f64(osc)[a]
        assert (np.diff(s, axis=1) >= 0).all() and (s >= FLT_MIN).all(), "affine scales are not ascending positive normals"
        Rq = quat_to_rot(oq[a])
        got = np.einsum("nab,nb,ncb->nac", Rq, s ** 2, Rq)
        ratios["cov"] = float((np.abs(got - Cv[a]) / Cb[a]).max())
    return ratios


def emulate_apply(means, quats, scales, idx, w, p, rest, flags, mode, now):
    """The apply kernel's arithmetic in NumPy: e, c, P, A and the affine mean in fp32 (fma chains in order of j), the
    solves in fp64 (eigh in place of the Jacobi sweeps).  Returns out_means, out_quats, out_scales, status."""
    means, quats, scales, now = _f32(means), _f32(quats), _f32(scales), _f32(now)
    w, p, rest, idx, flags = _f32(w), _f32(p), _f32(rest), np.asarray(idx), np.asarray(flags)
    n, m = means.shape[0], now.shape[0]
    om, oq, osc, status = means.copy(), quats.copy(), scales.copy(), np.zeros(n, np.uint8)
    for i in range(n):
        if flags[i] & FLAG_UNBOUND:
            status[i] = ST_UNBOUND
            continue
        j = idx[:, i]
        if ((j < 0) | (j >= m)).any() or not np.isfinite(now[np.clip(j, 0, m - 1)]).all():
            status[i] = ST_NONFINITE
            continue
        x = now[j]
        e = x[1:] - x[0]                                                  # fp32
        c = w[1, i] * e[0]
        P = np.outer(e[0], p[1, :, i]).astype(np.float32)
        for k in range(2, K):
            c = fma32(w[k, i], e[k - 1], c)
            P = fma32(e[k - 1][:, None], p[k, :, i][None, :], P)
        xbar = x[0] + c
        d0 = rest[0:3, i]
        Pd = _f64(P)
        lam, V = np.linalg.eigh(Pd.T @ Pd)
        lam, V = lam[::-1], V[:, ::-1]
        thin = bool(flags[i] & FLAG_THIN) or not lam[0] > 0 or lam[1] < TH * TH * lam[0]
        if thin:
            status[i] = ST_THIN
            om[i] = xbar + d0
            continue
        rigid = mode == 0
        if not rigid:
            if flags[i] & FLAG_FLAT:
                rigid = True
            else:
                Qi = _qinv_matrix(rest[:, i:i + 1])[0].astype(np.float32)
                A = np.zeros((3, 3), np.float32)
                for a in range(3):
                    for b in range(3):
                        A[a, b] = fma32(P[a, 2], Qi[2, b], fma32(P[a, 1], Qi[1, b], P[a, 0] * Qi[0, b]))
                if not np.linalg.det(_f64(A)) > 0:
                    rigid = True
            if rigid:
                status[i] = ST_FALLBACK
        if rigid:
            v1, v2 = V[:, 0], V[:, 1]
            u1 = Pd @ v1 / np.sqrt(lam[0])
            u2 = Pd @ v2
            u2 = u2 - (u1 @ u2) * u1
            u2 /= np.linalg.norm(u2)
            R = np.outer(u1, v1) + np.outer(u2, v2) + np.outer(np.cross(u1, u2), np.cross(v1, v2))
            om[i] = (_f64(xbar) + R @ _f64(d0)).astype(np.float32)
            q = quat_mul(rot_to_quat(R[None])[0], _f64(quats[i]))
            oq[i] = (q / np.linalg.norm(q)).astype(np.float32)
        else:
            Ad = fma32(A[:, 2], d0[2], fma32(A[:, 1], d0[1], A[:, 0] * d0[0]))
            om[i] = xbar + Ad
            M = _f64(A) @ quat_to_rot(quats[i][None])[0] * _f64(scales[i])[None, :]
            lam2, Z = np.linalg.eigh(M @ M.T)
            if np.linalg.det(Z) < 0:
                Z[:, 2] = -Z[:, 2]
            oq[i] = rot_to_quat(Z[None])[0].astype(np.float32)
            osc[i] = np.maximum(np.sqrt(np.maximum(lam2, 0.0)).astype(np.float32), np.float32(FLT_MIN))
    return om, oq, osc, status


# ---- scenes the tests share ------------------------------------------------------------------------------------------------
def random_rotation(rng):
    r, _ = np.linalg.qr(rng.normal(size=(3, 3)))
    if np.linalg.det(r) < 0:
        r[:, 0] = -r[:, 0]
    return r


def cloud(n, m, seed, kind="cloud"):
    """n Gaussians among m particles, fp32: kind "cloud" a uniform random volume, "sheet" a jittered coplanar grid (z = 0
    exactly), "strand" particles on a line.  Returns means [n,3], quats [n,4], scales [n,3], particles [m,3]."""
    rng = np.random.default_rng(seed)
    if kind == "cloud":
        parts = rng.uniform(-1, 1, (m, 3))
        means = rng.uniform(-0.9, 0.9, (n, 3))
    elif kind == "sheet":
        side = int(np.ceil(np.sqrt(m)))
        gx, gy = np.meshgrid(np.arange(side), np.arange(side), indexing="ij")
        parts = np.stack([gx.reshape(-1), gy.reshape(-1), np.zeros(side * side)], 1)[:m] * (2.0 / side) - [1, 1, 0]
        parts[:, :2] += rng.uniform(-0.2, 0.2, (m, 2)) / side
        means = np.concatenate([rng.uniform(-0.9, 0.9, (n, 2)), rng.uniform(-0.01, 0.01, (n, 1))], 1)
    elif kind == "strand":
        parts = np.outer(np.sort(rng.uniform(-1, 1, m)), [0.5, 0.25, 1.0]).astype(np.float32).astype(np.float64)
        parts[:, 0] = 2 * parts[:, 1]                                     # exactly colinear in fp32: x = 2 y, z free
        parts[:, 2] = 4 * parts[:, 1]
        means = parts[rng.integers(0, m, n)] + rng.uniform(-0.01, 0.01, (n, 3))
    else:
        raise ValueError(kind)
    quats = rng.normal(size=(n, 4))
    quats /= np.linalg.norm(quats, axis=1, keepdims=True)
    scales = np.exp(rng.uniform(-5, -3, (n, 3)))
    return _f32(means), _f32(quats), _f32(scales), _f32(parts)


def move(parts, kind, seed=0):
    """The particles at frame time, fp32: "rigid" a rotation and translation of all, "bend" a smooth bend about the y axis,
    "stretch" an anisotropic stretch and shear."""
    rng = np.random.default_rng(100 + seed)
    X = _f64(parts)
    if kind == "rigid":
        Y = X @ random_rotation(rng).T + rng.normal(size=3)
    elif kind == "bend":
        ang = 0.8 * X[:, 0]
        Y = np.stack([np.sin(ang) * (1.25 + X[:, 2]), X[:, 1], np.cos(ang) * (1.25 + X[:, 2]) - 1.25], 1)
    elif kind == "stretch":
        F = np.array([[1.4, 0.2, 0.0], [0.0, 0.8, 0.1], [0.1, 0.0, 1.1]])
        Y = X @ F.T + [0.3, -0.2, 0.1]
    else:
        raise ValueError(kind)
    return _f32(Y)
