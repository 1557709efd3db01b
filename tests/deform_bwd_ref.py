"""fp64 statement of mgs_deform_apply_bwd (include/mgs_deform_bwd.h, csrc/deform.hip) with the error bound each value is
held to.  A helper module, not a test file: tests/test_deform_bwd_host.py checks it against central differences of
deform_ref's forward and against a NumPy emulation of the kernels' arithmetic without a GPU, tests/test_gpu_deform_bwd.py
holds the kernels to it.

The formulas are the header's, evaluated in NumPy fp64 on the arrays the kernel reads: the stored fp32 binding, the fp32
particles and cotangents, and the forward's status, which is an INPUT of the statement (the branch is given, not decided
again).  U, GAMMA as in deform_ref: a value formed by k chained roundings of a sum of terms is within k GAMMA sum|terms|.
Factors 1.01 absorb second-order terms.  Norms are 2-norms of vectors and Frobenius norms of matrices unless marked.

What the kernel rounds.  P~ is the forward's fp32 fma chain, |P~ - P| <= eP = 8 GAMMA sum |e_k| |p_k|^T entrywise
(deform_ref, apply stage), nP = ||eP||_F.  Everything after it is fp64 on P~ and on exact fp32 inputs, and every stored
value is rounded to fp32 once (k = 1): so a value that does not depend on P is within 1 GAMMA |value| (plus FP64, the
noise of a dozen fp64 operations, 32 eps64 sum|terms|), and the rest follows P~ - P to first order.

Linear parts (k = 1 each, read off the kernel: fp64 products and sums, one final rounding).
  thin rows     v_x_k = w_k ct_mu: GAMMA |v_x_k|.  v_x_0 = ct_mu - sum_k w_k ct_mu: GAMMA |v_x_0| + FP64 (|ct_mu| + sum |w_k ct_mu|).
                v_d0, v_q, v_s are the cotangents' bits (bound 0).
  pass-through  the three rest gradients are the cotangents' bits and the 24 contributions are +0 (bound 0).
  v_s           the cotangent's bits on every row.

Rotation part, first order in nP.  g = sigma_2 + s sigma_3 is the smallest eigenvalue of G, so ||G^-1||_2 = 1 / g.
  dR      ||R~ - R||_F <= 1.01 * 2 nP / g + 8 eps64 sigma_1^2 / (sigma_2 g), as in deform_ref (rigid).
  dq      a rotation by theta moves R by 2 sqrt(2) sin(theta / 2) and its quaternion by 2 sin(theta / 4): the unit
          quaternions q_R and q' move by at most dq = 1.01 dR / (2 sqrt(2)).
  v_d0    = R^T ct_mu:  dR ||ct_mu|| + GAMMA |v_d0| per component.
  v_q     = L(q_R)^T (I - q' q'^T) ct_q / |q|: the projector moves by 2 dq, the left multiplication by dq:
          3 dq ||ct_q|| / |q| + GAMMA |v_q| per component.
  v_omega = (R d0) x ct_mu + 1/2 E(q') ct_q, E's rows (0, e_k) (x) q' orthonormal:  e_om = dR ||d0|| ||ct_mu|| + dq ||ct_q|| / 2.
  z       = R^T v_omega:  e_z = dR ||v_omega|| + e_om.
  S       = sym(R^T P):  ||dS||_F <= dR sigma_1 + nP =: e_S (the rotation's error enters the symmetric part at first order
          through sigma_1 - sigma_3);  G = tr(S) I - S:  ||dG||_2 <= (sqrt(3) + 1) e_S.
  y       = G^-1 z:  e_y = (e_z + (sqrt(3) + 1) e_S ||y||) / g.
  v_P     = R [y]x:  ||dv_P||_F <= dR ||y|| + sqrt(2) e_y =: e_vP.
  v_x_k   = w_k ct_mu + v_P p_k (k = 1..7):  1.01 e_vP ||p_k|| + GAMMA |v_x_k| + FP64 per component.
  v_x_0   = ct_mu - sum_k v_x_k:  1.01 e_vP sum_k ||p_k|| + GAMMA |v_x_0| + FP64.
Guarded rows (g < 1e-3 sigma_1): v_P = 0 and v_q = ct_q's bits; v_d0 = R^T ct_mu keeps its bound above (large: R is barely
  determined there) and the contributions are the thin rows'.
Guard bit.  Weyl: every singular value moves by at most nP, so g - 1e-3 sigma_1 moves by at most 1.01 (2 + 1e-3) nP +
  1e-11 sigma_1.  A row nearer to the threshold than that is "free": it follows the kernel's bwd_status.

Pivot.  q_R's sign comes from the pivot rule of the forward's rotmat_to_quat; where R is nearer to a change of pivot than
  2 dR the fp32 side may take the other sign (and v_q with it): such a row is free as well.

Particle sums, fp32.  v_particles[j] adds len_j contributions: lane l a chain over its entries (ceil(len_j / 64) - 1
  additions), then the tree (6 additions).  Against the fp64 sum of the reference's contributions:
      sum of the contributions' own bounds + (ceil(len_j / 64) - 1 + 6) GAMMA sum |contribution| (1 + bound terms absorbed by 1.01).
  A particle nobody references is +0 exactly.
"""
import numpy as np

import deform_ref as DR
from deform_ref import GAMMA, U, K, TH, EPS64, ST_UNBOUND, ST_THIN, ST_NONFINITE, FLAG_UNBOUND, _f32, _f64, fma32

FP64 = 32 * EPS64
SQ2, SQ3 = np.sqrt(2.0), np.sqrt(3.0)


# ---- the transposed binding --------------------------------------------------------------------------------------------
def transpose_loop(idx, m):
    """The transposed binding by a plain loop: t_start int32 [m + 1], t_entry int32 [8 n].  Entries of index -1 in front."""
    idx = np.asarray(idx)
    n = idx.shape[1]
    per = [[] for _ in range(m)]
    front, back = [], []
    for k in range(K):
        for i in range(n):
            j = int(idx[k, i])
            (front if j < 0 else back if j >= m else per[j]).append(k * n + i)
    entry, start = list(front), []
    for j in range(m):
        start.append(len(entry))
        entry += per[j]
    start.append(len(entry))
    return np.array(start, np.int32), np.array(entry + back, np.int32)


# ---- quaternion helpers (wxyz) -------------------------------------------------------------------------------------------
def _conj(q):
    return q * np.array([1.0, -1.0, -1.0, -1.0])


def _unit_rows(qp):
    """E(q') [n,3,4]: row k is (0, e_k) (x) q'."""
    w, x, y, z = (qp[:, k] for k in range(4))
    return np.stack([np.stack([-x, w, -z, y], -1), np.stack([-y, z, w, -x], -1), np.stack([-z, -y, x, w], -1)], 1)


def _skew(y):
    Z = np.zeros(len(y))
    return np.stack([np.stack([Z, -y[:, 2], y[:, 1]], -1), np.stack([y[:, 2], Z, -y[:, 0]], -1),
                     np.stack([-y[:, 1], y[:, 0], Z], -1)], 1)


def _chain(P, R, sig1, d0, q, ct_m, ct_q):
    """The header's chain in fp64 for rows that turned: returns dict(v_d0, v_q, v_om, y, v_P, g, S, qn)."""
    S = np.transpose(R, (0, 2, 1)) @ P
    S = 0.5 * (S + np.transpose(S, (0, 2, 1)))
    tr = np.trace(S, axis1=1, axis2=2)
    g = tr - sig1
    qR = DR.rot_to_quat(R)
    u = DR.quat_mul(qR, q)
    qn = np.linalg.norm(u, axis=1)
    qp = u / qn[:, None]
    v_d0 = np.einsum("nba,nb->na", R, ct_m)
    vu = (ct_q - (ct_q * qp).sum(1, keepdims=True) * qp) / qn[:, None]
    v_q = DR.quat_mul(_conj(qR), vu)
    h = np.einsum("nab,nb->na", R, d0)
    v_om = np.cross(h, ct_m) + 0.5 * np.einsum("nkc,nc->nk", _unit_rows(qp), ct_q)
    z = np.einsum("nba,nb->na", R, v_om)
    G = tr[:, None, None] * np.eye(3) - S
    with np.errstate(all="ignore"):
        y = np.where((np.abs(g) > 0)[:, None], np.linalg.solve(np.where((np.abs(g) > 0)[:, None, None], G, np.eye(3)), z[..., None])[..., 0], 0.0)
    v_P = R @ _skew(y)
    return dict(v_d0=v_d0, v_q=v_q, v_om=v_om, y=y, v_P=v_P, g=g, qn=qn)


def _gather(idx, now, status, flags):
    idx = np.asarray(idx)
    m = now.shape[0]
    st = np.asarray(status)
    passing = ((np.asarray(flags) & FLAG_UNBOUND) != 0) | ((st & (ST_UNBOUND | ST_NONFINITE)) != 0)
    passing |= ~((idx >= 0) & (idx < m)).all(0)
    return passing, (st & ST_THIN) != 0


# ---- the fp64 statement with its bounds ------------------------------------------------------------------------------------
def bwd_ref(quats, idx, w, p, rest, flags, now, status, ct_m, ct_q, ct_s, guard_seen=None, use_guard=True):
    """Returns a dict: v_means, v_quats (value, bound) [n,3] / [n,4]; v_scales (value, zero bound); contrib (value, bound)
    [8,3,n]; guard bool [n] (the reference's, with the kernel's on free rows when guard_seen is given); free bool [n];
    ratio [n] g / sigma_1 of the rows that turned (inf elsewhere); kind [n] 0 pass-through, 1 thin, 2 turned.
    ct_*: arrays or None (zero).  use_guard=False: the bare closed form (for finite differences)."""
    idx = np.asarray(idx)
    n = idx.shape[1]
    z3, z4 = np.zeros((n, 3)), np.zeros((n, 4))
    ct_m = z3 if ct_m is None else _f64(ct_m)
    ct_q = z4 if ct_q is None else _f64(ct_q)
    ct_s = z3 if ct_s is None else _f64(ct_s)
    quats, now, w, rest = _f64(quats), _f64(now), _f64(w), _f64(rest)
    pg_all = np.transpose(_f64(p), (0, 2, 1))                               # [8,n,3]
    passing, thin = _gather(idx, now, status, flags)
    vm, bm = ct_m.copy(), np.zeros((n, 3))
    vq, bq = ct_q.copy(), np.zeros((n, 4))
    con, bcon = np.zeros((K, 3, n)), np.zeros((K, 3, n))
    guard, free, ratio = np.zeros(n, bool), np.zeros(n, bool), np.full(n, np.inf)
    kind = np.where(passing, 0, np.where(thin, 1, 2))
    b = np.flatnonzero(~passing)
    if len(b):
        wg, pg, cm = w[:, b], pg_all[:, b], ct_m[b]
        wct = wg[1:, :, None] * cm[None]                                     # [7,nb,3]
        vP, evP = np.zeros((len(b), 3, 3)), np.zeros(len(b))
        t = np.flatnonzero(kind[b] == 2)
        if len(t):
            bt = b[t]
            x = now[idx[:, bt]]
            e = x[1:] - x[0]
            P = np.einsum("kna,knb->nab", e, pg[1:, t])
            eP = (K * GAMMA) * np.einsum("kna,knb->nab", np.abs(e), np.abs(pg[1:, t]))
            nP = np.linalg.norm(eP, axis=(1, 2))
            Rk, S, sdet = DR.kabsch(P)
            s1, s2, s3 = S[:, 0], S[:, 1], S[:, 2]
            d0 = rest[0:3].T[bt]
            c = _chain(P, Rk, s1, d0, quats[bt], cm[t], ct_q[bt])
            g = s2 + sdet * s3
            with np.errstate(divide="ignore", invalid="ignore"):
                ratio[bt] = np.where(s1 > 0, g / s1, 0.0)
                gd = g < TH * s1
                fr = np.abs(g - TH * s1) <= 1.01 * (2 + TH) * nP + 1e-11 * s1
                if guard_seen is not None:
                    gd = np.where(fr, np.asarray(guard_seen)[bt] != 0, gd)
                if not use_guard:
                    gd, fr = np.zeros(len(t), bool), np.zeros(len(t), bool)
                dR = np.where(g > 0, 1.01 * 2 * nP / g + 8 * EPS64 * s1 ** 2 / (s2 * g), np.inf)
                dq = 1.01 * dR / (2 * SQ2)
                ncm, ncq = np.linalg.norm(cm[t], axis=1), np.linalg.norm(ct_q[bt], axis=1)
                e_om = dR * np.linalg.norm(d0, axis=1) * ncm + 0.5 * dq * ncq
                e_z = dR * np.linalg.norm(c["v_om"], axis=1) + e_om
                e_S = dR * s1 + nP
                ny = np.linalg.norm(c["y"], axis=1)
                e_y = (e_z + (SQ3 + 1) * e_S * ny) / g
                e_vP = dR * ny + SQ2 * e_y
                vm[bt] = c["v_d0"]
                bm[bt] = dR[:, None] * ncm[:, None] + GAMMA * np.abs(c["v_d0"])
                turn = ~gd
                vq[bt[turn]] = c["v_q"][turn]
                bq[bt[turn]] = (3 * dq * ncq / c["qn"])[turn, None] + GAMMA * np.abs(c["v_q"][turn])
            # the sign of q_R is the pivot rule's (rot_to_quat): a row whose R lies nearer to a change of pivot than dR may
            # take the other sign on the fp32 side, and v_q with it; it is free
            dg = np.stack([Rk[:, 0, 0], Rk[:, 1, 1], Rk[:, 2, 2]], 1)
            trR, srt = dg.sum(1), np.sort(dg, axis=1)
            margin = np.where(trR > 0, trR, np.minimum(-trR, srt[:, 2] - srt[:, 1]))
            if use_guard:
                fr = fr | (turn & (margin <= 2 * dR))
            vP[t[turn]], evP[t[turn]] = c["v_P"][turn], e_vP[turn]
            guard[bt], free[bt] = gd, fr
        vpp = np.einsum("nab,knb->kna", vP, pg[1:])                           # [7,nb,3]
        vx = wct + vpp
        npk = np.linalg.norm(pg[1:], axis=2)                                  # [7,nb]
        noise = FP64 * (np.abs(wct) + np.einsum("nab,knb->kna", np.abs(vP), np.abs(pg[1:])))
        with np.errstate(invalid="ignore"):
            bx = 1.01 * evP[None, :, None] * npk[..., None] + GAMMA * np.abs(vx) + noise
            v0 = cm - vx.sum(0)
            b0 = 1.01 * evP[:, None] * npk.sum(0)[:, None] + GAMMA * np.abs(v0) + FP64 * np.abs(cm) + noise.sum(0) + FP64 * np.abs(vx).sum(0)
        con[1:, :, b], bcon[1:, :, b] = np.transpose(vx, (0, 2, 1)), np.transpose(bx, (0, 2, 1))
        con[0][:, b], bcon[0][:, b] = v0.T, b0.T
    return {"v_means": (vm, bm), "v_quats": (vq, bq), "v_scales": (ct_s, np.zeros((n, 3))), "contrib": (con, bcon),
            "guard": guard, "free": free, "ratio": ratio, "kind": kind}


def scatter_ref(contrib, idx, m):
    """contrib = (value, bound) [8,3,n] -> v_particles (value, bound) [m,3], counts [m]: the fp64 sums through idx and the
    bound of the kernel's fp32 sum of the fp32 contributions."""
    val, bnd = contrib
    idx = np.asarray(idx)
    ok = (idx >= 0) & (idx < m)
    j = idx[ok]
    cnt = np.bincount(j, minlength=m)
    out, ob = np.zeros((m, 3)), np.zeros((m, 3))
    depth = np.maximum(np.ceil(cnt / 64.0) - 1, 0) + 6
    for c in range(3):
        v, bb = val[:, c, :][ok], bnd[:, c, :][ok]
        with np.errstate(invalid="ignore"):
            out[:, c] = np.bincount(j, weights=v, minlength=m)
            ob[:, c] = np.bincount(j, weights=bb, minlength=m) + 1.01 * depth * GAMMA * np.bincount(j, weights=np.abs(v) + bb, minlength=m)
    ob[cnt == 0] = 0.0
    return (out, ob), cnt


def check_bwd(ref, vp_ref, got, ct_m, ct_q, ct_s, allow_free=None):
    """Hold the kernel's (or the emulation's) results got = dict(v_means, v_quats, v_scales, v_particles, contrib (optional),
    bwd_status (optional)) to ref = bwd_ref(...) and vp_ref = scatter_ref(...)[0].  Bits where the header promises bits.
    Free rows are left out of the per-Gaussian comparisons and must be at most max(1, 0.5 %) of the rows (allow_free
    overrides); a particle that a free row touches is left out too.  Returns {name: worst error / bound}."""
    n = len(ref["kind"])
    same = lambda a, b: _f32(a).view(np.uint32).tolist() == _f32(b).view(np.uint32).tolist()
    kind, free, guard = ref["kind"], ref["free"], ref["guard"]
    limit = max(1, int(0.005 * n)) if allow_free is None else allow_free
    assert free.sum() <= limit, f"{free.sum()} free rows of {n}, at most {limit} allowed"
    z3, z4 = np.zeros((n, 3), np.float32), np.zeros((n, 4), np.float32)
    ct_m = z3 if ct_m is None else _f32(ct_m)
    ct_q = z4 if ct_q is None else _f32(ct_q)
    ct_s = z3 if ct_s is None else _f32(ct_s)
    if got.get("bwd_status") is not None:
        bs = np.asarray(got["bwd_status"])
        assert (bs <= 1).all()
        diff = ((bs != 0) != guard) & ~free
        assert not diff.any(), f"guard bits differ at {np.flatnonzero(diff)[:8]} (ratio {ref['ratio'][diff][:8]})"
    ratios = {}
    if got.get("v_means") is not None:
        assert same(got["v_scales"], ct_s), "v_scales is not ct_scales bit for bit"
        assert same(_f32(got["v_means"])[kind <= 1], ct_m[kind <= 1]), "v_means of a pass-through or thin row is not its cotangent's bits"
        keepq = (kind <= 1) | (guard & ~free)
        assert same(_f32(got["v_quats"])[keepq], ct_q[keepq]), "v_quats of a pass-through, thin or guarded row is not its cotangent's bits"
        for name in ("v_means", "v_quats"):
            val, bnd = ref[name]
            rows = (kind == 2) & ~free
            held = rows[:, None] & (bnd > 0)
            err = np.abs(_f64(got[name]) - val)
            assert (err[rows[:, None] & (bnd == 0)] == 0).all(), f"{name}: a value with bound 0 differs"
            with np.errstate(invalid="ignore"):
                ratios[name] = float((err[held] / bnd[held]).max()) if held.any() else 0.0
    if got.get("contrib") is not None:
        val, bnd = ref["contrib"]
        c = _f64(got["contrib"])
        assert not c[:, :, kind == 0].any() and not np.signbit(c[:, :, kind == 0]).any(), "a pass-through row contributes"
        cols = ~free
        held = cols[None, None, :] & (bnd > 0)
        err = np.abs(c - val)
        assert (err[cols[None, None, :] & (bnd == 0)] == 0).all(), "contrib: a value with bound 0 differs"
        with np.errstate(invalid="ignore"):
            ratios["contrib"] = float((err[held] / bnd[held]).max()) if held.any() else 0.0
    val, bnd = vp_ref
    vp = _f64(got["v_particles"])
    touched = np.zeros(len(val), bool)
    if free.any():
        ids = np.asarray(got["idx"])[:, free].reshape(-1)
        touched[ids[(ids >= 0) & (ids < len(val))]] = True
    zero = (bnd == 0).all(1) & ~touched
    assert not vp[zero].any() and not np.signbit(vp[zero]).any(), "a particle nobody references (or only zero rows) is not +0"
    held = ~touched[:, None] & (bnd > 0) & np.isfinite(bnd)
    with np.errstate(invalid="ignore"):
        ratios["v_particles"] = float((np.abs(vp - val)[held] / bnd[held]).max()) if held.any() else 0.0
    return ratios


# ---- the kernels' arithmetic in NumPy --------------------------------------------------------------------------------------
def emulate_bwd(quats, idx, w, p, rest, flags, now, status, ct_m, ct_q, ct_s, t_start=None, t_entry=None):
    """Kernel 1: P in fp32 (the forward's fma chain), the forward's construction of R from the eigenpairs of P~^T P~ in
    fp64 (eigh in place of the Jacobi sweeps), the chain in fp64, every stored value rounded to fp32 once.  Kernel 2: the
    lanes' chains and the xor tree in fp32, in the header's order.  Returns dict(v_means, v_quats, v_scales, contrib
    [8,3,n], v_particles [m,3], bwd_status, idx)."""
    idx = np.asarray(idx)
    n, m = idx.shape[1], np.asarray(now).shape[0]
    z3, z4 = np.zeros((n, 3), np.float32), np.zeros((n, 4), np.float32)
    ct_m = z3 if ct_m is None else _f32(ct_m)
    ct_q = z4 if ct_q is None else _f32(ct_q)
    ct_s = z3 if ct_s is None else _f32(ct_s)
    w32, p32, now32, rest32, q32 = _f32(w), _f32(p), _f32(now), _f32(rest), _f32(quats)
    passing, thin = _gather(idx, now32, status, flags)
    vm, vq = ct_m.copy(), ct_q.copy()
    con = np.zeros((K, 3, n), np.float32)
    bst = np.zeros(n, np.uint8)
    b = np.flatnonzero(~passing)
    if len(b):
        x = now32[idx[:, b]]                                                  # [8,nb,3]
        e = x[1:] - x[0]                                                      # fp32
        pg = np.transpose(p32[:, :, b], (0, 2, 1))                            # [8,nb,3]
        P = (e[0][:, :, None] * pg[1][:, None, :]).astype(np.float32)
        for k in range(2, K):
            P = fma32(e[k - 1][:, :, None], pg[k][:, None, :], P)
        cm = _f64(ct_m[b])
        vP = np.zeros((len(b), 3, 3))
        t = np.flatnonzero(~thin[b])
        if len(t):
            bt = b[t]
            Pd = _f64(P[t])
            lam, V = np.linalg.eigh(np.transpose(Pd, (0, 2, 1)) @ Pd)
            lam, V = lam[:, ::-1], V[:, :, ::-1]
            v1, v2 = V[:, :, 0], V[:, :, 1]
            with np.errstate(all="ignore"):
                u1 = np.einsum("nab,nb->na", Pd, v1) / np.sqrt(lam[:, :1])
                u2 = np.einsum("nab,nb->na", Pd, v2)
                u2 = u2 - (u1 * u2).sum(1, keepdims=True) * u1
                u2 = u2 / np.linalg.norm(u2, axis=1, keepdims=True)
                R = (u1[:, :, None] * v1[:, None, :] + u2[:, :, None] * v2[:, None, :]
                     + np.cross(u1, u2)[:, :, None] * np.cross(v1, v2)[:, None, :])
                sig1 = np.sqrt(lam[:, 0])
                c = _chain(Pd, R, sig1, _f64(rest32[0:3].T[bt]), _f64(q32[bt]), cm[t], _f64(ct_q[bt]))
                gd = c["g"] < TH * sig1
            vm[bt] = c["v_d0"].astype(np.float32)
            vq[bt[~gd]] = c["v_q"][~gd].astype(np.float32)
            vP[t[~gd]] = c["v_P"][~gd]
            bst[bt] = gd
        with np.errstate(invalid="ignore"):
            vx = _f64(w32[1:, b])[:, :, None] * cm[None] + np.einsum("nab,knb->kna", vP, _f64(pg[1:]))
            v0 = cm.copy()
            for k in range(K - 1):
                v0 = v0 - vx[k]
        con[1:, :, b] = np.transpose(vx, (0, 2, 1)).astype(np.float32)
        con[0][:, b] = v0.T.astype(np.float32)
    if t_start is None:
        t_start, t_entry = transpose_loop(idx, m)
    vp = np.zeros((m, 3), np.float32)
    flat = con.transpose(1, 0, 2).reshape(3, K * n)                           # [3, k n + i]
    for j in range(m):
        ent = t_entry[t_start[j]:t_start[j + 1]]
        if len(ent) == 0:
            continue
        lanes = np.zeros((3, 64), np.float32)
        for r in range(0, len(ent), 64):
            chunk = flat[:, ent[r:r + 64]]
            lanes[:, :chunk.shape[1]] = lanes[:, :chunk.shape[1]] + chunk
        for d in (32, 16, 8, 4, 2, 1):
            lanes = lanes + lanes[:, np.arange(64) ^ d]
        vp[j] = lanes[:, 0]
    return {"v_means": vm, "v_quats": vq, "v_scales": ct_s.copy(), "contrib": con, "v_particles": vp, "bwd_status": bst,
            "idx": idx}


# ---- the forward as a scalar loss, for finite differences -----------------------------------------------------------------
def forward_loss(quats, idx, w, p, rest, flags, now, ct_m, ct_q, ct_s, scales):
    """Per-Gaussian <ct_mu, mu'> + <ct_q, q'> + <ct_s, s'> of deform_ref.apply_ref's rigid forward, fp64 [n]."""
    n = np.asarray(idx).shape[1]
    ref = DR.apply_ref(np.zeros((n, 3)), quats, scales, idx, w, p, rest, flags, 0, now)
    assert (ref["branch"] == 2).all(), "the finite-difference scenes are rigid rows only"
    Rq = DR.quat_to_rot(quats)
    Rk = ref["rot"][0] @ np.transpose(Rq, (0, 2, 1))
    u = DR.quat_mul(DR.rot_to_quat(Rk), _f64(quats))
    qp = u / np.linalg.norm(u, axis=1, keepdims=True)
    return (ct_m * ref["means"][0]).sum(1) + (ct_q * qp).sum(1) + (ct_s * _f64(scales)).sum(1)


# ---- scenes the tests share --------------------------------------------------------------------------------------------
def cotangents(n, seed):
    """fp32 cotangents of the deformed means, quats and scales."""
    rng = np.random.default_rng(1000 + seed)
    return _f32(rng.normal(size=(n, 3))), _f32(rng.normal(size=(n, 4))), _f32(rng.normal(size=(n, 3)))


def mirror(parts):
    """The particles reflected through the plane x = 0: det P < 0 in every neighbourhood of a volume."""
    Y = _f32(parts).copy()
    Y[:, 0] = -Y[:, 0]
    return Y


def lattice(side=5, seed=0):
    """Particles on an integer lattice (scaled by 1/4) and one Gaussian on every interior point.  A lattice point's 8
    nearest are itself, its 6 face neighbours and one edge neighbour, so Q has a double smallest eigenvalue: mirrored at
    frame time, sigma_2 - sigma_3 vanishes to rounding and every row is guarded.  Returns means, quats, scales, particles."""
    rng = np.random.default_rng(seed)
    g = np.arange(side)
    X = np.stack(np.meshgrid(g, g, g, indexing="ij"), -1).reshape(-1, 3) * 0.25
    inner = ((X > 0) & (X < (side - 1) * 0.25)).all(1)
    mu = X[inner]
    quats = rng.normal(size=(len(mu), 4))
    quats /= np.linalg.norm(quats, axis=1, keepdims=True)
    return _f32(mu), _f32(quats), _f32(np.exp(rng.uniform(-5, -3, (len(mu), 3)))), _f32(X)
