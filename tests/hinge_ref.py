"""fp64 NumPy restatement of the hinge fit (include/mgs_hinge.h) for the tests: chunked brute-force nearest neighbours, the
contact rule, the position, the PCA axis with the sign rule and the fallback.  The inputs are the fp32 points a kernel
reads, taken to fp64 exactly; nothing here is fp32 arithmetic, so it is what the kernels are held to.

    ref = fit(points_a, points_b, threshold)
    ref.contact_a / ref.contact_b    bool masks
    ref.min2, ref.min_distance       the A-side minimum of the squared nearest-neighbour distance, and its root
    ref.position, ref.axis, ref.axis_confidence, ref.eigenvalues (ascending), ref.fallback, ref.nonfinite
    ref.gap                          the smallest |d - (min_distance + threshold)| over all finite points of both sets: how
                                     far the contact decision is from flipping (the condition a GPU test asserts on its input)
"""
from types import SimpleNamespace

import numpy as np


def nn2(p, q, chunk=None):
    """min_j |p_i - q_j|^2 in fp64, in the difference form; rows of p or q with a non-finite coordinate take no part
    (their own result is NaN)."""
    p, q = np.asarray(p, np.float64), np.asarray(q, np.float64)
    out = np.full(len(p), np.nan)
    rows = np.flatnonzero(np.isfinite(p).all(1))
    q = q[np.isfinite(q).all(1)]
    if len(q) == 0:
        return out
    chunk = chunk or max(64, 2_000_000 // len(q))           # about 16 MB per temporary
    for s in range(0, len(rows), chunk):
        r = rows[s:s + chunk]
        dx, dy, dz = (p[r, c, None] - q[None, :, c] for c in range(3))
        out[r] = (dx * dx + dy * dy + dz * dz).min(1)
    return out


def sign_rule(axis):
    """The component of largest magnitude positive; ties go to the lowest index."""
    k = int(np.argmax(np.abs(axis)))              # argmax: the first of equals
    return -axis if axis[k] < 0 else axis


def fit(points_a, points_b, threshold=0.01):
    a32, b32 = np.asarray(points_a, np.float32), np.asarray(points_b, np.float32)
    a, b = a32.astype(np.float64), b32.astype(np.float64)
    thr = float(np.float32(threshold))            # the entry point takes a float
    na2, nb2 = nn2(a, b), nn2(b, a)
    min2 = np.nanmin(na2)
    da, db, dmin = np.sqrt(na2), np.sqrt(nb2), np.sqrt(min2)
    limit = dmin + thr
    with np.errstate(invalid="ignore"):
        ca, cb = da < limit, db < limit
    gap = float(np.nanmin(np.abs(np.concatenate([da, db]) - limit)))
    pa, pb = a[ca], b[cb]
    position = (pa.mean(0) + pb.mean(0)) / 2
    both = np.vstack([pa, pb])
    cov = np.cov((both - both.mean(0)).T) if len(both) > 1 else np.zeros((3, 3))
    w, v = np.linalg.eigh(cov)
    total = w.sum()
    conf = float(w[-1] / total) if total > 0 else 0.0
    fallback = not conf >= 0.5
    axis = np.array([1.0, 0.0, 0.0]) if fallback else sign_rule(v[:, -1] / np.linalg.norm(v[:, -1]))
    nonfinite = not (np.isfinite(a32).all() and np.isfinite(b32).all())
    return SimpleNamespace(contact_a=ca, contact_b=cb, min2=float(min2), min_distance=float(dmin), position=position, axis=axis,
                           axis_confidence=conf, eigenvalues=w, fallback=fallback, nonfinite=nonfinite, gap=gap,
                           n_contact=(int(ca.sum()), int(cb.sum())))
