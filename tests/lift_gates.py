"""Masks, the fp64 vote reference and the gate shared by tests/test_lift_host.py and tests/test_gpu_lift.py (a helper module,
not a test file).

Reference (`walk`).  The fp64 walk of ONE camera's lists on the given fp32 means2d / conics / opacities -- the loop of
test_labels_host._corrupt_blends' "ok" branch in float64 -- summed per Gaussian over the pixels of each mask class:
    V[g,k] = sum over p with mask(p) == k of w_g(p),     n[g,k] = the number of those pixels at which g is counted.
One walk serves every mask: the weights of a tile are a matrix [entries, pixels], a mask is a one-hot [pixels, K].
tests/test_lift_host.py checks it against v_feats of feature_channel_gates.BackwardReference (features ones, cotangent
one-hot(mask)) to 1e-9.

Bound.  A vote is a sum of the per-pixel weights that label_gates' gate (b) bounds by WEIGHT_TOL + 2 flip_weight, so
    B[g,k] = WEIGHT_TOL n[g,k] + 2 sum over the tiles t listing g of sum over p in t with mask(p) == k of flip_weight(p)
with flip_weight from feature_channel_gates.BlendReference under O.EPS_STAGE and WEIGHT_TOL = 1e-5 label_gates' own.
(The 1e-5 per counted pixel lets none of test_lift_host's corrupted walks through, so it is not tightened.)

Gate (`check_votes`).
  (a) |votes 2^-32 - V| <= B at every (g,k), zero exceptions; where B == 0 the vote is exactly 0
  (b) with top / second the two largest V[g,.], a Gaussian is DECIDED when top - second > B_top + B_second and
      |top - min_vote| > B_top, or when all of V[g,.] and B[g,.] are 0 (decided -1); every decided Gaussian carries the
      reference's class, zero exceptions, and its confidence is within (B_top + sum B) / total of the reference's
  (c) undecided Gaussians are at most 5 % of N -- asked of the stripes and ignore masks with K <= 7 only (CAPPED)
"""
import numpy as np

from feature_channel_gates import MAX_CH, TILE, BlendReference, tiles_of
from label_gates import WEIGHT_TOL

IGNORE = 255
Q32 = 4294967296.0
UNDECIDED_CAP = 0.05
# (mask kind, K): what both test files run
CASES = (("stripes", 1), ("stripes", 2), ("stripes", 7), ("stripes", 32), ("checker", 7), ("checker", 32), ("ignore", 7),
         ("high", 7))
CAPPED = {("stripes", 1), ("stripes", 2), ("stripes", 7), ("ignore", 7)}
BUGS = ("count_closing", "no_stop", "stale_T", "shift", "ignore_as_zero", "drop_quadrant", "first_class_only")


def _third_of_blocks(w, h):
    """bool [h,w]: a third of the 8x8 blocks."""
    y, x = np.mgrid[0:h, 0:w]
    return ((x // 8) + 2 * (y // 8)) % 3 == 0


def make_mask(kind, k, w, h):
    """uint8 [h,w].  stripes: x k // w, large regions, some tiles cut; checker: ((x // 4) + 5 (y // 4)) % k, 16 classes
    inside one tile at k = 32 (7 at k = 7); ignore: stripes with a third of the 8x8 blocks set to 255; high: stripes with that third set to values
    k..254 (all of them, pixel by pixel), which are no class and must vote for nothing."""
    y, x = np.mgrid[0:h, 0:w]
    if kind == "checker":
        return (((x // 4) + 5 * (y // 4)) % k).astype(np.uint8)
    m = (x * k // w).astype(np.uint8)
    if kind == "stripes":
        return m
    hole = _third_of_blocks(w, h)
    if kind == "ignore":
        return np.where(hole, IGNORE, m).astype(np.uint8)
    if kind == "high":
        return np.where(hole, k + (x + 31 * y) % (IGNORE - k), m).astype(np.uint8)
    raise ValueError(kind)


def masks_for(w, h, cases=CASES):
    return {case: (make_mask(case[0], case[1], w, h), case[1]) for case in cases}


def _one_hot(mask_tile, k, bug, lx, ly):
    """[P,K] float64 of a tile's mask values [P]; the mask bugs of test_lift_host live here."""
    m = mask_tile.astype(np.int64)
    if bug == "ignore_as_zero":
        m = np.where(m == IGNORE, 0, m)
    ok = m < k
    if bug == "shift":
        m = (m + 1) % k
    if bug == "drop_quadrant":
        ok = ok & ~((lx >= 8) & (ly >= 8))
    if bug == "first_class_only" and ok.any():
        ok = ok & (m == m[ok].min())
    out = np.zeros((len(m), k))
    out[np.nonzero(ok)[0], m[ok]] = 1.0
    return out


def walk(means2d, conics, opacities, flatten_ids, offsets, w, h, masks, dtype=np.float64, bug=None, flip_weight=None):
    """masks: {name: (uint8 [h,w], K)} -> {name: (V [n,K] float64, count [n,K] int64, flip [n,K] float64)}.
    dtype float64: the reference.  dtype float32: a plain fp32 blend that sums a tile's votes in fp32 and accumulates
    rint(sum 2^32) as integers, the stand-in for the kernel; `bug` corrupts it (BUGS).  flip [g,k] is the sum over the tiles
    listing g of the flip_weight of the tile's pixels of class k (zeros without flip_weight)."""
    mu, con, opa = np.asarray(means2d, dtype), np.asarray(conics, dtype), np.asarray(opacities, dtype)
    ids = np.asarray(flatten_ids).astype(np.int64)
    n = mu.shape[0]
    tw, th = tiles_of(w, h)
    flat = np.concatenate([np.asarray(offsets).reshape(-1), [len(ids)]]).astype(np.int64)
    exact = dtype == np.float64
    out = {name: (np.zeros((n, k), np.float64 if exact else np.int64), np.zeros((n, k), np.int64), np.zeros((n, k)))
           for name, (_, k) in masks.items()}
    one, half = dtype(1), dtype(0.5)
    for t in range(tw * th):
        s, e = flat[t], flat[t + 1]
        if s >= e:
            continue
        ty, tx = divmod(t, tw)
        y0, y1, x0, x1 = ty * TILE, min(ty * TILE + TILE, h), tx * TILE, min(tx * TILE + TILE, w)
        gy, gx = np.meshgrid(np.arange(y0, y1), np.arange(x0, x1), indexing="ij")
        gy, gx = gy.reshape(-1), gx.reshape(-1)
        px, py = gx.astype(dtype) + half, gy.astype(dtype) + half
        T, done = np.ones_like(px), np.zeros(px.shape, bool)
        Wt = np.zeros((e - s, len(px)), dtype)
        counted = np.zeros((e - s, len(px)), bool)
        for j, i in enumerate(range(s, e)):
            g = ids[i]
            dx, dy = mu[g, 0] - px, mu[g, 1] - py
            sig = half * (con[g, 0] * dx * dx + con[g, 2] * dy * dy) + con[g, 1] * dx * dy
            a = np.minimum(dtype(0.999), opa[g] * np.exp(-sig)).astype(dtype)
            hit = (sig >= 0) & (a >= dtype(1 / 255))
            if bug == "no_stop":                                 # never finished: T runs on past the stop rule
                Wt[j] = np.where(hit, a * T, 0)
                counted[j] = hit
                T = np.where(hit, T * (one - a), T)
                continue
            ok = hit & ~done
            Tn = T * (one - a)
            stop = ok & (Tn <= dtype(1e-4))
            acc = ok & ~stop
            cnt = ok if bug == "count_closing" else acc
            Wt[j] = np.where(cnt, a if bug == "stale_T" else a * T, 0)
            counted[j] = cnt
            T = np.where(acc, Tn, T)
            done |= stop
        rows = ids[s:e]                                           # (a Gaussian is listed once per tile)
        for name, (mask, k) in masks.items():
            oh = _one_hot(mask[gy, gx], k, bug, gx - x0, gy - y0)
            V, N, F = out[name]
            if exact:
                V[rows] += Wt @ oh
            else:
                V[rows] += np.rint((Wt @ oh.astype(dtype)).astype(dtype).astype(np.float64) * Q32).astype(np.int64)
            N[rows] += counted.astype(np.int64) @ oh.astype(np.int64)
            if flip_weight is not None:
                F[rows] += (np.asarray(flip_weight, np.float64)[gy, gx] @ oh)[None, :]
    return out


class VoteReference:
    """fp64 votes of ONE camera's lists on the given fp32 inputs for every mask of `masks`, with the gate's bound."""

    def __init__(self, means2d, conics, opacities, flatten_ids, offsets, w, h, masks):
        n = np.asarray(means2d).shape[0]
        self.blend = BlendReference(means2d, conics, np.zeros((n, MAX_CH), np.float32), opacities, flatten_ids, offsets, w, h)
        self.flip_weight = np.asarray(self.blend.flip_weight, np.float64)
        self.could_flip = int((self.flip_weight > 0).sum())
        self.args = (means2d, conics, opacities, flatten_ids, offsets, w, h)
        self.masks, self.out = {}, {}
        self.extend(masks)

    def extend(self, masks):
        """Further masks on the same lists (one more walk; the blend's flip weights are kept)."""
        masks = {name: m for name, m in masks.items() if name not in self.out}
        if masks:
            self.masks.update(masks)
            self.out.update(walk(*self.args, masks, flip_weight=self.flip_weight))
        return self

    def V(self, name):
        return self.out[name][0]

    def count(self, name):
        return self.out[name][1]

    def bound(self, name):
        _, cnt, flip = self.out[name]
        return WEIGHT_TOL * cnt + 2.0 * flip


def decide(V, B, min_vote=0.0):
    """(class [n] with -1 where the top vote does not exceed min_vote, top, total, decided, B_top) of fp64 votes V [n,K]."""
    V, B = np.asarray(V, np.float64), np.asarray(B, np.float64)
    order = np.argsort(-V, axis=1, kind="stable")                # (stable: the lowest class among equals comes first)
    rows = np.arange(len(V))
    i_top = order[:, 0]
    top, b_top = V[rows, i_top], B[rows, i_top]
    if V.shape[1] > 1:
        second, b_second = V[rows, order[:, 1]], B[rows, order[:, 1]]
    else:
        second, b_second = np.zeros_like(top), np.zeros_like(top)
    cls = np.where(top > min_vote, i_top, -1).astype(np.int64)
    empty = (V == 0).all(axis=1) & (B == 0).all(axis=1)
    decided = ((top - second > b_top + b_second) & (np.abs(top - min_vote) > b_top)) | empty
    return cls, top, V.sum(axis=1), decided, b_top


def check_votes(V, B, votes, class_ids=None, confidence=None, min_vote=0.0, capped=False, what="votes", raise_on_fail=True):
    """THE gate of these files.  V, B: the reference's votes and bound [n,K]; votes: int64 Q32 [n,K]; class_ids int32 [n] and
    confidence [n] (both or neither: without them only (a) is checked).  Prints and returns the statistics; asserts (a),
    (b) and -- capped -- (c) unless raise_on_fail=False."""
    V, B = np.asarray(V, np.float64), np.asarray(B, np.float64)
    votes = np.asarray(votes)
    assert votes.shape == V.shape and votes.dtype == np.int64 and (votes >= 0).all(), (votes.shape, votes.dtype)
    got = votes.astype(np.float64) / Q32
    err = np.abs(got - V)
    with np.errstate(divide="ignore", invalid="ignore"):
        ratio = np.where(B > 0, err / B, 0.0)
    st = dict(n=len(V), over=int((err > B).sum()), nonzero_at_zero_bound=int(((B == 0) & (votes != 0)).sum()),
              max_err=float(err.max()) if err.size else 0.0, max_ratio=float(ratio.max()) if ratio.size else 0.0,
              max_vote=float(V.max()) if V.size else 0.0, voted=int((V.sum(axis=1) > 0).sum()), undecided=0, wrong_class=0,
              confidence_over=0)
    if class_ids is not None:
        ref_cls, top, total, decided, b_top = decide(V, B, min_vote)
        class_ids, confidence = np.asarray(class_ids).astype(np.int64), np.asarray(confidence, np.float64)
        assert class_ids.shape == ref_cls.shape == confidence.shape
        st["undecided"] = int((~decided).sum())
        st["wrong_class"] = int(((class_ids != ref_cls) & decided).sum())
        with np.errstate(divide="ignore", invalid="ignore"):
            ref_conf = np.where(ref_cls >= 0, top / total, 0.0)
            tol = np.where(ref_cls >= 0, (b_top + B.sum(axis=1)) / total, 0.0)
        st["confidence_over"] = int(((np.abs(confidence - ref_conf) > tol) & decided).sum())
    print(f"\n{what}: {st['over']} of {V.size} votes over the bound (largest error {st['max_err']:.2e}, worst error / bound "
          f"{st['max_ratio']:.4f}, largest vote {st['max_vote']:.1f}), {st['nonzero_at_zero_bound']} non-zero where the bound is 0, "
          f"{st['voted']} of {st['n']} Gaussians voted, {st['undecided']} undecided ({st['undecided'] / max(1, st['n']):.2%}), "
          f"{st['wrong_class']} decided with another class, {st['confidence_over']} confidences over the bound")
    st["ok"] = (st["over"] == 0 and st["nonzero_at_zero_bound"] == 0 and st["wrong_class"] == 0 and st["confidence_over"] == 0
                and (not capped or st["undecided"] <= UNDECIDED_CAP * st["n"]))
    if raise_on_fail:
        assert st["over"] == 0, f"{what}: {st['over']} votes off by more than the bound"
        assert st["nonzero_at_zero_bound"] == 0, f"{what}: {st['nonzero_at_zero_bound']} votes where nothing can vote"
        assert st["wrong_class"] == 0, f"{what}: {st['wrong_class']} decided Gaussians carry another class than the reference"
        assert st["confidence_over"] == 0, f"{what}: {st['confidence_over']} confidences off by more than the bound"
        if capped:
            assert st["undecided"] <= UNDECIDED_CAP * st["n"], f"{what}: {st['undecided']} undecided Gaussians of {st['n']}"
    return st


def assign(votes, min_vote=0.0):
    """What lift_assign_kernel makes of Q32 votes [n,K]: (class_ids, confidence)."""
    votes = np.asarray(votes, np.int64)
    cls = votes.argmax(axis=1)
    top = votes[np.arange(len(votes)), cls]
    ok = top > int(np.rint(min_vote * Q32))
    total = votes.sum(axis=1)
    conf = np.where(ok, top / np.maximum(total, 1), 0.0).astype(np.float32)
    return np.where(ok, cls, -1).astype(np.int32), conf
