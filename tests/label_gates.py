"""Class assignments, the fp64 reference and the gate shared by tests/test_labels_host.py and tests/test_gpu_labels.py (a
helper module, not a test file).

Reference.  The fp64 class weights W_k(p) (include/mgs_labels.h) ARE the oracle's frame for one-hot features:
feature_channel_gates.BlendReference(means2d, conics, one_hot[N, 32], ...) gives img[..., k] = W_k, and flip_weight, what
the near-threshold decisions (alpha >= 1/255, sigma >= 0, T (1 - alpha) <= 1e-4) are worth at the pixel under O.EPS_STAGE.
The blend is linear in the features, so ONE oracle run per set of lists at 32 BASE classes serves every class count: an
assignment is a map m: base class -> class (or -1), its one-hot features are the base one-hot's columns summed over
m^-1(k), and so are its fp64 class weights (`LabelReference.weights`; a base class mapped to -1 is a zeroed one-hot row).
tests/test_labels_host.py checks that shortcut against the literal oracle call on the folded one-hot features.

Gate (`check_labels`).  With top and second the two largest W_k (second = 0 for a single class), a pixel is DECIDED if
top - second > 2 flip_weight + 1e-5, or if top == 0 and flip_weight == 0 (decided empty): a flipped decision moves two
class weights by at most flip_weight each, fp32 rounding of a weight is 2e-7 .. 6e-7.
  (a) every decided pixel carries the reference's label (255 where decided empty): zero exceptions
  (b) |label_weights - top| <= 1e-5 + 2 flip_weight at every pixel: zero exceptions
  (c) undecided pixels are at most 1 % of the frame
"""
import numpy as np

from feature_channel_gates import MAX_CH, BlendReference

NONE = 255
BASE = MAX_CH                       # base classes of a reference
CLASS_COUNTS = (1, 2, 7, 32)
# (kind, K): random classes and classes cut by world x at every count, and a third of the Gaussians ignored (-1)
CASES = tuple((kind, k) for kind in ("random", "spatial") for k in CLASS_COUNTS) + (("ignore", 7),)
UNDECIDED_CAP = 0.01
WEIGHT_TOL = 1e-5


def base_classes(kind, n, means=None, seed=5):
    """int64 [n] in 0..31.  "random": uniform; "spatial": 32 slabs of equal count along world x."""
    if kind in ("random", "ignore"):
        return np.random.default_rng(seed).integers(0, BASE, n)
    if kind == "spatial":
        rank = np.argsort(np.argsort(np.asarray(means)[:, 0], kind="stable"), kind="stable")
        return rank * BASE // n
    raise ValueError(kind)


def fold(kind, k):
    """int64 [32]: base class -> class in 0..k-1, or -1.  random: j mod k; spatial: k slabs of neighbouring base slabs;
    ignore: the base classes 21..31 (a third of the Gaussians) map to -1, the others to j mod k."""
    j = np.arange(BASE)
    if kind == "random":
        return j % k
    if kind == "spatial":
        return j * k // BASE
    if kind == "ignore":
        return np.where(j < 21, j % k, -1)
    raise ValueError(kind)


def class_ids(kind, k, base):
    """The int32 class ids of assignment (kind, k) for Gaussians of base classes `base`."""
    return fold(kind, k)[np.asarray(base)].astype(np.int32)


def one_hot(ids, width=MAX_CH):
    """float32 [n, width]; a row whose id is outside 0..width-1 is zero."""
    ids = np.asarray(ids)
    out = np.zeros((len(ids), width), np.float32)
    ok = (ids >= 0) & (ids < width)
    out[np.nonzero(ok)[0], ids[ok]] = 1.0
    return out


def fold_columns(img, mapping, k):
    """[..., 32] per base class -> [..., k] per class: column c = the sum of the base columns mapped to c."""
    img = np.asarray(img)
    out = np.zeros(img.shape[:-1] + (k,), img.dtype)
    for j, c in enumerate(mapping):
        if 0 <= c < k:
            out[..., c] += img[..., j]
    return out


class LabelReference:
    """fp64 class weights of ONE camera's lists on the given fp32 inputs, for base classes `base` [n]."""

    def __init__(self, means2d, conics, opacities, flatten_ids, offsets, w, h, base):
        self.blend = BlendReference(means2d, conics, one_hot(base), opacities, flatten_ids, offsets, w, h)
        self.flip_weight = np.asarray(self.blend.flip_weight, np.float64)
        self.w, self.h = w, h

    def weights(self, kind, k):
        return fold_columns(self.blend.img, fold(kind, k), k)


def decide(W, flip_weight):
    """(label [h,w] with 255 where the top weight is 0, top, decided) of fp64 class weights W [h,w,K]."""
    W = np.asarray(W, np.float64)
    srt = np.sort(W, axis=-1)
    top = srt[..., -1]
    second = srt[..., -2] if W.shape[-1] > 1 else np.zeros_like(top)
    label = W.argmax(axis=-1).astype(np.int64)           # (argmax: the lowest index among equals)
    label[top == 0] = NONE
    decided = np.where(top == 0, flip_weight == 0, top - second > 2.0 * flip_weight + WEIGHT_TOL)
    return label, top, decided


def check_labels(W, flip_weight, labels, weights, what="labels", raise_on_fail=True):
    """THE gate of these files.  W: the reference's fp64 class weights [h,w,K]; labels uint8 [h,w]; weights float [h,w] or
    None (then (b) is not checked).  Prints and returns the statistics; asserts (a), (b), (c) unless raise_on_fail=False."""
    ref_label, top, decided = decide(W, flip_weight)
    labels = np.asarray(labels)
    assert labels.shape == ref_label.shape and labels.dtype == np.uint8, (labels.shape, labels.dtype)
    st = dict(pixels=int(decided.size), undecided=int((~decided).sum()),
              wrong_labels=int(((labels.astype(np.int64) != ref_label) & decided).sum()), weight_over=0, max_weight_err=0.0)
    if weights is not None:
        err = np.abs(np.asarray(weights, np.float64) - top)
        st["weight_over"] = int((err > WEIGHT_TOL + 2.0 * flip_weight).sum())
        st["max_weight_err"] = float(err.max())
        st["max_weight_err_decided"] = float(err[decided].max()) if decided.any() else 0.0
    print(f"\n{what}: {st['undecided']} of {st['pixels']} pixels undecided, {st['wrong_labels']} decided pixels with another "
          f"label, {st['weight_over']} weights over the bound (largest error {st['max_weight_err']:.2e})")
    st["ok"] = (st["wrong_labels"] == 0 and st["weight_over"] == 0 and st["undecided"] <= UNDECIDED_CAP * st["pixels"])
    if raise_on_fail:
        assert st["wrong_labels"] == 0, f"{what}: {st['wrong_labels']} decided pixels carry another label than the reference"
        assert st["weight_over"] == 0, f"{what}: {st['weight_over']} label weights off by more than 1e-5 + 2 flip_weight"
        assert st["undecided"] <= UNDECIDED_CAP * st["pixels"], f"{what}: {st['undecided']} undecided pixels of {st['pixels']}"
    return st
