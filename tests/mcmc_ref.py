"""splatfacto-mcmc's refinement in NumPy fp64: the three operations of include/mgs_refine.h restated, and
the rounding bounds the GPU results are held to.  Shared by tests/test_refine_host.py and tests/test_gpu_refine.py (a helper
module, not a test file).  u = 2^-24 is one fp32 rounding; each bound names the roundings it counts where it is defined."""
import math

import numpy as np

U = 2.0 ** -24
MAX_RATIO = 51
O_MAX = 1.0 - 2.0 ** -23
RELOCATE, ADD = 0, 1


def sigmoid(x):
    x = np.asarray(x, dtype=np.float64)
    e = np.exp(-np.abs(x))
    return np.where(x >= 0, 1.0 / (1.0 + e), e / (1.0 + e))


# ---- (a) weights and dead list -------------------------------------------------------------------------------------
def weights(logits, min_opacity, mode):
    """-> (w, dead indices ascending, o), all from fp64 sigmoid of the fp32 logits."""
    o = sigmoid(logits)
    dead = o <= min_opacity
    w = o.copy() if mode == ADD else np.where(dead, 0.0, o)
    return w, np.flatnonzero(dead), o


# ---- (b) sampling --------------------------------------------------------------------------------------------------
def sample(w32, u32):
    """The source of each uniform from the fp32 weights the GPU stored: the smallest i with cdf64[i] > u T.
    -> (indices, margins): margins[j] is the distance of u[j] T to the nearest bucket edge, edges that are exact (the
    zero below the first positive weight: a sum of zeros in every summation order) not counted."""
    cdf = np.cumsum(np.asarray(w32, dtype=np.float32).astype(np.float64))
    total = cdf[-1]
    x = np.asarray(u32, dtype=np.float32).astype(np.float64) * total
    idx = np.searchsorted(cdf, x, "right")
    last = int(np.flatnonzero(np.asarray(w32) > 0)[-1]) if total > 0 else 0
    idx = np.minimum(idx, last)                                   # u T >= T by rounding: the last positive row
    upper = cdf[idx] - x
    lower_edge = np.where(idx > 0, cdf[np.maximum(idx - 1, 0)], 0.0)
    lower = np.where(lower_edge > 0, x - lower_edge, np.inf)
    return idx, np.minimum(upper, lower), total


# ---- (b) relocated values ------------------------------------------------------------------------------------------
def denominator_double_sum(o_new, r):
    """gsplat's D = sum_{i=1..r} sum_{k=0..i-1} C(i-1, k) (-1)^k o_new^(k+1) / sqrt(k+1), its terms summed exactly
    (math.fsum) -> (D, sum of |terms|)."""
    terms = [math.comb(i - 1, k) * (-1.0) ** k * o_new ** (k + 1) / math.sqrt(k + 1)
             for i in range(1, r + 1) for k in range(i)]
    return math.fsum(terms), math.fsum(abs(t) for t in terms)


def denominator_single_sum(o_new, r):
    """The same D with the inner sums over i done in closed form (sum_{i=k+1..r} C(i-1, k) = C(r, k+1)):
    sum_{k=0}^{r-1} C(r, k+1) (-1)^k o_new^(k+1) / sqrt(k+1) -> (D, sum of |terms|, dD / d o_new)."""
    terms = [math.comb(r, k + 1) * (-1.0) ** k * o_new ** (k + 1) / math.sqrt(k + 1) for k in range(r)]
    slope = [math.comb(r, k + 1) * (-1.0) ** k * math.sqrt(k + 1) * o_new ** k for k in range(r)]
    return math.fsum(terms), math.fsum(abs(t) for t in terms), math.fsum(slope)


def relocated(logit32, count, min_opacity):
    """What a source drawn `count` times becomes -> dict(r, o, o_new, kept, D, cond, slope, logit, shift): the new
    opacity `kept` (its logit `logit`) and the shift of the three log-scales, ln(o / D)."""
    r = min(int(count) + 1, MAX_RATIO)
    o = min(float(sigmoid(np.float32(logit32))), O_MAX)
    o_new = -math.expm1(math.log1p(-o) / r)
    D, mag = denominator_double_sum(o_new, r)
    _, _, slope = denominator_single_sum(o_new, r)
    kept = min(max(o_new, float(min_opacity)), O_MAX)
    return dict(r=r, o=o, o_new=o_new, kept=kept, D=D, cond=mag / abs(D), slope=slope,
                logit=math.log(kept / (1.0 - kept)), shift=math.log(o / D))


def powf_error(o, r):
    """The error an fp32 evaluation o_new = 1 - powf(1 - o, 1 / r) may make, absolute: 1 - o rounded (u), 1 / r rounded
    (u, which moves p = (1 - o)^(1/r) by u |ln p| p), powf itself (1 ulp = 2u of p), the subtraction (u of o_new)."""
    p = (1.0 - o) ** (1.0 / r)
    return U * p / r + U * abs(math.log(p)) * p + 2 * U * p + U * (1.0 - p)


def relocated_bounds(ref, log_s64):
    """-> (bound on |o_gpu - kept|, bound on |s_gpu / s_ref - 1|) for the opacity sigmoid(stored logit) and the scales
    exp(stored log-scale), from the reference's own numbers.
      o: the powf allowance above (only where the value is not clamped away) and the one rounding of the stored logit,
         u |logit| in the logit = u |logit| kept (1 - kept) in o, doubled for the second-order terms;
      s: D's own evaluation -- r terms of three roundings and r additions in fp64, each amplified by the condition
         number: 4 r cond 2^-53 --, D's sensitivity to o_new, |dD/do_new| powf_error / |D|, the shift rounded to fp32
         (u |shift|) and added to the log-scale in fp32 (u |log_s'|), doubled likewise."""
    e_pow = powf_error(ref["o"], ref["r"])
    o_bound = e_pow + 2 * U * abs(ref["logit"]) * ref["kept"] * (1.0 - ref["kept"]) + 1e-300
    fp64 = 4 * ref["r"] * ref["cond"] * 2.0 ** -53
    shifted = np.abs(np.asarray(log_s64, dtype=np.float64) + ref["shift"])
    s_bound = fp64 + abs(ref["slope"]) * e_pow / abs(ref["D"]) + 2 * U * (abs(ref["shift"]) + shifted)
    return o_bound, s_bound


# ---- (c) noise -----------------------------------------------------------------------------------------------------
def next_rate(lr, lr_final, decay_steps, t):
    """lr (lr_final / lr)^(min(t, decay_steps) / decay_steps) with t the updates already taken; decay_steps 0: lr."""
    if not decay_steps or lr_final is None:
        return lr
    return lr * (lr_final / lr) ** (min(t, decay_steps) / decay_steps)


def rotation(q):
    q = np.asarray(q, dtype=np.float64)
    w, x, y, z = (q / np.linalg.norm(q, axis=-1, keepdims=True)).T
    return np.stack([1 - 2 * (y * y + z * z), 2 * (x * y - w * z), 2 * (x * z + w * y),
                     2 * (x * y + w * z), 1 - 2 * (x * x + z * z), 2 * (y * z - w * x),
                     2 * (x * z - w * y), 2 * (y * z + w * x), 1 - 2 * (x * x + y * y)], -1).reshape(-1, 3, 3)


def noise(quats, log_scales, logits, z, lam):
    """-> (displacement Sigma (z gate lam) [n, 3], gate [n], bound [n]) in fp64 from the fp32 inputs.

    bound: |d_gpu - d| per component <= (G + 80u) A with A = gate lam (sum_k s_k^2) |z|_1 >= every partial sum of the
    two matrix products (|R_ij| <= 1), and
      G = 3u + 500u (1 - gate): 1 - o = 1 / (1 + expf(x)) carries expf's 1 ulp = 2u, the sum and the division (u each),
          and 0.995 rounded to fp32 (u / 2): 4.5u absolute on the difference, times 100 in the exponent; the product
          with 100 rounded (u of an exponent below 100: 100u); expf's own 2u: below 500u relative on e = exp(.), of
          which the gate 1 / (1 + e) takes the fraction e / (1 + e) = 1 - gate; then the sum and the division (u each,
          rounded up to 3u);
      80u: lambda rounded to fp32 (u), gate * lambda, z * (.) (u each), expf(2 log_s) (2u): 5u; the two products with
          R: a normalised component carries 6u (four squares and three additions of positive terms 4u, sqrtf 2u -> the
          norm 3u; its reciprocal u; the product u; rounded up), a product of two of them 13u of at most 1/2, an entry
          2 (a b +- c d) or 1 - 2 (a^2 + b^2) therefore at most 30u absolute, and a three-term dot product adds 3u:
          2 (30u + 3u) = 66u; together 71u, rounded up."""
    R = rotation(quats)
    s2 = np.exp(2.0 * np.asarray(log_scales, dtype=np.float64))
    rest = sigmoid(-np.asarray(logits, dtype=np.float64))                     # 1 - o
    gate = sigmoid(100.0 * (rest - 0.995))
    z = np.asarray(z, dtype=np.float64)
    v = z * (gate * lam)[:, None]
    d = np.einsum("nik,nk,njk,nj->ni", R, s2, R, v)
    G = 3 * U + 500 * U * (1.0 - gate)
    A = gate * lam * s2.sum(-1) * np.abs(z).sum(-1)
    return d, gate, (G + 80 * U) * A
