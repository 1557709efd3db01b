"""Adam in fp64 and the per-element rounding bounds the GPU update is held to, shared by tests/test_gpu_optim.py and
tests/test_gpu_training_loop.py (a helper module, not a test file).

u = 2^-24 is one fp32 rounding.  The bounds are derived in test_gpu_optim.py::test_one_step_matches_fp64_adam, next to
their first use; here they are stated once."""
import math

U = 2.0 ** -24
B1, B2, EPS = 0.9, 0.999, 1e-8


def bias_corrections(t, b1=B1, b2=B2):
    """1 - b1^t, 1 - b2^t without the cancellation of a plain power at small t."""
    return -math.expm1(t * math.log(b1)), -math.expm1(t * math.log(b2))


def update64(m, v, t, lr, b1=B1, b2=B2, eps=EPS):
    """The step of update number t in fp64 from given moments: (lr / (1 - b1^t)) m / (sqrt(v) / sqrt(1 - b2^t) + eps).
    lr: a float, or a tensor that broadcasts against m (a row trained at two rates)."""
    bc1, bc2 = bias_corrections(t, b1, b2)
    return (lr / bc1) * m.double() / (v.double().sqrt() / math.sqrt(bc2) + eps)


def moments64(m, v, g, b1=B1, b2=B2):
    """m' = b1 m + (1 - b1) g and v' = b2 v + (1 - b2) g^2 in fp64 from fp32 (or fp64) m, v, g."""
    g = g.double()
    return b1 * m.double() + (1 - b1) * g, b2 * v.double() + (1 - b2) * g * g


def scheduled_lr(lr, lr_final, decay_steps, t):
    """lr (lr_final / lr)^(min(t - 1, decay_steps) / decay_steps) at update number t; decay_steps 0 = constant."""
    if not decay_steps or lr_final is None:
        return lr
    return lr * (lr_final / lr) ** (min(t - 1, decay_steps) / decay_steps)


def first_moment_bound(m, g, b1=B1):
    """|m'gpu - m'64| <= 4u (b1 |m| + (1 - b1) |g|), from the pre-step m and the gradient."""
    return 4 * U * (b1 * m.double().abs() + (1 - b1) * g.double().abs())


def second_moment_bound(v64):
    """|v'gpu - v'64| <= 4u v'64."""
    return 4 * U * v64


def param_bound(p64, d64):
    """|p'gpu - p'64| <= u |p'64| + 16u |D64|, with p'64 = p - D64 and D64 = update64 of the GPU's own m', v'."""
    return U * p64.abs() + 16 * U * d64.abs()
