"""RCV_OP_LP_INPUT (include/rcv.h, csrc/lp_input.hip) restated in float64 numpy: per pixel of sample s

    out[s] = [Ycur, Yprev, Ycur - Yprev, prior_0 .. prior_4]          (returned NCHW: [B, 8, H, W])

Y = channel 0 of a [B, C, H, W] frame tensor (or a [B, H, W] plane).  Stream form: sample s reads cur[s], prev[s], prior[s].  Pair
form: ``cur`` is [B/2, 2, C, H, W] seen as B frames, sample s reads frames s and s ^ 1 and prior[s ^ 1] (labelPropTrain.py:181-182).
The prior is a class map (any integer dtype: +1 at the class, -1 elsewhere; a value outside [0, 5) selects no class) or logits
[B, 5, H, W] (2 * softmax - 1 with the maximum subtracted first).  ``variant`` names the wrong kernels the tests must tell apart."""
import numpy as np

CLASSES = 5
VARIANTS = (None, "no_max", "no_scale", "class_order", "own_prior")


def hard_prior(labels):
    """Class map [B, H, W] (any integer dtype, the full value decides) -> float64 [B, 5, H, W]."""
    lab = np.asarray(labels)
    out = -np.ones((lab.shape[0], CLASSES) + lab.shape[1:], dtype=np.float64)
    for c in range(CLASSES):
        out[:, c][lab == c] = 1.0
    return out


def soft_prior(logits, variant=None):
    """Logits [B, 5, H, W] -> 2 * softmax - 1 in float64.  ``no_max`` forms the exponentials in float32 without subtracting the
    maximum, as a kernel that forgot it would; ``no_scale`` is the plain softmax; ``class_order`` reverses the class channels."""
    z = np.asarray(logits).astype(np.float64)
    if variant == "no_max":
        with np.errstate(over="ignore", invalid="ignore"):
            e = np.exp(np.asarray(logits).astype(np.float32)).astype(np.float64)
            q = e / e.sum(axis=1, keepdims=True)
    else:
        e = np.exp(z - z.max(axis=1, keepdims=True))
        q = e / e.sum(axis=1, keepdims=True)
    if variant == "class_order":
        q = q[:, ::-1]
    return q if variant == "no_scale" else 2.0 * q - 1.0


def _y(frames):
    f = np.asarray(frames).astype(np.float64)
    return f if f.ndim == 3 else f[:, 0]


def lp_input(cur, prev, prior, pair=False, variant=None):
    """-> float64 [B, 8, H, W].  ``prev`` is ignored in the pair form.  The difference is formed in float32, as the op does (one
    fp32 subtraction of fp32 values), then widened."""
    prior = np.asarray(prior)
    if pair:
        frames = np.asarray(cur)
        frames = frames.reshape((-1,) + frames.shape[2:])          # [B/2, 2, C, H, W] -> B frames
        assert frames.shape[0] % 2 == 0
        other = np.arange(frames.shape[0]) ^ 1
        ycur, yprev = _y(frames), _y(frames)[other]
        if variant != "own_prior":
            prior = prior[other]
    else:
        ycur, yprev = _y(cur), _y(prev)
    p = soft_prior(prior, variant) if prior.dtype.kind == "f" else hard_prior(prior)
    diff = (ycur.astype(np.float32) - yprev.astype(np.float32)).astype(np.float64)
    return np.concatenate([ycur[:, None], yprev[:, None], diff[:, None], p], axis=1)


# ------------------------------------------------------------------------------------------ shared inputs of the tests
# The soft prior's error bound, in units of u = 2^-24, for one output out_c = 2 * (e_c / S) - 1 with m = max z, d_c = z_c - m <= 0,
# e_c = expf(d_c), S = (((e_0 + e_1) + e_2) + e_3) + e_4 in [1, 5], q_c = e_c / S <= 1 (first order in u; the float64 restatement's
# own error, ~1e-16, is noise against it):
#   * d_c: one rounding, relative u, which moves e_c by the relative amount |d_c| u;
#   * expf: ROCm's table of device-function accuracy is not on hand, so 2 ulp is ASSUMED: relative 2 * 2^-23 = 4 u;
#   * S: four additions, every term passes through at most four of them: relative 4 u on top of the terms' own errors, which are
#     (sum_j |d_j| e_j u + 4 u S) / S <= (4 / e) u + 4 u, since |d| exp(d) <= 1 / e and at most four classes have d != 0;
#   * the division: relative u.
#   relative error of q_c <= (|d_c| + 4 + 4 / e + 4 + 4 + 1) u, and with q_c |d_c| <= 1 / e and q_c <= 1:
#   |dq_c| <= (1 / e + 4 / e + 13) u = 14.84 u;  2 q_c is exact;  the final subtraction rounds a value of magnitude <= 1: <= u.
#   |d out_c| <= 2 * 14.84 u + u = 30.7 u, rounded up for the second-order terms:
SOFT_BOUND = 32 * 2.0 ** -24


def soft_logit_cases(B, H, W, seed):
    """name -> float32 [B, 5, H, W]: ordinary logits, five equal logits, logits spread over +-60, logits of 1e4 + small."""
    rng = np.random.default_rng(seed)
    shape = (B, CLASSES, H, W)
    equal = np.broadcast_to(rng.standard_normal((B, 1, H, W)), shape)
    return {"ordinary": (3.0 * rng.standard_normal(shape)).astype(np.float32),
            "equal": np.ascontiguousarray(equal).astype(np.float32),
            "spread60": rng.uniform(-60.0, 60.0, shape).astype(np.float32),
            "offset1e4": (1e4 + rng.standard_normal(shape)).astype(np.float32)}


def class_map_case(B, H, W, seed, dtype):
    """A class map that holds every class and the out-of-range values 5, 255 and, int64 only, -100 and 2^32 + 2."""
    rng = np.random.default_rng(seed)
    values = [0, 1, 2, 3, 4, 5, 255] + ([-100, 2 ** 32 + 2] if np.dtype(dtype) == np.int64 else [])
    flat = np.asarray(values, dtype=dtype)[rng.integers(0, len(values), B * H * W)]
    flat[:len(values)] = np.asarray(values, dtype=dtype)          # every value at least once (the smallest shape has 35 pixels)
    return flat.reshape(B, H, W)
