"""Reference restatements of ONE step of the fused Adam kernel (csrc/adam.hip) -- TEST INFRASTRUCTURE.

Two references, for two different questions:

  * `moments64` / `param64` (and `excess64`, which applies the bars): float64, stage-wise. From the kernel's fp32 inputs and the fp32-rounded scalars it receives
        m' = m + w1 (g - m)            v' = v beta2 + w2 g^2                    (from the OLD state)
        p' = p - step * m'_32 / (sqrt(v'_32) / bc2 + eps)                       (from the kernel's OWN fp32 m', v')
    Stage-wise because a cancelling m' is legitimately 1 ulp of max(|m|, |g|) off, and feeding that through
    step / denom would force a useless bar on p. Works on numpy arrays and on torch tensors (any device): the same few
    lines; tests/test_adam_ref_cpu.py pins the two to each other and to torch.optim.Adam run in float64.
  * `step32`: numpy, op by op in fp32 (every intermediate rounded to float32, no contraction), both forms of at::lerp.
    m' and v' are built from + - * only, so a correct kernel equals it bit for bit.

Bars of the float64 comparison, in units of u = 2^-24, derived from the operation count with correctly rounded
+ - * / sqrt and no contraction:
    m': 3 roundings: of g - m (<= 2 max) and of its product, both scaled by the weight the chosen at::lerp form keeps
        below 0.5, and of the final sum (<= max)                                         -> 2u max(|m|, |g|)
        (measured op by op: 1.2u with at::lerp's form, 2.0u - 3.6u with the other one)
    v': 4 roundings of non-negative terms that only add                                  -> 4u v'
    p': sqrt, /, +, /, *, + : 6 roundings, the last relative to max(|p|, |update|)        -> 8u max(|p|, |update|)
"""
import math

import numpy as np

U = 2.0 ** -24
TINY = float(np.finfo(np.float32).tiny)


class Scalars:
    """What adam_kernel receives: (float)(1 - beta1), (float)beta2, (float)(1 - beta2), (float)eps formed in double and
    rounded once (launch_adam), and the per-tensor step_size / bias_correction2_sqrt rounded by the float struct fields."""

    def __init__(self, lr, beta1, beta2, eps, t, rounded=True):
        r = np.float32 if rounded else np.float64       # rounded=False: the exact scalars, to pin the formula to torch in float64
        self.w1 = r(1.0 - beta1)
        self.beta2 = r(beta2)
        self.w2 = r(1.0 - beta2)
        self.eps = r(eps)
        self.step_size = r(lr / (1.0 - beta1 ** t))
        self.bc2_sqrt = r(math.sqrt(1.0 - beta2 ** t))


def _is_torch(x):
    return not isinstance(x, np.ndarray)


def _f64(x):
    return x.double() if _is_torch(x) else x.astype(np.float64)


def _sqrt(x):
    return x.sqrt() if _is_torch(x) else np.sqrt(x)


def moments64(g, m, v, s):
    """-> (m', v') in float64 from the old fp32 state."""
    g, m, v = _f64(g), _f64(m), _f64(v)
    w1 = float(s.w1)                  # m (1 - w1) + w1 g: the same value as m + w1 (g - m), without its float64 cancellation
    return m * (1.0 - w1) + w1 * g, v * float(s.beta2) + float(s.w2) * g * g


def param64(p, m_new32, v_new32, s):
    """-> (p', update) in float64 from the fp32 moments the kernel stored."""
    denom = _sqrt(_f64(v_new32)) / float(s.bc2_sqrt) + float(s.eps)
    upd = float(s.step_size) * (_f64(m_new32) / denom)
    return _f64(p) - upd, upd


def _abs(x):
    return x.abs() if _is_torch(x) else np.abs(x)


def _max(a, b):
    return a.maximum(b) if _is_torch(a) else np.maximum(a, b)


def excess64(p, g, m, v, p_new, m_new, v_new, s):
    """-> (em, ev, ep): the largest error of each stage divided by its bar's unit (u * scale). A correct kernel gives
    em <= 2, ev <= 4, ep <= 8. Non-finite outputs give inf."""
    m_ref, v_ref = moments64(g, m, v, s)
    p_ref, upd = param64(p, m_new, v_new, s)
    sm = _max(_abs(_f64(m)), _abs(_f64(g)))
    em = _abs(_f64(m_new) - m_ref) / (U * sm + 1e-300)
    ev = _abs(_f64(v_new) - v_ref) / (U * v_ref + TINY)
    ep = _abs(_f64(p_new) - p_ref) / (U * _max(_abs(_f64(p)), _abs(upd)) + 1e-300)
    out = []
    for e in (em, ev, ep):
        e = float(e.max())
        out.append(e if math.isfinite(e) else math.inf)
    return tuple(out)


def step32(p, g, m, v, s, lerp_form=None):
    """Op-by-op fp32 restatement of adam_one (numpy float32 arrays in, float32 arrays out: p', m', v').
    lerp_form: None = at::lerp's rule (weight < 0.5 -> first form), 1 / 2 = force a form (for the tests' own checks)."""
    f = np.float32
    p, g, m, v = (np.asarray(a, f) for a in (p, g, m, v))
    first = bool(s.w1 < f(0.5)) if lerp_form is None else lerp_form == 1
    with np.errstate(all="ignore"):
        d = (g - m).astype(f)
        if first:
            m2 = (m + (s.w1 * d).astype(f)).astype(f)
        else:
            m2 = (g - (d * f(f(1.0) - s.w1)).astype(f)).astype(f)
        v2 = (v * s.beta2).astype(f)
        v2 = (v2 + ((s.w2 * g).astype(f) * g).astype(f)).astype(f)
        denom = ((np.sqrt(v2, dtype=f) / s.bc2_sqrt).astype(f) + s.eps).astype(f)
        p2 = (p + (f(-s.step_size) * (m2 / denom).astype(f)).astype(f)).astype(f)
    return p2, m2, v2


def moments32_torch(g, m, v, s):
    """step32's m', v' with torch float32 tensors (CPU or GPU): one elementwise op per rounding, + - * only, so it is exact
    IEEE arithmetic wherever it runs. For tensors too large to bring back to the host."""
    w1, one_minus = float(s.w1), float(np.float32(1.0) - s.w1)
    d = g - m
    m2 = m + d * w1 if s.w1 < np.float32(0.5) else g - d * one_minus
    v2 = v * float(s.beta2)
    v2 = v2 + (g * float(s.w2)) * g
    return m2, v2


def param32_torch(p, m_new, v_new, s):
    """step32's p' with torch tensors (CPU or GPU), from the fp32 moments. sqrt and / are evaluated in float64 and rounded to
    float32: for these operations that double rounding is innocuous (53 >= 2 * 24 + 2), so the result is the correctly
    rounded fp32 one wherever it runs -- torch's own fp32 sqrt is not (its vectorised CPU sqrt is 1 ulp off on 0.6 % of
    inputs). + and * are single fp32 ops."""
    sq = v_new.double().sqrt().float()
    denom = (sq.double() / float(s.bc2_sqrt)).float() + float(s.eps)
    return p + (m_new.double() / denom.double()).float() * float(-s.step_size)


def ulp_diff(a, b):
    """|a - b| in units in the last place of fp32 (ordered-integer distance); arrays of float32."""
    def key(x):
        i = np.asarray(x, np.float32).view(np.int32).astype(np.int64)
        return np.where(i < 0, -(i & 0x7FFFFFFF), i)
    return np.abs(key(a) - key(b))
