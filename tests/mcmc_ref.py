"""Host restatement of MCMC density control (csrc/mcmc.hip; include/c3dgs_hip.h "MCMC density control"): numpy float64 on the
same fp32 raw inputs, Python integers for the prefix sums. Shared by tests/test_mcmc_ref_cpu.py (which pins this file's
mathematics) and tests/test_mcmc_gpu.py (which holds the kernels to it)."""
import itertools
import math

import numpy as np

WEIGHT_ONE = 1 << 20
MAX_N = 51
FLT_EPSILON = float(np.finfo(np.float32).eps)


def sigmoid(raw, dtype=np.float64):
    x = np.asarray(raw, dtype=np.float32).astype(dtype)
    with np.errstate(over="ignore"):
        return (1 / (1 + np.exp(-x))).astype(dtype)


def weights(raw_opacity, dead=None, min_opacity=None):
    """-> (q int64 [P], dead bool [P] | None). q = floor(sigmoid 2^20), 0 on excluded rows: `dead`, or with dead None and a
    min_opacity the rows with sigmoid <= min_opacity, or nobody."""
    o = sigmoid(np.asarray(raw_opacity).reshape(-1))
    q = np.floor(o * WEIGHT_ONE).astype(np.int64)
    if dead is None and min_opacity is not None:
        dead = o <= np.float64(np.float32(min_opacity))
    if dead is not None:
        dead = np.asarray(dead).astype(bool)
        q[dead] = 0
    return q, dead


def prefix(q):
    """Inclusive prefix of q as Python integers."""
    return list(itertools.accumulate(int(v) for v in np.asarray(q).tolist()))


def sample(q, draws):
    """-> (sources int32 [n], counts int32 [P], T). t_j = min(T - 1, floor(draws[j] * float(T))), one IEEE multiply; the source is
    the smallest i with C_i > t_j. T == 0: every source is -1."""
    q = np.asarray(q)
    draws = np.asarray(draws, dtype=np.float64)
    C = prefix(q)
    T = C[-1] if C else 0
    counts = np.zeros(len(C), dtype=np.int32)
    if T == 0:
        return np.full(draws.shape[0], -1, dtype=np.int32), counts, 0
    assert T < 2 ** 53                                            # float(T) is exact
    t = np.minimum(np.floor(draws * np.float64(T)), np.float64(T - 1)).astype(np.int64)     # both exact in a double
    Ca = np.array(C, dtype=np.int64)
    sources = np.searchsorted(Ca, t, side="right").astype(np.int32)
    np.add.at(counts, sources, 1)
    return sources, counts, T


def new_opacity(raw, N, min_opacity=0.005, dtype=np.float64):
    """o' = 1 - (1 - o)^(1/N) from the raw opacity, through log(1 - o) = -log(1 + e^raw), clamped to [min_opacity, 1 - FLT_EPSILON]."""
    x = np.asarray(raw, dtype=np.float32).astype(dtype)
    with np.errstate(over="ignore"):
        on = -np.expm1(-np.log1p(np.exp(x)) / np.asarray(N, dtype=dtype))
    return np.clip(on, dtype(np.float32(min_opacity)), dtype(1.0 - FLT_EPSILON)).astype(dtype)


def relocation(o, N, min_opacity=0.005):
    """Scalars, float64. -> (o', c): o' = 1 - (1 - o)^(1/N) clamped; c = o / sum_{i=1..N} sum_{k<i} C(i-1,k) (-1)^k o'^(k+1) / sqrt(k+1)."""
    N = int(N)
    o = float(o)
    on = -math.expm1(math.log1p(-o) / N)
    on = min(max(on, float(np.float32(min_opacity))), 1.0 - FLT_EPSILON)
    return on, o / _denominator(on, N)


def _denominator(on, N):
    denom = 0.0
    for i in range(1, N + 1):
        for k in range(i):
            denom += math.comb(i - 1, k) * (-1) ** k * on ** (k + 1) / math.sqrt(k + 1)
    return denom


def values(raw_opacity, counts, min_opacity=0.005):
    """Per row with count > 0, from the fp32 raw opacity in float64 -> (rows, o' [rows], c [rows])."""
    counts = np.asarray(counts)
    rows = np.nonzero(counts > 0)[0]
    raw = np.asarray(raw_opacity, dtype=np.float32).reshape(-1)
    on = np.empty(rows.shape[0])
    c = np.empty(rows.shape[0])
    for a, i in enumerate(rows):
        N = min(int(counts[i]) + 1, MAX_N)
        on[a] = float(new_opacity(raw[i], N, min_opacity))
        c[a] = float(sigmoid(raw[i])) / _denominator(on[a], N)
    return rows, on, c


def write_back(on, c, raw_scale_rows, dtype=np.float64):
    """The write-back step in `dtype` from the float64 (o', c): raw opacity = logit(o'), raw scale rows += log c."""
    on, c = np.asarray(on).astype(dtype), np.asarray(c).astype(dtype)
    raw_op = np.log(on / (1 - on))
    return raw_op.astype(dtype), (np.asarray(raw_scale_rows, dtype=np.float32).astype(dtype) + np.log(c)[:, None]).astype(dtype)


def apply(params, moments, dst, sources, counts, copy_rows, scale_key, min_opacity=0.005):
    """params: {name: float32 [P, ...]} with "opacity" among them, moments: {name: (exp_avg, exp_avg_sq)}. -> new (params,
    moments), every value computed from the state before the call: destinations take their source's row (copy_rows) and its
    relocation opacity / scale, sources their own, moments of both become zero. Opacity and scale are float64 here."""
    new = {k: np.array(v, dtype=np.float64) for k, v in params.items()}
    mom = {k: (np.array(a), np.array(b)) for k, (a, b) in moments.items()}
    P = params["opacity"].shape[0]
    rows, on, c = values(params["opacity"], counts, min_opacity)
    at = {int(r): a for a, r in enumerate(rows)}
    sc = np.asarray(params[scale_key], dtype=np.float32).reshape(P, -1)
    raw_op, raw_sc = write_back(on, c, sc[rows])
    for j, (d, s) in enumerate(zip(np.asarray(dst).tolist(), np.asarray(sources).tolist())):
        if s < 0:
            continue
        for k in new:
            if copy_rows:
                new[k][d] = params[k][s]
        for r in (d, s):
            new["opacity"][r] = raw_op[at[s]]
            new[scale_key].reshape(P, -1)[r] = raw_sc[at[s]]
            for k in mom:
                mom[k][0][r] = 0
                mom[k][1][r] = 0
    return new, mom


def noise(xyz_unused, rotation, scaling, scaling_factor, raw_opacity, xi, noise_lr, xyz_lr, dtype=np.float64):
    """-> the xyz delta [P,3]: R diag(s^2) R^T xi g(o) noise_lr xyz_lr, every step in `dtype` from the fp32 inputs."""
    f = lambda a: np.asarray(a, dtype=np.float32).astype(dtype)      # noqa: E731
    q = f(rotation)
    q = q / np.maximum(np.sqrt((q * q).sum(1, keepdims=True)), dtype(1e-12))
    r, x, y, z = q[:, 0], q[:, 1], q[:, 2], q[:, 3]
    two, one = dtype(2), dtype(1)
    R = np.stack([one - two * (y * y + z * z), two * (x * y - r * z), two * (x * z + r * y),
                  two * (x * y + r * z), one - two * (x * x + z * z), two * (y * z - r * x),
                  two * (x * z - r * y), two * (y * z + r * x), one - two * (x * x + y * y)], 1).reshape(-1, 3, 3).astype(dtype)
    s = f(scaling)
    if scaling_factor is None:
        s = np.exp(s)
    else:
        s = np.maximum(s, dtype(0))
        s = s / np.maximum(np.sqrt((s * s).sum(1, keepdims=True)), dtype(1e-12)) * np.exp(f(scaling_factor).reshape(-1, 1))
    s = s.astype(dtype)
    v = np.einsum("pij,pi->pj", R, f(xi)).astype(dtype) * (s * s)
    d = np.einsum("pij,pj->pi", R, v).astype(dtype)
    o = sigmoid(np.asarray(raw_opacity).reshape(-1), dtype)
    with np.errstate(over="ignore"):
        g = one / (one + np.exp(dtype(-100) * ((one - o) - dtype(0.995))))
    return (d * (g.astype(dtype) * dtype(noise_lr) * dtype(xyz_lr))[:, None]).astype(dtype)
