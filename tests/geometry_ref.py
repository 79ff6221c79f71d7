"""NumPy restatement of the geometry-evaluation contracts of include/c3dgs_hip.h ("geometry evaluation"):

    nearest(queries, xyz)                   the lexicographically smallest (d, j) per query; d in fp32 as tests/knn_ref.py forms it
    face_counts / sample_surface            the surface sampler: hash, stochastic rounding of area * density, positions
    reduce_direction / geometry_metrics     count, float64 sum of d = sqrt_rn(d2) and counts below thresholds; the derived metrics

Every fp32 operation is done on float32 arrays, one NumPy call per rounding, in the kernels' order. Also the two analytic spheres
(icosphere, Fibonacci lattice) that the sphere checks use, with the bounds derived from their construction."""
import numpy as np

FLT_MAX = np.float32(np.finfo(np.float32).max)
F32 = np.float32


# ---- nearest neighbour
def nearest(queries, xyz, chunk=512):
    """-> (idx int32 [Q], d2 float32 [Q]); P == 0 or a non-finite query: (-1, FLT_MAX)"""
    q = np.ascontiguousarray(queries, dtype=np.float32).reshape(-1, 3)
    x = np.ascontiguousarray(xyz, dtype=np.float32).reshape(-1, 3)
    Q, P = q.shape[0], x.shape[0]
    idx, d2 = np.full(Q, -1, np.int32), np.full(Q, FLT_MAX, np.float32)
    if P == 0:
        return idx, d2
    for a in range(0, Q, chunk):
        qq = q[a:a + chunk]
        with np.errstate(over="ignore", invalid="ignore"):
            dx = x[None, :, 0] - qq[:, None, 0]
            d = dx * dx
            dy = x[None, :, 1] - qq[:, None, 1]
            d = d + dy * dy
            dz = x[None, :, 2] - qq[:, None, 2]
            d = d + dz * dz
        j = np.argmin(d, axis=1)                          # the first occurrence of the minimum: the lowest index
        ok = np.isfinite(qq).all(axis=1)
        idx[a:a + chunk] = np.where(ok, j, -1)
        d2[a:a + chunk] = np.where(ok, d[np.arange(qq.shape[0]), j], FLT_MAX)
    return idx, d2


# ---- the sampler
def mix(x):
    x = np.asarray(x, dtype=np.uint32).copy()
    x ^= x >> np.uint32(16)
    x *= np.uint32(0x7feb352d)
    x ^= x >> np.uint32(15)
    x *= np.uint32(0x846ca68b)
    x ^= x >> np.uint32(16)
    return x


def base(f, seed):
    return mix(mix(f) ^ np.uint32(seed & 0xFFFFFFFF))


def u24(x):
    return (np.asarray(x, np.uint32) >> np.uint32(8)).astype(np.float32) * F32(2.0 ** -24)


def face_t(vertices, faces, density):
    """t = area * density per face in fp32 (NaN / inf where a vertex is non-finite or the area overflows)"""
    v = np.ascontiguousarray(vertices, dtype=np.float32)
    f = np.asarray(faces, dtype=np.int64).reshape(-1, 3)
    a, b, c = v[f[:, 0]], v[f[:, 1]], v[f[:, 2]]
    with np.errstate(over="ignore", invalid="ignore"):
        u, w = b - a, c - a
        cx = u[:, 1] * w[:, 2] - u[:, 2] * w[:, 1]
        cy = u[:, 2] * w[:, 0] - u[:, 0] * w[:, 2]
        cz = u[:, 0] * w[:, 1] - u[:, 1] * w[:, 0]
        area = F32(0.5) * np.sqrt(cx * cx + cy * cy + cz * cz)
        return area * F32(density)


def counts_of_t(t, seed, first_face=0):
    """n_f for the faces first_face, first_face + 1, ... with the given t (fp32); every t must be below 2^24 or non-finite"""
    t = np.asarray(t, np.float32)
    fin = np.isfinite(t)
    assert not (fin & (t >= F32(2.0 ** 24))).any(), "a face with t >= 2^24: the count call refuses it"
    ts = np.where(fin, t, F32(0))
    fl = np.floor(ts)
    f = np.arange(first_face, first_face + t.shape[0], dtype=np.uint32)
    up = u24(base(f, seed)) < (ts - fl)
    return np.where(fin, fl.astype(np.int64) + up, 0).astype(np.int64)


def face_counts(vertices, faces, density, seed=0):
    return counts_of_t(face_t(vertices, faces, density), seed)


def sample_surface(vertices, faces, density, seed=0):
    """-> (points float32 [S,3], face int32 [S], counts int64 [F])"""
    v = np.ascontiguousarray(vertices, dtype=np.float32)
    f = np.asarray(faces, dtype=np.int64).reshape(-1, 3)
    n = face_counts(v, f, density, seed)
    face = np.repeat(np.arange(f.shape[0], dtype=np.int64), n)
    start = np.cumsum(n) - n
    k = (np.arange(face.shape[0], dtype=np.int64) - start[face]).astype(np.uint32)
    h = base(face.astype(np.uint32), seed)
    u1 = u24(mix(h + np.uint32(2) * k + np.uint32(1)))
    u2 = u24(mix(h + np.uint32(2) * k + np.uint32(2)))
    flip = (u1 + u2) > F32(1)
    u1, u2 = np.where(flip, F32(1) - u1, u1), np.where(flip, F32(1) - u2, u2)
    a, b, c = v[f[face, 0]], v[f[face, 1]], v[f[face, 2]]
    p = (a + u1[:, None] * (b - a)) + u2[:, None] * (c - a)
    return p.astype(np.float32), face.astype(np.int32), n


# ---- the reduction
def reduce_direction(d2, points=None, bounds=None, max_dist=np.inf, thresholds=()):
    """-> (count, float64 sum of d, [counts below each threshold])"""
    d2 = np.asarray(d2, np.float32)
    with np.errstate(invalid="ignore"):
        d = np.sqrt(d2)
        keep = (d2 != FLT_MAX) & (d <= F32(max_dist))
        if bounds is not None:
            p = np.asarray(points, np.float32)
            lo, hi = np.asarray(bounds[0], np.float32), np.asarray(bounds[1], np.float32)
            keep &= ((p >= lo) & (p <= hi)).all(axis=1)
    below = [int((keep & (d < F32(t))).sum()) for t in thresholds]
    return int(keep.sum()), float(d[keep].astype(np.float64).sum()), below


def geometry_metrics(points, reference, thresholds=(), max_dist=np.inf, bounds=None):
    points, reference = np.asarray(points, np.float32).reshape(-1, 3), np.asarray(reference, np.float32).reshape(-1, 3)
    na, sa, ba = reduce_direction(nearest(points, reference)[1], points, bounds, max_dist, thresholds)
    nc, sc, bc = reduce_direction(nearest(reference, points)[1], reference, bounds, max_dist, thresholds)
    nan = float("nan")
    out = {"accuracy": sa / na if na else nan, "completeness": sc / nc if nc else nan, "n_accuracy": na, "n_completeness": nc,
           "precision": {}, "recall": {}, "fscore": {}, "sums": (sa, sc)}
    out["chamfer"] = 0.5 * (out["accuracy"] + out["completeness"])
    for t, tau in enumerate(float(t) for t in thresholds):
        p, r = (ba[t] / na if na else nan), (bc[t] / nc if nc else nan)
        out["precision"][tau], out["recall"][tau] = p, r
        out["fscore"][tau] = 2.0 * p * r / (p + r) if p + r > 0 else 0.0
    return out


# ---- two spheres
def icosphere(radius, subdivisions):
    """-> (vertices float32 [V,3] ON the sphere of `radius` (up to fp32 rounding), faces int32 [F,3], edge): a subdivided
    icosahedron; `edge`: the longest edge, measured (float64)."""
    g = (1.0 + 5.0 ** 0.5) / 2.0
    v = [(-1, g, 0), (1, g, 0), (-1, -g, 0), (1, -g, 0), (0, -1, g), (0, 1, g), (0, -1, -g), (0, 1, -g), (g, 0, -1), (g, 0, 1),
         (-g, 0, -1), (-g, 0, 1)]
    v = [np.asarray(p, np.float64) / np.linalg.norm(p) for p in v]
    f = [(0, 11, 5), (0, 5, 1), (0, 1, 7), (0, 7, 10), (0, 10, 11), (1, 5, 9), (5, 11, 4), (11, 10, 2), (10, 7, 6), (7, 1, 8),
         (3, 9, 4), (3, 4, 2), (3, 2, 6), (3, 6, 8), (3, 8, 9), (4, 9, 5), (2, 4, 11), (6, 2, 10), (8, 6, 7), (9, 8, 1)]
    for _ in range(subdivisions):
        cache, nf = {}, []

        def mid(a, b):
            key = (min(a, b), max(a, b))
            if key not in cache:
                m = v[a] + v[b]
                v.append(m / np.linalg.norm(m))
                cache[key] = len(v) - 1
            return cache[key]

        for a, b, c in f:
            ab, bc, ca = mid(a, b), mid(b, c), mid(c, a)
            nf += [(a, ab, ca), (b, bc, ab), (c, ca, bc), (ab, bc, ca)]
        f = nf
    v = (np.asarray(v) * radius).astype(np.float32)
    f = np.asarray(f, np.int32)
    vd = v.astype(np.float64)
    edge = max(np.linalg.norm(vd[f[:, i]] - vd[f[:, (i + 1) % 3]], axis=1).max() for i in range(3))
    return v, f, float(edge)


def icosphere_sag(radius, edge):
    """How far below the sphere of `radius` a point of a triangle with corners ON it and edges <= `edge` can lie. For weights
    w_i >= 0 that sum to 1, |sum w_i v_i|^2 = sum w_i |v_i|^2 - sum_{i<j} w_i w_j |v_i - v_j|^2 >= radius^2 - edge^2 / 3
    (sum_{i<j} w_i w_j <= 1/3), so the norm of the point is at least sqrt(radius^2 - edge^2 / 3)."""
    return radius - (radius * radius - edge * edge / 3.0) ** 0.5


def fibonacci_sphere(radius, n):
    """-> (points float32 [n,3], spacing): the Fibonacci lattice z_i = 1 - (2 i + 1) / n, phi_i = i * golden angle, and a covering
    radius: no point of the sphere is farther (chord length) than `spacing` from a lattice point. The lattice gives every point
    an equal-area cell of 4 pi R^2 / n; `spacing` is TWICE the side of a square of that area, 2 sqrt(4 pi / n) R. That a cell of a
    golden-angle lattice is never more than twice as long as a square one is the three-gap property of the golden ratio;
    tests/test_geometry_ref_cpu.py holds the figure to a dense sampling of the sphere instead of trusting the argument."""
    i = np.arange(n, dtype=np.float64) + 0.5
    z = 1.0 - 2.0 * i / n
    r = np.sqrt(1.0 - z * z)
    phi = np.pi * (3.0 - 5.0 ** 0.5) * i
    p = np.stack([r * np.cos(phi), r * np.sin(phi), z], 1) * radius
    return p.astype(np.float32), float(2.0 * (4.0 * np.pi * radius * radius / n) ** 0.5)
