"""CPU: tests/geometry_ref.py, the NumPy restatement the GPU tests of the geometry evaluation compare bits with, held to facts that
do not come from it: the stochastic rounding is a rounding and is fair, every sample lies in its triangle, and on two concentric
spheres the metrics are what geometry says, within bounds derived from the construction."""
import numpy as np
import pytest

from tests import geometry_ref as G


def _random_mesh(rng, V=60, F=200, scale=1.0):
    return (rng.standard_normal((V, 3)) * scale).astype(np.float32), rng.integers(0, V, (F, 3)).astype(np.int32)


def test_hash_is_the_stated_one():
    """mix() by hand for two inputs, in Python integers"""
    def mix(x):
        x ^= x >> 16; x = x * 0x7feb352d & 0xFFFFFFFF; x ^= x >> 15; x = x * 0x846ca68b & 0xFFFFFFFF; x ^= x >> 16
        return x
    xs = [0, 1, 2, 12345, 0xFFFFFFFF, 0x80000000]
    assert [int(v) for v in G.mix(np.asarray(xs, np.uint32))] == [mix(x) for x in xs]
    assert [int(v) for v in G.base(np.asarray(xs, np.uint32), 7)] == [mix(mix(x) ^ 7) for x in xs]
    u = G.u24(np.asarray([0, 0xFF, 0x100, 0xFFFFFFFF], np.uint32))
    assert u.dtype == np.float32 and list(u) == [0.0, 0.0, 2.0 ** -24, 1.0 - 2.0 ** -24]


def test_every_count_is_floor_or_floor_plus_one():
    rng = np.random.default_rng(1)
    v, f = _random_mesh(rng)
    for density in (0.3, 7.0, 150.0):
        t = G.face_t(v, f, density).astype(np.float64)
        n = G.face_counts(v, f, density, seed=3)
        assert ((n == np.floor(t)) | (n == np.floor(t) + 1)).all()
        assert (n[t == np.floor(t)] == t[t == np.floor(t)]).all()        # an integer t is never rounded up


@pytest.mark.parametrize("seed", [0, 1, 2, 0xDEADBEEF])
def test_round_up_is_fair(seed):
    """65,536 equal faces with fractional part 0.5: the number rounded up is binomial(65536, 1/2), sd = 128; within 5 sd"""
    F = 65536
    n = G.counts_of_t(np.full(F, 2.5, np.float32), seed)
    up = int((n == 3).sum())
    print("rounded up:", up, "of", F, "seed", seed)
    assert set(np.unique(n)) <= {2, 3} and abs(up - F // 2) <= 640


def test_every_sample_lies_in_its_triangle():
    rng = np.random.default_rng(2)
    v, f = _random_mesh(rng, V=40, F=120)
    p, face, n = G.sample_surface(v, f, 6.0, seed=11)
    assert p.shape[0] == n.sum() > 500 and (np.diff(face) >= 0).all() and (np.bincount(face, minlength=f.shape[0]) == n).all()
    a, b, c = (v[f[face, i]].astype(np.float64) for i in range(3))
    # barycentric coordinates by least squares in float64
    E = np.stack([b - a, c - a], axis=2)                                  # [S, 3, 2]
    rhs = (p.astype(np.float64) - a)[:, :, None]
    w = np.linalg.solve(E.transpose(0, 2, 1) @ E, E.transpose(0, 2, 1) @ rhs)[:, :, 0]
    resid = np.linalg.norm((E @ w[:, :, None])[:, :, 0] - rhs[:, :, 0], axis=1)
    size = np.maximum(np.abs(a).max(1), np.maximum(np.abs(b).max(1), np.abs(c).max(1)))
    # p is formed by four fp32 roundings of values no larger than 3 * size: 8 ulp of that is a generous cover; the weights are
    # held to the same figure relative to the shortest altitude-free scale of the triangle, its edge lengths
    eps = 8 * 2.0 ** -23
    assert (resid <= eps * 3 * size).all()
    edge = np.minimum(np.linalg.norm(b - a, axis=1), np.linalg.norm(c - a, axis=1))
    sin = np.linalg.norm(np.cross(b - a, c - a), axis=1) / (np.linalg.norm(b - a, axis=1) * np.linalg.norm(c - a, axis=1))
    tol = eps * 3 * size / (edge * sin)                                    # a displacement of eps * 3 size moves a weight by this
    assert (w[:, 0] >= -tol).all() and (w[:, 1] >= -tol).all() and (w.sum(1) <= 1 + 2 * tol).all()


def test_degenerate_faces_get_no_sample():
    v = np.asarray([[0, 0, 0], [1, 0, 0], [2, 0, 0], [0, 1, 0], [np.nan, 0, 0], [np.inf, 1, 1]], np.float32)
    f = np.asarray([[0, 1, 2], [0, 0, 3], [0, 1, 4], [0, 3, 5], [0, 1, 3]], np.int32)
    n = G.face_counts(v, f, 1000.0)
    assert list(n[:4]) == [0, 0, 0, 0] and n[4] in (500, 501)


def test_nearest_breaks_ties_by_index_and_skips_bad_queries():
    x = np.asarray([[1, 0, 0], [0, 0, 0], [0, 0, 0], [-1, 0, 0]], np.float32)
    q = np.asarray([[0, 0, 0], [0, 5, 0], [np.nan, 0, 0], [1e30, 0, 0]], np.float32)
    idx, d2 = G.nearest(q, x)
    assert list(idx) == [1, 1, -1, 0] and d2[0] == 0 and d2[1] == 25 and d2[2] == G.FLT_MAX and np.isinf(d2[3])
    idx, d2 = G.nearest(q, np.zeros((0, 3), np.float32))
    assert (idx == -1).all() and (d2 == G.FLT_MAX).all()


# ---- two concentric spheres
R, DELTA, SUBDIV, NREF = 1.0, 0.05, 3, 4000


@pytest.fixture(scope="module")
def spheres():
    v, f, edge = G.icosphere(R + DELTA, SUBDIV)
    ref, spacing = G.fibonacci_sphere(R, NREF)
    sag = G.icosphere_sag(R + DELTA, edge)
    return v, f, ref, sag, spacing


def sphere_bounds(sag, spacing):
    """(lowest, highest) distance a sample of the icosphere can have to its nearest lattice point. A sample has norm in
    [R + DELTA - sag, R + DELTA]; every lattice point has norm R, so the distance is at least norm - R; the sample's radial
    projection onto the lattice's sphere is norm - R away and has a lattice point within `spacing`. fp32 rounding of vertices,
    samples and lattice points moves each by a few ulp of 1: 1e-6 covers them."""
    return DELTA - sag - 1e-6, DELTA + spacing + 1e-6


def test_fibonacci_spacing_covers_the_sphere(spheres):
    _, _, ref, _, spacing = spheres
    rng = np.random.default_rng(5)
    p = rng.standard_normal((20000, 3))
    p = (p / np.linalg.norm(p, axis=1, keepdims=True) * R).astype(np.float32)
    p = np.concatenate([p, np.asarray([[0, 0, R], [0, 0, -R]], np.float32)])          # the poles, where the lattice is thinnest
    d = np.sqrt(G.nearest(p, ref)[1].astype(np.float64))
    print("largest distance to the lattice:", d.max(), "stated covering radius:", spacing)
    assert d.max() <= spacing


def test_sphere_against_sphere(spheres):
    v, f, ref, sag, spacing = spheres
    lo, hi = sphere_bounds(sag, spacing)
    assert sag < DELTA / 2 and spacing < 3 * DELTA                                   # the construction resolves the offset
    p, _, _ = G.sample_surface(v, f, 400.0, seed=1)
    m = G.geometry_metrics(p, ref, thresholds=(lo * 0.999, hi * 1.001))
    print("accuracy", m["accuracy"], "completeness", m["completeness"], "bounds", lo, hi, "samples", p.shape[0])
    assert abs(m["accuracy"] - DELTA) <= sag + spacing + 1e-6
    assert lo <= m["accuracy"] <= hi
    assert m["precision"][lo * 0.999] == 0.0 and m["precision"][hi * 1.001] == 1.0
    assert m["n_accuracy"] == p.shape[0] and m["n_completeness"] == ref.shape[0]
    assert m["chamfer"] == 0.5 * (m["accuracy"] + m["completeness"])


def test_metrics_of_empty_selection():
    rng = np.random.default_rng(3)
    a, b = rng.standard_normal((50, 3)).astype(np.float32), rng.standard_normal((40, 3)).astype(np.float32)
    m = G.geometry_metrics(a, b, thresholds=(0.5,), max_dist=-1.0)
    assert np.isnan(m["accuracy"]) and np.isnan(m["completeness"]) and m["fscore"][0.5] == 0.0 and m["n_accuracy"] == 0
    m = G.geometry_metrics(a, a, thresholds=(0.5,))
    assert m["accuracy"] == 0 and m["completeness"] == 0 and m["fscore"][0.5] == 1.0
