"""-m gpu: csrc/geometry_metrics.hip and the Python entries on top of it (metrics.geometry_metrics, mesh_metrics,
reference_spacing) against tests/geometry_ref.py: counts equal, fp64 sums within N * 2^-52 relative (the bound of an N-term fp64
sum of exact fp32 inputs, whatever the order), and the two sphere cases within the bounds derived from their construction."""
import math

import numpy as np
import pytest
import torch

from tests import geometry_ref as G
from tests import mesh_ref as mr
from tests.test_geometry_ref_cpu import DELTA, NREF, R, SUBDIV, sphere_bounds

pytestmark = pytest.mark.gpu


def _gpu(a, dtype=torch.float32):
    return torch.as_tensor(np.ascontiguousarray(a), dtype=dtype, device="cuda")


def gpu_reduce(d2, points=None, bounds=None, max_dist=math.inf, thresholds=()):
    from c3dgs_amd import metrics
    out = torch.full((10,), -7.0, dtype=torch.float64, device="cuda")
    flat = None if bounds is None else list(bounds[0]) + list(bounds[1])
    metrics._reduce_direction(_gpu(d2), None if points is None else _gpu(points), flat, max_dist, list(thresholds), out)
    return out.cpu().numpy()


def assert_reduce(d2, what, **kw):
    n, s, below = G.reduce_direction(d2, **kw)
    got = gpu_reduce(d2, **kw)
    T = len(kw.get("thresholds", ()))
    print(f"{what}: count {got[0]:.0f} (ref {n}), sum {got[1]!r} (ref {s!r}), below {got[2:2 + T]} (ref {below})")
    assert got[0] == n and list(got[2:2 + T]) == below, what
    assert (got[2 + T:] == -7.0).all(), "columns past 2 + T are not the kernel's"
    assert got[1] == s or abs(got[1] - s) <= len(d2) * 2.0 ** -52 * abs(s), what
    return got


@pytest.mark.parametrize("N", [0, 1, 255, 2049, 300_001, 2_500_000])
def test_counts_and_sums(hip, N):
    """N = 2049: two workgroups; 300,001: a ragged last one; 2,500,000: past the 1024-workgroup cap, several elements a lane"""
    rng = np.random.default_rng(N)
    d2 = (rng.uniform(0, 2, N) ** 2).astype(np.float32)
    d2[rng.integers(0, max(N, 1), N // 50)] = G.FLT_MAX                       # queries without a neighbour
    pts = rng.uniform(-1, 1, (N, 3)).astype(np.float32)
    taus = (0.25, 0.5, 1.0, 1.0000001, 1.5, 1.9, 2.5, 0.0)
    a = assert_reduce(d2, f"N={N} plain", thresholds=taus[:3])
    assert_reduce(d2, f"N={N} max_dist, 8 thresholds", max_dist=1.25, thresholds=taus)
    assert_reduce(d2, f"N={N} box", points=pts, bounds=((-0.5, -0.25, -1.0), (0.75, 0.5, 0.0)), max_dist=1.7, thresholds=taus[:1])
    b = gpu_reduce(d2, thresholds=taus[:3])
    assert a.tobytes() == b.tobytes()                                          # run to run: the same bits


def test_boundary_values(hip):
    """d == max_dist is counted, d == tau is not below it, p == lo or hi is inside; NaN coordinates and NaN / inf distances"""
    d2 = np.asarray([0.25, 0.25, 1.0, 4.0, np.inf, np.nan, G.FLT_MAX, 0.0, 0.25], np.float32)
    pts = np.asarray([[0, 0, 0], [1, 1, 1], [-1, -1, -1], [0, 0, 0], [0, 0, 0], [0, 0, 0], [0, 0, 0], [np.nan, 0, 0], [1.5, 0, 0]],
                     np.float32)
    got = assert_reduce(d2, "edges", points=pts, bounds=((-1, -1, -1), (1, 1, 1)), max_dist=2.0, thresholds=(0.5, 0.50001, 2.0))
    assert got[0] == 4 and got[1] == 0.5 + 0.5 + 1.0 + 2.0 and list(got[2:5]) == [0, 2, 3]
    got = assert_reduce(d2[[0, 4]], "an infinite distance under max_dist = inf")
    assert got[0] == 2 and np.isinf(got[1])


def test_a_set_against_itself(hip):
    from c3dgs_amd import metrics
    x = _gpu(np.random.default_rng(1).standard_normal((3000, 3)))
    m = metrics.geometry_metrics(x, x, thresholds=(1e-3, 0.1))
    assert m["accuracy"] == 0 and m["completeness"] == 0 and m["chamfer"] == 0
    assert m["n_accuracy"] == m["n_completeness"] == 3000
    assert m["precision"] == {1e-3: 1.0, 0.1: 1.0} and m["recall"] == m["precision"] and m["fscore"] == m["precision"]


def same_metrics(m, r, n_terms):
    assert m["n_accuracy"] == r["n_accuracy"] and m["n_completeness"] == r["n_completeness"]
    for k in ("accuracy", "completeness", "chamfer"):
        if math.isnan(r[k]):
            assert math.isnan(m[k]), k
        else:
            assert abs(m[k] - r[k]) <= (n_terms + 2) * 2.0 ** -52 * abs(r[k]), (k, m[k], r[k])
    for k in ("precision", "recall", "fscore"):
        assert m[k].keys() == r[k].keys()
        for tau in r[k]:
            assert m[k][tau] == r[k][tau] or (math.isnan(m[k][tau]) and math.isnan(r[k][tau])), (k, tau, m[k][tau], r[k][tau])


def test_metrics_are_the_restatement(hip):
    from c3dgs_amd import metrics
    rng = np.random.default_rng(2)
    a = rng.standard_normal((2500, 3)).astype(np.float32)
    b = (a[:1800] + rng.standard_normal((1800, 3)) * 0.05).astype(np.float32)
    taus = (0.02, 0.08, 0.3)
    for kw in (dict(), dict(max_dist=0.2), dict(bounds=((-1.0, -0.5, -2.0), (0.5, 1.0, 2.0))),
               dict(max_dist=0.5, bounds=((-0.3, -0.3, -0.3), (0.3, 0.3, 0.3)))):
        r = G.geometry_metrics(a, b, thresholds=taus, **kw)
        m = metrics.geometry_metrics(_gpu(a), _gpu(b), thresholds=taus, **kw)
        print(kw, {k: m[k] for k in ("accuracy", "completeness", "n_accuracy", "n_completeness")}, m["fscore"])
        assert 0 < r["n_accuracy"] <= 2500 and (not kw or r["n_accuracy"] < 2500)    # the filters exclude something
        same_metrics(m, r, 2500)


def test_empty_selections(hip):
    from c3dgs_amd import metrics
    rng = np.random.default_rng(3)
    a, b = _gpu(rng.standard_normal((400, 3))), _gpu(rng.standard_normal((300, 3)) + 4.0)
    for m in (metrics.geometry_metrics(a, b, thresholds=(0.5,), max_dist=1e-9),
              metrics.geometry_metrics(a, b, thresholds=(0.5,), bounds=((50, 50, 50), (51, 51, 51))),
              metrics.geometry_metrics(a, a[:0], thresholds=(0.5,)),
              metrics.geometry_metrics(a[:0], a[:0], thresholds=(0.5,))):
        assert math.isnan(m["accuracy"]) and math.isnan(m["completeness"]) and math.isnan(m["chamfer"])
        assert m["n_accuracy"] == m["n_completeness"] == 0 and m["fscore"][0.5] == 0.0
        assert math.isnan(m["precision"][0.5]) and math.isnan(m["recall"][0.5])
    m = metrics.geometry_metrics(a, b, thresholds=(0.5,), bounds=((-9, -9, -9), (2, 2, 2)))     # only one side is empty
    assert m["n_accuracy"] > 0 and m["n_completeness"] < 300 and m["fscore"][0.5] == 0.0
    with pytest.raises(ValueError, match="thresholds"):
        metrics.geometry_metrics(a, b, thresholds=range(9))


def test_sphere_against_sphere_end_to_end(hip):
    """the sphere case of tests/test_geometry_ref_cpu.py through mesh_metrics, within the same derived bounds"""
    from c3dgs_amd import metrics
    v, f, edge = G.icosphere(R + DELTA, SUBDIV)
    ref, spacing = G.fibonacci_sphere(R, NREF)
    sag = G.icosphere_sag(R + DELTA, edge)
    lo, hi = sphere_bounds(sag, spacing)
    taus = (lo * 0.999, hi * 1.001, DELTA + sag + spacing + 1e-6)
    m = metrics.mesh_metrics(_gpu(v), _gpu(f, torch.int32), _gpu(ref), 400.0, seed=1, thresholds=taus)
    print("accuracy", m["accuracy"], "completeness", m["completeness"], "bounds", lo, hi, "samples", m["samples"])
    assert abs(m["accuracy"] - DELTA) <= sag + spacing + 1e-6 and lo <= m["accuracy"] <= hi
    assert m["precision"][taus[0]] == 0.0 and m["precision"][taus[1]] == 1.0 and m["precision"][taus[2]] == 1.0
    assert m["samples"] == m["n_accuracy"] == G.face_counts(v, f, 400.0, 1).sum() and m["n_completeness"] == NREF
    same_metrics(m, G.geometry_metrics(G.sample_surface(v, f, 400.0, 1)[0], ref, thresholds=taus), m["samples"])


def test_extracted_sphere_against_points_on_it(hip):
    """extract_mesh's analytic sphere (tests/mesh_ref.py: radius 0.3 about (0.5, 0.5, 0.5) on a 33^3 lattice) against the Fibonacci
    lattice on that sphere. The bar is the feature request's: the linear-interpolation bound of tests/test_mesh_ref_cpu.py plus the
    lattice's covering radius. That bound holds for VERTICES; a sample inside a face lies up to about edge^2 / (6 R) (0.002 here)
    further in, a term the bar leaves out on purpose: it is a bar on the MEAN, and the covering radius (0.015) is the WORST distance
    from a point of the sphere to the lattice, several times the typical one. The figures are printed."""
    from c3dgs_amd import mesh, metrics
    radius, n = 0.3, 33
    tsdf, weight, origin, h = mr.sphere_lattice(n, radius)
    vol = mesh.TSDFVolume(origin, h, (n, n, n), 1.0, "cuda", color=False)
    vol.tsdf.copy_(torch.from_numpy(tsdf))
    vol.weight.copy_(torch.from_numpy(weight))
    vertices, _, faces = vol.extract()
    ref, spacing = G.fibonacci_sphere(radius, 20000)
    ref = _gpu(ref + np.float32(0.5))
    m = metrics.mesh_metrics(vertices, faces, ref, 1.0 / spacing ** 2 * 16, thresholds=(mr.radial_error_bound(h, radius) + spacing,))
    print("accuracy", m["accuracy"], "bound", mr.radial_error_bound(h, radius) + spacing, "samples", m["samples"],
          "completeness", m["completeness"])
    assert m["samples"] > 1000
    assert m["accuracy"] <= mr.radial_error_bound(h, radius) + spacing
    assert metrics.reference_spacing(ref) <= spacing                       # a lattice point's cell has side spacing / 2
    assert metrics.reference_spacing(ref) > 0
