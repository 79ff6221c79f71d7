"""CPU: the numpy 3-NN restatement (tests/knn_ref.py) the GPU tests compare against, checked against a plain loop and
against an independent k-d tree search."""
import numpy as np
import pytest

from tests import knn_ref


@pytest.mark.parametrize("P", [1, 2, 3, 4, 5, 13, 50])
def test_ref_matches_python_loop(P):
    g = np.random.default_rng(P)
    x = (g.normal(size=(P, 3)) * [1.0, 3.0, 0.2]).astype(np.float32)
    if P >= 5:
        x[1] = x[0]                                        # a duplicate contributes a 0
        x[3, 2] = x[2, 2]
    np.testing.assert_array_equal(knn_ref.mean_dist2(x, chunk=7).view(np.uint32), knn_ref.mean_dist2_loop(x).view(np.uint32))


def test_ref_small_clouds_use_flt_max():
    assert np.isinf(knn_ref.mean_dist2(np.zeros((1, 3), np.float32))[0])
    assert np.isinf(knn_ref.mean_dist2(np.array([[0, 0, 0], [1, 0, 0]], np.float32))).all()
    three = knn_ref.mean_dist2(np.array([[0, 0, 0], [1, 0, 0], [0, 2, 0]], np.float32))
    exp = (np.float32(1.0) + np.float32(4.0) + knn_ref.FLT_MAX) / np.float32(3.0)
    assert three[0] == exp and np.isfinite(three).all() and three.min() > 1e38


def test_ref_matches_kdtree():
    spatial = pytest.importorskip("scipy.spatial")
    g = np.random.default_rng(7)
    x = (g.normal(size=(3000, 3)) * [2.0, 0.5, 1.0]).astype(np.float32)
    x[100:130] = x[0]
    # float64 neighbours from the tree (4 = self + 3; ties among duplicates are all distance 0), then fp32 distances
    _, nb = spatial.cKDTree(x.astype(np.float64)).query(x.astype(np.float64), k=4)
    d = np.empty((x.shape[0], 4), np.float32)
    for c in range(4):
        diff = x[nb[:, c]] - x
        d[:, c] = (diff[:, 0] * diff[:, 0] + diff[:, 1] * diff[:, 1]) + diff[:, 2] * diff[:, 2]
    own = nb == np.arange(x.shape[0])[:, None]
    dup = (~own).all(axis=1)                               # self not returned: 4 zero-distance duplicates tied with it
    d[own] = np.inf
    d3 = np.sort(d, axis=1)[:, :3]
    d3[dup] = 0.0
    np.testing.assert_array_equal(knn_ref.mean_dist2(x).view(np.uint32), knn_ref.combine(d3).view(np.uint32))
