"""-m gpu: c3dgs_amd.knn.knn3 (the index-returning variant of csrc/knn.hip's search) against the brute force of
tests/densify_initial_ref.py.

Distances are bit-equal always. Indices are equal wherever the third distance is non-zero: the contract is the three smallest
(d2, index) pairs, so ties go to the lowest index whatever order the tree is walked in. Where it is zero (three or more
coincident other points) any three of them may be reported, in ascending index order. distCUDA2 must be what it was: the
mean of knn3's distances, and tests/knn_ref.py's brute force, bit for bit."""
import numpy as np
import pytest
import torch

from tests import densify_initial_ref as ref
from tests import knn_ref

pytestmark = pytest.mark.gpu
DEV = "cuda"


def _uniform(P, seed=0):
    return np.random.default_rng(seed).uniform(-1, 1, (P, 3)).astype(np.float32)


def _lattice():
    g = np.arange(17, dtype=np.float32)
    return np.stack(np.meshgrid(g, g, g, indexing="ij"), -1).reshape(-1, 3)          # six equidistant neighbours inside


def _clusters():
    x = _uniform(3000, 5)
    rng = np.random.default_rng(6)
    rows = rng.permutation(3000)                       # scattered indices: the members of a cluster are far apart by index
    at = 0
    for n in (2, 3, 4, 70):                            # 70 coincident points cross a 32-point leaf and a 64-lane wave
        x[rows[at:at + n]] = x[rows[at]]
        at += n
    return x


def _collinear():
    t = np.random.default_rng(7).uniform(-3, 3, 2000).astype(np.float32)
    return np.stack([t, np.float32(0.5) * t, np.zeros_like(t)], axis=1)


def _shifted_lattice():
    """A lattice whose points are shuffled by index: Morton order and index order disagree, so a search that keeps the first
    candidate it meets among equals, instead of the lowest index, is caught."""
    x = _lattice()[:9 * 17 * 17]
    return x[np.random.default_rng(8).permutation(len(x))]


CLOUDS = {"P1": lambda: _uniform(1), "P2": lambda: _uniform(2), "P3": lambda: _uniform(3), "P4": lambda: _uniform(4),
          "P33": lambda: _uniform(33), "P257": lambda: _uniform(257), "P5000": lambda: _uniform(5000), "lattice": _lattice,
          "lattice_shuffled": _shifted_lattice, "clusters": _clusters, "collinear": _collinear}
_cache = {}


def _case(name):
    """(x, brute-force idx, brute-force d2, knn3 idx, knn3 d2): every reference is computed once and shared."""
    if name not in _cache:
        from c3dgs_amd.knn import knn3
        x = CLOUDS[name]()
        widx, wd2 = ref.knn3_brute(x)
        idx, d2 = knn3(torch.from_numpy(x).to(DEV))
        assert idx.dtype == torch.int32 and d2.dtype == torch.float32 and tuple(idx.shape) == tuple(d2.shape) == (len(x), 3)
        _cache[name] = (x, widx, wd2, idx.cpu().numpy(), d2.cpu().numpy())
    return _cache[name]


@pytest.mark.parametrize("name", list(CLOUDS))
def test_knn3_equals_the_brute_force(name):
    x, widx, wd2, idx, d2 = _case(name)
    assert np.array_equal(d2.view(np.uint32), wd2.view(np.uint32))
    exact = wd2[:, 2] != 0
    bad = np.nonzero((idx != widx).any(axis=1) & exact)[0]
    assert bad.size == 0, (bad[:5], idx[bad[:5]], widx[bad[:5]])
    for i in np.nonzero(~exact)[0]:                       # three or more coincident other points: any three, ascending
        j = idx[i]
        assert j[0] < j[1] < j[2] and i not in j and (j >= 0).all() and (j < len(x)).all()
        assert (x[j] == x[i]).all()
    if name == "clusters":
        assert int((~exact).sum()) == 4 + 70              # the clusters of 4 and of 70; those of 2 and 3 are exact rows
        assert int((wd2[:, 1] == 0).sum()) == 3 + 4 + 70
    if name.startswith("lattice"):
        assert int(((wd2[:, 0] == 1) & (wd2[:, 2] == 1)).sum()) > 1000 and exact.all()
    if len(x) <= 3:
        assert (idx[:, len(x) - 1:] == -1).all() and (d2[:, len(x) - 1:] == ref.FLT_MAX).all()


def test_knn3_empty_and_argument_checks():
    from c3dgs_amd.knn import knn3
    idx, d2 = knn3(torch.zeros(0, 3, device=DEV))
    assert tuple(idx.shape) == (0, 3) and tuple(d2.shape) == (0, 3)
    with pytest.raises(RuntimeError, match="GPU tensor"):
        knn3(torch.zeros(4, 3))
    with pytest.raises(RuntimeError, match="num_points, 3"):
        knn3(torch.zeros(4, 2, device=DEV))
    with pytest.raises(RuntimeError, match="finite"):
        knn3(torch.full((4, 3), float("nan"), device=DEV))


@pytest.mark.parametrize("name", list(CLOUDS))
def test_distCUDA2_is_the_mean_of_knn3_and_unchanged(name):
    from c3dgs_amd.knn import distCUDA2
    x, _, wd2, _, d2 = _case(name)
    got = distCUDA2(torch.from_numpy(x).to(DEV)).cpu().numpy()
    assert np.array_equal(got.view(np.uint32), knn_ref.combine(d2).view(np.uint32))
    assert np.array_equal(got.view(np.uint32), knn_ref.mean_dist2(x).view(np.uint32))
