"""-m gpu: csrc/nn_query.hip against the brute force of tests/geometry_ref.py. idx equal and d2 bit-equal in every case, for both
query orders (Morton-sorted and the caller's): the contract fixes the result, the order only changes which nodes a wave shares."""
import ctypes as C

import numpy as np
import pytest
import torch

from tests import geometry_ref as G
from tests import poison

pytestmark = pytest.mark.gpu


def _gpu(a, dtype=torch.float32):
    return torch.as_tensor(np.ascontiguousarray(a), dtype=dtype, device="cuda")


def check(x, q, what="", index=None):
    """both query orders against the restatement; -> the index"""
    from c3dgs_amd import knn
    index = knn.NearestIndex(_gpu(x)) if index is None else index
    ri, rd = G.nearest(q, x)
    for sort in (False, True):
        idx, d2 = index.query(_gpu(q), sort=sort)
        idx, d2 = idx.cpu().numpy(), d2.cpu().numpy()
        assert idx.dtype == np.int32 and d2.dtype == np.float32 and idx.shape == d2.shape == (len(q),)
        bad = np.nonzero((idx != ri) | (d2.view(np.uint32) != rd.view(np.uint32)))[0]
        assert bad.size == 0, (f"{what} sort={sort}: {bad.size} of {len(q)} queries differ, the first is query {bad[0]}: "
                               f"got ({idx[bad[0]]}, {d2[bad[0]]!r}), expected ({ri[bad[0]]}, {rd[bad[0]]!r})")
    return index


def test_random(hip):
    rng = np.random.default_rng(0)
    x = rng.standard_normal((5000, 3)).astype(np.float32)
    q = (rng.standard_normal((3000, 3)) * 1.3).astype(np.float32)
    check(x, q, "random")


@pytest.mark.parametrize("P", [1, 31, 32, 33, 167])
@pytest.mark.parametrize("Q", [1, 63, 257])
def test_small_trees_and_ragged_grids(hip, P, Q):
    rng = np.random.default_rng(P * 1000 + Q)
    check(rng.uniform(-1, 1, (P, 3)).astype(np.float32), rng.uniform(-1.5, 1.5, (Q, 3)).astype(np.float32), f"P={P} Q={Q}")


def test_queries_far_outside_the_box(hip):
    rng = np.random.default_rng(1)
    x = rng.uniform(-1, 1, (700, 3)).astype(np.float32)
    q = (rng.standard_normal((200, 3)) * np.float32(1e4)).astype(np.float32)
    q[:6] = np.asarray([[1e30, 0, 0], [-1e30, 1e30, 0], [0, 0, 3e19], [1e19, 1e19, 1e19], [1e6, -1e6, 0], [2, 2, 2]], np.float32)
    check(x, q, "far outside")
    from c3dgs_amd import knn
    idx, d2 = knn.nearest(_gpu(q[:1]), _gpu(x))
    assert int(idx[0]) == 0 and np.isinf(float(d2[0]))                   # every distance overflows: +inf, the lowest index


def test_duplicates_lowest_index_wins_at_zero(hip):
    rng = np.random.default_rng(2)
    x = rng.uniform(-1, 1, (300, 3)).astype(np.float32)
    x = np.concatenate([x, x[::-1], x[:100]])                             # every point two or three times, far apart in index
    x = x[rng.permutation(x.shape[0])]
    q = x[rng.integers(0, x.shape[0], 400)]
    index = check(x, q, "duplicates")
    idx, d2 = index.query(_gpu(q))
    assert (d2 == 0).all()


def test_lattice_eight_way_ties(hip):
    g = np.arange(6, dtype=np.float32)
    x = np.stack(np.meshgrid(g, g, g, indexing="ij"), -1).reshape(-1, 3)
    x = x[np.random.default_rng(3).permutation(x.shape[0])]
    c = np.arange(5, dtype=np.float32) + np.float32(0.5)
    q = np.stack(np.meshgrid(c, c, c, indexing="ij"), -1).reshape(-1, 3)
    ri, rd = G.nearest(q, x)
    assert (rd == np.float32(0.75)).all()                                  # the case is what it claims: exact ties
    check(x, q, "lattice")


def test_coincident_planar_and_clustered_references(hip):
    rng = np.random.default_rng(4)
    q = rng.uniform(-2, 2, (300, 3)).astype(np.float32)
    check(np.tile(np.asarray([[0.25, -0.5, 1.0]], np.float32), (200, 1)), q, "coincident")
    plane = rng.uniform(-1, 1, (900, 3)).astype(np.float32)
    plane[:, 2] = np.float32(0.125)
    check(plane, q, "planar")
    centres = rng.uniform(-1, 1, (12, 3))
    clusters = (centres[:, None, :] + rng.standard_normal((12, 64, 3)) * 1e-3).reshape(-1, 3).astype(np.float32)
    check(clusters, np.concatenate([q, clusters[::7] + np.float32(1e-4)]), "clusters")


def test_permuting_the_queries_permutes_the_results(hip):
    from c3dgs_amd import knn
    rng = np.random.default_rng(5)
    x, q = rng.standard_normal((2000, 3)).astype(np.float32), rng.standard_normal((1000, 3)).astype(np.float32)
    index = knn.NearestIndex(_gpu(x))
    perm = rng.permutation(1000)
    for sort in (False, True):
        i0, d0 = index.query(_gpu(q), sort=sort)
        i1, d1 = index.query(_gpu(q[perm]), sort=sort)
        assert torch.equal(i0[_gpu(perm, torch.int64)], i1) and torch.equal(d0[_gpu(perm, torch.int64)], d1)


def test_an_index_serves_many_queries_and_is_not_disturbed_by_another(hip):
    from c3dgs_amd import knn
    rng = np.random.default_rng(6)
    x, y = rng.standard_normal((1500, 3)).astype(np.float32), rng.uniform(5, 6, (800, 3)).astype(np.float32)
    q = rng.standard_normal((700, 3)).astype(np.float32)
    first = check(x, q, "first")
    a = first.query(_gpu(q))
    b = first.query(_gpu(q))
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])
    second = check(y, q, "second")
    check(x, q, "first, after the second was built and queried", index=first)
    check(y, q[::-1].copy(), "second again", index=second)


def test_nan_query_through_the_c_abi(hip):
    """a query with a non-finite coordinate gives (-1, FLT_MAX); the 63 other lanes of its wave are still right"""
    from c3dgs_amd import _lib
    L = _lib.lib()
    rng = np.random.default_rng(7)
    x, q = rng.standard_normal((1000, 3)).astype(np.float32), rng.standard_normal((200, 3)).astype(np.float32)
    q[5, 1], q[70, 0], q[71, 2], q[199, 0] = np.nan, np.inf, -np.inf, np.nan
    ri, rd = G.nearest(q, x)
    assert list(ri[[5, 70, 71, 199]]) == [-1] * 4
    xs, qs = _gpu(x), _gpu(q)
    for byte in poison.POISON_BYTES:
        index = poison.buffer(L.c3dgs_nn_index_bytes(1000), byte)
        assert L.c3dgs_nn_build(1000, xs.data_ptr(), index.ptr, None) == 0, L.c3dgs_last_error()
        for sort in (0, 1):
            ws = poison.buffer(L.c3dgs_nn_query_workspace_bytes(200), byte)
            idx, d2, leaves = poison.buffer(800, byte), poison.buffer(800, byte), poison.buffer(800, byte)
            assert L.c3dgs_nn_query(1000, index.ptr, 200, qs.data_ptr(), sort, idx.ptr, d2.ptr, leaves.ptr, ws.ptr, None) == 0, \
                L.c3dgs_last_error()
            torch.cuda.synchronize()
            assert (idx.payload.view(torch.int32).cpu().numpy() == ri).all()
            assert (d2.payload.view(torch.int32).cpu().numpy() == rd.view(np.int32)).all()
            n = leaves.payload.view(torch.int32).cpu().numpy()
            assert (n[ri < 0] == 0).all() and (n[ri >= 0] >= 1).all() and n.max() <= 32          # 1000 points: 32 leaves
            for g in (ws, idx, d2, leaves, index):
                g.check()


def test_no_reference_points(hip):
    from c3dgs_amd import knn
    q = _gpu(np.random.default_rng(8).standard_normal((70, 3)))
    for sort in (False, True):
        idx, d2 = knn.NearestIndex(torch.zeros((0, 3), device="cuda")).query(q, sort=sort)
        assert (idx == -1).all() and (d2 == float(G.FLT_MAX)).all()
    idx, d2 = knn.nearest(torch.zeros((0, 3), device="cuda"), q)
    assert idx.shape == d2.shape == (0,)
    with pytest.raises(RuntimeError, match="finite"):
        knn.NearestIndex(torch.full((4, 3), float("nan"), device="cuda"))
