"""CPU: the 3-NN entry points of the C ABI are exported with prototypes, validate their arguments without touching the
device, and size a workspace that grows with P."""
import pytest


@pytest.fixture(scope="module")
def L():
    from c3dgs_amd import build, _lib
    build.build()
    return _lib.lib()


def test_knn_symbols_exported_with_prototypes(L):
    from c3dgs_amd import _lib
    for name in ("c3dgs_knn_workspace_bytes", "c3dgs_knn_mean_dist2"):
        assert hasattr(L, name)
        assert name in _lib.PROTOTYPES
    assert L.c3dgs_abi_version() == 4


def test_knn_validation_codes(L):
    assert L.c3dgs_knn_mean_dist2(0, None, None, None, None) == 0          # P == 0: no pointer is touched
    assert L.c3dgs_knn_mean_dist2(-1, None, None, None, None) == 1
    assert b"P must be >= 0" in L.c3dgs_last_error()
    assert L.c3dgs_knn_mean_dist2(5, None, None, None, None) == 1
    assert b"bad arguments" in L.c3dgs_last_error()
    assert L.c3dgs_knn_mean_dist2(5, 16, None, 16, None) == 1             # any NULL among xyz / out / workspace
    assert L.c3dgs_knn_mean_dist2(5, 16, 16, None, None) == 1


def test_knn_workspace_monotone(L):
    sizes = [L.c3dgs_knn_workspace_bytes(P) for P in (0, 1, 2, 31, 32, 33, 1000, 4097, 65536, 1_000_000, 3_000_000)]
    assert all(s > 0 for s in sizes)
    assert sizes == sorted(sizes)
    assert sizes[-1] >= 3_000_000 * (8 + 8 + 4 + 4 + 16)                      # codes x2, ids x2, sorted float4 points
