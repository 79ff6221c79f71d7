"""CPU: the entry points of the initial densification (c3dgs_knn_neighbours, c3dgs_ray_fill_plan, c3dgs_ray_fill_xyz) are
exported with prototypes, reject bad arguments with C3DGS_E_INVALID before any launch, and size workspaces that grow with
the problem. Pointers here are never dereferenced: every call returns before it touches the device."""
import ctypes as C

import pytest

INVALID = 1
F = C.c_float


@pytest.fixture(scope="module")
def L():
    from c3dgs_amd import build, _lib
    build.build()
    return _lib.lib()


def test_symbols_exported_with_prototypes(L):
    from c3dgs_amd import _lib
    for name in ("c3dgs_knn_neighbours", "c3dgs_ray_fill_plan_workspace_bytes", "c3dgs_ray_fill_plan", "c3dgs_ray_fill_xyz"):
        assert hasattr(L, name)
        assert name in _lib.PROTOTYPES
    assert L.c3dgs_abi_version() == 4                                    # new entry points only


def test_knn_neighbours_validation(L):
    assert L.c3dgs_knn_neighbours(0, None, None, None, None, None) == 0   # P == 0: no pointer is touched
    assert L.c3dgs_knn_neighbours(-1, None, None, None, None, None) == INVALID
    assert b"P must be >= 0" in L.c3dgs_last_error()
    for args in ((None, 16, 16, 16), (16, None, 16, 16), (16, 16, None, 16), (16, 16, 16, None)):
        assert L.c3dgs_knn_neighbours(5, *args, None) == INVALID
        assert b"knn_neighbours: bad arguments" in L.c3dgs_last_error()


def test_ray_fill_plan_validation(L):
    plan = L.c3dgs_ray_fill_plan
    assert plan(-1, 16, F(1.0), 0, None, None, None, 16, 16, 1 << 20, None) == INVALID
    assert plan(5, 16, F(1.0), -1, None, None, None, 16, 16, 1 << 20, None) == INVALID
    assert b"must be >= 0" in L.c3dgs_last_error()
    assert plan(2**31 - 255, 16, F(1.0), 0, None, None, None, 16, 16, 1 << 20, None) == INVALID
    for bad in (0.0, -1.0, float("inf"), float("nan")):
        assert plan(5, 16, F(bad), 0, None, None, None, 16, 16, 1 << 20, None) == INVALID
        assert b"step" in L.c3dgs_last_error()
    assert plan(5, 16, F(1.0), 0, None, None, None, None, 16, 1 << 20, None) == INVALID       # NULL totals
    assert b"totals" in L.c3dgs_last_error()
    assert plan(0, None, F(1.0), 0, None, None, None, None, None, 0, None) == INVALID         # ... also for P == 0
    assert plan(5, 16, F(1.0), 0, None, None, None, 16, None, 1 << 20, None) == INVALID       # NULL workspace
    assert plan(5, None, F(1.0), 0, None, None, None, 16, 16, 1 << 20, None) == INVALID       # NULL d2
    assert b"NULL buffer" in L.c3dgs_last_error()
    assert plan(5, 16, F(1.0), 8, 16, None, 16, 16, 16, 1 << 20, None) == INVALID             # src without slot
    assert plan(5, 16, F(1.0), 8, 16, 16, None, 16, 16, 1 << 20, None) == INVALID             # src without level
    assert b"go together" in L.c3dgs_last_error()
    assert plan(5, 16, F(1.0), 0, None, None, None, 16, 16, 64, None) == INVALID              # workspace too small
    assert b"workspace" in L.c3dgs_last_error()


def test_ray_fill_xyz_validation(L):
    xyz = L.c3dgs_ray_fill_xyz
    assert xyz(5, None, None, None, F(1.0), 0, None, None, None, None, None) == 0             # no new row: nothing touched
    assert xyz(-1, 16, 16, 16, F(1.0), 4, 16, 16, 16, 16, None) == INVALID
    assert xyz(5, 16, 16, 16, F(1.0), -4, 16, 16, 16, 16, None) == INVALID
    assert xyz(5, 16, 16, 16, F(1.0), 2**31 - 255, 16, 16, 16, 16, None) == INVALID
    assert xyz(5, 16, 16, 16, F(0.0), 4, 16, 16, 16, 16, None) == INVALID
    for k in range(7):
        ptrs = [16] * 7
        ptrs[k] = None
        assert xyz(5, ptrs[0], ptrs[1], ptrs[2], F(1.0), 4, ptrs[3], ptrs[4], ptrs[5], ptrs[6], None) == INVALID
        assert b"NULL buffer" in L.c3dgs_last_error()


def test_ray_fill_workspace_grows(L):
    ws = L.c3dgs_ray_fill_plan_workspace_bytes
    by_p = [ws(P, 0) for P in (0, 1, 4, 257, 5000, 1_000_000, 3_000_000)]
    assert all(s > 0 for s in by_p) and by_p == sorted(by_p)
    assert by_p[-1] >= 3 * 3_000_000 * (4 + 8)                           # a count and a 64-bit offset per (slot, point)
    by_rows = [ws(1000, r) for r in (0, 1, 1000, 100_000, 3_000_000)]
    assert by_rows == sorted(by_rows) and by_rows[1] > by_rows[0]
    assert by_rows[-1] - by_rows[0] >= 3_000_000 * 16                    # (level, src) in and out of the order step
