"""CPU: the density-control entry points of the C ABI are exported with prototypes, validate their arguments without
touching the device, and size a plan workspace that grows with P. The ABI version stays 4 (new entry points only)."""
import ctypes as C

import pytest

NAMES = ("c3dgs_densify_classify", "c3dgs_rows_plan_workspace_bytes", "c3dgs_rows_plan", "c3dgs_rows_apply",
         "c3dgs_densify_stats")
FAKE = 16            # a non-NULL "pointer" that validation must never dereference


@pytest.fixture(scope="module")
def L():
    from c3dgs_amd import build, _lib
    build.build()
    return _lib.lib()


def test_symbols_exported_with_prototypes(L):
    from c3dgs_amd import _lib
    for name in NAMES:
        assert hasattr(L, name)
        assert name in _lib.PROTOTYPES
    assert L.c3dgs_abi_version() == 4
    assert C.sizeof(_lib.RowsTensor) == 6 * 8 + 2 * 4


def test_classify_validation(L):
    thr = (0.0002, 0.01, 0.005, 0.1)
    assert L.c3dgs_densify_classify(0, None, None, None, None, None, None, None, *thr, None, None) == 0   # P == 0 touches nothing
    assert L.c3dgs_densify_classify(-1, None, None, None, None, None, None, None, *thr, None, None) == 1
    assert b"P must be >= 0" in L.c3dgs_last_error()
    assert L.c3dgs_densify_classify(5, *[FAKE] * 7, 0.0, 0.01, 0.005, 0.1, FAKE, None) == 1
    assert b"max_grad must be > 0" in L.c3dgs_last_error()
    assert L.c3dgs_densify_classify(5, *[FAKE] * 7, float("nan"), 0.01, 0.005, 0.1, FAKE, None) == 1
    for i in (0, 1, 2, 3, 6, 7):                                # accum, denom, scale_clone, scale_split, opacity, code
        args = [FAKE, FAKE, FAKE, FAKE, None, None, FAKE, FAKE]
        args[i] = None
        assert L.c3dgs_densify_classify(5, *args[:7], *thr, args[7], None) == 1, i
        assert b"NULL buffer" in L.c3dgs_last_error()
    assert L.c3dgs_densify_classify(5, FAKE, FAKE, FAKE, FAKE, FAKE, None, FAKE, *thr, FAKE, None) == 1
    assert b"go together" in L.c3dgs_last_error()


def test_plan_validation(L):
    assert L.c3dgs_rows_plan(-1, None, 2, 0, None, None, None, FAKE, None, None) == 1
    assert b"P must be >= 0" in L.c3dgs_last_error()
    for N in (0, -3, 251):
        assert L.c3dgs_rows_plan(5, FAKE, N, 0, None, None, None, FAKE, FAKE, None) == 1, N
        assert b"N must be between 1 and 250" in L.c3dgs_last_error()
    assert L.c3dgs_rows_plan(5, FAKE, 2, -1, None, None, None, FAKE, FAKE, None) == 1
    assert b"capacity" in L.c3dgs_last_error()
    assert L.c3dgs_rows_plan(5, FAKE, 2, 0, None, None, None, None, FAKE, None) == 1
    assert b"totals is required" in L.c3dgs_last_error()
    assert L.c3dgs_rows_plan(600_000_000, FAKE, 2, 0, None, None, None, FAKE, FAKE, None) == 1
    assert b"31 bits" in L.c3dgs_last_error()
    assert L.c3dgs_rows_plan(5, None, 2, 0, None, None, None, FAKE, FAKE, None) == 1
    assert L.c3dgs_rows_plan(5, FAKE, 2, 0, None, None, None, FAKE, None, None) == 1
    assert b"NULL buffer" in L.c3dgs_last_error()
    assert L.c3dgs_rows_plan(5, FAKE, 2, 9, FAKE, None, FAKE, FAKE, FAKE, None) == 1
    assert b"go together" in L.c3dgs_last_error()


def test_apply_validation(L):
    from c3dgs_amd import _lib

    def table(**kw):
        t = _lib.RowsTensor()
        t.in_param = t.out_param = FAKE
        t.row_floats, t.role = 3, 0
        for k, v in kw.items():
            setattr(t, k, v)
        return (_lib.RowsTensor * 1)(t)

    call = lambda P, Pn, n, tab, N=2, nd=0, rot=None, std=None, z=None, src=FAKE: L.c3dgs_rows_apply(  # noqa: E731
        P, Pn, src, FAKE, FAKE, n, tab, N, nd, rot, std, z, 0, 0, None)
    assert call(0, 0, 1, table()) == 0                          # nothing to write: no pointer is touched
    assert call(5, 0, 1, table()) == 0
    assert call(5, 7, 0, None) == 0
    assert call(-1, 7, 1, table()) == 1 and b"sizes must be >= 0" in L.c3dgs_last_error()
    assert call(5, -7, 1, table()) == 1
    assert call(5, 7, 1, table(), N=0) == 1 and b"N must be" in L.c3dgs_last_error()
    assert call(5, 7, 17, table()) == 1 and b"between 0 and 16 tensors" in L.c3dgs_last_error()
    assert call(0, 7, 1, table()) == 1 and b"cannot come from P = 0" in L.c3dgs_last_error()
    assert call(5, 7, 1, table(), src=None) == 1 and b"NULL buffer" in L.c3dgs_last_error()
    assert call(5, 7, 1, None) == 1
    assert call(5, 7, 1, table(row_floats=0)) == 1 and b"row_floats" in L.c3dgs_last_error()
    assert call(5, 7, 1, table(out_param=None)) == 1 and b"NULL tensor pointer" in L.c3dgs_last_error()
    assert call(5, 7, 1, table(in_exp_avg=FAKE)) == 1 and b"four moment pointers" in L.c3dgs_last_error()
    assert call(5, 7, 1, table(role=9)) == 1 and b"unknown role" in L.c3dgs_last_error()
    assert call(5, 7, 1, table(role=_lib.ROLE_XYZ, row_floats=4)) == 1 and b"3 floats" in L.c3dgs_last_error()
    assert call(5, 7, 1, table(role=_lib.ROLE_XYZ), nd=4, std=FAKE, z=FAKE) == 1 and b"children need" in L.c3dgs_last_error()
    assert call(5, 7, 1, table(role=_lib.ROLE_SCALING), nd=4, std=None, z=FAKE) == 1


def test_stats_validation(L):
    assert L.c3dgs_densify_stats(0, None, None, None, None, None, None, None) == 0
    assert L.c3dgs_densify_stats(-1, None, None, None, None, None, None, None) == 1
    assert b"P must be >= 0" in L.c3dgs_last_error()
    for i in (0, 1, 3, 4):
        args = [FAKE, FAKE, None, FAKE, FAKE, None]
        args[i] = None
        assert L.c3dgs_densify_stats(5, *args, None) == 1, i
        assert b"NULL buffer" in L.c3dgs_last_error()
    assert L.c3dgs_densify_stats(5, FAKE, FAKE, FAKE, FAKE, FAKE, None, None) == 1
    assert b"go together" in L.c3dgs_last_error()


def test_plan_workspace_monotone(L):
    sizes = [L.c3dgs_rows_plan_workspace_bytes(P) for P in (0, 1, 63, 64, 65, 1000, 100_003, 1_000_000, 3_000_000, 6_000_000)]
    assert all(s > 0 for s in sizes)
    assert sizes == sorted(sizes)
    assert sizes[-2] >= 3_000_000 * 16                          # the four exclusive counts of every row
