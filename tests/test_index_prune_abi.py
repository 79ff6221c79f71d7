"""CPU: the indexed-prune entry points of the C ABI are exported with prototypes, refuse bad arguments before any device work,
and size a workspace that grows with P, K0 and K1. The ABI version stays 4 (new entry points only)."""
import pytest

NAMES = ("c3dgs_index_plan_workspace_bytes", "c3dgs_index_plan")
FAKE = 16            # a non-NULL "pointer" that validation must never dereference


@pytest.fixture(scope="module")
def L():
    from c3dgs_amd import build, _lib
    build.build()
    return _lib.lib()


def _call(L, P=5, keep=FAKE, idx0=FAKE, K0=3, idx1=FAKE, K1=4, caps=(0, 0, 0), outs=(None,) * 5, totals=FAKE, ws=FAKE):
    return L.c3dgs_index_plan(P, keep, idx0, K0, idx1, K1, *caps, *outs, totals, ws, None)


def test_symbols_exported_with_prototypes(L):
    from c3dgs_amd import _lib
    for name in NAMES:
        assert hasattr(L, name)
        assert name in _lib.PROTOTYPES
    assert L.c3dgs_abi_version() == 4


def test_plan_validation(L):
    for kw in (dict(P=-1), dict(K0=-1, idx0=None), dict(K1=-2, idx1=None)):
        assert _call(L, **kw) == 1, kw
        assert b"must be >= 0" in L.c3dgs_last_error()
    big = 2 ** 31 - 255                                                      # one past the largest size
    for kw in (dict(P=big), dict(K0=big), dict(K1=big)):
        assert _call(L, **kw) == 1, kw
        assert b"INT32_MAX - 255" in L.c3dgs_last_error()
    for caps in ((-1, 0, 0), (0, -1, 0), (0, 0, -1)):
        assert _call(L, caps=caps) == 1, caps
        assert b"capacities" in L.c3dgs_last_error()
    assert _call(L, K0=0) == 1 and b"K > 0" in L.c3dgs_last_error()          # idx0 given without a codebook
    assert _call(L, K1=0) == 1 and b"K > 0" in L.c3dgs_last_error()
    assert _call(L, totals=None) == 1 and b"totals is required" in L.c3dgs_last_error()
    assert _call(L, ws=None) == 1 and b"workspace is required" in L.c3dgs_last_error()
    assert _call(L, P=0, totals=None) == 1 and _call(L, P=0, ws=None) == 1   # also when there is nothing to do
    # src given: new_idx and cb_src of every index space given are required
    for missing in (1, 2, 3, 4):
        outs = [FAKE] * 5
        outs[missing] = None
        assert _call(L, caps=(9, 9, 9), outs=tuple(outs)) == 1, missing
        assert b"go together" in L.c3dgs_last_error()


def test_workspace_grows_with_every_size(L):
    ws = L.c3dgs_index_plan_workspace_bytes
    assert ws(0, 0, 0) > 0
    sizes = [ws(P, 1000, 1000) for P in (0, 1, 255, 256, 257, 70_001, 1_000_000, 6_000_000)]
    assert sizes == sorted(sizes) and sizes[-1] >= 6_000_000 * 4             # the exclusive count of every Gaussian
    for which in (1, 2):
        sizes = []
        for K in (0, 1, 300, 70_003, 754_000, 6_000_000):
            args = [1000, 1000, 1000]
            args[which] = K
            sizes.append(ws(*args))
        assert sizes == sorted(sizes) and sizes[-1] >= 6_000_000 * 5         # a flag byte and a count per codebook row
