"""CPU: the depth sort's digit plan and key transform (csrc/common.hpp: depth_sort_plan, depth_key_biased, depth_sort_digit;
through the host-only c3dgs_debug_depth_plan). An LSD radix sort orders by the digit tuple read from the last pass to the first,
so for every pair of keys a plan admits, comparing those tuples must order exactly as comparing the keys, and the culled sentinel
must sort behind every visible key."""
import ctypes as C

import numpy as np
import pytest

CULLED, BIAS = 0xFFFFFFFF, 0x3C000000
LIMIT3 = BIAS + (1 << 27) - 1


@pytest.fixture(scope="module")
def L():
    from c3dgs_amd import build, _lib
    build.build()
    return _lib.lib()


def _plan(L, biased, max_key, keys):
    from c3dgs_amd import _lib
    keys = np.ascontiguousarray(keys, dtype=np.uint32)
    plan = np.zeros(6, np.uint32)
    digits = np.zeros((keys.size, 4), np.uint32)
    _lib.check(L.c3dgs_debug_depth_plan(int(biased), int(max_key), keys.size, keys.ctypes.data_as(C.c_void_p), plan.ctypes.data_as(C.c_void_p),
                                        digits.ctypes.data_as(C.c_void_p)))
    return int(plan[0]), [int(b) for b in plan[1:5]], int(plan[5]), digits


def _rank_by_digits(digits, passes):
    """position of every key in the order of its digit tuple, most significant (last pass) first; equal tuples share a rank"""
    tup = [tuple(int(d) for d in row[:passes][::-1]) for row in digits]
    ranks = {t: r for r, t in enumerate(sorted(set(tup)))}
    return np.array([ranks[t] for t in tup])


def _rank_by_key(keys):
    return np.unique(keys, return_inverse=True)[1]


def _f(x):
    return int(np.float32(x).view(np.uint32))


def test_plans(L):
    assert _plan(L, 0, 0, [])[:3] == (4, [8, 8, 8, 8], 0)
    assert _plan(L, 0, CULLED - 1, [])[:3] == (4, [8, 8, 8, 8], 0)
    for mk in (0, BIAS, _f(0.0100001), _f(12.0), _f(511.99), LIMIT3 - 1):
        assert _plan(L, 1, mk, [])[:3] == (3, [9, 9, 9, 0], BIAS), hex(mk)
    for mk in (LIMIT3, _f(512.0), _f(600.0), _f(1e6), _f(np.inf), 0x7FC00000, 0xFFC00000, CULLED - 1):
        assert _plan(L, 1, mk, [])[:3] == (4, [9, 9, 9, 5], BIAS), hex(mk)
    assert LIMIT3 == _f(512.0) - 1                       # every depth below 512 but the last float in front of it takes three passes
    assert BIAS == _f(2.0 ** -7) and BIAS < _f(0.01)     # below every key that passed the near-plane test (z > 0.01)


@pytest.mark.parametrize("biased,max_key", [(1, LIMIT3 - 1), (1, _f(12.0)), (1, LIMIT3), (1, _f(1e6)), (1, CULLED - 1), (0, CULLED - 1)])
def test_digit_tuples_order_as_the_keys(L, biased, max_key):
    rng = np.random.default_rng(max_key % 65521 + biased)
    lo = BIAS if biased else 0
    edge = [lo, lo + 1, max_key, max_key - 1, CULLED, CULLED]
    if biased:
        edge += [_f(0.0100001), min(_f(2.0), max_key), min(_f(2.0) + 1, max_key), min(LIMIT3 - 1, max_key), min(LIMIT3, max_key)]
        edge += [BIAS + (1 << 9) - 1, BIAS + (1 << 9), BIAS + (1 << 18) - 1, BIAS + (1 << 18)]       # digit boundaries
    else:
        edge += [0, 1, 255, 256, _f(-0.5), _f(1e-5), _f(5.0), 0x80000000, 0x7FFFFFFF]
    edge = [k for k in edge if k == CULLED or lo <= k <= max_key]
    keys = np.concatenate([np.array(edge, np.uint64), rng.integers(lo, max_key + 1, 4000, dtype=np.uint64),
                           np.float32(rng.uniform(2.0, 12.0, 1000)).view(np.uint32).astype(np.uint64)])
    keys = keys[(keys == CULLED) | ((keys >= lo) & (keys <= max_key))].astype(np.uint32)
    passes, bits, bias, digits = _plan(L, biased, max_key, keys)
    assert sum(bits[:passes]) == (27 if passes == 3 else 32) and bias == (BIAS if biased else 0)
    for p in range(passes):
        assert int(digits[:, p].max()) < (1 << bits[p])
    np.testing.assert_array_equal(_rank_by_digits(digits, passes), _rank_by_key(keys))
    # the sentinel: the top of every digit range it takes part in, strictly behind every visible key
    sent = digits[keys == CULLED][0]
    assert [int(d) for d in sent[:passes]] == [(1 << b) - 1 for b in bits[:passes]]
    vis = keys != CULLED
    assert _rank_by_digits(digits, passes)[vis].max() < _rank_by_digits(digits, passes)[~vis].min()
