"""CPU: the geometry-evaluation entries of include/c3dgs_hip.h (nearest neighbour of external queries, surface sampling, the
reduction) validate their arguments before any device work, so every case here runs without a GPU: C3DGS_E_INVALID with a message,
the zero-count no-ops, monotone byte-size functions, and the six stage names."""
import ctypes as C

import pytest


@pytest.fixture(scope="module")
def L():
    from c3dgs_amd import build, _lib
    build.build()
    return _lib.lib()


FAKE = C.c_void_p(4096)          # non-NULL, 256-byte aligned, never dereferenced: validation comes first


def refused(L, rc, *words):
    msg = L.c3dgs_last_error()
    assert rc == 1, msg
    assert msg and all(w in msg for w in words), msg


def test_nn_build_and_query_validation(L):
    refused(L, L.c3dgs_nn_build(-1, FAKE, FAKE, None), b"nn_build")
    refused(L, L.c3dgs_nn_build(5, None, FAKE, None), b"nn_build")
    refused(L, L.c3dgs_nn_build(5, FAKE, None, None), b"nn_build")
    refused(L, L.c3dgs_nn_build(5, FAKE, C.c_void_p(4100), None), b"aligned")
    assert L.c3dgs_nn_build(0, None, None, None) == 0
    q = lambda P, index, Q, queries, idx, d2, ws, sort=1: L.c3dgs_nn_query(P, index, Q, queries, sort, idx, d2, None, ws, None)
    refused(L, q(-1, FAKE, 4, FAKE, FAKE, FAKE, FAKE), b"nn_query")
    refused(L, q(4, FAKE, -1, FAKE, FAKE, FAKE, FAKE), b"nn_query")
    refused(L, q(4, None, 4, FAKE, FAKE, FAKE, FAKE), b"index")
    for i in range(4):
        args = [FAKE] * 4
        args[i] = None
        refused(L, q(4, FAKE, 4, *args, sort=1), b"nn_query")
        if i < 3:                                                     # the workspace belongs to the sorted form with P > 0 alone
            refused(L, q(4, FAKE, 4, *args, sort=0), b"nn_query")
            refused(L, q(0, None, 4, *args), b"nn_query")            # without a reference set the outputs are still written
    refused(L, q(4, FAKE, 4, FAKE, FAKE, FAKE, C.c_void_p(4100)), b"aligned")
    assert q(4, FAKE, 0, None, None, None, None) == 0                 # Q == 0 touches no pointer
    assert q(0, None, 0, None, None, None, None) == 0


def test_mesh_sample_validation(L):
    total = C.c_uint64(77)
    big = 1 << 30
    count = lambda V, v, F, f, density, ws, nbytes, tot: L.c3dgs_mesh_sample_count(V, v, F, f, density, 0, ws, nbytes, tot, None)
    emit = lambda V, v, F, f, ws, nbytes, S, p, face: L.c3dgs_mesh_sample_emit(V, v, F, f, 0, ws, nbytes, S, p, face, None)
    refused(L, count(-1, FAKE, 4, FAKE, 1.0, FAKE, big, C.byref(total)), b"mesh_sample_count")
    refused(L, count(4, FAKE, -1, FAKE, 1.0, FAKE, big, C.byref(total)), b"mesh_sample_count")
    refused(L, count(4, None, 4, FAKE, 1.0, FAKE, big, C.byref(total)), b"vertices")
    refused(L, count(4, FAKE, 4, None, 1.0, FAKE, big, C.byref(total)), b"faces")
    refused(L, count(4, FAKE, 4, FAKE, 1.0, None, big, C.byref(total)), b"workspace")
    refused(L, count(4, FAKE, 4, FAKE, 1.0, C.c_void_p(4100), big, C.byref(total)), b"workspace")
    need = L.c3dgs_mesh_sample_workspace_bytes(4)
    refused(L, count(4, FAKE, 4, FAKE, 1.0, FAKE, need - 1, C.byref(total)), b"workspace")
    refused(L, count(4, FAKE, 4, FAKE, 1.0, FAKE, big, None), b"total")
    for density in (0.0, -1.0, float("inf"), float("nan")):
        refused(L, count(4, FAKE, 4, FAKE, density, FAKE, big, C.byref(total)), b"density")
    assert total.value == 77                                           # a refused call leaves the total alone
    assert count(4, FAKE, 0, None, 1.0, None, 0, C.byref(total)) == 0 and total.value == 0        # no face: no launch
    refused(L, emit(-1, FAKE, 4, FAKE, FAKE, big, 3, FAKE, FAKE), b"mesh_sample_emit")
    refused(L, emit(4, FAKE, 4, FAKE, FAKE, need - 1, 3, FAKE, FAKE), b"workspace")
    refused(L, emit(4, FAKE, 4, FAKE, FAKE, big, -1, FAKE, FAKE), b"S must")
    refused(L, emit(4, FAKE, 4, FAKE, FAKE, big, 1 << 31, FAKE, FAKE), b"S must")
    refused(L, emit(4, FAKE, 4, FAKE, FAKE, big, 3, None, FAKE), b"points")
    refused(L, emit(4, FAKE, 4, FAKE, FAKE, big, 3, FAKE, None), b"face")
    refused(L, emit(4, FAKE, 0, None, None, 0, 3, FAKE, FAKE), b"without faces")
    assert emit(4, FAKE, 4, FAKE, FAKE, big, 0, None, None) == 0       # no sample: no launch
    assert emit(0, None, 0, None, None, 0, 0, None, None) == 0


def test_geometry_reduce_validation(L):
    tau = (C.c_float * 8)(*[0.1] * 8)
    box = (C.c_float * 6)(0, 0, 0, 1, 1, 1)
    big = 1 << 30
    red = lambda N, d2, pts, bounds, T, th, ws, nbytes, out: L.c3dgs_geometry_reduce(N, d2, pts, bounds, 1.0, T, th, ws, nbytes, out, None)
    refused(L, red(-1, FAKE, None, None, 0, None, FAKE, big, FAKE), b"geometry_reduce")
    refused(L, red(10, FAKE, None, None, 9, tau, FAKE, big, FAKE), b"T must")
    refused(L, red(10, FAKE, None, None, -1, tau, FAKE, big, FAKE), b"T must")
    refused(L, red(10, FAKE, None, None, 2, None, FAKE, big, FAKE), b"thresholds")
    refused(L, red(10, FAKE, FAKE, None, 0, None, FAKE, big, FAKE), b"pair")
    refused(L, red(10, FAKE, None, box, 0, None, FAKE, big, FAKE), b"pair")
    refused(L, red(10, None, None, None, 0, None, FAKE, big, FAKE), b"d2")
    refused(L, red(10, FAKE, None, None, 0, None, FAKE, big, None), b"out")
    refused(L, red(10, FAKE, None, None, 0, None, None, big, FAKE), b"workspace")
    refused(L, red(10, FAKE, None, None, 0, None, FAKE, L.c3dgs_geometry_reduce_workspace_bytes(10) - 1, FAKE), b"workspace")
    refused(L, red(10, FAKE, None, None, 0, None, C.c_void_p(4100), big, FAKE), b"workspace")


def test_byte_sizes_are_monotone(L):
    sizes = (0, 1, 31, 32, 33, 255, 256, 257, 5000, 70_000, 1_000_000, 4_000_000)
    for fn in (L.c3dgs_nn_index_bytes, L.c3dgs_nn_query_workspace_bytes, L.c3dgs_mesh_sample_workspace_bytes,
               L.c3dgs_geometry_reduce_workspace_bytes):
        got = [fn(n) for n in sizes]
        assert all(v > 0 and v % 256 == 0 for v in got[1:]), got
        assert all(a <= b for a, b in zip(got, got[1:])), got
        assert fn(-1) == 0
    assert L.c3dgs_nn_index_bytes(1_000_000) >= 1_000_000 * (16 + 8 + 4)          # points, codes, ids
    assert L.c3dgs_nn_index_bytes(5000) == L.c3dgs_knn_workspace_bytes(5000)       # the index is the 3-NN workspace
    assert L.c3dgs_nn_query_workspace_bytes(1_000_000) >= 1_000_000 * 24           # keys and ids, twice
    assert L.c3dgs_mesh_sample_workspace_bytes(70_000) >= 70_000 * 4


STAGES = ("nn_query_sort", "nn_query", "mesh_sample_count", "mesh_sample_scan", "mesh_sample_emit", "geometry_reduce")


def test_profile_only_knows_the_new_stage_names(L):
    try:
        for name in STAGES + ("knn_sort", "knn_bounds"):
            assert L.c3dgs_profile_only(name.encode()) == 0, name
        assert L.c3dgs_profile_only(b"nn_build") == 1
    finally:
        assert L.c3dgs_profile_only(None) == 0
