"""CPU: the C ABI of sparse Adam (c3dgs_sparse_adam_workspace_bytes / _select / _step; csrc/sparse_adam.hip). The symbols are
exported and bound, the ABI version did not move (new entry points only), the kernel file is built with adam.hip's flags, the
workspace holds the count and P row ids and is monotone in P, the stage names are known, and every invalid call is refused
with a message that names the entry before any device work -- the pointers are fakes that are never read, which is why
these run without a GPU."""
import ctypes as C

import pytest

from c3dgs_amd import _lib, build


@pytest.fixture(scope="module")
def L():
    build.build()
    return _lib.lib()


FAKE = 4096          # 256-byte aligned, never dereferenced
FAKE16 = 4096 + 16   # 16-byte aligned only


def _bytes(L, P):
    n = C.c_size_t(0)
    rc = L.c3dgs_sparse_adam_workspace_bytes(P, C.byref(n))
    return rc, n.value


def _tensors(P, row_lens=(3,), **change):
    arr = (_lib.SparseAdamTensor * len(row_lens))()
    for a, rl in zip(arr, row_lens):
        a.param = a.grad = a.exp_avg = a.exp_avg_sq = FAKE16
        a.n, a.row_len, a.step_size, a.bias_correction2_sqrt = P * rl, rl, 0.01, 1.0
        for k, v in change.items():
            setattr(a, k, v)
    return arr


def _step(L, arr, P, ws=FAKE, n=None):
    return L.c3dgs_sparse_adam_step(len(arr) if n is None else n, arr, P, ws, 0.9, 0.999, 1e-15, None)


def test_symbols_are_exported_and_bound(L):
    for name, n_args in (("c3dgs_sparse_adam_workspace_bytes", 2), ("c3dgs_sparse_adam_select", 5), ("c3dgs_sparse_adam_step", 8)):
        assert hasattr(L, name), name
        res, args = _lib.PROTOTYPES[name]
        assert res is C.c_int and len(args) == n_args, name
    assert L.c3dgs_abi_version() == 4
    names = [f[0] for f in _lib.SparseAdamTensor._fields_]
    assert names == [f[0] for f in _lib.AdamTensor._fields_] + ["row_len"]
    assert C.sizeof(_lib.SparseAdamTensor) == 56


def test_kernel_file_is_built_with_the_dense_kernels_flags():
    assert build.SOURCES["sparse_adam.hip"] == build.SOURCES["adam.hip"] == ["-ffp-contract=off"]
    assert any(h.endswith("adam_common.hpp") for h in build.HEADERS)        # a change of adam_one rebuilds both


def test_stage_names(L):
    try:
        for name in (b"sparse_adam_select", b"sparse_adam_step", b"adam_step"):
            assert L.c3dgs_profile_only(name) == 0, name
        assert L.c3dgs_profile_only(b"sparse_adam") == 1
    finally:
        assert L.c3dgs_profile_only(None) == 0


def test_workspace_bytes_is_monotone_and_holds_the_count_and_the_list(L):
    prev = 0
    for P in (0, 1, 63, 64, 65, 255, 256, 257, 1025, 65536, 65537, 3_000_000, 4_194_305, 2**31 - 1):
        rc, b = _bytes(L, P)
        assert rc == 0, P
        assert b >= 256 + 4 * P and b % 256 == 0 and b >= prev, (P, b)
        prev = b


@pytest.mark.parametrize("P", [-1, 2**31, 2**40])
def test_a_row_count_outside_32_bit_ids_is_refused_everywhere(L, P):
    rc, _ = _bytes(L, P)
    assert rc == 1 and L.c3dgs_last_error().startswith(b"sparse_adam_workspace_bytes: P must be")
    assert L.c3dgs_sparse_adam_select(P, FAKE16, 0, FAKE, None) == 1
    assert L.c3dgs_last_error().startswith(b"sparse_adam_select: P must be")
    assert _step(L, _tensors(1), P) == 1
    assert L.c3dgs_last_error().startswith(b"sparse_adam_step: P must be")


def test_workspace_bytes_needs_somewhere_to_write(L):
    assert L.c3dgs_sparse_adam_workspace_bytes(10, None) == 1
    assert b"sparse_adam_workspace_bytes" in L.c3dgs_last_error()


@pytest.mark.parametrize("what,args,message", [
    ("mask_kind_2", (10, FAKE16, 2, FAKE), "mask_kind must be 0"),
    ("mask_kind_negative", (10, FAKE16, -1, FAKE), "mask_kind must be 0"),
    ("mask_kind_even_with_nothing_to_list", (0, FAKE16, 7, FAKE), "mask_kind must be 0"),
    ("null_mask", (10, None, 0, FAKE), "mask is NULL"),
    ("null_workspace", (10, FAKE16, 1, None), "256-byte aligned"),
    ("workspace_16_byte_aligned", (10, FAKE16, 1, FAKE16), "256-byte aligned"),
    ("workspace_128_byte_aligned", (10, FAKE16, 0, FAKE + 128), "256-byte aligned"),
])
def test_select_rejections(L, what, args, message):
    assert L.c3dgs_sparse_adam_select(*args, None) == 1
    msg = L.c3dgs_last_error().decode()
    assert msg.startswith("sparse_adam_select: ") and message in msg, msg


@pytest.mark.parametrize("what,change,message", [
    ("row_len_zero", dict(row_len=0, n=0), "row_len must be > 0"),
    ("row_len_negative", dict(row_len=-3, n=-30), "row_len must be > 0"),
    ("n_is_not_P_row_len", dict(n=31), "n must be P * row_len"),
    ("n_of_another_P", dict(n=33), "n must be P * row_len"),
    ("null_param", dict(param=None), "NULL tensor pointer"),
    ("null_grad", dict(grad=None), "NULL tensor pointer"),
    ("null_exp_avg", dict(exp_avg=None), "NULL tensor pointer"),
    ("null_exp_avg_sq", dict(exp_avg_sq=None), "NULL tensor pointer"),
])
def test_step_rejects_a_bad_tensor(L, what, change, message):
    for arr in (_tensors(10, (3,), **change), ):
        assert _step(L, arr, 10) == 1
        msg = L.c3dgs_last_error().decode()
        assert msg.startswith("sparse_adam_step: ") and message in msg, msg
    arr = _tensors(10, (1, 45, 3))                         # the bad one last: every tensor is looked at
    for k, v in change.items():
        setattr(arr[2], k, v)
    assert _step(L, arr, 10) == 1 and message.encode() in L.c3dgs_last_error()


def test_step_rejects_bad_counts_and_workspaces(L):
    arr = _tensors(10, (3,) * 16)
    assert _step(L, arr, 10, n=17) == 1 and b"sparse_adam_step: between 0 and 16 tensors" in L.c3dgs_last_error()
    assert _step(L, arr, 10, n=-1) == 1 and b"between 0 and 16" in L.c3dgs_last_error()
    assert L.c3dgs_sparse_adam_step(2, None, 10, FAKE, 0.9, 0.999, 1e-15, None) == 1 and b"tensors is NULL" in L.c3dgs_last_error()
    for ws in (None, FAKE16, FAKE + 128):
        assert _step(L, arr, 10, ws=ws) == 1
        assert L.c3dgs_last_error().startswith(b"sparse_adam_step: the workspace must be non-NULL and 256-byte aligned")


def test_nothing_to_do_returns_0_and_touches_nothing(L):
    assert L.c3dgs_sparse_adam_select(0, None, 0, None, None) == 0            # P == 0
    assert L.c3dgs_sparse_adam_select(0, FAKE16, 1, FAKE, None) == 0
    assert _step(L, _tensors(0, (3, 45)), 0) == 0                              # P == 0: n == 0 everywhere
    assert _step(L, _tensors(0, (3,)), 0, ws=None) == 0
    assert L.c3dgs_sparse_adam_step(0, None, 10, None, 0.9, 0.999, 1e-15, None) == 0      # n_tensors == 0
    assert _step(L, _tensors(10), 10, n=0) == 0
