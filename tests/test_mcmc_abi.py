"""CPU: the C ABI of MCMC density control (c3dgs_mcmc_workspace_bytes / _sample / _apply / _noise; csrc/mcmc.hip). The symbols
are exported, declared and bound, the ABI version did not move (new entry points only), the kernel file is part of the product
build, the workspace is 256-aligned and monotone in P, and every invalid call is refused with a message that names the entry
before any device work -- the pointers are fakes that are never read, which is why these run without a GPU."""
import ctypes as C
import os
import re

import pytest

from c3dgs_amd import _lib, build

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FAKE = 4096          # 256-byte aligned, never dereferenced
FAKE16 = 4096 + 16
SYMBOLS = {"c3dgs_mcmc_workspace_bytes": 2, "c3dgs_mcmc_sample": 15, "c3dgs_mcmc_apply": 12, "c3dgs_mcmc_noise": 10}


@pytest.fixture(scope="module")
def L():
    build.build()
    return _lib.lib()


def _bytes(L, P):
    n = C.c_size_t(0)
    return L.c3dgs_mcmc_workspace_bytes(P, C.byref(n)), n.value


def _sample(L, P=10, raw=FAKE16, dead=None, derive=0, min_opacity=0.005, dead_out=None, n=4, draws=FAKE16, reuse=0, q=FAKE16,
            sources=FAKE16, counts=FAKE16, T=FAKE16, ws=FAKE):
    return L.c3dgs_mcmc_sample(P, raw, dead, derive, min_opacity, dead_out, n, draws, reuse, q, sources, counts, T, ws, None)


def _table(roles=(_lib.ROLE_COPY, _lib.MCMC_ROLE_OPACITY, _lib.MCMC_ROLE_SCALE), floats=(3, 1, 1), **change):
    arr = (_lib.RowsTensor * len(roles))()
    for a, role, rf in zip(arr, roles, floats):
        a.in_param = a.out_param = FAKE16
        a.in_exp_avg = a.out_exp_avg = a.in_exp_avg_sq = a.out_exp_avg_sq = FAKE16
        a.row_floats, a.role = rf, role
    for k, v in change.items():
        setattr(arr[0], k, v)
    return arr


def _apply(L, P=10, n=4, dst=FAKE16, dst_base=0, sources=FAKE16, counts=FAKE16, table=None, n_tensors=None, copy_rows=1,
           min_opacity=0.005, ws=FAKE):
    table = _table() if table is None else table
    return L.c3dgs_mcmc_apply(P, n, dst, dst_base, sources, counts, len(table) if n_tensors is None else n_tensors, table, copy_rows,
                              min_opacity, ws, None)


def _noise(L, P=10, ptrs=(FAKE16,) * 6):
    return L.c3dgs_mcmc_noise(P, *ptrs, 5e5, 1e-4, None)


def test_symbols_are_exported_declared_and_bound(L):
    header = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "c3dgs_hip.h")).read(), flags=re.S)
    for name, n_args in SYMBOLS.items():
        assert hasattr(L, name), name
        assert re.search(r"\bint\s+" + name + r"\s*\(", header), f"{name} is not declared in include/c3dgs_hip.h"
        res, args = _lib.PROTOTYPES[name]
        assert res is C.c_int and len(args) == n_args, name
    assert L.c3dgs_abi_version() == 4
    assert "#define C3DGS_ABI_VERSION 4" in header
    assert (_lib.MCMC_ROLE_OPACITY, _lib.MCMC_ROLE_SCALE) == (3, 4)
    assert "#define C3DGS_MCMC_ROLE_OPACITY 3" in header and "#define C3DGS_MCMC_ROLE_SCALE 4" in header


def test_kernel_file_is_in_the_product_build_and_every_variant():
    assert build.SOURCES["mcmc.hip"] == ["-ffp-contract=off"]          # t = floor(u * T) is one IEEE multiply
    assert any(h.endswith("mcmc.hpp") for h in build.HEADERS)
    for flags in list(build.VARIANTS.values()) + list(build.DIAG_VARIANTS.values()):
        assert "mcmc.hip" not in flags                                  # shared with the product build, never rebuilt differently


def test_stage_names(L):
    try:
        for name in (b"mcmc_weights", b"mcmc_search", b"mcmc_values", b"mcmc_apply", b"mcmc_noise"):
            assert L.c3dgs_profile_only(name) == 0, name
        assert L.c3dgs_profile_only(b"mcmc") == 1
    finally:
        assert L.c3dgs_profile_only(None) == 0


def test_workspace_bytes_is_aligned_and_monotone(L):
    prev = 0
    for P in (0, 1, 63, 64, 65, 255, 256, 257, 1025, 65536, 65537, 1_048_833, 3_000_000, 6_000_000, 2**31 - 1):
        rc, b = _bytes(L, P)
        assert rc == 0, P
        assert b % 256 == 0 and b >= prev and b >= 20 * P, (P, b)        # the local prefix, the staged opacity and 3 scale floats
        prev = b
    assert L.c3dgs_mcmc_workspace_bytes(10, None) == 1 and b"mcmc_workspace_bytes" in L.c3dgs_last_error()


@pytest.mark.parametrize("P", [-1, 2**31, 2**40])
def test_a_row_count_outside_32_bit_ids_is_refused_everywhere(L, P):
    assert _bytes(L, P)[0] == 1 and L.c3dgs_last_error().startswith(b"mcmc_workspace_bytes: P must be")
    assert _sample(L, P=P) == 1 and L.c3dgs_last_error().startswith(b"mcmc_sample: P must be")
    assert _apply(L, P=P) == 1 and L.c3dgs_last_error().startswith(b"mcmc_apply: P must be")
    assert _noise(L, P=P) == 1 and L.c3dgs_last_error().startswith(b"mcmc_noise: P must be")


def test_negative_and_oversized_n_is_refused(L):
    for n in (-1, 2**31):
        assert _sample(L, n=n) == 1 and L.c3dgs_last_error().startswith(b"mcmc_sample: n must be")
        assert _apply(L, n=n) == 1 and L.c3dgs_last_error().startswith(b"mcmc_apply: n must be")


def test_nothing_to_do_returns_0_and_touches_nothing(L):
    none = dict(raw=None, draws=None, q=None, sources=None, counts=None, T=None, ws=None)
    assert _sample(L, P=0, n=0, **none) == 0
    assert _sample(L, P=0, n=5, **none) == 0
    assert _apply(L, P=0, n=0, dst=None, sources=None, counts=None, ws=None) == 0
    assert _apply(L, P=10, n=0, dst=None, sources=None, counts=None, ws=None) == 0
    assert _apply(L, P=10, n=0, n_tensors=0, dst=None, sources=None, counts=None, ws=None) == 0
    assert _noise(L, P=0, ptrs=(None,) * 6) == 0


@pytest.mark.parametrize("what,change,message", [
    ("null_opacity", dict(raw=None), "raw_opacity, q and T are required"),
    ("null_q", dict(q=None), "raw_opacity, q and T are required"),
    ("null_T", dict(T=None), "raw_opacity, q and T are required"),
    ("null_counts", dict(counts=None), "counts is NULL"),
    ("null_counts_on_reuse", dict(counts=None, reuse=1), "counts is NULL"),
    ("null_draws", dict(draws=None), "n > 0 needs draws and sources"),
    ("null_sources", dict(sources=None), "n > 0 needs draws and sources"),
    ("mask_and_derive", dict(dead=FAKE16, derive=1, dead_out=FAKE16), "exclude each other"),
    ("derive_without_output", dict(derive=1), "derive_dead needs dead_out"),
    ("derive_negative_threshold", dict(derive=1, dead_out=FAKE16, min_opacity=-0.1), "min_opacity must be >= 0"),
    ("derive_nan_threshold", dict(derive=1, dead_out=FAKE16, min_opacity=float("nan")), "min_opacity must be >= 0"),
    ("null_workspace", dict(ws=None), "256-byte aligned"),
    ("workspace_16_byte_aligned", dict(ws=FAKE16), "256-byte aligned"),
])
def test_sample_rejections(L, what, change, message):
    assert _sample(L, **change) == 1
    msg = L.c3dgs_last_error().decode()
    assert msg.startswith("mcmc_sample: ") and message in msg, msg


@pytest.mark.parametrize("what,kwargs,message", [
    ("null_sources", dict(sources=None), "NULL buffer"),
    ("null_counts", dict(counts=None), "NULL buffer"),
    ("seventeen_tensors", dict(n_tensors=17), "between 0 and 16 tensors"),
    ("negative_tensors", dict(n_tensors=-1), "between 0 and 16 tensors"),
    ("min_opacity_one", dict(min_opacity=1.0), "min_opacity must be in [0, 1)"),
    ("min_opacity_nan", dict(min_opacity=float("nan")), "min_opacity must be in [0, 1)"),
    ("base_beyond_P", dict(dst=None, dst_base=8), "dst_base + n must lie inside"),
    ("negative_base", dict(dst=None, dst_base=-1), "dst_base + n must lie inside"),
    ("no_opacity_tensor", dict(table=_table(roles=(0, 0, _lib.MCMC_ROLE_SCALE))), "needs the opacity and the scale tensor"),
    ("no_scale_tensor", dict(table=_table(roles=(0, _lib.MCMC_ROLE_OPACITY, 0))), "needs the opacity and the scale tensor"),
    ("two_opacity_tensors", dict(table=_table(roles=(_lib.MCMC_ROLE_OPACITY, _lib.MCMC_ROLE_OPACITY, _lib.MCMC_ROLE_SCALE), floats=(1, 1, 1))),
     "one opacity tensor"),
    ("wide_opacity", dict(table=_table(floats=(3, 2, 1))), "one opacity tensor"),
    ("wide_scale", dict(table=_table(floats=(3, 1, 4))), "one scale tensor"),
    ("densify_role", dict(table=_table(roles=(_lib.ROLE_XYZ, _lib.MCMC_ROLE_OPACITY, _lib.MCMC_ROLE_SCALE))), "unknown role"),
    ("row_floats_zero", dict(table=_table(row_floats=0)), "row_floats must be between 1 and 4096"),
    ("not_in_place", dict(table=_table(in_param=FAKE)), "in place"),
    ("null_param", dict(table=_table(in_param=None, out_param=None)), "in place"),
    ("one_moment", dict(table=_table(in_exp_avg=None, out_exp_avg=None)), "moment pointers go together"),
    ("moments_not_in_place", dict(table=_table(in_exp_avg=FAKE)), "moment pointers go together"),
    ("null_workspace", dict(ws=None), "256-byte aligned"),
    ("workspace_16_byte_aligned", dict(ws=FAKE16), "256-byte aligned"),
])
def test_apply_rejections(L, what, kwargs, message):
    assert _apply(L, **kwargs) == 1
    msg = L.c3dgs_last_error().decode()
    assert msg.startswith("mcmc_apply: ") and message in msg, msg


def test_apply_needs_a_table(L):
    assert L.c3dgs_mcmc_apply(10, 4, FAKE16, 0, FAKE16, FAKE16, 3, None, 1, 0.005, FAKE, None) == 1
    assert b"mcmc_apply: NULL buffer" in L.c3dgs_last_error()


def test_noise_rejects_null_buffers(L):
    for i in (0, 1, 2, 4, 5):                                  # xyz, rotation, scaling, opacity, xi; the factor (3) is optional
        ptrs = [FAKE16] * 6
        ptrs[i] = None
        assert _noise(L, ptrs=tuple(ptrs)) == 1, i
        assert L.c3dgs_last_error().startswith(b"mcmc_noise: NULL buffer")
