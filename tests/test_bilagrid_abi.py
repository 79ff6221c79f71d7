"""CPU: the C ABI of the bilateral-grid entries (c3dgs_bilagrid_workspace_bytes / _slice / _slice_backward / _tv / _tv_backward;
csrc/bilagrid.hip). The symbols are exported, declared and bound, the ABI version did not move (new entry points only), the
kernel file is part of the product build, the stage names are known, and every invalid call is refused with a message that
names the entry before any device work -- the pointers are fakes that are never read, which is why these run without a GPU."""
import ctypes as C
import os
import re

import pytest

from c3dgs_amd import _lib, build

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FAKE = 4096          # never dereferenced
SYMBOLS = {"c3dgs_bilagrid_workspace_bytes": (C.c_size_t, 5), "c3dgs_bilagrid_slice": (C.c_int, 9),
           "c3dgs_bilagrid_slice_backward": (C.c_int, 12), "c3dgs_bilagrid_tv": (C.c_int, 8),
           "c3dgs_bilagrid_tv_backward": (C.c_int, 8)}
OK_SIZES = dict(H=4, W=5, L=2, Hg=3, Wg=3)


@pytest.fixture(scope="module")
def L():
    build.build()
    return _lib.lib()


def _slice(lib, grid=FAKE, rgb=FAKE, out=FAKE, **sizes):
    s = dict(OK_SIZES, **sizes)
    return lib.c3dgs_bilagrid_slice(s["H"], s["W"], s["L"], s["Hg"], s["Wg"], grid, rgb, out, None)


def _backward(lib, grid=FAKE, rgb=FAKE, dout=FAKE, dgrid=FAKE, drgb=FAKE, ws=FAKE, **sizes):
    s = dict(OK_SIZES, **sizes)
    return lib.c3dgs_bilagrid_slice_backward(s["H"], s["W"], s["L"], s["Hg"], s["Wg"], grid, rgb, dout, dgrid, drgb, ws, None)


def _tv(lib, Cn=2, grids=FAKE, ws=FAKE, out=FAKE, **sizes):
    s = dict(OK_SIZES, **sizes)
    return lib.c3dgs_bilagrid_tv(Cn, s["L"], s["Hg"], s["Wg"], grids, ws, out, None)


def _tv_backward(lib, Cn=2, grids=FAKE, dtv=FAKE, dgrids=FAKE, **sizes):
    s = dict(OK_SIZES, **sizes)
    return lib.c3dgs_bilagrid_tv_backward(Cn, s["L"], s["Hg"], s["Wg"], grids, dtv, dgrids, None)


def _bytes(lib, **sizes):
    s = dict(OK_SIZES, **sizes)
    return lib.c3dgs_bilagrid_workspace_bytes(s["H"], s["W"], s["L"], s["Hg"], s["Wg"])


def _refused(lib, rc, entry, message):
    msg = lib.c3dgs_last_error().decode()
    assert rc == 1 and msg.startswith(entry + ": ") and message in msg, (rc, msg)


def test_symbols_are_exported_declared_and_bound(L):
    header = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "c3dgs_hip.h")).read(), flags=re.S)
    for name, (res, n_args) in SYMBOLS.items():
        assert hasattr(L, name), name
        assert re.search(r"\b(int|size_t)\s+" + name + r"\s*\(", header), f"{name} is not declared in include/c3dgs_hip.h"
        got_res, args = _lib.PROTOTYPES[name]
        assert got_res is res and len(args) == n_args, name
    assert L.c3dgs_abi_version() == 4
    assert "#define C3DGS_ABI_VERSION 4" in header


def test_kernel_file_is_in_the_product_build_and_every_variant():
    assert build.SOURCES["bilagrid.hip"] == []                          # no test needs separately rounded operations
    assert os.path.exists(os.path.join(build.CSRC, "bilagrid.hip"))
    assert any(h.endswith("bilagrid.hpp") for h in build.HEADERS)
    for flags in list(build.VARIANTS.values()) + list(build.DIAG_VARIANTS.values()):
        assert "bilagrid.hip" not in flags


def test_stage_names(L):
    try:
        for name in (b"bilagrid_slice", b"bilagrid_slice_backward", b"bilagrid_gather", b"bilagrid_fold", b"bilagrid_rgb_backward",
                     b"bilagrid_tv", b"bilagrid_tv_backward"):
            assert L.c3dgs_profile_only(name) == 0, name
        assert L.c3dgs_profile_only(b"bilagrid") == 1
    finally:
        assert L.c3dgs_profile_only(None) == 0


def test_workspace_bytes(L):
    assert _bytes(L) >= 8192 and _bytes(L, H=1, W=1) >= 8192                     # the total variation's 1024 doubles fit
    for H, W, shape in ((1080, 1920, (8, 16, 16)), (1080, 1920, (1, 1, 1)), (70, 130, (1, 1, 1)), (5, 3, (8, 16, 16))):
        b = _bytes(L, H=H, W=W, L=shape[0], Hg=shape[1], Wg=shape[2])
        assert b % 256 == 0 and b >= 48 * shape[0] * shape[1] * shape[2], (H, W, shape, b)   # at least one partial row per vertex
    # a (1, 1, 1) grid's one vertex sees every pixel: the footprint is cut into many slabs, one partial row (48 B) each
    assert _bytes(L, H=1080, W=1920, L=1, Hg=1, Wg=1) >= 48 * (1080 * 1920 // 8192)


@pytest.mark.parametrize("what,sizes,message", [
    ("zero_H", dict(H=0), "must be positive"), ("negative_W", dict(W=-3), "must be positive"), ("zero_L", dict(L=0), "must be positive"),
    ("zero_Hg", dict(Hg=0), "must be positive"), ("negative_Wg", dict(Wg=-1), "must be positive"),
    ("grid_2^31", dict(L=2**14, Hg=2**7, Wg=2**7), "12 * L * Hg * Wg must be below 2^31"),
    ("grid_product_overflows_64_bits", dict(L=2**31 - 1, Hg=2**31 - 1, Wg=2**31 - 1), "12 * L * Hg * Wg must be below 2^31"),
    ("image_2^31", dict(H=2**15, W=2**15), "3 * H * W must be below 2^31"),
])
def test_bad_sizes_are_refused_by_every_entry(L, what, sizes, message):
    _refused(L, _slice(L, **sizes), "bilagrid_slice", message)
    _refused(L, _backward(L, **sizes), "bilagrid_slice_backward", message)
    assert _bytes(L, **sizes) == 0 and L.c3dgs_last_error().decode().startswith("bilagrid_workspace_bytes: ")
    assert message in L.c3dgs_last_error().decode()
    if not set(sizes) & {"H", "W"}:
        _refused(L, _tv(L, **sizes), "bilagrid_tv", message)
        _refused(L, _tv_backward(L, **sizes), "bilagrid_tv_backward", message)


def test_largest_sizes_pass_the_size_check(L):
    # just below both limits: the sizes are accepted, so the NULL pointer is what is refused
    _refused(L, _slice(L, grid=None, H=2**14, W=2**15, L=1, Hg=2**13, Wg=2**14), "bilagrid_slice", "are required")


@pytest.mark.parametrize("Cn,message", [(0, "must be positive"), (-2, "must be positive"), (2**27, "C * 12 * L * Hg * Wg must be below 2^31")])
def test_tv_camera_count(L, Cn, message):
    _refused(L, _tv(L, Cn=Cn), "bilagrid_tv", message)
    _refused(L, _tv_backward(L, Cn=Cn), "bilagrid_tv_backward", message)


@pytest.mark.parametrize("arg", ["grid", "rgb", "out"])
def test_slice_rejects_null_pointers(L, arg):
    _refused(L, _slice(L, **{arg: None}), "bilagrid_slice", "grid, rgb and out are required")


@pytest.mark.parametrize("arg", ["grid", "rgb", "dout", "dgrid"])
def test_slice_backward_rejects_null_pointers(L, arg):
    _refused(L, _backward(L, **{arg: None}), "bilagrid_slice_backward", "grid, rgb, dL_dout and dL_dgrid are required")


def test_slice_backward_rejects_a_null_workspace_with_and_without_drgb(L):
    _refused(L, _backward(L, ws=None), "bilagrid_slice_backward", "the workspace is NULL")
    _refused(L, _backward(L, ws=None, drgb=None), "bilagrid_slice_backward", "the workspace is NULL")


def test_slice_backward_rejects_a_gather_that_does_not_fit(L):
    _refused(L, _backward(L, L=2**20, Hg=1, Wg=1), "bilagrid_slice_backward", "does not fit")


def test_tv_rejects_null_pointers(L):
    for arg in ("grids", "out"):
        _refused(L, _tv(L, **{arg: None}), "bilagrid_tv", "grids and out are required")
    _refused(L, _tv(L, ws=None), "bilagrid_tv", "the workspace is NULL")
    for arg in ("grids", "dtv", "dgrids"):
        _refused(L, _tv_backward(L, **{arg: None}), "bilagrid_tv_backward", "grids, dL_dtv and dL_dgrids are required")
