"""CPU: the C ABI of the per-Gaussian error scores (c3dgs_render_error, c3dgs_error_workspace_bytes, c3dgs_error_map_l1,
c3dgs_error_accumulate; csrc/render_error.hip). The symbols are exported and bound, the ABI version did not move (new entry
points only), the kernel's file is built with render.hip's flags, the workspace is R floats + R flag bytes in 256-byte aligned
regions, and every invalid call is refused with its message before any device work -- which is why these run without a GPU."""
import ctypes as C

import pytest

from c3dgs_amd import _lib, build


@pytest.fixture(scope="module")
def L():
    return _lib.lib()


def test_symbols_are_exported_and_bound(L):
    for name, n_args in (("c3dgs_render_error", 11), ("c3dgs_error_workspace_bytes", 2), ("c3dgs_error_map_l1", 7),
                         ("c3dgs_error_accumulate", 8)):
        assert hasattr(L, name), name
        res, args = _lib.PROTOTYPES[name]
        assert len(args) == n_args, name
    assert _lib.PROTOTYPES["c3dgs_error_workspace_bytes"][0] is C.c_size_t
    assert L.c3dgs_abi_version() == 4


def test_kernel_file_is_built_with_the_blend_kernels_flags():
    assert "render_error.hip" in build.SOURCES
    assert build.SOURCES["render_error.hip"] == build.SOURCES["render.hip"] == build.SOURCES["render_contrib.hip"]


def test_stage_names(L):
    try:
        for name in (b"render_error", b"render_error_blend", b"render_error_sum", b"error_map_l1"):
            assert L.c3dgs_profile_only(name) == 0, name
    finally:
        assert L.c3dgs_profile_only(None) == 0


def _up(v):
    return (v + 255) // 256 * 256


def test_workspace_bytes_formula_and_alignment(L):
    prev = 0
    for R in (0, 1, 2, 63, 64, 255, 256, 257, 4096, 100_000, 16_400_000, 2**31 - 1):
        r = max(R, 1)
        for P in (0, 1, 3_000_000):
            b = L.c3dgs_error_workspace_bytes(P, R)
            assert b == _up(4 * r) + _up(r), (P, R, b)          # R floats | R flag bytes, each region 256-byte aligned
            assert b % 256 == 0 and b >= 512
        assert b >= prev
        prev = b
        assert b < L.c3dgs_contrib_workspace_bytes(0, R) or R <= 64       # a third of the slot bytes of render_contrib
    assert L.c3dgs_error_workspace_bytes(10, 0) == L.c3dgs_error_workspace_bytes(10, 1)


B = 0x1000          # a non-NULL "buffer": the calls below must fail before anything dereferences it
INVALID = [
    ("W", dict(W=0), "W and H must be positive"),
    ("H", dict(H=-3), "W and H must be positive"),
    ("P", dict(P=-1), "P and R must be >= 0"),
    ("R", dict(R=-1), "P and R must be >= 0"),
    ("output", dict(out=None), "the output is required"),
    ("map", dict(map=None), "the pixel map is required"),
    ("geom", dict(geom=None), "buffers and a workspace are required"),
    ("binning", dict(binning=None), "buffers and a workspace are required"),
    ("image", dict(image=None), "buffers and a workspace are required"),
    ("workspace", dict(ws=None), "buffers and a workspace are required"),
    ("instances_of_nothing", dict(P=0), "R > 0 instances cannot come from P = 0"),
]


@pytest.mark.parametrize("what,change,message", INVALID, ids=[c[0] for c in INVALID])
def test_invalid_arguments_return_1_with_a_message(L, what, change, message):
    a = dict(P=10, W=32, H=32, R=5, geom=B, binning=B, image=B, ws=B, map=B, out=B)
    a.update(change)
    rc = L.c3dgs_render_error(a["P"], a["W"], a["H"], a["R"], a["geom"], a["binning"], a["image"], a["ws"], a["map"], a["out"], None)
    assert rc == 1
    msg = L.c3dgs_last_error().decode()
    assert msg.startswith("render_error: ") and message in msg, msg


def test_a_null_map_is_refused_even_with_nothing_to_blend(L):
    assert L.c3dgs_render_error(10, 32, 32, 0, None, None, None, None, None, B, None) == 1
    assert b"pixel map" in L.c3dgs_last_error()
    assert L.c3dgs_render_error(10, 32, 32, 0, None, None, None, None, B, None, None) == 1


def test_error_map_l1_validates_before_any_device_work(L):
    for C_, H, W in ((0, 4, 4), (3, 0, 4), (3, 4, -1)):
        assert L.c3dgs_error_map_l1(C_, H, W, B, B, B, None) == 1
        assert L.c3dgs_last_error().decode().startswith("error_map_l1: ")
    for args in ((None, B, B), (B, None, B), (B, B, None)):
        assert L.c3dgs_error_map_l1(3, 4, 4, *args, None) == 1
        assert b"required" in L.c3dgs_last_error()


def test_accumulate_validates_before_any_device_work(L):
    assert L.c3dgs_error_accumulate(-1, 0, None, None, B, B, B, None) == 1
    assert L.c3dgs_error_accumulate(5, -1, B, B, B, B, B, None) == 1
    assert L.c3dgs_error_accumulate(5, 3, B, None, B, B, B, None) == 1 and b"pair" in L.c3dgs_last_error()
    assert L.c3dgs_error_accumulate(5, 3, None, None, B, B, B, None) == 1           # identity mapping needs P_rows == P_model
    assert L.c3dgs_error_accumulate(5, 5, None, None, None, B, B, None) == 1
    assert L.c3dgs_error_accumulate(5, 5, None, None, B, None, B, None) == 1
    assert L.c3dgs_error_accumulate(5, 5, None, None, B, B, None, None) == 1
    assert L.c3dgs_error_accumulate(0, 0, None, None, None, None, None, None) == 0     # nothing to fold
    assert L.c3dgs_error_accumulate(5, 0, B, B, None, B, B, None) == 0                 # no row is visible
