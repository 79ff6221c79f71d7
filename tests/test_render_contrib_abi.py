"""CPU: the C ABI of the per-Gaussian blend statistics (c3dgs_render_contrib, c3dgs_contrib_workspace_bytes,
c3dgs_contrib_accumulate; csrc/render_contrib.hip). The symbols are exported and bound, the ABI version did not move (new entry
points only), the kernel's file is built with render.hip's flags, the workspace size is monotone in R and 256-byte aligned, and
every invalid call is refused with its message before any device work -- which is why these run without a GPU."""
import ctypes as C

import pytest

from c3dgs_amd import _lib, build


@pytest.fixture(scope="module")
def L():
    return _lib.lib()


def test_symbols_are_exported_and_bound(L):
    for name, n_args in (("c3dgs_render_contrib", 12), ("c3dgs_contrib_workspace_bytes", 2), ("c3dgs_contrib_accumulate", 12)):
        assert hasattr(L, name), name
        res, args = _lib.PROTOTYPES[name]
        assert len(args) == n_args, name
    assert _lib.PROTOTYPES["c3dgs_contrib_workspace_bytes"][0] is C.c_size_t
    assert L.c3dgs_abi_version() == 4


def test_kernel_file_is_built_with_the_blend_kernels_flags():
    assert "render_contrib.hip" in build.SOURCES
    assert build.SOURCES["render_contrib.hip"] == build.SOURCES["render.hip"]


def test_stage_names(L):
    try:
        for name in (b"render_contrib", b"render_contrib_blend", b"render_contrib_sum"):
            assert L.c3dgs_profile_only(name) == 0, name
    finally:
        assert L.c3dgs_profile_only(None) == 0


def test_workspace_bytes_are_monotone_and_aligned(L):
    prev = 0
    for R in (0, 1, 2, 255, 256, 257, 4096, 100_000, 16_400_000, 2**31 - 1):
        for P in (0, 1, 3_000_000):
            b = L.c3dgs_contrib_workspace_bytes(P, R)
            assert b % 256 == 0 and b >= 256, (P, R, b)
            assert b >= 13 * max(R, 1), (P, R, b)             # {sum, max, hits} + a flag byte per instance
        assert b >= prev, (R, b, prev)
        prev = b
    assert L.c3dgs_contrib_workspace_bytes(10, 0) == L.c3dgs_contrib_workspace_bytes(10, 1)


B = 0x1000          # a non-NULL "buffer": the calls below must fail before anything dereferences it
INVALID = [
    ("W", dict(W=0), "W and H must be positive"),
    ("H", dict(H=-3), "W and H must be positive"),
    ("P", dict(P=-1), "P and R must be >= 0"),
    ("R", dict(R=-1), "P and R must be >= 0"),
    ("outputs", dict(sum=None, max=None, hits=None), "at least one output is required"),
    ("geom", dict(geom=None), "buffers and a workspace are required"),
    ("binning", dict(binning=None), "buffers and a workspace are required"),
    ("image", dict(image=None), "buffers and a workspace are required"),
    ("workspace", dict(ws=None), "buffers and a workspace are required"),
    ("instances_of_nothing", dict(P=0), "R > 0 instances cannot come from P = 0"),
]


@pytest.mark.parametrize("what,change,message", INVALID, ids=[c[0] for c in INVALID])
def test_invalid_arguments_return_1_with_a_message(L, what, change, message):
    a = dict(P=10, W=32, H=32, R=5, geom=B, binning=B, image=B, ws=B, sum=B, max=B, hits=B)
    a.update(change)
    rc = L.c3dgs_render_contrib(a["P"], a["W"], a["H"], a["R"], a["geom"], a["binning"], a["image"], a["ws"], a["sum"], a["max"],
                                a["hits"], None)
    assert rc == 1
    msg = L.c3dgs_last_error().decode()
    assert msg.startswith("render_contrib: ") and message in msg, msg


def test_accumulate_validates_before_any_device_work(L):
    acc = [B] * 4
    rows = [B] * 3
    assert L.c3dgs_contrib_accumulate(-1, 0, None, None, *rows, *acc, None) == 1
    assert L.c3dgs_contrib_accumulate(5, -1, B, B, *rows, *acc, None) == 1
    assert L.c3dgs_contrib_accumulate(5, 3, B, None, *rows, *acc, None) == 1 and b"pair" in L.c3dgs_last_error()
    assert L.c3dgs_contrib_accumulate(5, 3, None, None, *rows, *acc, None) == 1           # identity mapping needs P_rows == P_model
    assert L.c3dgs_contrib_accumulate(5, 5, None, None, None, B, B, *acc, None) == 1
    assert L.c3dgs_contrib_accumulate(5, 5, None, None, *rows, B, B, None, B, None) == 1
    assert L.c3dgs_contrib_accumulate(0, 0, None, None, None, None, None, None, None, None, None, None) == 0     # nothing to fold
    assert L.c3dgs_contrib_accumulate(5, 0, B, B, None, None, None, *acc, None) == 0                             # no row is visible
