"""CPU: the C ABI of the depth / alpha / median-depth pass (c3dgs_render_depth, csrc/render_depth.hip). The symbol is exported and
bound, the ABI version did not move (a new entry point only), the kernel's file is built with render.hip's flags (the two share
the alpha expression and must compile it alike), and every invalid call is refused with its message before any device work --
which is why these run without a GPU."""
import ctypes as C

import pytest

from c3dgs_amd import _lib, build


@pytest.fixture(scope="module")
def L():
    return _lib.lib()


def test_symbol_is_exported_and_bound(L):
    assert hasattr(L, "c3dgs_render_depth")
    res, args = _lib.PROTOTYPES["c3dgs_render_depth"]
    assert res is C.c_int and len(args) == 11
    assert args[:4] == [C.c_int32] * 4 and all(a is C.c_void_p for a in args[4:])
    assert L.c3dgs_abi_version() == 4


def test_kernel_file_is_built_with_the_blend_kernels_flags():
    assert "render_depth.hip" in build.SOURCES
    assert build.SOURCES["render_depth.hip"] == build.SOURCES["render.hip"]
    assert any(h.endswith("render_common.hpp") for h in build.HEADERS)       # a change of the shared helpers rebuilds both


B = 0x1000          # a non-NULL "buffer": the calls below must fail before anything dereferences it
INVALID = [
    ("W", dict(W=0), "W and H must be positive"),
    ("H", dict(H=-3), "W and H must be positive"),
    ("P", dict(P=-1), "P and R must be >= 0"),
    ("R", dict(R=-1), "P and R must be >= 0"),
    ("outputs", dict(depth=None, alpha=None, median=None), "at least one output is required"),
    ("geom", dict(geom=None), "geometry, binning and image buffers are required"),
    ("binning", dict(binning=None), "geometry, binning and image buffers are required"),
    ("image", dict(image=None), "geometry, binning and image buffers are required"),
    ("instances_of_nothing", dict(P=0), "R > 0 instances cannot come from P = 0"),
]


@pytest.mark.parametrize("what,change,message", INVALID, ids=[c[0] for c in INVALID])
def test_invalid_arguments_return_1_with_a_message(L, what, change, message):
    a = dict(P=10, W=32, H=32, R=5, geom=B, binning=B, image=B, depth=B, alpha=B, median=B)
    a.update(change)
    rc = L.c3dgs_render_depth(a["P"], a["W"], a["H"], a["R"], a["geom"], a["binning"], a["image"], a["depth"], a["alpha"],
                              a["median"], None)
    assert rc == 1
    msg = L.c3dgs_last_error().decode()
    assert msg.startswith("render_depth: ") and message in msg, msg
