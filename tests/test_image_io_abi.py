"""CPU: c3dgs_image_from_u8 is exported and bound, and refuses every invalid argument its header lists before any device work
(so this runs without a GPU)."""
import ctypes as C

import pytest


@pytest.fixture(scope="module")
def L():
    from c3dgs_amd import build, _lib
    build.build()
    return _lib.lib()


def test_symbol_is_exported_bound_and_built_without_contraction(L):
    from c3dgs_amd import _lib, build
    assert hasattr(L, "c3dgs_image_from_u8") and "c3dgs_image_from_u8" in _lib.PROTOTYPES
    assert build.SOURCES["image_io.hip"] == ["-ffp-contract=off"]
    assert L.c3dgs_abi_version() == 4                       # a new entry point only


def test_invalid_arguments_are_refused_before_any_launch(L):
    fake = C.c_void_p(4096)

    def call(Hs=4, Ws=4, Cn=3, src=fake, flip=0, bg=None, Hd=4, Wd=4, out=fake):
        return L.c3dgs_image_from_u8(Hs, Ws, Cn, src, flip, bg, Hd, Wd, out, None)

    assert call(src=None) == 1 and b"NULL buffer" in L.c3dgs_last_error()
    assert call(out=None) == 1 and b"NULL buffer" in L.c3dgs_last_error()
    for Cn in (0, 1, 2, 5, -3):
        assert call(Cn=Cn) == 1 and b"C must be 3 or 4" in L.c3dgs_last_error(), Cn
    assert call(Cn=3, bg=fake) == 1 and b"alpha" in L.c3dgs_last_error()
    for name in ("Hs", "Ws", "Hd", "Wd"):
        for bad in (0, -1, 32769, 2 ** 31 - 1):
            assert call(**{name: bad}) == 1, (name, bad)
            assert b"[1, 32768]" in L.c3dgs_last_error(), (name, bad)
