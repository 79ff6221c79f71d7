"""CPU: the C ABI of the backward through the depth and alpha maps (c3dgs_rasterize_gaussians_backward_depth,
c3dgs_rasterize_gaussians_backward_depth_indexed, c3dgs_depth_backward_workspace_bytes; csrc/render_maps_backward.hip). The
symbols are exported and bound, the ABI version did not move (new entry points only, c3dgs_raster_params unchanged), the
kernel's file is built with render.hip's flags, the two new launches have stage names, the workspace is the backward's plus
the dL/dz plane, and every invalid call is refused with its message before any device work -- which is why these run without
a GPU."""
import ctypes as C

import pytest

from c3dgs_amd import _lib, build

ENTRIES = ("c3dgs_rasterize_gaussians_backward_depth", "c3dgs_rasterize_gaussians_backward_depth_indexed")


@pytest.fixture(scope="module")
def L():
    return _lib.lib()


def test_symbols_are_exported_and_bound(L):
    for name in ENTRIES:
        assert hasattr(L, name), name
        res, args = _lib.PROTOTYPES[name]
        plain = _lib.PROTOTYPES[name.replace("_depth", "")][1]
        assert res is C.c_int and len(args) == len(plain) + 2          # the plain backward's arguments + dL_ddepth, dL_dalpha
        assert args[:7] == plain[:7] and args[9:] == plain[7:] and args[7] is C.c_void_p and args[8] is C.c_void_p
    assert hasattr(L, "c3dgs_depth_backward_workspace_bytes")
    assert _lib.PROTOTYPES["c3dgs_depth_backward_workspace_bytes"] == (C.c_size_t, [C.c_int32, C.c_int32])
    assert L.c3dgs_abi_version() == 4
    assert C.sizeof(_lib.RasterParams) == 7 * 4 + 4 + 14 * 8 + 3 * 4 + 3 * 4        # c3dgs_raster_params as it was


def test_kernel_file_is_built_with_the_blend_kernels_flags():
    assert "render_maps_backward.hip" in build.SOURCES
    assert build.SOURCES["render_maps_backward.hip"] == build.SOURCES["render.hip"] == build.SOURCES["render_depth.hip"]


def test_stage_names(L):
    try:
        for name in (b"render_depth_backward", b"depth_backward_fold", b"render_backward", b"backward_preprocess"):
            assert L.c3dgs_profile_only(name) == 0, name
    finally:
        assert L.c3dgs_profile_only(None) == 0


def test_workspace_is_the_backwards_plus_the_dz_plane(L):
    for P in (0, 1, 1024, 1025, 3_000_000):
        prev = 0
        for R in (0, 1, 2, 63, 64, 255, 256, 257, 4096, 100_000, 16_400_000, 2**31 - 1):
            b = L.c3dgs_depth_backward_workspace_bytes(P, R)
            plain = L.c3dgs_backward_workspace_bytes(P, R)
            assert b >= plain + 4 * max(R, 1), (P, R, b, plain)
            assert b <= plain + 4 * max(R, 1) + 256 and b % 256 == 0       # one 256-byte aligned region behind the plain layout
            assert b >= prev, (P, R)                                        # monotone in R
            prev = b
        assert L.c3dgs_depth_backward_workspace_bytes(P, 0) == L.c3dgs_depth_backward_workspace_bytes(P, 1)


B = 0x1000          # a non-NULL "buffer": the calls below must fail before anything dereferences it


def _params(**kw):
    p = _lib.RasterParams()
    p.P, p.D, p.M, p.W, p.H = 10, 0, 0, 32, 32
    for k in ("background", "means3D", "colors_precomp", "opacities", "scales", "rotations", "viewmatrix", "projmatrix", "campos"):
        setattr(p, k, B)
    p.tan_fovx = p.tan_fovy = 0.5
    p.scale_modifier = 1.0
    for k, v in kw.items():
        setattr(p, k, v)
    return p


@_lib.RESIZE_FN
def _never(_user, _nbytes):          # a workspace callback that must not be reached
    raise AssertionError("the workspace was requested for an invalid call")


def _call(L, entry, p, *, radii=B, geom=B, binning=B, image=B, R=5, dpix=B, ddepth=B, dalpha=B, ws=_never, grads=True):
    g = _lib.RasterGrads()
    return getattr(L, entry)(C.byref(p) if p is not None else None, radii, geom, binning, image, R, dpix, ddepth, dalpha, ws, None,
                             C.byref(g) if grads else None, None)


def _indexed(entry, p):
    if entry.endswith("_indexed"):
        p.sh_indices = p.g_indices = p.scale_factors = B
    return p


INVALID = [
    ("params", dict(p=None), "params is NULL"),
    ("negative_P", dict(pk=dict(P=-1)), "P, W, H must be"),
    ("W", dict(pk=dict(W=0)), "P, W, H must be"),
    ("H", dict(pk=dict(H=-2)), "P, W, H must be"),
    ("means3D", dict(pk=dict(means3D=None)), "means3D"),
    ("camera", dict(pk=dict(viewmatrix=None)), "viewmatrix"),
    ("grads", dict(grads=False), "grads is NULL"),
    ("radii", dict(radii=None), "forward buffers"),
    ("geom", dict(geom=None), "forward buffers"),
    ("image", dict(image=None), "forward buffers"),
    ("binning", dict(binning=None), "forward buffers"),
    ("nothing_to_differentiate", dict(dpix=None, ddepth=None, dalpha=None), "dL_dout_color"),
    ("workspace", dict(ws=C.cast(None, _lib.RESIZE_FN)), "workspace callback is required"),
    ("negative_R", dict(R=-1), "R must be >= 0"),
]


@pytest.mark.parametrize("entry", ENTRIES)
@pytest.mark.parametrize("what,change,message", INVALID, ids=[c[0] for c in INVALID])
def test_invalid_arguments_are_refused_before_any_launch(L, entry, what, change, message):
    change = dict(change)
    p = _indexed(entry, _params(**change.pop("pk", {}))) if "p" not in change else change.pop("p")
    rc = _call(L, entry, p, **change)
    assert rc == 1, what
    assert message in L.c3dgs_last_error().decode(), L.c3dgs_last_error()


@pytest.mark.parametrize("entry", ENTRIES)
def test_nothing_to_do_returns_0(L, entry):
    # P == 0: nothing to differentiate, whatever else is passed (the plain backward's rule), no workspace request
    assert _call(L, entry, _indexed(entry, _params(P=0)), radii=None, geom=None, binning=None, image=None, R=0) == 0
    assert _call(L, entry, _indexed(entry, _params(P=0)), radii=None, geom=None, binning=None, image=None, R=0, dpix=None) == 0
