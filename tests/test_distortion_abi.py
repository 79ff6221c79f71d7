"""CPU: the C ABI of the depth-distortion map and its backward (c3dgs_render_distortion,
c3dgs_rasterize_gaussians_backward_distortion, c3dgs_rasterize_gaussians_backward_distortion_indexed,
c3dgs_distortion_backward_workspace_bytes; csrc/render_distortion.hip, csrc/render_maps_backward.hip). The symbols are
exported and bound, the header names them, the ABI version did not move (new entry points only), the two kernel files are built
with render.hip's flags, the two new launches have stage names, the workspace is the depth backward's, and every invalid call is
refused with its message before any device work -- which is why these run without a GPU."""
import ctypes as C
import os

import pytest

from c3dgs_amd import _lib, build

BWD = ("c3dgs_rasterize_gaussians_backward_distortion", "c3dgs_rasterize_gaussians_backward_distortion_indexed")
NAN = float("nan")


@pytest.fixture(scope="module")
def L():
    return _lib.lib()


def test_symbols_are_exported_and_bound(L):
    for name in BWD:
        assert hasattr(L, name), name
        res, args = _lib.PROTOTYPES[name]
        depth = _lib.PROTOTYPES[name.replace("_distortion", "_depth")][1]
        # the *_backward_depth arguments + dL_ddistortion, moment, near, far behind the two maps
        assert res is C.c_int and len(args) == len(depth) + 4
        assert args[:9] == depth[:9] and args[13:] == depth[9:]
        assert args[9:13] == [C.c_void_p, C.c_void_p, C.c_float, C.c_float]
    assert hasattr(L, "c3dgs_render_distortion") and hasattr(L, "c3dgs_distortion_backward_workspace_bytes")
    res, args = _lib.PROTOTYPES["c3dgs_render_distortion"]
    assert res is C.c_int and args == [C.c_int32] * 4 + [C.c_void_p] * 3 + [C.c_float] * 2 + [C.c_void_p] * 3
    assert _lib.PROTOTYPES["c3dgs_distortion_backward_workspace_bytes"] == (C.c_size_t, [C.c_int32, C.c_int32])
    assert L.c3dgs_abi_version() == 4
    assert C.sizeof(_lib.RasterParams) == 7 * 4 + 4 + 14 * 8 + 3 * 4 + 3 * 4        # c3dgs_raster_params as it was


def test_header_names_the_entries():
    with open(os.path.join(os.path.dirname(build.HERE), "include", "c3dgs_hip.h")) as fh:
        text = fh.read()
    for name in BWD + ("c3dgs_render_distortion", "c3dgs_distortion_backward_workspace_bytes"):
        assert f" {name}(" in text, name
    assert "#define C3DGS_ABI_VERSION 4" in text
    for stage in ('"render_distortion"', '"render_distortion_backward"'):
        assert stage in text, stage


def test_kernel_files_are_built_with_the_blend_kernels_flags():
    for src in ("render_distortion.hip", "render_maps_backward.hip"):
        assert src in build.SOURCES and os.path.exists(os.path.join(build.CSRC, src)), src
        assert build.SOURCES[src] == build.SOURCES["render.hip"] == build.SOURCES["render_depth.hip"]


def test_stage_names(L):
    try:
        for name in (b"render_distortion", b"render_distortion_backward", b"render_depth", b"render_depth_backward",
                     b"depth_backward_fold"):
            assert L.c3dgs_profile_only(name) == 0, name
        assert L.c3dgs_profile_only(b"render_distortion_forward") == 1          # not a stage
    finally:
        assert L.c3dgs_profile_only(None) == 0


def test_workspace_is_the_depth_backwards(L):
    for P in (0, 1, 1024, 1025, 3_000_000):
        for R in (0, 1, 2, 63, 64, 255, 256, 257, 4096, 100_000, 16_400_000, 2**31 - 1):
            assert L.c3dgs_distortion_backward_workspace_bytes(P, R) == L.c3dgs_depth_backward_workspace_bytes(P, R), (P, R)


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


def _call(L, entry, p, *, radii=B, geom=B, binning=B, image=B, R=5, dpix=B, ddepth=B, dalpha=B, ddist=B, moment=B, near=0.0, far=0.0,
          ws=_never, grads=True):
    g = _lib.RasterGrads()
    return getattr(L, entry)(C.byref(p) if p is not None else None, radii, geom, binning, image, R, dpix, ddepth, dalpha, ddist, moment,
                             near, far, ws, None, C.byref(g) if grads else None, None)


def _indexed(entry, p):
    if entry.endswith("_indexed"):
        p.sh_indices = p.g_indices = p.scale_factors = B
    return p


INVALID = [
    # the *_backward_depth entries' own cases, with and without the distortion map
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
    ("nothing_to_differentiate", dict(dpix=None, ddepth=None, dalpha=None, ddist=None), "dL_dout_color"),
    ("workspace", dict(ws=C.cast(None, _lib.RESIZE_FN)), "workspace callback is required"),
    ("workspace_distortion_alone", dict(ws=C.cast(None, _lib.RESIZE_FN), dpix=None, ddepth=None, dalpha=None),
     "workspace callback is required"),
    ("negative_R", dict(R=-1), "R must be >= 0"),
    # the distortion map's own
    ("moment", dict(moment=None), "moment is required"),
    ("near_zero", dict(near=0.0, far=100.0), "0 < near < far"),
    ("near_negative", dict(near=-0.2, far=100.0), "0 < near < far"),
    ("near_equals_far", dict(near=5.0, far=5.0), "0 < near < far"),
    ("near_above_far", dict(near=7.0, far=5.0), "0 < near < far"),
    ("near_nan", dict(near=NAN, far=100.0), "0 < near < far"),
    ("far_nan", dict(near=0.2, far=NAN), "0 < near < far"),
]


@pytest.mark.parametrize("entry", BWD)
@pytest.mark.parametrize("what,change,message", INVALID, ids=[c[0] for c in INVALID])
def test_invalid_backward_arguments_are_refused_before_any_launch(L, entry, what, change, message):
    change = dict(change)
    p = _indexed(entry, _params(**change.pop("pk", {}))) if "p" not in change else change.pop("p")
    rc = _call(L, entry, p, **change)
    assert rc == 1, what
    assert message in L.c3dgs_last_error().decode(), L.c3dgs_last_error()


@pytest.mark.parametrize("entry", BWD)
def test_without_the_distortion_gradient_its_arguments_are_not_looked_at(L, entry):
    """dL_ddistortion NULL: the call is the *_backward_depth call, so a missing moment or a near / far that no mode accepts is no
    error of its own -- the call gets as far as that entry gets (here: refused for its missing radii, or done for P == 0)"""
    for kw in (dict(moment=None), dict(near=7.0, far=5.0), dict(near=NAN, far=NAN)):
        assert _call(L, entry, _indexed(entry, _params()), ddist=None, radii=None, **kw) == 1
        assert "forward buffers" in L.c3dgs_last_error().decode()
        assert _call(L, entry, _indexed(entry, _params(P=0)), ddist=None, radii=None, geom=None, binning=None, image=None, R=0, **kw) == 0


@pytest.mark.parametrize("entry", BWD)
def test_nothing_to_do_returns_0(L, entry):
    assert _call(L, entry, _indexed(entry, _params(P=0)), radii=None, geom=None, binning=None, image=None, R=0) == 0
    assert _call(L, entry, _indexed(entry, _params(P=0)), radii=None, geom=None, binning=None, image=None, R=0, dpix=None,
                 near=0.2, far=100.0) == 0


def _render(L, *, P=10, W=32, H=32, R=5, geom=B, binning=B, image=B, near=0.0, far=0.0, out=B, moment=B):
    return L.c3dgs_render_distortion(P, W, H, R, geom, binning, image, near, far, out, moment, None)


RENDER_INVALID = [
    ("W", dict(W=0), "W and H must be positive"),
    ("H", dict(H=-1), "W and H must be positive"),
    ("negative_P", dict(P=-1), "P and R must be >= 0"),
    ("negative_R", dict(R=-1), "P and R must be >= 0"),
    ("no_output", dict(out=None), "out_distortion is required"),
    ("moment_alone", dict(out=None, moment=B), "out_distortion is required"),
    ("near_zero", dict(near=0.0, far=100.0), "0 < near < far"),
    ("near_negative", dict(near=-1.0, far=100.0), "0 < near < far"),
    ("near_equals_far", dict(near=3.0, far=3.0), "0 < near < far"),
    ("near_above_far", dict(near=4.0, far=3.0), "0 < near < far"),
    ("near_nan", dict(near=NAN, far=100.0), "0 < near < far"),
    ("far_nan", dict(near=0.2, far=NAN), "0 < near < far"),
    ("R_without_P", dict(P=0, R=5), "cannot come from P = 0"),
    ("geom", dict(geom=None), "buffers are required"),
    ("binning", dict(binning=None), "buffers are required"),
    ("image", dict(image=None), "buffers are required"),
]


@pytest.mark.parametrize("what,change,message", RENDER_INVALID, ids=[c[0] for c in RENDER_INVALID])
def test_invalid_render_distortion_arguments_are_refused_before_any_launch(L, what, change, message):
    assert _render(L, **change) == 1, what
    assert message in L.c3dgs_last_error().decode(), L.c3dgs_last_error()
