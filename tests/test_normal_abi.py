"""CPU: the C ABI of the normal maps (c3dgs_gaussian_normals, c3dgs_render_normal, c3dgs_rasterize_gaussians_backward_normal(_indexed),
c3dgs_normal_backward_workspace_bytes, c3dgs_depth_to_normal, c3dgs_depth_to_normal_backward; csrc/normals.hip,
csrc/render_normal.hip, csrc/render_maps_backward.hip). The symbols are exported and bound, the header names them, the ABI
version did not move (new entry points only), the kernel files are built with their siblings' flags, the new launches have stage
names, the workspace is the depth backward's plus three floats per slot, and every invalid call is refused with its message before
any device work -- which is why these run without a GPU."""
import ctypes as C
import os

import pytest

from c3dgs_amd import _lib, build

BWD = ("c3dgs_rasterize_gaussians_backward_normal", "c3dgs_rasterize_gaussians_backward_normal_indexed")
OTHERS = ("c3dgs_gaussian_normals", "c3dgs_render_normal", "c3dgs_normal_backward_workspace_bytes", "c3dgs_depth_to_normal",
          "c3dgs_depth_to_normal_backward")
STAGES = (b"gaussian_normals", b"render_normal", b"render_normal_backward", b"normal_backward_fold", b"depth_to_normal",
          b"depth_to_normal_backward")


@pytest.fixture(scope="module")
def L():
    return _lib.lib()


def test_symbols_are_exported_and_bound(L):
    for name in BWD:
        assert hasattr(L, name), name
        res, args = _lib.PROTOTYPES[name]
        dist = _lib.PROTOTYPES[name.replace("_normal", "_distortion")][1]
        # the *_backward_distortion arguments with dL_dnormal, normals and the three axes arguments behind the two depth maps
        assert res is C.c_int and len(args) == len(dist) + 5
        assert args[:9] == dist[:9] and args[9:14] == [C.c_void_p] * 5 and args[14:] == dist[9:]
    for name in OTHERS:
        assert hasattr(L, name) and name in _lib.PROTOTYPES, name
    assert _lib.PROTOTYPES["c3dgs_gaussian_normals"] == (C.c_int, [C.c_int32] + [C.c_void_p] * 7)
    assert _lib.PROTOTYPES["c3dgs_render_normal"] == (C.c_int, [C.c_int32] * 4 + [C.c_void_p] * 6)
    assert _lib.PROTOTYPES["c3dgs_depth_to_normal"] == (C.c_int, [C.c_int32] * 2 + [C.c_void_p] + [C.c_float] * 2 + [C.c_void_p] * 2)
    assert _lib.PROTOTYPES["c3dgs_depth_to_normal_backward"] == (C.c_int, [C.c_int32] * 2 + [C.c_void_p] * 2 + [C.c_float] * 2 +
                                                                  [C.c_void_p] * 2)
    assert L.c3dgs_abi_version() == 4
    assert C.sizeof(_lib.RasterParams) == 7 * 4 + 4 + 14 * 8 + 3 * 4 + 3 * 4        # c3dgs_raster_params as it was


def test_header_names_the_entries():
    with open(os.path.join(os.path.dirname(build.HERE), "include", "c3dgs_hip.h")) as fh:
        text = fh.read()
    for name in BWD + OTHERS:
        assert f" {name}(" in text, name
    assert "#define C3DGS_ABI_VERSION 4" in text
    for stage in STAGES:
        assert f'"{stage.decode()}"' in text, stage


def test_kernel_files_and_flags():
    for src in ("render_normal.hip", "render_maps_backward.hip"):
        assert src in build.SOURCES and os.path.exists(os.path.join(build.CSRC, src)), src
        assert build.SOURCES[src] == build.SOURCES["render.hip"] == build.SOURCES["render_depth.hip"]
    # the per-Gaussian chains of gsgrad.hpp are compiled as everywhere else they are called
    assert build.SOURCES["normals.hip"] == ["-ffp-contract=off"] == build.SOURCES["filter3d.hip"]


def test_stage_names(L):
    try:
        for name in STAGES + (b"render_depth_backward", b"render_distortion_backward", b"depth_backward_fold"):
            assert L.c3dgs_profile_only(name) == 0, name
        assert L.c3dgs_profile_only(b"render_normals") == 1                      # not a stage
    finally:
        assert L.c3dgs_profile_only(None) == 0


def test_workspace_is_the_depth_backwards_plus_three_floats_per_slot(L):
    for P in (0, 1, 1024, 1025, 3_000_000):
        for R in (0, 1, 2, 63, 64, 255, 256, 257, 4096, 100_000, 16_400_000, 2**31 - 1):
            base, got = L.c3dgs_depth_backward_workspace_bytes(P, R), L.c3dgs_normal_backward_workspace_bytes(P, R)
            assert base % 256 == 0 and got % 256 == 0
            assert 12 * max(R, 1) <= got - base < 12 * max(R, 1) + 256, (P, R)


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


def _call(L, entry, p, *, radii=B, geom=B, binning=B, image=B, R=5, dpix=B, ddepth=B, dalpha=B, dnormal=B, normals=B, axes=None,
          axes_gi=None, daxes=None, ddist=None, moment=None, near=0.0, far=0.0, ws=_never, grads=True):
    g = _lib.RasterGrads()
    return getattr(L, entry)(C.byref(p) if p is not None else None, radii, geom, binning, image, R, dpix, ddepth, dalpha, dnormal,
                             normals, axes, axes_gi, daxes, ddist, moment, near, far, ws, None, C.byref(g) if grads else None, None)


INVALID = [
    ("params", dict(p=None), "params is NULL"),
    ("negative_P", dict(pk=dict(P=-1)), "P, W, H must be"),
    ("grads", dict(grads=False), "grads is NULL"),
    ("radii", dict(radii=None), "forward buffers"),
    ("binning", dict(binning=None), "forward buffers"),
    ("nothing_to_differentiate", dict(dpix=None, ddepth=None, dalpha=None, dnormal=None), "dL_dout_color"),
    ("workspace_normal_alone", dict(ws=C.cast(None, _lib.RESIZE_FN), dpix=None, ddepth=None, dalpha=None), "workspace callback is required"),
    ("normals_missing", dict(normals=None), "normals is required"),
    ("covariance", dict(pk=dict(cov3D_precomp=B, scales=None, rotations=None)), "no axes"),
    ("axes_without_their_gradient", dict(axes=B), "dL_daxes_rotations is required"),
    ("covariance_with_axes_reaches_the_workspace", dict(pk=dict(cov3D_precomp=B, scales=None, rotations=None), axes=B, daxes=B,
                                                         ws=C.cast(None, _lib.RESIZE_FN)), "workspace callback is required"),
    ("moment_missing", dict(ddist=B), "moment is required"),
    ("near_far", dict(ddist=B, moment=B, near=2.0, far=1.0), "0 < near < far"),
]


@pytest.mark.parametrize("entry", BWD)
@pytest.mark.parametrize("label,kw,message", INVALID, ids=[c[0] for c in INVALID])
def test_backward_refuses_invalid_calls_before_any_device_work(L, entry, label, kw, message):
    kw = dict(kw)
    p = kw.pop("p", "default")
    if p == "default":
        p = _params(**kw.pop("pk", {}))
        if entry.endswith("_indexed"):
            p.sh_indices = p.g_indices = p.scale_factors = B
    assert _call(L, entry, p, **kw) == 1
    assert message.encode() in L.c3dgs_last_error(), L.c3dgs_last_error()


def test_without_the_normal_gradient_the_normals_are_not_looked_at(L):
    """dL_dnormal NULL: the *_backward_distortion entry's validation, whatever `normals` is"""
    for entry in BWD:
        p = _params()
        if entry.endswith("_indexed"):
            p.sh_indices = p.g_indices = p.scale_factors = B
        assert _call(L, entry, p, dnormal=None, normals=None, ws=C.cast(None, _lib.RESIZE_FN)) == 1
        assert b"workspace callback is required" in L.c3dgs_last_error()


def test_the_other_entries_validate(L):
    assert L.c3dgs_gaussian_normals(0, None, None, None, None, None, None, None) == 0           # nothing to do
    assert L.c3dgs_gaussian_normals(-1, B, B, B, None, B, B, None) == 1 and b"P must be" in L.c3dgs_last_error()
    for k in (1, 2, 3, 5, 6):                                   # g_indices (4) is optional
        a = [B] * 7
        a[k - 1] = None
        assert L.c3dgs_gaussian_normals(4, *a, None) == 1 and b"are required" in L.c3dgs_last_error(), k
    assert L.c3dgs_render_normal(4, 0, 8, 1, B, B, B, B, B, None) == 1 and b"W and H" in L.c3dgs_last_error()
    assert L.c3dgs_render_normal(4, 8, 8, -1, B, B, B, B, B, None) == 1 and b"P and R" in L.c3dgs_last_error()
    assert L.c3dgs_render_normal(4, 8, 8, 1, B, B, B, B, None, None) == 1 and b"out_normal is required" in L.c3dgs_last_error()
    assert L.c3dgs_render_normal(0, 8, 8, 1, B, B, B, B, B, None) == 1 and b"cannot come from P = 0" in L.c3dgs_last_error()
    assert L.c3dgs_render_normal(4, 8, 8, 1, B, B, B, None, B, None) == 1 and b"normals are required" in L.c3dgs_last_error()
    assert L.c3dgs_depth_to_normal(0, 4, B, 0.5, 0.5, B, None) == 1 and b"W and H" in L.c3dgs_last_error()
    assert L.c3dgs_depth_to_normal(4, 4, B, 0.0, 0.5, B, None) == 1 and b"tan_fovx" in L.c3dgs_last_error()
    assert L.c3dgs_depth_to_normal(4, 4, None, 0.5, 0.5, B, None) == 1 and b"are required" in L.c3dgs_last_error()
    assert L.c3dgs_depth_to_normal_backward(4, 4, B, None, 0.5, 0.5, B, None) == 1 and b"are required" in L.c3dgs_last_error()
    assert L.c3dgs_depth_to_normal_backward(4, 4, B, B, 0.5, float("nan"), B, None) == 1 and b"tan_fovx" in L.c3dgs_last_error()


def test_python_surface_without_a_gpu():
    """the settings attribute and the refusals that need no device"""
    import torch
    from c3dgs_amd import rasterizer as rz
    rs = rz.GaussianRasterizationSettings(intrinsic=torch.eye(3), extrinsic_vector=torch.zeros(7), bg=torch.zeros(3), scale_modifier=1.0,
                                          sh_degree=0, prefiltered=False, debug=False, clamp_color=True, normal=True)
    assert rs.normal is True and "normal" not in rs._fields and len(rs) == 9
    assert rs._replace(scale_modifier=2.0).normal is True and rs._replace(normal=False).normal is False
    assert rz.GaussianRasterizationSettings(*rs).normal is False
    for cls, mode in ((rz.GaussianRasterizer, "exact"), (rz.GaussianRasterizerIndexed, True), (rz.GaussianRasterizerIndexed, "exact")):
        with pytest.raises(ValueError, match="normal"):
            cls(rs, optimize_camera=mode)
    for fn in ("gaussian_normals", "render_normal"):
        assert callable(getattr(rz._C, fn))
    from c3dgs_amd import normals
    assert callable(normals.depth_to_normal) and callable(normals.normal_consistency)
    with pytest.raises(RuntimeError, match="GPU"):
        normals.depth_to_normal(torch.zeros(4, 4), torch.eye(3))
