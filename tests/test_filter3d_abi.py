"""CPU: the C ABI of the 3D smoothing filter's entries (c3dgs_filter3d_workspace_bytes, _compute, _apply, _apply_backward;
csrc/filter3d.hip). The symbols are exported and bound, the ABI version did not move (new entry points only, the raster structs
unchanged), the kernel's file is built with preprocess.hip's flags, the three stages have names, every invalid call is refused
with its message before anything is dereferenced -- which is why these run without a GPU -- and P == 0 / n == 0 launch nothing."""
import ctypes as C

import pytest

from c3dgs_amd import _lib, build


@pytest.fixture(scope="module")
def L():
    return _lib.lib()


def test_symbols_are_exported_and_bound(L):
    vp = C.c_void_p
    for name in ("c3dgs_filter3d_workspace_bytes", "c3dgs_filter3d_compute", "c3dgs_filter3d_apply", "c3dgs_filter3d_apply_backward"):
        assert hasattr(L, name), name
    assert _lib.PROTOTYPES["c3dgs_filter3d_workspace_bytes"] == (C.c_size_t, [C.c_int32])
    assert _lib.PROTOTYPES["c3dgs_filter3d_compute"] == (C.c_int, [C.c_int32, C.c_int32, vp, vp, vp, vp, vp, C.c_size_t, vp])
    assert _lib.PROTOTYPES["c3dgs_filter3d_apply"] == (C.c_int, [C.POINTER(_lib.Filter3DRows), vp, vp, vp])
    assert _lib.PROTOTYPES["c3dgs_filter3d_apply_backward"] == (C.c_int, [C.POINTER(_lib.Filter3DRows),
                                                                         C.POINTER(_lib.Filter3DGrads), vp])
    assert L.c3dgs_abi_version() == 4
    assert C.sizeof(_lib.RasterParams) == 7 * 4 + 4 + 14 * 8 + 3 * 4 + 3 * 4        # c3dgs_raster_params as it was
    assert C.sizeof(_lib.RasterGrads) == 9 * 8
    assert C.sizeof(_lib.Filter3DRows) == 2 * 4 + 9 * 8 + 4 + 4                     # two ints, nine pointers, a float, padding
    assert C.sizeof(_lib.Filter3DGrads) == 6 * 8
    assert L.c3dgs_filter3d_workspace_bytes(1000) >= 8


def test_kernel_file_is_built_with_preprocess_flags():
    assert build.SOURCES["filter3d.hip"] == build.SOURCES["preprocess.hip"] == ["-ffp-contract=off"]


def test_stage_names(L):
    try:
        for name in (b"filter3d_compute", b"filter3d_apply", b"filter3d_apply_backward", b"preprocess"):
            assert L.c3dgs_profile_only(name) == 0, name
        assert L.c3dgs_profile_only(b"filter3d") == 1
    finally:
        assert L.c3dgs_profile_only(None) == 0


B = 0x1000          # a non-NULL, 8-byte aligned "buffer": the calls below must fail before anything dereferences it


def _compute(L, P=10, Cn=3, xyz=B, cams=B, out=B, seen=B, ws=B, ws_bytes=256):
    return L.c3dgs_filter3d_compute(P, Cn, xyz, cams, out, seen, ws, ws_bytes, None)


COMPUTE = [
    ("negative_P", dict(P=-1), "P must be >= 0"),
    ("no_camera", dict(Cn=0), "C must be positive"),
    ("no_camera_no_rows", dict(P=0, Cn=0), "C must be positive"),
    ("xyz", dict(xyz=None), "xyz, cameras and filter_3D"),
    ("cameras", dict(cams=None), "xyz, cameras and filter_3D"),
    ("filter_3D", dict(out=None), "xyz, cameras and filter_3D"),
    ("workspace", dict(ws=None), "workspace"),
    ("workspace_small", dict(ws_bytes=4), "workspace"),
    ("workspace_misaligned", dict(ws=B + 4), "workspace"),
]


@pytest.mark.parametrize("what,kw,message", COMPUTE, ids=[c[0] for c in COMPUTE])
def test_invalid_compute_is_refused(L, what, kw, message):
    assert _compute(L, **kw) == 1, what
    assert message in L.c3dgs_last_error().decode(), L.c3dgs_last_error()


def test_compute_nothing_to_do_returns_0(L):
    assert _compute(L, P=0, xyz=None, cams=None, out=None, seen=None, ws=None, ws_bytes=0) == 0


def _rows(indexed=False, **kw):
    r = _lib.Filter3DRows()
    r.n, r.P_model, r.scale_modifier = 10, 0, 1.0
    for k in ("opacities", "scales", "rotations", "filter_3D"):
        setattr(r, k, B)
    if indexed:
        r.g_indices = r.scale_factors = B
    for k, v in kw.items():
        setattr(r, k, v)
    return r


def _grads(**kw):
    g = _lib.Filter3DGrads()
    for n, _ in _lib.Filter3DGrads._fields_:
        setattr(g, n, B)
    for k, v in kw.items():
        setattr(g, k, v)
    return g


def _apply(L, r, cov=B, opac=B):
    return L.c3dgs_filter3d_apply(C.byref(r) if r is not None else None, cov, opac, None)


def _backward(L, r, g="default"):
    g = _grads() if g == "default" else g
    return L.c3dgs_filter3d_apply_backward(C.byref(r) if r is not None else None, C.byref(g) if g is not None else None, None)


SHARED = [
    ("rows", None, "rows is NULL"),
    ("negative_n", _rows(n=-1), "n must be >= 0"),
    ("g_indices_without_scale_factors", _rows(True, scale_factors=None), "g_indices need scale_factors"),
    ("visible_without_rank", _rows(visible=B), "visible needs rank"),
    ("visible_negative_P", _rows(visible=B, rank=B, P_model=-1), "visible needs rank"),
    ("opacities", _rows(opacities=None), "opacities, scales, rotations (unless cov3D_precomp is given) and filter_3D"),
    ("scales", _rows(scales=None), "opacities, scales, rotations (unless cov3D_precomp is given) and filter_3D"),
    ("scales_with_cov3D", _rows(scales=None, cov3D_precomp=B), "opacities, scales, rotations (unless cov3D_precomp is given) and filter_3D"),
    ("rotations", _rows(True, rotations=None), "opacities, scales, rotations (unless cov3D_precomp is given) and filter_3D"),
    ("filter_3D", _rows(filter_3D=None), "opacities, scales, rotations (unless cov3D_precomp is given) and filter_3D"),
    ("rotations_misaligned", _rows(rotations=B + 8), "rotations must be 16-byte aligned"),
]


@pytest.mark.parametrize("what,r,message", SHARED, ids=[c[0] for c in SHARED])
def test_invalid_rows_are_refused_by_both_entries(L, what, r, message):
    for call in (_apply, _backward):
        assert call(L, r) == 1, what
        assert message in L.c3dgs_last_error().decode(), L.c3dgs_last_error()


@pytest.mark.parametrize("indexed", [False, True])
def test_invalid_outputs_are_refused(L, indexed):
    assert _apply(L, _rows(indexed), cov=None) == 1 and "cov3D_out and opacity_out" in L.c3dgs_last_error().decode()
    assert _apply(L, _rows(indexed), opac=None) == 1 and "cov3D_out and opacity_out" in L.c3dgs_last_error().decode()
    assert _backward(L, _rows(indexed), g=None) == 1 and "grads is NULL" in L.c3dgs_last_error().decode()
    none = _grads(dL_dopacity=None, dL_dscales=None, dL_drotations=None, dL_dscale_factors=None)
    assert _backward(L, _rows(indexed), g=none) == 1 and "at least one output" in L.c3dgs_last_error().decode()
    assert _backward(L, _rows(indexed), g=_grads(dL_drotations=B + 4)) == 1 and "dL_drotations must be 16-byte aligned" in L.c3dgs_last_error().decode()


@pytest.mark.parametrize("indexed", [False, True])
def test_nothing_to_do_returns_0(L, indexed):
    bare = dict(n=0, opacities=None, scales=None, rotations=None, filter_3D=None)
    assert _apply(L, _rows(indexed, **bare), cov=None, opac=None) == 0
    assert _backward(L, _rows(indexed, **bare)) == 0
    # a caller's covariance: the rotations are not read and may be absent
    assert _apply(L, _rows(indexed, **dict(bare, cov3D_precomp=B)), cov=None, opac=None) == 0
