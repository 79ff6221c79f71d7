"""CPU: the C ABI of the antialiased mode's two entries (c3dgs_aa_opacity, c3dgs_aa_opacity_backward; csrc/aa_opacity.hip). The
symbols are exported and bound, the ABI version did not move (new entry points only, c3dgs_raster_params unchanged), the kernel's
file is built with preprocess.hip's flags, the two launches have stage names, every invalid call is refused with its message
before anything is dereferenced -- which is why these run without a GPU -- and P == 0 launches nothing."""
import ctypes as C

import pytest

from c3dgs_amd import _lib, build


@pytest.fixture(scope="module")
def L():
    return _lib.lib()


def test_symbols_are_exported_and_bound(L):
    assert hasattr(L, "c3dgs_aa_opacity") and hasattr(L, "c3dgs_aa_opacity_backward")
    vp = C.c_void_p
    assert _lib.PROTOTYPES["c3dgs_aa_opacity"] == (C.c_int, [C.POINTER(_lib.RasterParams), vp, vp, vp])
    assert _lib.PROTOTYPES["c3dgs_aa_opacity_backward"] == (C.c_int, [C.POINTER(_lib.RasterParams), vp, C.POINTER(_lib.RasterGrads), vp])
    assert L.c3dgs_abi_version() == 4
    assert C.sizeof(_lib.RasterParams) == 7 * 4 + 4 + 14 * 8 + 3 * 4 + 3 * 4        # c3dgs_raster_params as it was
    assert C.sizeof(_lib.RasterGrads) == 9 * 8


def test_kernel_file_is_built_with_preprocess_flags():
    assert "aa_opacity.hip" in build.SOURCES
    assert build.SOURCES["aa_opacity.hip"] == build.SOURCES["preprocess.hip"] == ["-ffp-contract=off"]


def test_stage_names(L):
    try:
        for name in (b"aa_opacity", b"aa_opacity_backward", b"preprocess", b"backward_preprocess"):
            assert L.c3dgs_profile_only(name) == 0, name
        assert L.c3dgs_profile_only(b"aa_opacity_forward") == 1
    finally:
        assert L.c3dgs_profile_only(None) == 0


B = 0x1000          # a non-NULL "buffer": the calls below must fail before anything dereferences it


def _params(form="sr", **kw):
    p = _lib.RasterParams()
    p.P, p.W, p.H = 10, 32, 32
    for k in ("means3D", "opacities", "viewmatrix"):
        setattr(p, k, B)
    if form == "sr":
        p.scales = p.rotations = B
    elif form == "indexed":
        p.scales = p.rotations = p.g_indices = p.scale_factors = B
    else:
        p.cov3D_precomp = B
    p.tan_fovx = p.tan_fovy = 0.5
    p.scale_modifier = 1.0
    for k, v in kw.items():
        setattr(p, k, v)
    return p


def _grads(**kw):
    g = _lib.RasterGrads()
    for n, _ in _lib.RasterGrads._fields_:
        setattr(g, n, B)
    for k, v in kw.items():
        setattr(g, k, v)
    return g


def _forward(L, p, out=B, rho=B):
    return L.c3dgs_aa_opacity(C.byref(p) if p is not None else None, out, rho, None)


def _backward(L, p, radii=B, g="default"):
    g = _grads() if g == "default" else g
    return L.c3dgs_aa_opacity_backward(C.byref(p) if p is not None else None, radii, C.byref(g) if g is not None else None, None)


# (id, params, message) refused by BOTH entries
SHARED = [
    ("params", None, "params is NULL"),
    ("negative_P", _params(P=-1), "P must be >= 0"),
    ("both_forms", _params(cov3D_precomp=B), "exactly one of"),
    ("neither_form", _params(scales=None, rotations=None), "exactly one of"),
    ("scales_alone", _params(rotations=None), "exactly one of"),
    ("rotations_alone", _params(scales=None), "exactly one of"),
    ("g_indices_without_scale_factors", _params("indexed", scale_factors=None), "g_indices need scale_factors"),
    ("W", _params(W=0), "W and H"),
    ("means3D", _params(means3D=None), "means3D"),
    ("opacities", _params(opacities=None), "opacities"),
    ("viewmatrix", _params(viewmatrix=None), "viewmatrix"),
]


@pytest.mark.parametrize("what,p,message", SHARED, ids=[c[0] for c in SHARED])
def test_invalid_params_are_refused_by_both_entries(L, what, p, message):
    for call in (_forward, _backward):
        assert call(L, p) == 1, what
        assert message in L.c3dgs_last_error().decode(), L.c3dgs_last_error()


@pytest.mark.parametrize("form", ["sr", "indexed", "cov"])
def test_invalid_outputs_are_refused(L, form):
    assert _forward(L, _params(form), out=None) == 1 and "opacity_out" in L.c3dgs_last_error().decode()
    assert _forward(L, _params(form, P=0), out=None) == 1 and "opacity_out" in L.c3dgs_last_error().decode()
    assert _backward(L, _params(form), g=None) == 1 and "grads is NULL" in L.c3dgs_last_error().decode()
    assert _backward(L, _params(form), g=_grads(dL_dopacity=None)) == 1 and "dL_dopacity" in L.c3dgs_last_error().decode()
    assert _backward(L, _params(form), radii=None) == 1 and "radii" in L.c3dgs_last_error().decode()
    rc = _backward(L, _params(form, P=0), g=_grads(dL_dcov3D=None))
    if form == "cov":
        assert rc == 1 and "dL_dcov3D" in L.c3dgs_last_error().decode()
    else:
        assert rc == 0                  # the covariance gradient is optional with scales and rotations


@pytest.mark.parametrize("form", ["sr", "indexed", "cov"])
def test_nothing_to_do_returns_0(L, form):
    # P == 0: nothing is launched and nothing dereferenced, whatever else is passed; rho stays optional
    bare = dict(P=0, W=0, H=0, means3D=None, opacities=None, viewmatrix=None)
    assert _forward(L, _params(form, **bare)) == 0
    assert _forward(L, _params(form, **bare), rho=None) == 0
    assert _backward(L, _params(form, **bare), radii=None) == 0
    only_opacity = _grads(**{n: None for n, _ in _lib.RasterGrads._fields_ if n not in ("dL_dopacity", "dL_dcov3D")})
    assert _backward(L, _params(form, **bare), radii=None, g=only_opacity) == 0
