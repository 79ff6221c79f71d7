"""CPU: the C ABI of the mesh extraction (c3dgs_tsdf_integrate, c3dgs_mesh_extract_workspace_bytes, c3dgs_mesh_extract_count,
c3dgs_mesh_extract_emit; csrc/mesh.hip). The symbols are exported and bound, the header names them, the ABI version did not move
(new entry points only), mesh.hip is built without contraction, the launches have stage names, the workspace is about five bytes
a point, and every invalid call is refused with its message before any device work -- which is why these run without a GPU."""
import ctypes as C
import math
import os

import pytest

from c3dgs_amd import _lib, build

ENTRIES = ("c3dgs_tsdf_integrate", "c3dgs_mesh_extract_workspace_bytes", "c3dgs_mesh_extract_count", "c3dgs_mesh_extract_emit")
STAGES = (b"tsdf_integrate", b"mesh_classify", b"mesh_scan", b"mesh_emit_vertices", b"mesh_emit_faces")
B = 0x1000          # a non-NULL "buffer": the calls below must fail before anything dereferences it
INF = math.inf


@pytest.fixture(scope="module")
def L():
    return _lib.lib()


def test_symbols_are_exported_and_bound(L):
    vp = C.c_void_p
    for name in ENTRIES:
        assert hasattr(L, name) and name in _lib.PROTOTYPES, name
    assert _lib.PROTOTYPES["c3dgs_tsdf_integrate"] == (C.c_int, [C.POINTER(_lib.Lattice)] + [C.c_int32] * 3 + [vp] * 3 +
                                                       [C.c_float] * 3 + [vp] * 4)
    assert _lib.PROTOTYPES["c3dgs_mesh_extract_workspace_bytes"] == (C.c_size_t, [C.c_int32] * 3)
    assert _lib.PROTOTYPES["c3dgs_mesh_extract_count"] == (C.c_int, [C.POINTER(_lib.Lattice)] + [vp] * 3 + [C.c_size_t, C.POINTER(C.c_int64), vp])
    assert _lib.PROTOTYPES["c3dgs_mesh_extract_emit"] == (C.c_int, [C.POINTER(_lib.Lattice)] + [vp] * 4 + [C.c_size_t, C.c_int64, C.c_int64] +
                                                          [vp] * 4)
    assert C.sizeof(_lib.Lattice) == 7 * 4
    assert L.c3dgs_abi_version() == 4


def test_header_names_the_entries():
    with open(os.path.join(os.path.dirname(build.HERE), "include", "c3dgs_hip.h")) as fh:
        text = fh.read()
    for name in ENTRIES:
        assert f" {name}(" in text, name
    assert "#define C3DGS_ABI_VERSION 4" in text and "} c3dgs_lattice;" in text
    for stage in STAGES:
        assert f'"{stage.decode()}"' in text, stage


def test_kernel_file_and_flags():
    assert "mesh.hip" in build.SOURCES and os.path.exists(os.path.join(build.CSRC, "mesh.hip"))
    assert build.SOURCES["mesh.hip"] == ["-ffp-contract=off"] == build.SOURCES["filter3d.hip"]


def test_stage_names(L):
    try:
        for name in STAGES:
            assert L.c3dgs_profile_only(name) == 0, name
        assert L.c3dgs_profile_only(b"mesh_extract") == 1                        # not a stage
    finally:
        assert L.c3dgs_profile_only(None) == 0


def test_workspace_is_about_five_bytes_a_point(L):
    for dims in ((1, 1, 1), (7, 6, 5), (33, 33, 33), (256, 256, 256), (512, 512, 512), (2**31 - 1, 1, 1), (1290, 1290, 1290)):
        n = dims[0] * dims[1] * dims[2]
        got = L.c3dgs_mesh_extract_workspace_bytes(*dims)
        blocks = (n + 255) // 256
        assert got % 256 == 0 and 5 * n + 8 * blocks <= got <= 5 * n + 8 * blocks + 6 * 256 + 2 * 72, dims
    for dims in ((0, 4, 4), (4, -1, 4), (2**16, 2**16, 1), (2048, 2048, 512)):   # no lattice: no workspace
        assert L.c3dgs_mesh_extract_workspace_bytes(*dims) == 0, dims


def _lat(Nx=4, Ny=4, Nz=4, h=0.1):
    return _lib.Lattice(Nx, Ny, Nz, 0.0, 0.0, 0.0, h)


def _integrate(L, lat="default", K=2, W=8, H=8, depth=B, color=None, cams=B, trunc=0.1, dmin=0.2, dmax=INF, tsdf=B, weight=B, vcol=None):
    lat = _lat() if lat == "default" else lat
    return L.c3dgs_tsdf_integrate(lat, K, W, H, depth, color, cams, trunc, dmin, dmax, tsdf, weight, vcol, None)


INTEGRATE_INVALID = [
    ("lattice", dict(lat=None), "lattice is NULL"),
    ("zero_dim", dict(lat=_lat(Nx=0)), "must be positive"),
    ("negative_dim", dict(lat=_lat(Nz=-3)), "must be positive"),
    ("too_many_points", dict(lat=_lat(2048, 2048, 512)), "at most 2^31 - 1"),
    ("product_wraps_32_bits", dict(lat=_lat(2**16, 2**16, 1)), "at most 2^31 - 1"),
    ("voxel_size", dict(lat=_lat(h=0.0)), "voxel_size must be positive"),
    ("tsdf_plane", dict(tsdf=None), "planes are required"),
    ("weight_plane", dict(weight=None), "planes are required"),
    ("K", dict(K=0), "K must be at least 1"),
    ("W", dict(W=0), "W and H must be positive"),
    ("H", dict(H=-1), "W and H must be positive"),
    ("sdf_trunc_zero", dict(trunc=0.0), "sdf_trunc must be positive"),
    ("sdf_trunc_nan", dict(trunc=float("nan")), "sdf_trunc must be positive"),
    ("depth_range_equal", dict(dmin=1.0, dmax=1.0), "depth_min < depth_max"),
    ("depth_range_reversed", dict(dmin=2.0, dmax=1.0), "depth_min < depth_max"),
    ("depth", dict(depth=None), "depth and cameras are required"),
    ("cameras", dict(cams=None), "depth and cameras are required"),
    ("color_without_planes", dict(color=B), "come as a pair"),
    ("planes_without_color", dict(vcol=B), "come as a pair"),
]


@pytest.mark.parametrize("label,kw,message", INTEGRATE_INVALID, ids=[c[0] for c in INTEGRATE_INVALID])
def test_integrate_refuses_invalid_calls_before_any_device_work(L, label, kw, message):
    assert _integrate(L, **kw) == 1
    assert message.encode() in L.c3dgs_last_error(), L.c3dgs_last_error()


def test_extract_refuses_invalid_calls_before_any_device_work(L):
    counts = (C.c_int64 * 2)()
    need = L.c3dgs_mesh_extract_workspace_bytes(4, 4, 4)
    ws = 0x10000                                                                 # 256-byte aligned, never dereferenced
    cases = [
        (dict(lat=None), "lattice is NULL"),
        (dict(lat=_lat(Ny=0)), "must be positive"),
        (dict(lat=_lat(2048, 2048, 512)), "at most 2^31 - 1"),
        (dict(tsdf=None), "planes are required"),
        (dict(weight=None), "planes are required"),
        (dict(ws=None), "workspace must hold"),
        (dict(ws=ws + 8), "workspace must hold"),
        (dict(nbytes=need - 1), "workspace must hold"),
    ]
    for kw, message in cases:
        a = dict(lat=_lat(), tsdf=B, weight=B, ws=ws, nbytes=need)
        a.update(kw)
        assert L.c3dgs_mesh_extract_count(a["lat"], a["tsdf"], a["weight"], a["ws"], a["nbytes"], counts, None) == 1, kw
        assert message.encode() in L.c3dgs_last_error(), (kw, L.c3dgs_last_error())
        assert L.c3dgs_mesh_extract_emit(a["lat"], a["tsdf"], a["weight"], None, a["ws"], a["nbytes"], 3, 1, B, None, B, None) == 1, kw
        assert message.encode() in L.c3dgs_last_error(), (kw, L.c3dgs_last_error())
    assert L.c3dgs_mesh_extract_count(_lat(), B, B, ws, need, None, None) == 1 and b"counts is NULL" in L.c3dgs_last_error()
    emit = lambda V, F, vcol, v, c, f: L.c3dgs_mesh_extract_emit(_lat(), B, B, vcol, ws, need, V, F, v, c, f, None)     # noqa: E731
    assert emit(-1, 0, None, B, None, B) == 1 and b"V and F" in L.c3dgs_last_error()
    assert emit(3, 2**31, None, B, None, B) == 1 and b"V and F" in L.c3dgs_last_error()
    assert emit(3, 1, B, B, None, B) == 1 and b"come as a pair" in L.c3dgs_last_error()
    assert emit(3, 1, None, B, B, B) == 1 and b"come as a pair" in L.c3dgs_last_error()
    assert emit(3, 1, None, None, None, B) == 1 and b"vertices and faces are required" in L.c3dgs_last_error()
    assert emit(3, 1, None, B, None, None) == 1 and b"vertices and faces are required" in L.c3dgs_last_error()
    assert emit(0, 0, B, None, None, None) == 0                                  # an empty mesh: nothing to write, nothing launched


def test_python_surface_without_a_gpu(tmp_path):
    import numpy as np
    import torch
    from c3dgs_amd import mesh, ply
    assert callable(ply.write_mesh_ply) and callable(ply.read_mesh_ply)
    with pytest.raises(RuntimeError, match="GPU"):
        mesh.TSDFVolume((0, 0, 0), 0.1, (4, 4, 4), 0.4, "cpu")
    with pytest.raises(ValueError, match="2\\^31 - 1"):
        mesh.TSDFVolume((0, 0, 0), 0.1, (2048, 2048, 512), 0.4, "cuda")
    with pytest.raises(ValueError, match="positive"):
        mesh.TSDFVolume((0, 0, 0), 0.1, (4, 0, 4), 0.4, "cuda")
    with pytest.raises(ValueError, match="positive"):
        mesh.TSDFVolume((0, 0, 0), 0.1, (4, 4, 4), 0.0, "cuda")
    vol = object.__new__(mesh.TSDFVolume)                            # integrate's checks come before any use of the planes
    vol.color, vol.device = None, torch.device("cuda")
    with pytest.raises(RuntimeError, match="GPU"):
        vol.integrate(torch.zeros(1, 4, 4), torch.zeros(1, 16))
    pkg = dict(alpha=torch.ones(4, 4), depth=torch.ones(4, 4), median_depth=torch.ones(4, 4))
    with pytest.raises(RuntimeError, match="GPU"):
        mesh.surface_depth(pkg)
    with pytest.raises(ValueError, match="mode"):
        mesh.surface_depth(pkg, mode="mean")
    # the voxel size a refusal names fits, and is not much larger than it has to be
    extent = np.array([10.0, 8.0, 6.0])
    h = mesh.fitting_voxel_size(extent, 0.001)
    dims = [mesh._axis_points(e, h) for e in extent]
    assert np.prod(dims, dtype=np.float64) <= mesh.MAX_POINTS < np.prod([mesh._axis_points(e, h / 1.03) for e in extent], dtype=np.float64)
    lo, hi = mesh.camera_bounds(torch.tensor([[1, 0, 0, -1.0, 0, 1, 0, 0, 0, 0, 1, 0, 50, 50, 8, 8],
                                              [1, 0, 0, 1.0, 0, 1, 0, 0, 0, 0, 1, 0, 50, 50, 8, 8]]))
    np.testing.assert_allclose(lo, [-2.1, -1.1, -1.1])                # centres (+-1, 0, 0), scene radius 1.1
    np.testing.assert_allclose(hi, [2.1, 1.1, 1.1])
