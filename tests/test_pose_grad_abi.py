"""CPU: the C ABI of the exact pose gradient (c3dgs_pose_grad, c3dgs_pose_grad_workspace_bytes; csrc/pose_grad.hip). The symbols
are exported and bound, the ABI version did not move (new entry points only), the kernel's file is built with the flags
gsmath.hpp asks for, the workspace is 24 floats per 256 Gaussians and monotone in P, and every invalid call is refused with its
message before any device work -- which is why these run without a GPU."""
import ctypes as C

import pytest

from c3dgs_amd import _lib, build


@pytest.fixture(scope="module")
def L():
    return _lib.lib()


def test_symbols_are_exported_and_bound(L):
    for name, n_args in (("c3dgs_pose_grad", 21), ("c3dgs_pose_grad_workspace_bytes", 1)):
        assert hasattr(L, name), name
        res, args = _lib.PROTOTYPES[name]
        assert len(args) == n_args, name
    assert _lib.PROTOTYPES["c3dgs_pose_grad_workspace_bytes"][0] is C.c_size_t
    assert _lib.PROTOTYPES["c3dgs_pose_grad"][1][3] is C.c_float          # scale_modifier
    assert L.c3dgs_abi_version() == 4


def test_kernel_file_is_built_without_contraction():
    assert build.SOURCES["pose_grad.hip"] == ["-ffp-contract=off"] == build.SOURCES["preprocess.hip"]


def test_stage_names(L):
    try:
        for name in (b"pose_grad", b"pose_grad_sums", b"pose_grad_fold"):
            assert L.c3dgs_profile_only(name) == 0, name
    finally:
        assert L.c3dgs_profile_only(None) == 0


def test_workspace_bytes_formula_and_monotone(L):
    prev = 0
    for P in (0, 1, 63, 64, 255, 256, 257, 10752, 10753, 65536, 65537, 3_000_000, 2**31 - 1):
        b = L.c3dgs_pose_grad_workspace_bytes(P)
        rows = (max(P, 1) + 255) // 256
        assert b == (rows * 96 + 255) // 256 * 256, (P, b)               # 24 floats per 256 Gaussians, 256-byte aligned
        assert b >= prev and b >= 256
        prev = b
    assert L.c3dgs_pose_grad_workspace_bytes(-5) == L.c3dgs_pose_grad_workspace_bytes(1)


B = 0x1000          # a non-NULL "buffer": the calls below must fail before anything dereferences it
NAMES = ("means3D", "dL_dmeans3D", "dL_dcov3D", "dL_dcolors", "sh", "sh_indices", "cov3D_precomp", "scales", "rotations",
         "scale_factors", "g_indices", "geom", "radii", "pose", "ws", "out")
# a valid indexed call: SH through sh_indices, codebooks through g_indices with scale factors
VALID = dict(P=10, D=3, M=16, means3D=B, dL_dmeans3D=B, dL_dcov3D=B, dL_dcolors=B, sh=B, sh_indices=B, cov3D_precomp=None, scales=B,
             rotations=B, scale_factors=B, g_indices=B, geom=B, radii=B, pose=B, ws=B, out=B)
INVALID = [
    ("P", dict(P=-1), "P must be >= 0"),
    ("degree", dict(D=4), "degree must be 0..3"),
    ("degree_negative", dict(D=-1), "degree must be 0..3"),
    ("M", dict(M=-1), "M >= 0"),
    ("pose", dict(pose=None), "the pose and the output are required"),
    ("out", dict(out=None), "the pose and the output are required"),
    ("means3D", dict(means3D=None), "are required"),
    ("dL_dmeans3D", dict(dL_dmeans3D=None), "are required"),
    ("dL_dcov3D", dict(dL_dcov3D=None), "are required"),
    ("radii", dict(radii=None), "are required"),
    ("geom", dict(geom=None), "geometry buffer and a workspace are required"),
    ("workspace", dict(ws=None), "geometry buffer and a workspace are required"),
    ("scales_without_rotations", dict(rotations=None), "scales and rotations come as a pair"),
    ("rotations_without_scales", dict(scales=None), "scales and rotations come as a pair"),
    ("both_covariances", dict(cov3D_precomp=B), "exactly one of cov3D_precomp"),
    ("no_covariance", dict(scales=None, rotations=None, g_indices=None, scale_factors=None), "exactly one of cov3D_precomp"),
    ("g_indices_without_factors", dict(scale_factors=None), "g_indices and scale_factors come as a pair"),
    ("factors_without_g_indices", dict(g_indices=None), "g_indices and scale_factors come as a pair"),
    ("g_indices_with_precomp", dict(scales=None, rotations=None, cov3D_precomp=B), "g_indices need the scale / rotation codebooks"),
    ("sh_indices_without_sh", dict(sh=None), "sh_indices need sh"),
    ("sh_without_dL_dcolors", dict(dL_dcolors=None), "dL_dcolors is required"),
    ("M_too_small", dict(M=15), "M must hold"),
]


def _call(L, a):
    return L.c3dgs_pose_grad(a["P"], a["D"], a["M"], 1.0, *[a[k] for k in NAMES], None)


@pytest.mark.parametrize("what,change,message", INVALID, ids=[c[0] for c in INVALID])
def test_invalid_arguments_return_1_with_a_message(L, what, change, message):
    a = dict(VALID)
    a.update(change)
    assert _call(L, a) == 1
    msg = L.c3dgs_last_error().decode()
    assert msg.startswith("pose_grad: ") and message in msg, msg


def test_a_null_pose_or_output_is_refused_even_with_nothing_to_sum(L):
    a = dict(VALID, P=0, pose=None)
    assert _call(L, a) == 1 and b"pose" in L.c3dgs_last_error()
    a = dict(VALID, P=0, out=None)
    assert _call(L, a) == 1
