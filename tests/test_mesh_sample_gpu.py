"""-m gpu: csrc/mesh_sample.hip against the sampler of tests/geometry_ref.py: per-face counts equal, points bit-equal and in the
same order (face ascending, then sample index), for every case."""
import numpy as np
import pytest
import torch

from tests import geometry_ref as G

pytestmark = pytest.mark.gpu


def _gpu(a, dtype):
    return torch.as_tensor(np.ascontiguousarray(a), dtype=dtype, device="cuda")


def check(v, f, density, seed=0, what=""):
    from c3dgs_amd import mesh
    rp, rf, rn = G.sample_surface(v, f, density, seed)
    points, face = mesh.sample_surface(_gpu(v, torch.float32), _gpu(f, torch.int32), density, seed)
    assert points.dtype == torch.float32 and face.dtype == torch.int32
    points, face = points.cpu().numpy(), face.cpu().numpy()
    assert points.shape == (rn.sum(), 3) and face.shape == (rn.sum(),), (what, points.shape, int(rn.sum()))
    assert (np.bincount(face, minlength=len(f)) == rn).all() if len(f) else face.size == 0, what
    assert (face == rf).all(), what
    bad = np.nonzero((points.view(np.uint32) != rp.view(np.uint32)).any(axis=1))[0]
    assert bad.size == 0, f"{what}: {bad.size} of {len(rp)} points differ, the first is sample {bad[0]}: {points[bad[0]]} vs {rp[bad[0]]}"
    return rn


def test_small_random_mesh(hip):
    rng = np.random.default_rng(0)
    v = rng.standard_normal((50, 3)).astype(np.float32)
    f = rng.integers(0, 50, (333, 3)).astype(np.int32)
    for density, seed in ((0.4, 0), (3.0, 1), (40.0, 0xFFFFFFFF)):
        n = check(v, f, density, seed, f"random density={density}")
        assert n.sum() > 0
    a = check(v, f, 3.0, 5, "seed 5")
    assert (a != G.face_counts(v, f, 3.0, 6)).any()                       # the seed matters


def test_degenerate_faces(hip):
    v = np.asarray([[0, 0, 0], [1, 0, 0], [2, 0, 0], [0, 1, 0], [np.nan, 0, 0], [np.inf, 1, 1], [3e19, 0, 0], [0, 3e19, 0]],
                   np.float32)
    f = np.asarray([[0, 1, 2], [0, 0, 3], [0, 1, 4], [0, 3, 5], [0, 1, 3], [4, 4, 4], [0, 6, 7], [1, 3, 0]], np.int32)
    n = check(v, f, 100.0, 2, "degenerate")
    assert list(n[[0, 1, 2, 3, 5, 6]]) == [0] * 6 and n[4] in (50, 51) and n[7] in (50, 51)


def test_one_large_face_among_tiny_ones(hip):
    rng = np.random.default_rng(1)
    v = (rng.standard_normal((90, 3)) * 0.02).astype(np.float32)
    f = rng.integers(0, 87, (400, 3)).astype(np.int32)
    v[87:] = np.asarray([[0, 0, 0], [10, 0, 0], [0, 10, 0]], np.float32)
    f[123] = (87, 88, 89)                                                  # area 50
    n = check(v, f, 60.0, 3, "one large face")
    assert n[123] > 1000 and n[123] > 4 * 256 and np.delete(n, 123).max() < 3  # its samples span several workgroups of the emit


def test_more_faces_than_one_scan_sweep(hip):
    """F = 70,000: 274 workgroups of 256 faces, a ragged last one. The block-total scan (scan_blocks.hpp) takes 16,384 totals a
    sweep, so its second sweep starts at 16,384 x 256 = 4,194,304 faces: F = that + 777, tiny faces, once."""
    rng = np.random.default_rng(2)
    F = 70_000
    v = rng.uniform(0, 1, (5000, 3)).astype(np.float32)
    f = rng.integers(0, 5000, (F, 3)).astype(np.int32)
    n = check(v, f, 2.0, 4, "F = 70,000")
    assert 0 < n.sum() < 200_000
    F = 16384 * 256 + 777
    base = rng.integers(0, 4990, F).astype(np.int32)
    f = np.stack([base, base + 3, base + 7], 1)
    n = check(v, f, 0.5, 5, "two sweeps of the block-total scan")
    assert n[-777:].sum() > 0


def test_no_faces(hip):
    from c3dgs_amd import mesh
    points, face = mesh.sample_surface(torch.zeros((5, 3), device="cuda"), torch.zeros((0, 3), dtype=torch.int32, device="cuda"), 3.0)
    assert points.shape == (0, 3) and face.shape == (0,)
    points, face = mesh.sample_surface(torch.zeros((5, 3), device="cuda"), torch.zeros((4, 3), dtype=torch.int32, device="cuda"), 3.0)
    assert points.shape == (0, 3) and face.shape == (0,)                   # faces without area


def test_bad_meshes_raise(hip):
    from c3dgs_amd import mesh
    v = _gpu([[0, 0, 0], [1, 0, 0], [0, 1, 0], [0, 0, 1]], torch.float32)
    for bad in (4, -1, 2 ** 31 - 1, -2 ** 31):
        f = _gpu([[0, 1, 2], [1, 2, bad], [0, 2, 3]], torch.int32)
        with pytest.raises(RuntimeError, match="outside"):
            mesh.sample_surface(v, f, 10.0)
    f = _gpu([[0, 1, 2], [0, 2, 3]], torch.int32)
    with pytest.raises(RuntimeError, match="2\\^24"):
        mesh.sample_surface(v, f, 2.0 ** 25)                               # t = 2^24 exactly
    points, _ = mesh.sample_surface(v, f, 2.0 ** 12)                       # the library is fine afterwards
    assert points.shape[0] in range(2 ** 12 - 1, 2 ** 12 + 2)
    with pytest.raises(RuntimeError, match="2\\^31"):
        mesh.sample_surface(v * 64.0, _gpu(np.tile([[0, 1, 2]], (300, 1)), torch.int32), 4095.0)   # 300 x 8,386,560 samples
    for density in (0.0, -1.0, float("nan"), float("inf")):
        with pytest.raises(ValueError, match="density"):
            mesh.sample_surface(v, f, density)
    with pytest.raises(RuntimeError, match="GPU"):
        mesh.sample_surface(v.cpu(), f, 1.0)
