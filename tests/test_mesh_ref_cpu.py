"""CPU: tests/mesh_ref.py, the NumPy restatement the GPU tests hold csrc/mesh.hip to, is itself a correct marching tetrahedra: on a
sphere SDF (radius 0.3 in the unit box) at 12^3 and 20^3 the mesh is a closed oriented 2-manifold of Euler characteristic 2 with
positive signed volume, inside the linear-interpolation bound; degenerate lattices give an empty mesh; the welded result equals an
unwelded, geometrically wound brute force after merging by edge; and the mesh PLY round-trips."""
import math

import numpy as np
import pytest

from c3dgs_amd import ply
from tests import mesh_ref as mr

RADIUS = 0.3


@pytest.fixture(scope="module", params=[12, 20])
def sphere(request):
    n = request.param
    tsdf, weight, origin, h = mr.sphere_lattice(n, RADIUS)
    v, c, f = mr.extract(tsdf, weight, origin, h)
    return n, h, v, f


def test_sphere_is_a_closed_oriented_manifold(sphere):
    n, h, v, f = sphere
    assert len(f) > 0 and c_used(v, f)
    assert mr.closed_oriented(f)                       # every directed edge once, its opposite once
    assert mr.euler(len(v), f) == 2
    assert mr.signed_volume(v, f) > 0
    assert (mr.triangle_areas(v, f) > 0).all()


def c_used(v, f):
    return np.array_equal(np.unique(f), np.arange(len(v)))          # no vertex is unused


def test_sphere_radial_error(sphere):
    """| |v - c| - r | <= 3 h^2 / (8 (r - sqrt(3) h)) + 1e-5, linear interpolation over an edge of at most sqrt(3) h, with
    h = 1 / (n - 1): 0.0217 at 12^3 and 0.0050 at 20^3. The feature request quotes 0.0042 for 20^3, which the formula gives for no
    spacing of a 20^3 lattice over the unit box; the smaller figure is held as well. Measured: 0.0091 at 12^3, 0.0025 at 20^3."""
    n, h, v, f = sphere
    err = np.abs(np.linalg.norm(v.astype(np.float64) - 0.5, axis=1) - RADIUS).max()
    bound = mr.radial_error_bound(h, RADIUS)
    print(f"n = {n}: max radial error {err:.4f}, bound {bound:.4f}")
    assert err <= min(bound, {12: 0.0217, 20: 0.0042}[n] + 1e-5)


def test_degenerate_lattices_are_empty():
    rng = np.random.default_rng(0)
    for shape in ((1, 6, 7), (5, 1, 7), (5, 6, 1)):
        v, c, f = mr.extract(rng.uniform(-1, 1, shape).astype(np.float32), np.ones(shape, np.float32), (0, 0, 0), 0.1)
        assert v.shape == (0, 3) and f.shape == (0, 3) and c is None
    t = rng.uniform(0.1, 1, (5, 6, 7)).astype(np.float32)
    v, c, f = mr.extract(t, np.ones_like(t), (0, 0, 0), 0.1, np.zeros((3,) + t.shape, np.float32))
    assert v.shape == (0, 3) and c.shape == (0, 3) and f.shape == (0, 3)
    v, c, f = mr.extract(-t, np.zeros_like(t), (0, 0, 0), 0.1)       # signs, but no weight anywhere
    assert v.shape == (0, 3) and f.shape == (0, 3)


@pytest.mark.parametrize("case", ["random", "sphere"])
def test_welded_equals_unwelded_brute_force(case):
    if case == "random":
        tsdf, weight, _, origin, h = mr.random_lattice()
    else:
        tsdf, weight, origin, h = mr.sphere_lattice(9, RADIUS)
    v, _, f = mr.extract(tsdf, weight, origin, h)
    keys = [tuple(k) for k in mr.edge_keys(tsdf, weight)]
    assert len(set(keys)) == len(keys) == len(v)
    index = {k: n for n, k in enumerate(keys)}
    brute = mr.brute_force(tsdf, weight, origin, h)
    assert len(brute) == len(f) > 0
    used, merged, degenerate = set(), [], []
    for tri_keys, P, wound in brute:
        ids = [index[k] for k in tri_keys]                            # KeyError: a vertex the welded mesh does not have
        used.update(ids)
        for n, p in zip(ids, P):
            assert np.array_equal(v[n].astype(np.float64), p)        # the same fp32 position, bit for bit
        (merged if wound else degenerate).append(ids)
    assert used == set(range(len(v)))                                # no vertex is unused
    got = mr.canonical_faces(f)
    got_set = {tuple(r) for r in got}
    for ids in mr.canonical_faces(np.array(merged)):
        assert tuple(ids) in got_set                                 # wound by geometry == wound by the rule
    for ids in degenerate:                                           # zero-area triangles are kept, in either winding
        a = mr.canonical_faces(np.array([ids]))[0]
        b = mr.canonical_faces(np.array([[ids[0], ids[2], ids[1]]]))[0]
        assert tuple(a) in got_set or tuple(b) in got_set
    if case == "random":
        assert degenerate, "the random lattice has exact zeros: some triangle must be degenerate"
    assert len(got) == len(merged) + len(degenerate)


def test_zero_and_negative_zero_are_outside():
    t = np.full((2, 2, 2), 1.0, np.float32)
    for z in (0.0, -0.0):
        t[0, 0, 0] = np.float32(z)
        v, _, f = mr.extract(t, np.ones_like(t), (0, 0, 0), 1.0)
        assert len(v) == 0 and len(f) == 0
    t[0, 0, 0] = -1.0
    v, _, f = mr.extract(t, np.ones_like(t), (0, 0, 0), 1.0)
    assert len(v) == 7 and len(f) == 6                               # the corner every tetrahedron shares


def test_integrate_restatement_on_a_plane():
    """a fronto-parallel plane at depth 1 seen by one camera: sdf = 1 - z, truncated, weight 1 inside the frustum band"""
    W, H = 32, 24
    row = mr.look_at_row((0.5, 0.5, -1.0), (0.5, 0.5, 0.0), 40.0, W, H)
    depth = np.ones((1, H, W), np.float32)
    z0 = np.zeros((5, 6, 7), np.float32)
    t, w, c = mr.integrate(z0, z0, None, (0.3, 0.3, -0.2), 0.05, depth, row[None], 0.1, depth_min=0.2)
    zs = -0.2 + 0.05 * np.arange(5) + 1.0                            # view-space z of the five lattice planes
    for k in range(5):
        sdf = 1.0 - zs[k]
        if sdf < -0.1 - 1e-6:
            assert (w[k] == 0).all() and (t[k] == 0).all()
        elif sdf > -0.1 + 1e-6:
            assert (w[k] == 1).all()
            np.testing.assert_allclose(t[k], min(1.0, sdf / 0.1), atol=1e-5)
    assert c is None
    t2, w2, _ = mr.integrate(t, w, None, (0.3, 0.3, -0.2), 0.05, depth, row[None], 0.1, depth_min=0.2)
    assert np.array_equal(w2, 2 * w) and np.allclose(t2, t, atol=1e-6)


def test_mesh_ply_round_trip(tmp_path):
    tsdf, weight, colors, origin, h = mr.random_lattice()
    v, c, f = mr.extract(tsdf, weight, origin, h, colors)
    c[0] = (-0.5, 1.5, float("nan"))                                 # clamped; NaN writes 0
    path = tmp_path / "mesh.ply"
    ply.write_mesh_ply(path, v, c, f)
    v2, c2, f2 = ply.read_mesh_ply(path)
    assert v2.dtype == np.float32 and np.array_equal(v2.view(np.uint32), v.view(np.uint32))
    assert f2.dtype == np.int32 and np.array_equal(f2, f)
    assert c2.dtype == np.uint8 and np.array_equal(c2, np.rint(np.clip(np.nan_to_num(c.astype(np.float64)), 0, 1) * 255).astype(np.uint8))
    assert tuple(c2[0]) == (0, 255, 0)
    with open(path, "rb") as fh:
        head = fh.read(400)
    assert b"format binary_little_endian 1.0" in head and b"property list uchar int vertex_indices" in head
    assert b"property uchar red" in head and f"element face {len(f)}".encode() in head
    ply.write_mesh_ply(path, v[:0], None, f[:0])                     # an empty mesh is a valid file
    v3, c3, f3 = ply.read_mesh_ply(path)
    assert v3.shape == (0, 3) and c3.shape == (0, 3) and f3.shape == (0, 3)
    with pytest.raises(ValueError, match="face indices"):
        ply.write_mesh_ply(path, v, c, f + len(v))
    xyz = ply.read_ply(tmp_path / "mesh.ply")                        # the point reader still reads a mesh file's vertices
    assert set(xyz) == {"x", "y", "z", "red", "green", "blue"} and math.isclose(len(xyz["x"]), 0)
