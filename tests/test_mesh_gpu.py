"""-m gpu: csrc/mesh.hip against tests/mesh_ref.py. The TSDF planes are bit-equal to the NumPy restatement in every integrate case
(one and several cameras per launch, with and without colours, maps of a second size onto the same volume, a camera inside the
lattice, a depth_max inside the measured range); the marching tetrahedra give the restatement's vertices and colours bit for bit
in its order and its faces as a set; degenerate lattices give an empty mesh; a sphere gives a closed surface of Euler
characteristic 2; a lattice larger than one sweep of the block-total scan works; and extract_mesh is its hand-composed sequence."""
import functools

import numpy as np
import pytest
import torch

from tests import mesh_ref as mr

pytestmark = pytest.mark.gpu

DIMS = (24, 20, 17)
H_VOX = 1.0 / 23.0
ORIGIN = (0.0, 0.0, 0.0)
CENTRE = (0.5, 0.41, 0.35)
RADIUS = 0.25
TRUNC = 3.0 * H_VOX
W0, H0 = 64, 48


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


@functools.lru_cache(maxsize=None)
def cameras(kind):
    """-> (table [K, 16], depth [K, H, W], color [K, 3, H, W]) of the analytic sphere, NumPy"""
    if kind == "six":
        table, W, H = mr.six_cameras(W0, H0, 60.0, 1.2, CENTRE), W0, H0
    elif kind == "nineteen":
        table, W, H = mr.perturbed(mr.six_cameras(W0, H0, 60.0, 1.2, CENTRE), 19), W0, H0
    elif kind == "small":
        table, W, H = mr.perturbed(mr.six_cameras(40, 30, 38.0, 1.3, CENTRE), 3, seed=4), 40, 30
    elif kind == "inside":                                   # at x = 0.1: the lattice planes i = 0..2 are behind it
        table, W, H = mr.look_at_row((0.1, 0.4, 0.3), CENTRE, 60.0, W0, H0)[None], W0, H0
    maps = [mr.sphere_depth(row, W, H, CENTRE, RADIUS) for row in table]
    return table, np.stack([m[0] for m in maps]), np.stack([m[1] for m in maps])


def zero_planes(color):
    Nx, Ny, Nz = DIMS
    z = np.zeros((Nz, Ny, Nx), np.float32)
    return z, z.copy(), (np.zeros((3, Nz, Ny, Nx), np.float32) if color else None)


def ref_integrate(planes, kind, color, sel=slice(None), **kw):
    table, depth, col = cameras(kind)
    return mr.integrate(*planes, ORIGIN, H_VOX, depth[sel], table[sel], TRUNC, color=col[sel] if color else None, **kw)


def gpu_integrate(vol, kind, color, sel=slice(None), **kw):
    table, depth, col = cameras(kind)
    c = torch.from_numpy(col[sel]).cuda() if color else None
    vol.integrate(torch.from_numpy(depth[sel]).cuda(), torch.from_numpy(table[sel]).cuda(), c, **kw)
    return vol


def new_volume(color, dims=DIMS, origin=ORIGIN, h=H_VOX, trunc=TRUNC):
    from c3dgs_amd import mesh
    return mesh.TSDFVolume(origin, h, dims, trunc, "cuda", color=color)


def assert_planes(vol, ref, what):
    t, w, c = ref
    assert float(w.max()) > 0, f"{what}: the reference integrated nothing"
    for name, got, want in (("tsdf", vol.tsdf, t), ("weight", vol.weight, w), ("color", vol.color, c)):
        if want is None:
            assert got is None
            continue
        got = got.cpu().numpy()
        diff = np.nonzero(_bits(got) != _bits(want))
        assert diff[0].size == 0, (f"{what}: {name} differs from the restatement in {diff[0].size} of {want.size} values, the first at "
                                   f"{tuple(int(d[0]) for d in diff)}: {got[tuple(d[0] for d in diff)]!r} != "
                                   f"{want[tuple(d[0] for d in diff)]!r}")


@pytest.mark.parametrize("color", [False, True], ids=["plain", "color"])
@pytest.mark.parametrize("K", [1, 6])
def test_integrate_is_the_restatement(hip, K, color):
    sel = slice(0, K)
    ref = ref_integrate(zero_planes(color), "six", color, sel)
    vol = gpu_integrate(new_volume(color), "six", color, sel)
    assert_planes(vol, ref, f"K = {K}")
    assert (ref[1] == 0).any() and ref[1].max() >= min(K, 2)          # untouched points, and points more than one camera saw


def test_six_calls_of_one_map_are_one_call_of_six(hip):
    one = gpu_integrate(new_volume(True), "six", True)
    six = new_volume(True)
    for k in range(6):
        gpu_integrate(six, "six", True, slice(k, k + 1))
    for a, b in ((one.tsdf, six.tsdf), (one.weight, six.weight), (one.color, six.color)):
        assert torch.equal(a.view(torch.int32), b.view(torch.int32))
    assert_planes(six, ref_integrate(zero_planes(True), "six", True), "six calls")


def test_nineteen_cameras_in_one_launch(hip):
    assert_planes(gpu_integrate(new_volume(True), "nineteen", True), ref_integrate(zero_planes(True), "nineteen", True), "K = 19")


def test_maps_of_a_second_size_onto_the_same_volume(hip):
    first = ref_integrate(zero_planes(True), "six", True)
    ref = ref_integrate(first, "small", True)
    vol = gpu_integrate(gpu_integrate(new_volume(True), "six", True), "small", True)
    assert_planes(vol, ref, "64x48 then 40x30")
    assert ref[1].sum() > first[1].sum() and ((ref[1] > first[1]) & (first[1] > 0)).any()      # the second call added to the first


def test_a_camera_with_the_lattice_partly_behind_it(hip):
    ref = ref_integrate(zero_planes(True), "inside", True)
    assert_planes(gpu_integrate(new_volume(True), "inside", True), ref, "camera inside the lattice")
    assert not ref[1][:, :, :3].any() and ref[1][:, :, 6:].any()                   # nothing behind the camera, something in front


def test_depth_max_inside_the_measured_range(hip):
    _, depth, _ = cameras("six")
    hit = depth[depth > 0]
    cut = float(np.float32(0.5 * (hit.min() + hit.max())))
    assert hit.min() < cut < hit.max()
    ref = ref_integrate(zero_planes(False), "six", False, depth_max=cut)
    full = ref_integrate(zero_planes(False), "six", False)
    assert 0 < ref[1].sum() < full[1].sum()
    assert_planes(gpu_integrate(new_volume(False), "six", False, depth_max=cut), ref, "depth_max")


# ---- extract
def gpu_extract(tsdf, weight, origin, h, colors=None):
    Nz, Ny, Nx = tsdf.shape
    vol = new_volume(colors is not None, (Nx, Ny, Nz), origin, h, 1.0)
    vol.tsdf.copy_(torch.from_numpy(tsdf))
    vol.weight.copy_(torch.from_numpy(weight))
    if colors is not None:
        vol.color.copy_(torch.from_numpy(colors))
    v, c, f = vol.extract()
    assert v.dtype == torch.float32 and f.dtype == torch.int32 and v.shape[1:] == (3,) and f.shape[1:] == (3,)
    return v.cpu().numpy(), None if c is None else c.cpu().numpy(), f.cpu().numpy()


def assert_mesh(got, ref, what):
    (v, c, f), (rv, rc, rf) = got, ref
    assert v.shape == rv.shape and f.shape == rf.shape, (what, v.shape, rv.shape, f.shape, rf.shape)
    assert np.array_equal(_bits(v), _bits(rv)), f"{what}: vertices differ"
    if rc is None:
        assert c is None
    else:
        assert np.array_equal(_bits(c), _bits(rc)), f"{what}: colours differ"
    assert np.array_equal(mr.canonical_faces(f), mr.canonical_faces(rf)), f"{what}: faces differ"


def test_extract_random_lattice_with_zeros_and_holes(hip):
    tsdf, weight, colors, origin, h = mr.random_lattice()
    assert (tsdf == 0).any() and (np.signbit(tsdf) & (tsdf == 0)).any() and (weight == 0).mean() > 0.1
    ref = mr.extract(tsdf, weight, origin, h, colors)
    assert len(ref[0]) > 0 and len(ref[2]) > 0
    got = gpu_extract(tsdf, weight, origin, h, colors)
    assert_mesh(got, ref, "random 7x6x5")
    again = gpu_extract(tsdf, weight, origin, h, colors)             # two runs: identical bits, faces in the same order too
    for a, b in zip(got, again):
        assert np.array_equal(a.view(np.uint32) if a.dtype == np.float32 else a, b.view(np.uint32) if b.dtype == np.float32 else b)
    assert_mesh(gpu_extract(tsdf, weight, origin, h), mr.extract(tsdf, weight, origin, h), "random 7x6x5 without colours")


def test_extract_degenerate_lattices_are_empty(hip):
    rng = np.random.default_rng(2)
    for shape in ((1, 9, 9), (9, 1, 9), (9, 9, 1)):
        v, c, f = gpu_extract(rng.uniform(-1, 1, shape).astype(np.float32), np.ones(shape, np.float32), (0, 0, 0), 0.1)
        assert v.shape == (0, 3) and f.shape == (0, 3)
    t = rng.uniform(0.1, 1, (6, 7, 8)).astype(np.float32)
    v, c, f = gpu_extract(t, np.ones_like(t), (0, 0, 0), 0.1, np.zeros((3,) + t.shape, np.float32))
    assert v.shape == (0, 3) and c.shape == (0, 3) and f.shape == (0, 3)


def test_extract_sphere_is_closed(hip):
    tsdf, weight, origin, h = mr.sphere_lattice(33, 0.3)
    v, c, f = gpu_extract(tsdf, weight, origin, h)
    assert len(f) > 0 and mr.closed_oriented(f) and mr.euler(len(v), f) == 2 and mr.signed_volume(v, f) > 0
    assert np.array_equal(np.unique(f), np.arange(len(v)))
    err = np.abs(np.linalg.norm(v.astype(np.float64) - 0.5, axis=1) - 0.3).max()
    assert err <= mr.radial_error_bound(h, 0.3)
    assert_mesh((v, c, f), mr.extract(tsdf, weight, origin, h), "sphere 33^3")


def test_extract_lattice_larger_than_one_scan_sweep(hip):
    """170 x 160 x 157 points = 16,681 blocks of 256: more than the 16,384 block totals one sweep of the scan covers, not a multiple
    of either; a tilted wavy sheet crosses every k, so there are vertices and faces behind the sweep boundary"""
    Nx, Ny, Nz = 170, 160, 157
    assert (Nx * Ny * Nz) % 256 and (Nx * Ny * Nz + 255) // 256 > 16384 and ((Nx * Ny * Nz + 255) // 256) % 16384
    z, y, x = np.meshgrid(np.linspace(0, 1, Nz), np.linspace(0, 1, Ny), np.linspace(0, 1, Nx), indexing="ij")
    tsdf = (x - 0.5 + 0.2 * (z - 0.5) + 0.03 * np.sin(9 * y)).astype(np.float32)
    weight = ((x - 0.45) ** 2 + (y - 0.5) ** 2 < 0.2).astype(np.float32)           # the sheet leaves the weighted region
    ref = mr.extract(tsdf, weight, (0.0, 0.0, 0.0), 0.01)
    got = gpu_extract(tsdf, weight, (0.0, 0.0, 0.0), 0.01)
    assert len(ref[2]) > 50_000
    assert_mesh(got, ref, "170x160x157")


def test_extract_mesh_is_its_hand_composed_sequence(hip, tmp_path):
    from c3dgs_amd import filter3d, mesh, ply
    from c3dgs_amd.model import PipelineParams
    from tests import synth, train_scene
    W, H, focal = 64, 48, 60.0
    model, _ = train_scene.teacher_model(4000, W, H, focal, "cuda")
    cams = []
    for k in range(8):
        a = 2 * np.pi * k / 8
        ev = (0.015 * np.sin(a), 0.015 * np.cos(a), 0.0, 1.0, 0.25 * np.cos(a), 0.25 * np.sin(a), 0.0)
        cams.append(train_scene.Cam(*synth.camera(W, H, focal, extrinsic_vector=ev), "cuda"))
    pipe, bg = PipelineParams(), torch.zeros(3, device="cuda")
    bounds, h = ((-2.0, -1.5, 2.5), (2.0, 1.5, 6.0)), 0.08
    kw = dict(depth_mode="expected", alpha_min=0.2, depth_max=7.0)
    v, c, f = mesh.extract_mesh(model, cams, pipe, bg, h, bounds=bounds, batch=3, **kw)

    table = filter3d.camera_table(cams, "cuda")
    dims = tuple(int(np.ceil((hi - lo) / h)) + 1 for lo, hi in zip(*bounds))
    vol = mesh.TSDFVolume(bounds[0], h, dims, 4 * h, "cuda")
    with torch.no_grad():
        pkgs = [model.render(cam, pipe, bg, return_depth=True) for cam in cams]
    depth = torch.stack([mesh.surface_depth(p, "expected", 0.2) for p in pkgs])
    vol.integrate(depth, table, torch.stack([p["render"] for p in pkgs]), depth_max=7.0)
    v2, c2, f2 = vol.extract()
    assert v.shape[0] > 0 and f.shape[0] > 0
    assert torch.equal(v.view(torch.int32), v2.view(torch.int32)) and torch.equal(c.view(torch.int32), c2.view(torch.int32))
    assert torch.equal(f, f2)
    assert int(f.min()) == 0 and int(f.max()) == v.shape[0] - 1
    # the maps themselves: depth / alpha where alpha >= alpha_min, 0 elsewhere; the median where asked
    p = pkgs[0]
    seen = p["alpha"] >= 0.2
    assert torch.equal(depth[0], torch.where(seen, p["depth"] / p["alpha"].clamp_min(1e-6), torch.zeros_like(p["depth"])))
    assert torch.equal(mesh.surface_depth(p), torch.where(p["alpha"] >= 0.5, p["median_depth"], torch.zeros_like(p["depth"])))
    path = tmp_path / "mesh.ply"
    ply.write_mesh_ply(path, v.cpu().numpy(), c.cpu().numpy(), f.cpu().numpy())
    rv, rc, rf = ply.read_mesh_ply(path)
    assert np.array_equal(_bits(rv), _bits(v.cpu().numpy())) and np.array_equal(rf, f.cpu().numpy())
    assert np.array_equal(rc, np.rint(np.clip(c.cpu().numpy().astype(np.float64), 0, 1) * 255).astype(np.uint8))
    with pytest.raises(ValueError, match="would fit"):
        mesh.extract_mesh(model, cams, pipe, bg, 1e-4, bounds=bounds)
