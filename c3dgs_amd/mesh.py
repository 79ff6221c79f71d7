"""Mesh extraction (not in the reference): bounded TSDF fusion of rendered depth maps into a dense volume, then welded marching
tetrahedra over it -- the step 2DGS ends in, in HIP on the device where the maps already are (csrc/mesh.hip).

    vol = TSDFVolume(origin, voxel_size, dims, sdf_trunc, device)        # fp32 planes [Nz, Ny, Nx]: vol.tsdf, vol.weight, vol.color
    vol.integrate(depth [K, H, W], table [K, 16], color [K, 3, H, W])    # one launch for the K maps; filter3d.camera_table's rows
    vertices, colors, faces = vol.extract()                              # [V, 3] f32, [V, 3] f32 | None, [F, 3] int32
    surface_depth(render_pkg, mode="median" | "expected", alpha_min=0.5) # the depth map a render(return_depth=True) describes
    extract_mesh(gaussians, cameras, pipe, bg, voxel_size, ...)          # render every camera, fuse, extract

The mathematics is the contract of include/c3dgs_hip.h ("mesh extraction"); both halves are bitwise reproducible. GPU tensors only."""
import ctypes as C
import math

import numpy as np
import torch

from . import _lib
from ._lib import ptr as _ptr, stream as _stream
from .normals import _check

MAX_POINTS = 2 ** 31 - 1


def fitting_voxel_size(extent, voxel_size):
    """the smallest voxel size >= `voxel_size` (in steps of 1 %) at which a box of `extent` has at most 2^31 - 1 lattice points"""
    h = float(voxel_size)
    while np.prod([_axis_points(e, h) for e in extent], dtype=np.float64) > MAX_POINTS:
        h *= 1.01
    return h


def _axis_points(extent, h):
    return int(math.ceil(max(float(extent), 0.0) / h)) + 1


class TSDFVolume:
    """A dense TSDF volume on `device`: Nx x Ny x Nz = `dims` lattice points at origin + (i, j, k) voxel_size, planes [Nz, Ny, Nx]
    (x fastest) `tsdf`, `weight` and, with color=True, `color` [3, Nz, Ny, Nx], all zero at first."""

    def __init__(self, origin, voxel_size, dims, sdf_trunc, device, color=True):
        dims = tuple(int(v) for v in dims)
        if len(dims) != 3 or min(dims) < 1:
            raise ValueError(f"TSDFVolume: dims must be three positive integers, not {dims}")
        if dims[0] * dims[1] * dims[2] > MAX_POINTS:
            raise ValueError(f"TSDFVolume: {dims[0]} x {dims[1]} x {dims[2]} lattice points exceed 2^31 - 1")
        if not float(voxel_size) > 0 or not float(sdf_trunc) > 0:
            raise ValueError("TSDFVolume: voxel_size and sdf_trunc must be positive")
        device = torch.device(device)
        if device.type != "cuda":
            raise RuntimeError("c3dgs_amd: TSDFVolume lives on a GPU (there is no CPU path)")
        self.origin = tuple(float(v) for v in origin)
        self.voxel_size, self.dims, self.sdf_trunc, self.device = float(voxel_size), dims, float(sdf_trunc), device
        Nx, Ny, Nz = dims
        self.tsdf = torch.zeros((Nz, Ny, Nx), dtype=torch.float32, device=device)
        self.weight = torch.zeros((Nz, Ny, Nx), dtype=torch.float32, device=device)
        self.color = torch.zeros((3, Nz, Ny, Nx), dtype=torch.float32, device=device) if color else None
        self.device = self.tsdf.device                      # with its index: what the tensors of integrate() are compared with

    def _lattice(self):
        return _lib.Lattice(*self.dims, *self.origin, self.voxel_size)

    def integrate(self, depth, table, color=None, depth_min=0.2, depth_max=math.inf):
        """Fuse the K maps `depth` [K, H, W] (view-space z, 0 = no measurement) of the cameras `table` [K, 16]
        (filter3d.camera_table; its W and H are the maps') and, for a volume with colour, their colours `color` [K, 3, H, W]: one
        launch on the current stream, no host read. K maps in one call leave the bits of K calls of one map."""
        _check(depth, None, "depth")
        if depth.dim() != 3 or depth.numel() == 0:
            raise RuntimeError(f"c3dgs_amd: depth must have shape (K, H, W), not {tuple(depth.shape)}")
        K, H, W = (int(v) for v in depth.shape)
        _check(table, (K, 16), "table")
        if (self.color is None) != (color is None):
            raise RuntimeError("c3dgs_amd: a volume with colour planes takes color, one without does not")
        if color is not None:
            _check(color, (K, 3, H, W), "color")
        for t in (depth, table, color):
            if t is not None and t.device != self.device:
                raise RuntimeError(f"c3dgs_amd: every tensor must be on the volume's device {self.device}")
        depth, table = depth.detach().contiguous(), table.detach().contiguous()
        color = None if color is None else color.detach().contiguous()
        with torch.cuda.device(self.device):
            rc = _lib.lib().c3dgs_tsdf_integrate(self._lattice(), K, W, H, _ptr(depth), _ptr(color), _ptr(table), self.sdf_trunc,
                                                 float(depth_min), float(depth_max), _ptr(self.tsdf), _ptr(self.weight),
                                                 _ptr(self.color), _stream(self.device))
        _lib.check(rc)
        return self

    def extract(self):
        """-> (vertices [V, 3] f32, colors [V, 3] f32 or None without colour planes, faces [F, 3] int32): marching tetrahedra over
        the cells whose eight corners all have weight > 0, vertices welded. Four launches and one host read (the two counts)."""
        lib, lat, dev = _lib.lib(), self._lattice(), self.device
        counts = (C.c_int64 * 2)()
        with torch.cuda.device(dev):
            ws = _lib.workspace("mesh", dev, int(lib.c3dgs_mesh_extract_workspace_bytes(*self.dims)))
            _lib.check(lib.c3dgs_mesh_extract_count(lat, _ptr(self.tsdf), _ptr(self.weight), ws.data_ptr(), ws.numel(), counts,
                                                    _stream(dev)))
            V, F = int(counts[0]), int(counts[1])
            vertices = torch.empty((V, 3), dtype=torch.float32, device=dev)
            colors = torch.empty((V, 3), dtype=torch.float32, device=dev) if self.color is not None else None
            faces = torch.empty((F, 3), dtype=torch.int32, device=dev)
            _lib.check(lib.c3dgs_mesh_extract_emit(lat, _ptr(self.tsdf), _ptr(self.weight), _ptr(self.color), ws.data_ptr(), ws.numel(),
                                                   V, F, _ptr(vertices), _ptr(colors), _ptr(faces), _stream(dev)))
        return vertices, colors, faces


def surface_depth(render_pkg, mode="median", alpha_min=0.5):
    """The depth map [H, W] that a render(return_depth=True) describes: "median" its median depth, "expected" depth / alpha, where
    alpha >= alpha_min, and 0 (no measurement) elsewhere."""
    if mode not in ("median", "expected"):
        raise ValueError(f'surface_depth: mode must be "median" or "expected", not {mode!r}')
    alpha = render_pkg["alpha"]
    _check(alpha, None, "alpha")
    seen = alpha >= alpha_min
    if mode == "median":
        z = render_pkg["median_depth"]
    else:
        z = render_pkg["depth"] / alpha.clamp_min(1e-6)
    return torch.where(seen, z, torch.zeros_like(z))


def camera_bounds(table):
    """(lo [3], hi [3]) float64: the bounding box of the camera centres of `table` (camera_table's rows), grown by the scene radius
    of scene.getNerfppNorm (1.1 x the largest distance of a centre from their mean)"""
    t = table.detach().cpu().numpy().astype(np.float64)
    m = t[:, :12].reshape(-1, 3, 4)
    centres = -np.einsum("kji,kj->ki", m[:, :, :3], m[:, :, 3])
    radius = 1.1 * np.linalg.norm(centres - centres.mean(0, keepdims=True), axis=1).max()
    return centres.min(0) - radius, centres.max(0) + radius


def extract_mesh(gaussians, cameras, pipe, bg, voxel_size, sdf_trunc=None, bounds=None, depth_mode="median", alpha_min=0.5,
                 depth_max=math.inf, batch=8, depth_min=0.2, timings=None):
    """Render every camera with return_depth=True (no grad), fuse surface_depth(...) and the rendered colours into a TSDFVolume over
    `bounds` = (lo [3], hi [3]) -- default camera_bounds -- with `voxel_size` and `sdf_trunc` (default 4 voxel_size), `batch` maps
    of one image size per launch, and extract -> (vertices, colors, faces). `timings`: a dict that receives the seconds spent in
    "render", "integrate" and "extract" (each ends in a device synchronise) and the lattice's "dims"."""
    import time
    from . import filter3d
    cameras = list(cameras)
    device = gaussians.device
    table = filter3d.camera_table(cameras, device)
    lo, hi = camera_bounds(table) if bounds is None else (np.asarray(bounds[0], np.float64), np.asarray(bounds[1], np.float64))
    if not float(voxel_size) > 0 or not (hi >= lo).all():
        raise ValueError("extract_mesh: voxel_size must be positive and bounds (lo, hi) ordered")
    dims = tuple(_axis_points(e, float(voxel_size)) for e in hi - lo)
    if np.prod(dims, dtype=np.float64) > MAX_POINTS:
        raise ValueError(f"extract_mesh: {dims[0]} x {dims[1]} x {dims[2]} lattice points exceed 2^31 - 1; "
                         f"voxel_size = {fitting_voxel_size(hi - lo, voxel_size):.6g} would fit")
    vol = TSDFVolume(lo, voxel_size, dims, 4.0 * float(voxel_size) if sdf_trunc is None else sdf_trunc, device)
    spent = dict(render=0.0, integrate=0.0, extract=0.0)

    def timed(stage, fn):
        t0 = time.perf_counter()
        out = fn()
        torch.cuda.synchronize(device)
        spent[stage] += time.perf_counter() - t0
        return out

    groups, sizes = {}, table[:, 14:16].cpu().tolist()
    for k, (W, H) in enumerate(sizes):
        groups.setdefault((int(W), int(H)), []).append(k)
    for ids in groups.values():
        for b0 in range(0, len(ids), max(int(batch), 1)):
            chunk = ids[b0:b0 + max(int(batch), 1)]

            def render_chunk():
                depths, colours = [], []
                with torch.no_grad():
                    for k in chunk:
                        pkg = gaussians.render(cameras[k], pipe, bg, return_depth=True)
                        depths.append(surface_depth(pkg, depth_mode, alpha_min))
                        colours.append(pkg["render"])
                return torch.stack(depths), torch.stack(colours)

            depth, colour = timed("render", render_chunk)
            rows = table[torch.as_tensor(chunk, device=device)]
            timed("integrate", lambda: vol.integrate(depth, rows, colour, depth_min=depth_min, depth_max=depth_max))
    vertices, colors, faces = timed("extract", vol.extract)
    if timings is not None:
        timings.update(spent, dims=dims)
    return vertices, colors, faces


def sample_surface(vertices, faces, density, seed=0):
    """-> (points [S, 3] f32, face [S] int32): points on the mesh `vertices` [V, 3], `faces` [F, 3] (int32) at `density` points per
    unit area, what a DTU-style evaluation compares with the scanned cloud (csrc/mesh_sample.hip). A face of area a gets floor(a
    density) samples plus one more with probability frac(a density), decided by a hash of (face, seed); the samples are uniform in
    the triangle, ordered by face. A pure function of its arguments, bit for bit. Zero-area faces and faces with a non-finite vertex
    get none. Raises for a vertex index outside [0, V), for a face with 2^24 or more samples and for more than 2^31 - 1 samples.
    Three launches and one host read (the total). GPU tensors only."""
    density = float(density)
    if not (math.isfinite(density) and density > 0):
        raise ValueError(f"sample_surface: density must be finite and positive, not {density}")
    _check(vertices, None, "vertices")
    if vertices.dim() != 2 or vertices.size(1) != 3:
        raise RuntimeError(f"c3dgs_amd: vertices must have shape (V, 3), not {tuple(vertices.shape)}")
    if not isinstance(faces, torch.Tensor) or faces.dim() != 2 or faces.size(1) != 3:
        raise RuntimeError("c3dgs_amd: faces must be a tensor of shape (F, 3)")
    dev = vertices.device
    v = vertices.detach().contiguous()
    f = _lib.gpu_tensor(faces.detach(), "faces", torch.int32)
    if f.device != dev:
        raise RuntimeError(f"c3dgs_amd: faces must be on the vertices' device {dev}")
    V, F, seed = int(v.size(0)), int(f.size(0)), int(seed) & 0xFFFFFFFF
    lib, total = _lib.lib(), C.c_uint64(0)
    with torch.cuda.device(dev):
        ws = _lib.workspace("mesh_sample", dev, int(lib.c3dgs_mesh_sample_workspace_bytes(F)))
        _lib.check(lib.c3dgs_mesh_sample_count(V, _ptr(v), F, _ptr(f), density, seed, ws.data_ptr(), ws.numel(), C.byref(total),
                                               _stream(dev)))
        S = int(total.value)
        points = torch.empty((S, 3), dtype=torch.float32, device=dev)
        face = torch.empty(S, dtype=torch.int32, device=dev)
        _lib.check(lib.c3dgs_mesh_sample_emit(V, _ptr(v), F, _ptr(f), seed, ws.data_ptr(), ws.numel(), S, _ptr(points), _ptr(face),
                                              _stream(dev)))
    return points, face
