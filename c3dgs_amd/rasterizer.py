"""Host-side mirror of the reference's rasterizer package
(submodules/diff-gaussian-rasterization-no-camera/diff_gaussian_rasterization_no_camera/__init__.py)
on top of the MI355X C-ABI library.  Same names, argument order and error behaviour:

    GaussianRasterizationSettings, GaussianRasterizer, GaussianRasterizerIndexed,
    rasterize_gaussians, rasterize_gaussians_indexed, rasterize_gaussians_indexed_camera,
    getProjectionMatrix, quat_to_mat, mat_to_quat, and `_C` with the five pybind entry points
    (submodules/diff-gaussian-rasterization/ext.cpp:15-21) plus `render_depth`, `render_distortion`, `gaussian_normals`, `render_normal`,
    `render_contrib`, `render_error`, `error_map_l1`, `pose_grad`, `aa_opacity` and `aa_opacity_backward`.

Beyond the reference: `GaussianRasterizationSettings(depth=True)` / `_C.render_depth` add depth, accumulated-opacity and
median-depth maps of a forward (forward-only, csrc/render_depth.hip); `GaussianRasterizationSettings(contrib=True)` /
`_C.render_contrib` add every Gaussian's blend statistics: sum and max of alpha T and the number of (pixel, entry) pairs the
forward blended (forward-only, csrc/render_contrib.hip); `GaussianRasterizationSettings(error_target=gt)` / `_C.render_error` /
`_C.error_map_l1` add every Gaussian's error score, the sum of alpha T x a per-pixel error map (forward-only,
csrc/render_error.hip); `GaussianRasterizer(rs, optimize_camera="exact")` / `GaussianRasterizerIndexed(rs, optimize_camera="exact")`
/ `_C.pose_grad` give the exact gradient of the render with respect to the 7-element pose (csrc/pose_grad.hip, one pass behind
the backward), where `optimize_camera=True` keeps the reference's formula; `GaussianRasterizationSettings(depth_grad=True)` makes
the depth and alpha maps differentiable outputs (csrc/render_maps_backward.hip, one blend replay and one fold in the backward);
`GaussianRasterizationSettings(antialiasing=True)` / `_C.aa_opacity` / `_C.aa_opacity_backward` compensate every opacity for the
0.3 px^2 low-pass (csrc/aa_opacity.hip, one per-Gaussian launch in front of the forward and one behind the backward);
`GaussianRasterizationSettings(distortion=True | (near, far))` / `_C.render_distortion` append the depth-distortion map of
Mip-NeRF 360 as a differentiable last output (csrc/render_distortion.hip; in the backward ONE blend replay for the depth, alpha
and distortion maps, csrc/render_maps_backward.hip); `GaussianRasterizationSettings(normal=True)` / `_C.gaussian_normals` /
`_C.render_normal` append the blended map of the Gaussians' view-space normals as a differentiable last output (csrc/normals.hip,
csrc/render_normal.hip; in the backward ONE blend replay for every map of the call, csrc/render_maps_backward.hip, and the
gradient to the rotations through the normals); c3dgs_amd/normals.py has the depth -> normal stencil and the normal-consistency
term on top of it.

PyTorch is plumbing only here (device memory, streams, autograd bookkeeping); every numeric stage
runs in libc3dgs_hip.so.  There is no CPU path: tensors must live on the GPU.
"""
import ctypes as C
import threading
import math
import weakref
from types import SimpleNamespace
from typing import NamedTuple

import numpy as np
import torch
import torch.nn as nn

from . import _lib
from ._lib import RESIZE_FN, RasterGrads, RasterParams, ptr as _ptr, stream as _stream


# ----------------------------------------------------------------------------- camera helpers
def getProjectionMatrix(intrinsic, device=None):
    """reference __init__.py:19-30 (znear 0.01, zfar 100; returned transposed)."""
    znear, zfar, z_sign = 0.01, 100.0, 1.0
    tanHalfFovY = math.tan((float(intrinsic[1, 1]) / 2))
    tanHalfFovX = math.tan((float(intrinsic[0, 0]) / 2))
    m = torch.tensor([
        [1.0 / tanHalfFovX, 0.0, 0.0, 0.0],
        [0.0, 1.0 / tanHalfFovY, 0.0, 0.0],
        [0.0, 0.0, z_sign * zfar / (zfar - znear), -(zfar * znear) / (zfar - znear)],
        [0.0, 0.0, z_sign, 0.0]], dtype=torch.float32).transpose(0, 1).contiguous()
    return m if device is None else m.to(device)


def quat_to_mat(extrinsic_vector, device=None):
    """reference __init__.py:32-40: (qx,qy,qz,qw,tx,ty,tz) -> 4x4 world->camera, returned transposed.
    The reference evaluates the entries with fp32 tensor arithmetic on the pose's elements; the same fp32 operations in
    the same order here (numpy scalars; one device->host transfer instead of the reference's seven scalar reads).
    The rendering path does not call this: it builds the matrices on the device (camera_matrices)."""
    f = np.float32
    x, y, z, w, tx, ty, tz = [f(v) for v in extrinsic_vector.detach().cpu().float().tolist()]
    one, two = f(1.0), f(2.0)
    d2 = y * y + z * z + x * x
    m = torch.from_numpy(np.array([
        [one + two * (x * x - d2), two * (x * y - w * z), two * (x * z + w * y), tx],
        [two * (x * y + w * z), one + two * (y * y - d2), two * (y * z - w * x), ty],
        [two * (x * z - w * y), two * (y * z + w * x), one + two * (z * z - d2), tz],
        [0.0, 0.0, 0.0, 1.0]], dtype=np.float32)).transpose(0, 1).contiguous()
    return m if device is None else m.to(device)


def mat_to_quat(m, normed=True):
    """reference __init__.py:42-52."""
    w = torch.sqrt(1.0 + m[0, 0] + m[1, 1] + m[2, 2]) / 2.0
    w4 = 4.0 * w
    x = (m[2, 1] - m[1, 2]) / w4
    y = (m[0, 2] - m[2, 0]) / w4
    z = (m[1, 0] - m[0, 1]) / w4
    if normed:
        norm2 = (x * x + y * y + z * z + w * w) ** 0.5
        x, y, z, w = x / norm2, y / norm2, z / norm2, w / norm2
    return x, y, z, w, m[0, 3], m[1, 3], m[2, 3]


# ---- intrinsic -> host scalars. W, H size the outputs and tan(FoV/2) are kernel arguments, so they must be known on the
# host. For a CUDA intrinsic the values are cached per tensor object + in-place version (no device->host read on a hit)
# and VERIFIED by value at the forward's own synchronisation point (see _IntrinsicGuard), so a write the version counter
# does not see (`.data`, raw pointers) cannot go unnoticed either.
_INTRINSIC_CACHE = {}
_INTRINSIC_CACHE_MAX = 512


def _intrinsic_scalars_from_values(vals):
    """vals: the 9 floats of the reference's intrinsic ([0,0]=FoVx, [1,1]=FoVy, [0,2]=W, [1,2]=H; scene/cameras.py:39-41)
    -> (tanfovx, tanfovy, H, W, 1/tan(FoVx/2) as fp32, 1/tan(FoVy/2) as fp32); __init__.py:19-30, 152-157."""
    fovx, fovy = float(vals[0]), float(vals[4])
    tanfovx, tanfovy = float(math.tan(fovx * 0.5)), float(math.tan(fovy * 0.5))
    # getProjectionMatrix divides the fp32 FoV by 2 (exact) and takes tan / reciprocal in double; torch.Tensor rounds to fp32
    inv_x = float(np.float32(1.0 / math.tan(fovx / 2))) if tanfovx != 0 else float("inf")
    inv_y = float(np.float32(1.0 / math.tan(fovy / 2))) if tanfovy != 0 else float("inf")
    return tanfovx, tanfovy, int(vals[5]), int(vals[2]), inv_x, inv_y


def _intrinsic_scalars(intrinsic):
    """-> (scalars, values tuple, cached: bool)."""
    if not intrinsic.is_cuda:
        vals = tuple(intrinsic.detach().reshape(-1).float().tolist())
        return _intrinsic_scalars_from_values(vals), vals, False
    key = id(intrinsic)
    ent = _INTRINSIC_CACHE.get(key)
    if ent is not None and ent[0]() is intrinsic and ent[1] == intrinsic._version and not intrinsic.requires_grad:
        return ent[2], ent[3], True
    vals = tuple(intrinsic.detach().reshape(-1).float().cpu().tolist())            # one device->host read per new tensor
    sc = _intrinsic_scalars_from_values(vals)
    if len(_INTRINSIC_CACHE) >= _INTRINSIC_CACHE_MAX:
        _INTRINSIC_CACHE.clear()
    _INTRINSIC_CACHE[key] = (weakref.ref(intrinsic), intrinsic._version, sc, vals)
    return sc, vals, False


class _IntrinsicGuard:
    """Checks a cache hit of _intrinsic_scalars by VALUE without an extra synchronisation: the 9 floats are copied to pinned
    memory on the caller's stream BEFORE the forward is queued; the forward itself waits for a later event on that stream
    (its read of num_rendered), so afterwards the copy is complete and comparing costs nothing. `ok()` False -> the cache
    entry was stale: it has been dropped and the caller renders again with fresh values."""
    _pinned = threading.local()

    def __init__(self, intrinsic, vals, cached):
        self.active = bool(cached)
        if not self.active:
            return
        ring = getattr(self._pinned, "ring", None)
        if ring is None:
            ring = self._pinned.ring = [[torch.empty(9, dtype=torch.float32).pin_memory(), torch.cuda.Event()] for _ in range(4)]
            self._pinned.k = 0
        self.host, self.ev = ring[self._pinned.k % 4]
        self._pinned.k += 1
        self.ev.synchronize()                                   # the slot's previous copy (four guards ago): long done
        self.intrinsic, self.vals = intrinsic, vals
        with torch.cuda.device(intrinsic.device):
            self.host.copy_(intrinsic.detach().reshape(-1).float(), non_blocking=True)
            self.ev.record(torch.cuda.current_stream(intrinsic.device))

    def ok(self):
        if not self.active:
            return True
        self.ev.synchronize()
        if tuple(self.host.tolist()) == self.vals:
            return True
        _INTRINSIC_CACHE.pop(id(self.intrinsic), None)
        return False


def _camera_on_host(intrinsic_scalars, extrinsic_vector):
    """CPU restatement of csrc/preprocess.hip:camera_from_pose_kernel (same fp32 operations; used for CPU tensors, i.e. by
    the host-logic tests, and as what the GPU tests compare the kernel with)."""
    _, _, _, _, inv_x, inv_y = intrinsic_scalars
    f = np.float32
    view = quat_to_mat(extrinsic_vector).numpy()                 # transposed: view[i][j] = M[j][i]
    pa, pb = f(1.0 * 100.0 / (100.0 - 0.01)), f(-(100.0 * 0.01) / (100.0 - 0.01))
    proj = np.empty((4, 4), np.float32)
    proj[:, 0] = view[:, 0] * f(inv_x)
    proj[:, 1] = view[:, 1] * f(inv_y)
    proj[:, 2] = view[:, 2] * pa + view[:, 3] * pb
    proj[:, 3] = view[:, 2]
    R, t = view[:3, :3].T.astype(np.float64), view[3, :3].astype(np.float64)
    a, b, c, d, e, ff, g, h, k = R.reshape(-1)
    A, B, Cc = e * k - ff * h, -(d * k - ff * g), d * h - e * g
    det = a * A + b * B + c * Cc
    inv = np.array([[A / det, -(b * k - c * h) / det, (b * ff - c * e) / det],
                    [B / det, (a * k - c * g) / det, -(a * ff - c * d) / det],
                    [Cc / det, -(a * h - b * g) / det, (a * e - b * d) / det]])
    campos = (-(inv @ t)).astype(np.float32)
    return torch.from_numpy(view.copy()), torch.from_numpy(proj), torch.from_numpy(campos)


def camera_matrices(intrinsic, extrinsic_vector, device, _guard=None):
    """(viewmatrix, projmatrix, campos, tanfovx, tanfovy, H, W) as the reference's autograd wrapper assembles them
    (__init__.py:152-172). On a GPU the three tensors are computed BY THE DEVICE from the pose's live values
    (c3dgs_camera_from_pose, stream-ordered): nothing about the pose is cached on the host, so in-place optimiser updates of
    the pose -- torch ops, `.data` writes or the package's fused Adam writing through raw pointers -- are always seen, and the
    call never synchronises. The host scalars come from `intrinsic` (cached per tensor, verified by value at the forward's
    synchronisation point when `_guard` is given a list to receive the _IntrinsicGuard)."""
    dev = torch.device(device)
    sc, vals, cached = _intrinsic_scalars(intrinsic)
    tanfovx, tanfovy, image_height, image_width, inv_x, inv_y = sc
    if extrinsic_vector.dim() == 2:
        # the sibling packages' pose: the 4x4 world->camera matrix itself (transposed, as quat_to_mat returns it), set up with
        # the reference's own three tensor operations (diff_gaussian_rasterization/__init__.py:129-135): stream-ordered torch
        # ops on the pose's device, nothing cached on the host
        if tuple(extrinsic_vector.shape) != (4, 4):
            raise RuntimeError("extrinsic must be a 4x4 matrix")
        if _guard is not None and dev.type == "cuda":
            _guard.append(_IntrinsicGuard(intrinsic, vals, cached))
        view = extrinsic_vector.detach().to(device=dev, dtype=torch.float32).contiguous()
        pa, pb = np.float32(1.0 * 100.0 / (100.0 - 0.01)), np.float32(-(100.0 * 0.01) / (100.0 - 0.01))
        P = torch.tensor([[inv_x, 0.0, 0.0, 0.0], [0.0, inv_y, 0.0, 0.0], [0.0, 0.0, float(pa), float(pb)], [0.0, 0.0, 1.0, 0.0]],
                         dtype=torch.float32).transpose(0, 1).contiguous().to(dev)      # == getProjectionMatrix(intrinsic)
        return view, (view @ P).contiguous(), view.inverse()[3, :3].contiguous(), tanfovx, tanfovy, image_height, image_width
    if dev.type != "cuda":
        view, proj, campos = _camera_on_host(sc, extrinsic_vector)
        return view, proj, campos, tanfovx, tanfovy, image_height, image_width
    if _guard is not None:
        _guard.append(_IntrinsicGuard(intrinsic, vals, cached))
    pose = extrinsic_vector.detach()
    if pose.device != dev or pose.dtype != torch.float32 or not pose.is_contiguous():
        pose = pose.to(device=dev, dtype=torch.float32).contiguous()
    if pose.numel() != 7:
        raise RuntimeError("extrinsic_vector must have 7 elements (qx, qy, qz, qw, tx, ty, tz)")
    with torch.cuda.device(dev):
        out = torch.empty(36, dtype=torch.float32, device=dev)
        _lib.check(_lib.lib().c3dgs_camera_from_pose(pose.data_ptr(), inv_x, inv_y, out.data_ptr(), out.data_ptr() + 64,
                                                     out.data_ptr() + 128, _stream(dev)))
    return out[:16].view(4, 4), out[16:32].view(4, 4), out[32:35], tanfovx, tanfovy, image_height, image_width


def cpu_deep_copy_tuple(input_tuple):
    return tuple(item.cpu().clone() if isinstance(item, torch.Tensor) else item for item in input_tuple)


# ----------------------------------------------------------------------------- C-ABI plumbing
class _Scratch:
    """Owns torch uint8 buffers grown by the library through the resize callbacks
    (the reference's resizeFunctional lambdas, rasterize_points.cu:27-33)."""

    def __init__(self, device):
        self.device = device
        self.bufs = {}
        self._cbs = {}

    def callback(self, name):
        def _resize(_user, nbytes):
            t = torch.empty(max(int(nbytes), 1), dtype=torch.uint8, device=self.device)
            self.bufs[name] = t
            return t.data_ptr()
        cb = RESIZE_FN(_resize)
        self._cbs[name] = cb
        return cb

    def release(self):
        """-> the buffers; drops the callbacks. Must be called once the library call has returned: each callback
        closes over `self`, so the object sits in a reference cycle and would otherwise keep its buffers (hundreds of
        MB per call) alive until the cyclic garbage collector runs -- the caching allocator then has to hipMalloc new
        blocks every few calls."""
        bufs, self.bufs, self._cbs = self.bufs, {}, {}
        return bufs


def _buffer_or_empty(bufs, name, device):
    t = bufs.get(name)
    return t if t is not None else torch.empty(0, dtype=torch.uint8, device=device)


def _optional(t, name, dtype=torch.float32):
    """An optional input of the library: None or empty -> None (absent), otherwise checked by _lib.gpu_tensor."""
    if t is None:
        return None
    if not isinstance(t, torch.Tensor):
        raise RuntimeError(f"{name} must be a tensor")
    if t.numel() == 0:
        return None
    return _lib.gpu_tensor(t, name, dtype)


def _params(*, background, means3D, colors, opacity, scales, scale_factors, rotations, scale_modifier, cov3D_precomp,
            viewmatrix, projmatrix, tan_fovx, tan_fovy, H, W, sh, degree, campos, sh_indices, g_indices, prefiltered,
            debug, clamp_color):
    """-> (RasterParams, tensors). `tensors` owns the memory the struct points into: hold it until the call has returned."""
    if means3D.dim() != 2 or means3D.size(1) != 3:
        raise RuntimeError("means3D must have dimensions (num_points, 3)")      # rasterize_points.cu:58-60
    if not means3D.is_cuda:
        raise RuntimeError("c3dgs_amd: means3D must be a GPU tensor (there is no CPU path)")
    t = dict(background=_optional(background, "background"), means3D=_optional(means3D, "means3D"), sh=_optional(sh, "sh"),
             colors_precomp=_optional(colors, "colors_precomp"), opacities=_optional(opacity, "opacities"),
             scales=_optional(scales, "scales"), scale_factors=_optional(scale_factors, "scale_factors"),
             rotations=_optional(rotations, "rotations"), cov3D_precomp=_optional(cov3D_precomp, "cov3D_precomp"),
             sh_indices=_optional(sh_indices, "sh_indices", torch.int64), g_indices=_optional(g_indices, "g_indices", torch.int64),
             viewmatrix=_optional(viewmatrix, "viewmatrix"), projmatrix=_optional(projmatrix, "projmatrix"),
             campos=_optional(campos, "campos"))
    p = RasterParams()
    p.P = int(means3D.size(0))
    p.D = int(degree)
    shp = t["sh"]
    p.M = int(shp.size(1)) if shp is not None else 0                           # rasterize_points.cu:84-88
    p.W, p.H = int(W), int(H)
    p.SHS = int(shp.size(0)) if shp is not None else 0
    p.GS = int(t["scales"].size(0)) if t["scales"] is not None else 0
    for k, v in t.items():
        setattr(p, k, _ptr(v))
    p.tan_fovx, p.tan_fovy, p.scale_modifier = float(tan_fovx), float(tan_fovy), float(scale_modifier)
    p.prefiltered, p.clamp_color, p.debug = int(bool(prefiltered)), int(bool(clamp_color)), int(bool(debug))
    return p, t


def _forward(indexed, background, means3D, colors, opacity, scales, scale_factors, rotations, scale_modifier, cov3D_precomp,
             viewmatrix, projmatrix, tan_fovx, tan_fovy, image_height, image_width, sh, degree, campos, sh_indices,
             g_indices, prefiltered, debug, clamp_color):
    L = _lib.lib()
    p, tensors = _params(background=background, means3D=means3D, colors=colors, opacity=opacity, scales=scales,
                         scale_factors=scale_factors, rotations=rotations, scale_modifier=scale_modifier,
                         cov3D_precomp=cov3D_precomp, viewmatrix=viewmatrix, projmatrix=projmatrix, tan_fovx=tan_fovx,
                         tan_fovy=tan_fovy, H=image_height, W=image_width, sh=sh, degree=degree, campos=campos,
                         sh_indices=sh_indices, g_indices=g_indices, prefiltered=prefiltered, debug=debug, clamp_color=clamp_color)
    dev = means3D.device
    P, H, W = p.P, p.H, p.W
    with torch.cuda.device(dev):
        out_color = torch.empty((3, H, W), dtype=torch.float32, device=dev)
        radii = torch.empty((P,), dtype=torch.int32, device=dev)
        scratch = _Scratch(dev)
        num_rendered = C.c_int32(0)
        fn = L.c3dgs_rasterize_gaussians_indexed if indexed else L.c3dgs_rasterize_gaussians
        rc = fn(C.byref(p), scratch.callback("geom"), None, scratch.callback("binning"), None, scratch.callback("img"), None,
                out_color.data_ptr(), radii.data_ptr() if P > 0 else None, C.byref(num_rendered), _stream(dev))
    bufs = scratch.release()
    _lib.check(rc)
    return (int(num_rendered.value), out_color, radii, _buffer_or_empty(bufs, "geom", dev), _buffer_or_empty(bufs, "binning", dev),
            _buffer_or_empty(bufs, "img", dev))


def _backward(indexed, background, means3D, radii, colors, scales, scale_factors, rotations, scale_modifier, cov3D_precomp,
              viewmatrix, projmatrix, tan_fovx, tan_fovy, dL_dout_color, sh, degree, campos, geomBuffer, R, binningBuffer,
              imageBuffer, debug, sh_indices, g_indices, skip=(), dL_ddepth=None, dL_dalpha=None, dL_ddistortion=None, moment=None,
              near_far=None, dL_dnormal=None, normals=None, normal_axes=None):
    """`dL_ddepth` / `dL_dalpha`: [H, W] fp32 gradients of the depth / alpha maps of _C.render_depth, or None. With either, the call
    goes to the library's *_backward_depth entry (csrc/render_maps_backward.hip: one blend replay in front of the per-Gaussian
    kernels, one small fold behind them) and `dL_dout_color` may be None (the loss does not use the image: no colour blend
    launch). With neither it is the plain backward, launch for launch.
    `dL_ddistortion`: [H, W] fp32 gradient of the distortion map of _C.render_distortion, or None; with it `moment` is that call's
    second output and `near_far` its mode (None: raw), and the call goes to the *_backward_distortion entry
    (csrc/render_maps_backward.hip: one blend replay for the three maps in the place of the depth one). Without it the three
    arguments are ignored.
    `dL_dnormal`: [3, H, W] fp32 gradient of the normal map of _C.render_normal, or None; with it `normals` is the [P, 4] buffer
    of _C.gaussian_normals for the same forward, and the call goes to the *_backward_normal entry
    (csrc/render_maps_backward.hip: one blend replay for EVERY map of the call in the place of the other two, and one more
    fold, which adds into dL_drotations). `normal_axes` = (rotations, g_indices | None): the rows the normals were made from where
    the call blends a `cov3D_precomp` (a filtered covariance, say), which has no axes; the fold's gradient then comes back as one
    more element at the END of the returned tuple, of the shape of those rotations. Without `dL_dnormal` both are ignored.
    `skip`: names among ("dL_dcolors", "dL_dcov3D") that are neither allocated nor written and come back as None. The
    autograd wrappers name the gradients of ABSENT optional inputs: dL_dcolors (12 B x P) and dL_dcov3D (24 B x P) are
    108 MB of stores per 3M-Gaussian backward. The pybind-order entry points (_C.*) skip nothing, like the reference."""
    L = _lib.lib()
    dist = dL_ddistortion is not None
    nrm = dL_dnormal is not None
    maps = dL_ddepth is not None or dL_dalpha is not None or dist or nrm
    if dL_dout_color is not None:
        H, W = int(dL_dout_color.size(1)), int(dL_dout_color.size(2))           # rasterize_points.cu:143-145
    elif maps:
        H, W = (int(v) for v in next(m for m in (dL_ddepth, dL_dalpha, dL_ddistortion, dL_dnormal) if m is not None).shape[-2:])
    else:
        raise RuntimeError("dL_dout_color is required")
    if dist and moment is None:
        raise RuntimeError("c3dgs_amd: dL_ddistortion needs the moment map of _C.render_distortion")
    for name, m in (("dL_ddepth", dL_ddepth), ("dL_dalpha", dL_dalpha), ("dL_ddistortion", dL_ddistortion),
                    ("moment", moment if dist else None)):
        if m is not None:
            _check_map(m, (H, W), means3D.device, name)
    if nrm:
        if normals is None:
            raise RuntimeError("c3dgs_amd: dL_dnormal needs the normals buffer of _C.gaussian_normals")
        if cov3D_precomp is not None and cov3D_precomp.numel() and normal_axes is None:
            raise ValueError("normal: a precomputed covariance has no axes, so no normal (pass normal_axes beside it)")
        _check_map(dL_dnormal, (3, H, W), means3D.device, "dL_dnormal")
        _check_map(normals, (int(means3D.size(0)), 4), means3D.device, "normals")
    # opacities are not an input of the reference's backward either (they live in the geometry buffer)
    p, t = _params(background=background, means3D=means3D, colors=colors, opacity=None, scales=scales,
                   scale_factors=scale_factors, rotations=rotations, scale_modifier=scale_modifier,
                   cov3D_precomp=cov3D_precomp, viewmatrix=viewmatrix, projmatrix=projmatrix, tan_fovx=tan_fovx,
                   tan_fovy=tan_fovy, H=H, W=W, sh=sh, degree=degree, campos=campos, sh_indices=sh_indices,
                   g_indices=g_indices, prefiltered=False, debug=debug, clamp_color=False)
    dev = means3D.device
    P, M = p.P, p.M
    SHS, GS = p.SHS, p.GS
    opt = dict(dtype=torch.float32, device=dev)
    with torch.cuda.device(dev):
        dL_dmeans3D = torch.empty((P, 3), **opt)
        dL_dmeans2D = torch.empty((P, 3), **opt)
        dL_dcolors = None if "dL_dcolors" in skip else torch.empty((P, 3), **opt)
        dL_dopacity = torch.empty((P, 1), **opt)
        dL_dcov3D = None if "dL_dcov3D" in skip else torch.empty((P, 6), **opt)
        if indexed:
            # zeroed + scatter-added inside the library; carved from ONE allocation (sh | rotations | scales, every start
            # 16-byte aligned) so that the library clears them with a single fill
            n_sh, n_rot, n_sc = SHS * M * 3, GS * 4, GS * 3
            flat = torch.empty(n_sh + n_rot + n_sc, **opt)
            dL_dsh = flat[:n_sh].view(SHS, M, 3)
            dL_drotations = flat[n_sh:n_sh + n_rot].view(GS, 4)
            dL_dscales = flat[n_sh + n_rot:].view(GS, 3)
            dL_dscale_factors = torch.empty((P, 1), **opt)
        else:
            # reference shapes (rasterize_points.cu:153-162): [P,M,3], [P,3], [P,4]; rows stay zero when the
            # corresponding input is absent
            dL_dsh = torch.empty((P, M, 3), **opt) if t["sh"] is not None else torch.zeros((P, M, 3), **opt)
            dL_dscales = torch.empty((P, 3), **opt) if t["scales"] is not None else torch.zeros((P, 3), **opt)
            dL_drotations = torch.empty((P, 4), **opt) if t["scales"] is not None else torch.zeros((P, 4), **opt)
            dL_dscale_factors = None
        g = RasterGrads()
        g.dL_dmeans2D, g.dL_dcolors, g.dL_dopacity = dL_dmeans2D.data_ptr(), _ptr(dL_dcolors), dL_dopacity.data_ptr()
        g.dL_dmeans3D, g.dL_dcov3D = dL_dmeans3D.data_ptr(), _ptr(dL_dcov3D)
        g.dL_dsh = dL_dsh.data_ptr() if dL_dsh.numel() else None
        g.dL_dscales = dL_dscales.data_ptr() if dL_dscales.numel() else None
        g.dL_drotations = dL_drotations.data_ptr() if dL_drotations.numel() else None
        g.dL_dscale_factors = dL_dscale_factors.data_ptr() if (dL_dscale_factors is not None and P > 0) else None
        radii_c = radii.contiguous()
        dpix = _optional(dL_dout_color, "dL_dout_color")
        axes_rot = axes_gi = dL_daxes = None
        if nrm and normal_axes is not None:
            axes_rot = _lib.gpu_tensor(normal_axes[0], "normal_axes rotations", torch.float32)
            axes_gi = _optional(normal_axes[1], "normal_axes g_indices", torch.int64)
            dL_daxes = torch.zeros_like(axes_rot)               # the fold adds into it
        scratch = _Scratch(dev)
        if nrm:
            fn = L.c3dgs_rasterize_gaussians_backward_normal_indexed if indexed else L.c3dgs_rasterize_gaussians_backward_normal
            near, far = _near_far(near_far)
            extra = (_ptr(dL_ddepth), _ptr(dL_dalpha), _ptr(dL_dnormal), _ptr(normals), _ptr(axes_rot), _ptr(axes_gi), _ptr(dL_daxes),
                     _ptr(dL_ddistortion), _ptr(moment if dist else None), near, far)
        elif dist:
            fn = (L.c3dgs_rasterize_gaussians_backward_distortion_indexed if indexed else
                  L.c3dgs_rasterize_gaussians_backward_distortion)
            near, far = _near_far(near_far)
            extra = (_ptr(dL_ddepth), _ptr(dL_dalpha), _ptr(dL_ddistortion), _ptr(moment), near, far)
        elif maps:
            fn = L.c3dgs_rasterize_gaussians_backward_depth_indexed if indexed else L.c3dgs_rasterize_gaussians_backward_depth
            extra = (_ptr(dL_ddepth), _ptr(dL_dalpha))
        else:
            fn = L.c3dgs_rasterize_gaussians_backward_indexed if indexed else L.c3dgs_rasterize_gaussians_backward
            extra = ()
        rc = fn(C.byref(p), radii_c.data_ptr() if P > 0 else None,
                geomBuffer.data_ptr() if geomBuffer.numel() else None,
                binningBuffer.data_ptr() if binningBuffer.numel() else None,
                imageBuffer.data_ptr() if imageBuffer.numel() else None, int(R), _ptr(dpix), *extra,
                scratch.callback("ws"), None, C.byref(g), _stream(dev))
    scratch.release()       # the workspace goes back to the (stream-ordered) caching allocator right away
    _lib.check(rc)
    tail = (dL_daxes,) if dL_daxes is not None else ()
    if indexed:
        if t["scales"] is None:
            dL_dscale_factors.zero_()
        return (dL_dmeans2D, dL_dcolors, dL_dopacity, dL_dmeans3D, dL_dcov3D, dL_dsh, dL_dscales, dL_dscale_factors,
                dL_drotations) + tail
    return (dL_dmeans2D, dL_dcolors, dL_dopacity, dL_dmeans3D, dL_dcov3D, dL_dsh, dL_dscales, dL_drotations) + tail


# ---- the five entry points with the pybind argument order (ext.cpp:15-21, rasterize_points.h:18-122), and render_depth
def _c_rasterize_gaussians(background, means3D, colors, opacity, scales, rotations, scale_modifier, cov3D_precomp, viewmatrix,
                           projmatrix, tan_fovx, tan_fovy, image_height, image_width, sh, degree, campos, prefiltered, debug,
                           clamp_color):
    return _forward(False, background, means3D, colors, opacity, scales, None, rotations, scale_modifier, cov3D_precomp,
                    viewmatrix, projmatrix, tan_fovx, tan_fovy, image_height, image_width, sh, degree, campos, None, None,
                    prefiltered, debug, clamp_color)


def _c_rasterize_gaussians_indexed(background, means3D, colors, opacity, scales, scale_factors, rotations, scale_modifier,
                                   cov3D_precomp, viewmatrix, projmatrix, tan_fovx, tan_fovy, image_height, image_width, sh,
                                   degree, campos, sh_indices, g_indices, prefiltered, debug, clamp_color):
    return _forward(True, background, means3D, colors, opacity, scales, scale_factors, rotations, scale_modifier,
                    cov3D_precomp, viewmatrix, projmatrix, tan_fovx, tan_fovy, image_height, image_width, sh, degree, campos,
                    sh_indices, g_indices, prefiltered, debug, clamp_color)


def _c_rasterize_gaussians_backward(background, means3D, radii, colors, scales, rotations, scale_modifier, cov3D_precomp,
                                    viewmatrix, projmatrix, tan_fovx, tan_fovy, dL_dout_color, sh, degree, campos,
                                    geomBuffer, R, binningBuffer, imageBuffer, debug, skip=(), dL_ddepth=None, dL_dalpha=None,
                                    **distortion):
    return _backward(False, background, means3D, radii, colors, scales, None, rotations, scale_modifier, cov3D_precomp,
                     viewmatrix, projmatrix, tan_fovx, tan_fovy, dL_dout_color, sh, degree, campos, geomBuffer, R,
                     binningBuffer, imageBuffer, debug, None, None, skip, dL_ddepth, dL_dalpha, **distortion)


def _c_rasterize_gaussians_backward_indexed(background, means3D, radii, colors, scales, scale_factors, rotations,
                                            scale_modifier, cov3D_precomp, viewmatrix, projmatrix, tan_fovx, tan_fovy,
                                            dL_dout_color, sh, degree, campos, geomBuffer, R, binningBuffer, imageBuffer,
                                            debug, sh_indices, g_indices, skip=(), dL_ddepth=None, dL_dalpha=None, **distortion):
    return _backward(True, background, means3D, radii, colors, scales, scale_factors, rotations, scale_modifier,
                     cov3D_precomp, viewmatrix, projmatrix, tan_fovx, tan_fovy, dL_dout_color, sh, degree, campos, geomBuffer,
                     R, binningBuffer, imageBuffer, debug, sh_indices, g_indices, skip, dL_ddepth, dL_dalpha, **distortion)


def _c_mark_visible(means3D, viewmatrix, projmatrix):
    """rasterize_points.cu:202-221 -> bool[P]."""
    L = _lib.lib()
    if not means3D.is_cuda:
        raise RuntimeError("c3dgs_amd: means3D must be a GPU tensor (there is no CPU path)")
    m = _optional(means3D, "means3D")
    P = int(means3D.size(0))
    present = torch.empty((P,), dtype=torch.bool, device=means3D.device)     # the kernel writes every element
    if P != 0:
        v, pr = _optional(viewmatrix, "viewmatrix"), _optional(projmatrix, "projmatrix")
        with torch.cuda.device(means3D.device):
            rc = L.c3dgs_mark_visible(P, m.data_ptr(), v.data_ptr(), pr.data_ptr(), present.data_ptr(), _stream(means3D.device))
        _lib.check(rc)
    return present


def _mark_visible_from_pose(positions, extrinsic_vector):
    """markVisible for a 7-element pose on the GPU in ONE launch (c3dgs_mark_visible_pose: same flags, bit for bit, as
    camera_matrices + _C.mark_visible, without the single-thread matrix kernel in front). None: not that case."""
    if not positions.is_cuda or extrinsic_vector.dim() != 1 or extrinsic_vector.numel() != 7:
        return None
    dev = positions.device
    pose = extrinsic_vector.detach()
    if pose.device != dev or pose.dtype != torch.float32 or not pose.is_contiguous():
        pose = pose.to(device=dev, dtype=torch.float32).contiguous()
    m = _optional(positions, "means3D")
    P = int(positions.size(0))
    present = torch.empty((P,), dtype=torch.bool, device=dev)
    if P != 0:
        with torch.cuda.device(dev):
            rc = _lib.lib().c3dgs_mark_visible_pose(P, m.data_ptr(), pose.data_ptr(), present.data_ptr(), _stream(dev))
        _lib.check(rc)
    return present


def _c_render_depth(P, W, H, R, geomBuffer, binningBuffer, imgBuffer):
    """Depth, accumulated opacity and median depth of the forward that filled the three buffers (c3dgs_render_depth):
    -> (depth, alpha, median), each [H, W] fp32, on the current stream. `depth` = sum_k alpha_k T_k z_k is NOT normalised
    (divide by `alpha`); `median` = depth of the first blended Gaussian that takes T below 0.5, 0 where none does.
    Forward-only. Valid before or after the matching backward."""
    if not imgBuffer.is_cuda:
        raise RuntimeError("c3dgs_amd: render_depth needs the forward's GPU buffers (there is no CPU path)")
    dev = imgBuffer.device
    P, W, H, R = int(P), int(W), int(H), int(R)
    with torch.cuda.device(dev):
        out = torch.empty((3, max(H, 0), max(W, 0)), dtype=torch.float32, device=dev)
        ptr = lambda t: t.data_ptr() if t is not None and t.numel() else None
        rc = _lib.lib().c3dgs_render_depth(P, W, H, R, ptr(geomBuffer), ptr(binningBuffer), ptr(imgBuffer), ptr(out[0]), ptr(out[1]),
                                           ptr(out[2]), _stream(dev))
    _lib.check(rc)
    return out[0], out[1], out[2]


def _near_far(near_far):
    """None / False / True -> (0.0, 0.0), the library's raw mode; (near, far) with 0 < near < far -> the two floats, as the fp32
    values the library receives: a pair that is in order as doubles but not as floats (a near that underflows, a pair that
    rounds to one value) is refused here, with ValueError, and not by the library"""
    if near_far is None or near_far is True or near_far is False:
        return 0.0, 0.0
    try:
        with np.errstate(over="ignore"):                        # a far beyond fp32 becomes inf, which is refused below
            near, far = (float(np.float32(float(v))) for v in near_far)
    except (TypeError, ValueError):
        raise ValueError(f"distortion must be False, True or (near, far), not {near_far!r}") from None
    if not 0.0 < near < far or math.isinf(far):
        raise ValueError(f"distortion=(near, far) needs 0 < near < far, finite; got {near_far!r}")
    return near, far


def _c_render_distortion(P, W, H, R, geomBuffer, binningBuffer, imgBuffer, near_far=None):
    """The depth-distortion map of the forward that filled the three buffers (c3dgs_render_distortion): -> (distortion, moment),
    each [H, W] fp32, on the current stream. distortion = sum_i sum_j w_i w_j |s_i - s_j| over the pixel's blended entries, with
    w = alpha T and s = the view-space depth z (`near_far` None) or 2DGS's far / (far - near) (1 - near / z) (`near_far` a pair with
    0 < near < far); moment = sum_k w_k s_k, which the backward needs next to the gradient of `distortion`. Valid before or after
    the matching backward."""
    if not imgBuffer.is_cuda:
        raise RuntimeError("c3dgs_amd: render_distortion needs the forward's GPU buffers (there is no CPU path)")
    dev = imgBuffer.device
    P, W, H, R = int(P), int(W), int(H), int(R)
    near, far = _near_far(near_far)
    with torch.cuda.device(dev):
        out = torch.empty((2, max(H, 0), max(W, 0)), dtype=torch.float32, device=dev)
        ptr = lambda t: t.data_ptr() if t is not None and t.numel() else None
        rc = _lib.lib().c3dgs_render_distortion(P, W, H, R, ptr(geomBuffer), ptr(binningBuffer), ptr(imgBuffer), near, far,
                                                ptr(out[0]), ptr(out[1]), _stream(dev))
    _lib.check(rc)
    return out[0], out[1]


def _c_gaussian_normals(means3D, scales, rotations, g_indices, viewmatrix):
    """The per-Gaussian normals of a view (c3dgs_gaussian_normals): -> [P, 4] fp32 {n_x, n_y, n_z, sigma (m + 1)} on the current
    stream. n is the Gaussian's shortest axis in VIEW space (x right, y down, z forward), unit length, facing the camera: with
    q, s the Gaussian's rows of `rotations` / `scales` (`g_indices` None) or the codebook rows g_indices selects,
    m = argmin_j s[j] on the raw row (lowest j on a tie), c = column m of the rotation matrix of q (q not normalised),
    v = R_view c / |c| (0 where |c| == 0), sigma = -1 where v . p > 0 for the view-space mean p, else +1, n = sigma v. Every row
    is written, culled or not."""
    if not means3D.is_cuda:
        raise RuntimeError("c3dgs_amd: gaussian_normals needs GPU tensors (there is no CPU path)")
    dev = means3D.device
    P = int(means3D.size(0))
    t = [_lib.gpu_tensor(means3D, "means3D", torch.float32) if P else None, _optional(scales, "scales"),
         _optional(rotations, "rotations"), _optional(g_indices, "g_indices", torch.int64), _optional(viewmatrix, "viewmatrix")]
    if P and (t[1] is None or t[2] is None):
        raise ValueError("normal: scales and rotations are required (a precomputed covariance has no axes, so no normal)")
    with torch.cuda.device(dev):
        out = torch.empty((P, 4), dtype=torch.float32, device=dev)
        rc = _lib.lib().c3dgs_gaussian_normals(P, *(_ptr(v) for v in t), _ptr(out) if P else None, _stream(dev))
    _lib.check(rc)
    return out


def _c_render_normal(P, W, H, R, geomBuffer, binningBuffer, imgBuffer, normals):
    """The normal map of the forward that filled the three buffers (c3dgs_render_normal): -> [3, H, W] fp32 on the current stream,
    sum_k w_k n_k over the pixel's blended entries with w = alpha T and n = the rows of `normals` (_C.gaussian_normals);
    accumulated like a colour channel, not normalised, no background term. Valid before or after the matching backward."""
    if not imgBuffer.is_cuda:
        raise RuntimeError("c3dgs_amd: render_normal needs the forward's GPU buffers (there is no CPU path)")
    dev = imgBuffer.device
    P, W, H, R = int(P), int(W), int(H), int(R)
    _check_map(normals, (P, 4), dev, "normals")
    with torch.cuda.device(dev):
        out = torch.empty((3, max(H, 0), max(W, 0)), dtype=torch.float32, device=dev)
        ptr = lambda t: t.data_ptr() if t is not None and t.numel() else None
        rc = _lib.lib().c3dgs_render_normal(P, W, H, R, ptr(geomBuffer), ptr(binningBuffer), ptr(imgBuffer), ptr(normals),
                                            ptr(out), _stream(dev))
    _lib.check(rc)
    return out


class _GrowOnly:
    """One uint8 device buffer per device that only grows (a _Scratch whose buffer outlives the call): the workspace of
    _C.render_contrib, R x 13 bytes per call. Its content means nothing between calls (the library clears the flag bytes it reads),
    so calls on one stream may share it; like every scratch here it belongs to the stream the calls are queued on."""

    def __init__(self):
        self.bufs = {}

    def get(self, device, nbytes):
        t = self.bufs.get(device)
        if t is None or t.numel() < nbytes:
            t = self.bufs[device] = torch.empty(max(int(nbytes), 256), dtype=torch.uint8, device=device)
        return t


_contrib_workspace = _GrowOnly()


def _c_render_contrib(P, W, H, R, geomBuffer, binningBuffer, imgBuffer):
    """Blend statistics of the forward that filled the three buffers (c3dgs_render_contrib): -> (weight_sum f32 [P],
    weight_max f32 [P], hits int32 [P] holding the library's uint32 counts), on the current stream. Over the (pixel, entry)
    pairs the forward blended, with w = alpha T: sum of w, max of w, number of pairs. Rows of culled or never-blended Gaussians
    are exact zeros. Forward-only. Valid before or after the matching backward."""
    if not imgBuffer.is_cuda:
        raise RuntimeError("c3dgs_amd: render_contrib needs the forward's GPU buffers (there is no CPU path)")
    dev = imgBuffer.device
    P, W, H, R = int(P), int(W), int(H), int(R)
    L = _lib.lib()
    with torch.cuda.device(dev):
        out = torch.empty((2, max(P, 0)), dtype=torch.float32, device=dev)
        hits = torch.empty((max(P, 0),), dtype=torch.int32, device=dev)
        if P == 0:
            return out[0], out[1], hits
        ws = _contrib_workspace.get(dev, L.c3dgs_contrib_workspace_bytes(P, R))
        ptr = lambda t: t.data_ptr() if t is not None and t.numel() else None
        rc = L.c3dgs_render_contrib(P, W, H, R, ptr(geomBuffer), ptr(binningBuffer), ptr(imgBuffer), ws.data_ptr(), ptr(out[0]),
                                    ptr(out[1]), ptr(hits), _stream(dev))
    _lib.check(rc)
    return out[0], out[1], hits


_error_workspace = _GrowOnly()


def _c_render_error(P, W, H, R, geomBuffer, binningBuffer, imgBuffer, pixel_map):
    """Error scores of the forward that filled the three buffers (c3dgs_render_error): -> err_sum f32 [P] on the current stream:
    per Gaussian, over the (pixel, entry) pairs the forward blended, the sum of fl(alpha T x pixel_map[pixel]). `pixel_map` is
    any finite fp32 [H, W] device tensor. Rows of culled or never-blended Gaussians are exact zeros; a map of ones gives
    _C.render_contrib's weight_sum bit for bit. Forward-only. Valid before or after the matching backward. Its workspace
    (R x 5 bytes, grow-only) is its own."""
    if not imgBuffer.is_cuda:
        raise RuntimeError("c3dgs_amd: render_error needs the forward's GPU buffers (there is no CPU path)")
    dev = imgBuffer.device
    P, W, H, R = int(P), int(W), int(H), int(R)
    _check_map(pixel_map, (H, W), dev, "render_error: pixel_map")
    L = _lib.lib()
    with torch.cuda.device(dev):
        out = torch.empty((max(P, 0),), dtype=torch.float32, device=dev)
        if P == 0:
            return out
        ws = _error_workspace.get(dev, L.c3dgs_error_workspace_bytes(P, R))
        ptr = lambda t: t.data_ptr() if t is not None and t.numel() else None
        rc = L.c3dgs_render_error(P, W, H, R, ptr(geomBuffer), ptr(binningBuffer), ptr(imgBuffer), ws.data_ptr(),
                                  pixel_map.data_ptr(), out.data_ptr(), _stream(dev))
    _lib.check(rc)
    return out


_pose_workspace = _GrowOnly()


def _c_pose_grad(means3D, dL_dmeans3D, dL_dcov3D, dL_dcolors, sh, degree, sh_indices, cov3D_precomp, scales, rotations,
                 scale_factors, g_indices, scale_modifier, geomBuffer, radii, extrinsic_vector):
    """Exact dL/dpose [7] (qx, qy, qz, qw, tx, ty, tz) from a finished backward's outputs (c3dgs_pose_grad), on the current stream:
    two launches, no float atomics, bitwise reproducible. `dL_dmeans3D`, `dL_dcov3D` and (with `sh`) `dL_dcolors` are the backward's
    own tensors, not skipped; the other arguments are the forward's inputs, absent ones None or empty; `geomBuffer` and `radii`
    are the forward's. The pose is read on the device by the kernels: nothing about it is cached on the host. Its workspace
    (96 bytes per 256 Gaussians, grow-only) is its own."""
    if not means3D.is_cuda:
        raise RuntimeError("c3dgs_amd: pose_grad needs GPU tensors (there is no CPU path)")
    dev = means3D.device
    P = int(means3D.size(0))
    pose = extrinsic_vector.detach()
    if pose.device != dev or pose.dtype != torch.float32 or not pose.is_contiguous():
        pose = pose.to(device=dev, dtype=torch.float32).contiguous()
    if pose.dim() != 1 or pose.numel() != 7:
        raise RuntimeError("pose_grad: extrinsic_vector must have 7 elements (qx, qy, qz, qw, tx, ty, tz)")
    t = dict(means3D=_optional(means3D, "means3D"), dL_dmeans3D=_optional(dL_dmeans3D, "dL_dmeans3D"),
             dL_dcov3D=_optional(dL_dcov3D, "dL_dcov3D"), dL_dcolors=_optional(dL_dcolors, "dL_dcolors"), sh=_optional(sh, "sh"),
             sh_indices=_optional(sh_indices, "sh_indices", torch.int64), cov3D_precomp=_optional(cov3D_precomp, "cov3D_precomp"),
             scales=_optional(scales, "scales"), rotations=_optional(rotations, "rotations"),
             scale_factors=_optional(scale_factors, "scale_factors"), g_indices=_optional(g_indices, "g_indices", torch.int64),
             radii=_optional(radii, "radii", torch.int32))
    for name, width in (("dL_dmeans3D", 3), ("dL_dcov3D", 6), ("dL_dcolors", 3), ("cov3D_precomp", 6), ("scale_factors", 1),
                        ("sh_indices", 1), ("g_indices", 1), ("radii", 1)):
        if t[name] is not None and t[name].numel() != P * width:
            raise RuntimeError(f"pose_grad: {name} must have {P} x {width} elements, not {t[name].numel()}")
    shp = t["sh"]
    M = int(shp.size(1)) if shp is not None else 0
    L = _lib.lib()
    with torch.cuda.device(dev):
        out = torch.empty(7, dtype=torch.float32, device=dev)
        ws = _pose_workspace.get(dev, L.c3dgs_pose_grad_workspace_bytes(P))
        rc = L.c3dgs_pose_grad(P, int(degree), M, float(scale_modifier), _ptr(t["means3D"]), _ptr(t["dL_dmeans3D"]),
                               _ptr(t["dL_dcov3D"]), _ptr(t["dL_dcolors"]), _ptr(shp), _ptr(t["sh_indices"]),
                               _ptr(t["cov3D_precomp"]), _ptr(t["scales"]), _ptr(t["rotations"]), _ptr(t["scale_factors"]),
                               _ptr(t["g_indices"]), geomBuffer.data_ptr() if geomBuffer.numel() else None, _ptr(t["radii"]),
                               pose.data_ptr(), ws.data_ptr(), out.data_ptr(), _stream(dev))
    _lib.check(rc)
    return out


def _aa_params(means3D, opacities, scales, rotations, scale_factors, g_indices, cov3D_precomp, scale_modifier, viewmatrix,
               tan_fovx, tan_fovy, image_height, image_width, prefiltered, debug):
    """the RasterParams of the two aa_opacity entries: the projection's inputs alone; the index pair only with its codebooks"""
    if not means3D.is_cuda:
        raise RuntimeError("c3dgs_amd: aa_opacity needs GPU tensors (there is no CPU path)")
    by_codebook = scales is not None and scales.numel() != 0 and g_indices is not None and g_indices.numel() != 0
    p, t = _params(background=None, means3D=means3D, colors=None, opacity=opacities, scales=scales,
                   scale_factors=scale_factors if by_codebook else None, rotations=rotations, scale_modifier=scale_modifier,
                   cov3D_precomp=cov3D_precomp, viewmatrix=viewmatrix, projmatrix=None, tan_fovx=tan_fovx, tan_fovy=tan_fovy,
                   H=image_height, W=image_width, sh=None, degree=0, campos=None, sh_indices=None,
                   g_indices=g_indices if by_codebook else None, prefiltered=prefiltered, debug=debug, clamp_color=False)
    P = p.P
    for name, width in (("opacities", 1), ("cov3D_precomp", 6), ("scale_factors", 1), ("g_indices", 1)):
        if t[name] is not None and t[name].numel() != P * width:
            raise RuntimeError(f"aa_opacity: {name} must have {P} x {width} elements, not {t[name].numel()}")
    if P > 0 and t["opacities"] is None:
        raise RuntimeError("aa_opacity: opacities is required")
    return p, t


def _c_aa_opacity(means3D, opacities, scales, rotations, scale_factors, g_indices, cov3D_precomp, scale_modifier, viewmatrix,
                  tan_fovx, tan_fovy, image_height, image_width, prefiltered=False, debug=False, rho=True):
    """Opacity compensation of the antialiased mode (c3dgs_aa_opacity), one launch on the current stream: -> (o', rho) with
    o' = opacities * rho shaped like `opacities` and rho f32 [P] (None with rho=False). Absent inputs None or empty; `g_indices`
    and `scale_factors` count only with `scales` / `rotations`. Forward-only: its gradient is _C.aa_opacity_backward."""
    p, t = _aa_params(means3D, opacities, scales, rotations, scale_factors, g_indices, cov3D_precomp, scale_modifier, viewmatrix,
                      tan_fovx, tan_fovy, image_height, image_width, prefiltered, debug)
    dev = means3D.device
    with torch.cuda.device(dev):
        out = torch.empty_like(t["opacities"]) if t["opacities"] is not None else torch.empty((0, 1), dtype=torch.float32, device=dev)
        rho_t = torch.empty((p.P,), dtype=torch.float32, device=dev) if rho else None
        if p.P > 0:                                 # an empty tensor has no address to hand over, and nothing would be launched
            _lib.check(_lib.lib().c3dgs_aa_opacity(C.byref(p), out.data_ptr(), _ptr(rho_t), _stream(dev)))
    return out, rho_t


def _c_aa_opacity_backward(means3D, opacities, radii, scales, rotations, scale_factors, g_indices, cov3D_precomp, scale_modifier,
                           viewmatrix, tan_fovx, tan_fovy, image_height, image_width, dL_dopacity, dL_dmeans3D=None,
                           dL_dcov3D=None, dL_dscales=None, dL_drotations=None, dL_dscale_factors=None, prefiltered=False,
                           debug=False):
    """The chain through rho behind a finished backward (c3dgs_aa_opacity_backward), one launch on the current stream, IN PLACE:
    `dL_dopacity` holds the rasterizer's gradient with respect to o' and becomes rho times it; the terms through rho are added into
    the other gradient tensors given (contiguous fp32, the backward's own; None is skipped). `opacities` are the raw ones."""
    p, t = _aa_params(means3D, opacities, scales, rotations, scale_factors, g_indices, cov3D_precomp, scale_modifier, viewmatrix,
                      tan_fovx, tan_fovy, image_height, image_width, prefiltered, debug)
    dev = means3D.device
    g = RasterGrads()
    P = p.P
    widths = dict(dL_dopacity=P, dL_dmeans3D=3 * P, dL_dcov3D=6 * P, dL_dscale_factors=P,
                  dL_dscales=3 * (p.GS if p.g_indices else P), dL_drotations=4 * (p.GS if p.g_indices else P))
    for name, gt in (("dL_dopacity", dL_dopacity), ("dL_dmeans3D", dL_dmeans3D), ("dL_dcov3D", dL_dcov3D), ("dL_dscales", dL_dscales),
                     ("dL_drotations", dL_drotations), ("dL_dscale_factors", dL_dscale_factors)):
        if gt is None or gt.numel() == 0:
            continue
        if not gt.is_cuda or gt.device != dev or gt.dtype != torch.float32 or not gt.is_contiguous():
            raise RuntimeError(f"aa_opacity_backward: {name} must be a contiguous float32 tensor on {dev}")
        if gt.numel() != widths[name]:
            raise RuntimeError(f"aa_opacity_backward: {name} must have {widths[name]} elements, not {gt.numel()}")
        setattr(g, name, gt.data_ptr())
    radii_c = _optional(radii, "radii", torch.int32)
    if radii_c is not None and radii_c.numel() != P:
        raise RuntimeError(f"aa_opacity_backward: radii must have {P} elements, not {radii_c.numel()}")
    if P == 0:                                      # empty tensors have no address to hand over, and nothing would be launched
        return
    with torch.cuda.device(dev):
        rc = _lib.lib().c3dgs_aa_opacity_backward(C.byref(p), _ptr(radii_c), C.byref(g), _stream(dev))
    _lib.check(rc)


def _check_map(t, shape, dev, what):
    """the usual RuntimeError for a map or image of the wrong kind"""
    if not isinstance(t, torch.Tensor) or not t.is_cuda or t.device != dev:
        raise RuntimeError(f"c3dgs_amd: {what} must be a tensor on {dev}")
    if t.dtype != torch.float32:
        raise RuntimeError(f"c3dgs_amd: {what} must be float32, not {t.dtype}")
    if tuple(t.shape) != tuple(shape):
        raise RuntimeError(f"c3dgs_amd: {what} must have shape {tuple(shape)}, not {tuple(t.shape)}")
    if not t.is_contiguous():
        raise RuntimeError(f"c3dgs_amd: {what} must be contiguous")


def _c_error_map_l1(img, gt):
    """planar fp32 [C, H, W] image and target on one device -> [H, W]: the mean over the channels of |img - gt|, channels added
    in ascending order, then one division by C (c3dgs_error_map_l1), on the current stream."""
    if not isinstance(img, torch.Tensor) or img.dim() != 3 or not img.is_cuda:
        raise RuntimeError("c3dgs_amd: error_map_l1: img must be a [C, H, W] tensor on the GPU (there is no CPU path)")
    _check_map(img, img.shape, img.device, "error_map_l1: img")
    _check_map(gt, img.shape, img.device, "error_map_l1: gt")
    C, H, W = (int(v) for v in img.shape)
    with torch.cuda.device(img.device):
        out = torch.empty((H, W), dtype=torch.float32, device=img.device)
        rc = _lib.lib().c3dgs_error_map_l1(C, H, W, img.data_ptr(), gt.data_ptr(), out.data_ptr(), _stream(img.device))
    _lib.check(rc)
    return out


_C = SimpleNamespace(
    render_depth=_c_render_depth,
    render_distortion=_c_render_distortion,
    gaussian_normals=_c_gaussian_normals,
    render_normal=_c_render_normal,
    render_contrib=_c_render_contrib,
    render_error=_c_render_error,
    error_map_l1=_c_error_map_l1,
    pose_grad=_c_pose_grad,
    aa_opacity=_c_aa_opacity,
    aa_opacity_backward=_c_aa_opacity_backward,
    rasterize_gaussians=_c_rasterize_gaussians,
    rasterize_gaussians_backward=_c_rasterize_gaussians_backward,
    rasterize_gaussians_indexed=_c_rasterize_gaussians_indexed,
    rasterize_gaussians_backward_indexed=_c_rasterize_gaussians_backward_indexed,
    mark_visible=_c_mark_visible,
)


# ----------------------------------------------------------------------------- autograd functions
def _call_debug(fn, args, debug, dump, **kwargs):
    """reference __init__.py:179-206: on failure under debug, dump a CPU copy of the (positional) arguments and re-raise."""
    if debug:
        cpu_args = cpu_deep_copy_tuple(args)
        try:
            return fn(*args, **kwargs)
        except Exception as ex:
            torch.save(cpu_args, dump)
            print(f"\nAn error occured. Writing {dump} for debugging.")
            raise ex
    return fn(*args, **kwargs)


def _autograd_forward(ctx, indexed, means3D, sh, sh_indices, g_indices, colors_precomp, opacities, scales, scale_factors,
                      rotations, cov3Ds_precomp, raster_settings, extrinsic_vector):
    """forward of the three Functions (reference __init__.py:138-211, 328-408, 539-620). Not indexed: sh_indices, g_indices
    and scale_factors are None. `args` is the pybind order of the entry it goes to (what snapshot_fw.dump holds)."""
    rs = raster_settings
    dev = means3D.device
    antialiasing = bool(getattr(rs, "antialiasing", False))
    normal = bool(getattr(rs, "normal", False))
    axes = None
    if normal and cov3Ds_precomp is not None and cov3Ds_precomp.numel():
        # a covariance has no axes. Where the caller blends one it has built itself (a filtered one: Sigma + f^2 I has the axes of
        # Sigma, and adding the same amount to every squared scale leaves the shortest axis where it was), the scales and rotations
        # given BESIDE it are the rows the normals are made from; the rasterizer itself sees the covariance alone
        if scales is None or rotations is None or not scales.numel() or not rotations.numel():
            raise ValueError("normal=True: a precomputed covariance has no axes, so no normal (pass scales and rotations beside it)")
        axes = (scales, rotations)
        scales = rotations = _empty()
    raw_opacities = opacities
    for _attempt in range(2):          # a second pass only if the cached intrinsic scalars turn out stale (_IntrinsicGuard)
        guard = []
        view, proj, campos, tanfovx, tanfovy, H, W = camera_matrices(rs.intrinsic, extrinsic_vector, dev, guard)
        if antialiasing:
            # one per-Gaussian launch in front of the forward: the rasterizer runs on o' = o rho (csrc/aa_opacity.hip)
            opacities = _C.aa_opacity(means3D, raw_opacities, scales, rotations, scale_factors, g_indices, cov3Ds_precomp,
                                      rs.scale_modifier, view, tanfovx, tanfovy, H, W, rs.prefiltered, rs.debug, rho=False)[0]
        if indexed:
            fn = _C.rasterize_gaussians_indexed
            args = (rs.bg, means3D, colors_precomp, opacities, scales, scale_factors, rotations, rs.scale_modifier, cov3Ds_precomp,
                    view, proj, tanfovx, tanfovy, H, W, sh, rs.sh_degree, campos, sh_indices, g_indices, rs.prefiltered, rs.debug,
                    rs.clamp_color)
        else:
            fn = _C.rasterize_gaussians
            args = (rs.bg, means3D, colors_precomp, opacities, scales, rotations, rs.scale_modifier, cov3Ds_precomp, view, proj,
                    tanfovx, tanfovy, H, W, sh, rs.sh_degree, campos, rs.prefiltered, rs.debug, rs.clamp_color)
        num_rendered, color, radii, geomBuffer, binningBuffer, imgBuffer = _call_debug(fn, args, rs.debug, "snapshot_fw.dump")
        if all(g.ok() for g in guard):
            break
    # with `raster_settings.depth`: the (depth, alpha, median) maps, queued right behind the forward on the same stream;
    # otherwise no launch
    extras = ()
    # `raster_settings.distortion` implies depth_grad's outputs, in their positions
    distortion = getattr(rs, "distortion", False)
    depth_grad = bool(getattr(rs, "depth_grad", False)) or distortion is not False or normal
    if getattr(rs, "depth", False) or depth_grad:
        extras = _C.render_depth(int(means3D.size(0)), W, H, num_rendered, geomBuffer, binningBuffer, imgBuffer)
    # with `raster_settings.contrib`: (weight_sum, weight_max, hits) per Gaussian, behind whatever `depth` added
    if getattr(rs, "contrib", False):
        extras = tuple(extras) + _C.render_contrib(int(means3D.size(0)), W, H, num_rendered, geomBuffer, binningBuffer, imgBuffer)
    # with `raster_settings.error_target`: err_sum per Gaussian under the map mean |color - target|, behind the others
    target = getattr(rs, "error_target", None)
    if target is not None:
        _check_map(target, color.shape, color.device, "error_target")
        emap = _C.error_map_l1(color.detach(), target)
        extras = tuple(extras) + (_C.render_error(int(means3D.size(0)), W, H, num_rendered, geomBuffer, binningBuffer, imgBuffer, emap),)
    # with `raster_settings.distortion`: the distortion map, the LAST output and a differentiable one; its moment map stays here
    # for the backward
    n_fixed = len(extras)
    moment = None
    if distortion is not False:
        dist_map, moment = _C.render_distortion(int(means3D.size(0)), W, H, num_rendered, geomBuffer, binningBuffer, imgBuffer,
                                                distortion)
        extras = tuple(extras) + (dist_map,)
    # with `raster_settings.normal`: one per-Gaussian launch and one more replay; the normal map goes behind everything else and
    # is differentiable, the per-Gaussian normals stay here for the backward
    normals = None
    if normal:
        normals = _C.gaussian_normals(means3D, *(axes or (scales, rotations)), g_indices if indexed else None, view)
        extras = tuple(extras) + (_C.render_normal(int(means3D.size(0)), W, H, num_rendered, geomBuffer, binningBuffer, imgBuffer,
                                                   normals),)
    ctx.raster_settings = rs
    ctx.indexed = indexed
    ctx.num_rendered = num_rendered
    ctx.camera = (view, proj, campos, tanfovx, tanfovy)
    # the raw opacities are an input of the backward in the antialiased mode only (the plain backward reads o' from the geometry buffer)
    ctx.antialiasing = antialiasing
    ctx.image_size = (H, W)
    ctx.save_for_backward(extrinsic_vector, colors_precomp, means3D, scales, scale_factors, rotations, cov3Ds_precomp, radii, sh,
                          geomBuffer, binningBuffer, imgBuffer, sh_indices, g_indices, *((raw_opacities,) if antialiasing else ()),
                          *((normals,) if normals is not None else ()), *((axes[1],) if axes is not None else ()),
                          *((moment,) if moment is not None else ()))
    ctx.distortion = distortion
    ctx.normal = normal
    ctx.normal_axes = axes is not None
    ctx.image_shape = tuple(color.shape)
    # without this, autograd hands backward a zero-filled int32[P] "gradient" for radii on every call (a 12 MB fill at P = 3M)
    ctx.set_materialize_grads(False)
    # the extras are forward-only: non-differentiable like radii, no gradient flows through them -- except, with
    # `raster_settings.depth_grad`, the depth and alpha maps (outputs 2 and 3), whose gradients the backward takes
    ctx.depth_grad = depth_grad
    ctx.mark_non_differentiable(radii, *(extras[2:n_fixed] if depth_grad else extras))
    return (color, radii) + tuple(extras)


def _fit(grad, inp):
    """The reference returns full-size gradients even for absent ("empty") inputs; autograd ignores them because
    those inputs never require grad. Returning None for them is equivalent and skips the shape check."""
    if inp is None or inp.numel() == 0:
        return None
    return grad


def _map_grads(ctx, params):
    """(dL_ddepth, dL_dalpha) among the gradients of the outputs behind the image (radii, depth, alpha, median, ...): what the
    loss sent through the two maps of a `depth_grad` forward, as contiguous fp32, or (None, None)."""
    if not getattr(ctx, "depth_grad", False):
        return None, None
    fit = lambda g: None if g is None else g.to(torch.float32).contiguous()            # noqa: E731
    # behind them, of a `distortion` forward: dL_ddistortion, the gradient of the last output; of a `normal` forward the normal
    # map is the last output and the distortion map, if any, the one in front of it: then (.., dL_ddistortion | None, dL_dnormal)
    if getattr(ctx, "normal", False):
        dist = fit(params[-2]) if getattr(ctx, "distortion", False) is not False else None
        return tuple(fit(g) for g in params[1:3]) + (dist, fit(params[-1]))
    last = (fit(params[-1]),) if getattr(ctx, "distortion", False) is not False else ()
    return tuple(fit(g) for g in params[1:3]) + last


def _autograd_backward(ctx, grad_out_color, exact_pose=False, map_grads=(None, None)):
    """backward of the Functions -> the gradients BY THE NAME OF THE forward INPUT they belong to (None for an absent
    input); each Function lays them out in its own input order. `args`: pybind order again (snapshot_bw.dump).
    `exact_pose`: the pose requires grad in exact mode. Then dL_dcov3D (and, with SH, dL_dcolors) are not skipped, _C.pose_grad is
    queued behind the backward on the same stream and its 7-vector comes back as `.pose`; the caller-visible gradients of absent
    inputs stay None (_fit). False: exactly the launches and stores of a backward without it, `.pose` is None."""
    rs = ctx.raster_settings
    (extrinsic_vector, colors_precomp, means3D, scales, scale_factors, rotations, cov3Ds_precomp, radii, sh, geomBuffer,
     binningBuffer, imgBuffer, sh_indices, g_indices) = ctx.saved_tensors[:14]
    grad_depth, grad_alpha = map_grads[:2]
    grad_dist = map_grads[2] if len(map_grads) > 2 else None
    maps = dict(dL_ddepth=grad_depth, dL_dalpha=grad_alpha) if (grad_depth is not None or grad_alpha is not None) else {}
    if grad_dist is not None:
        # the moment map is the last saved tensor; without a gradient for the distortion map the backward is today's
        maps = dict(dL_ddepth=grad_depth, dL_dalpha=grad_alpha, dL_ddistortion=grad_dist, moment=ctx.saved_tensors[-1],
                    near_far=ctx.distortion)
    grad_normal = map_grads[3] if len(map_grads) > 3 else None
    if grad_normal is not None:
        # the per-Gaussian normals sit behind the 14 fixed tensors and the raw opacities; without a gradient for the normal map
        # the backward is what the other settings give
        at = 14 + int(bool(getattr(ctx, "antialiasing", False)))
        maps = dict(maps or dict(dL_ddepth=grad_depth, dL_dalpha=grad_alpha), dL_dnormal=grad_normal, normals=ctx.saved_tensors[at])
        if getattr(ctx, "normal_axes", False):
            # the rotations the normals were made from, beside a precomputed covariance: the fold's gradient is theirs
            maps["normal_axes"] = (ctx.saved_tensors[at + 1], g_indices if ctx.indexed else None)
    if grad_out_color is None and not maps:
        # set_materialize_grads(False): an image nobody differentiated through arrives as None (backward still runs when only
        # `radii` was used downstream of a graph that needs grad); the library wants a dense dL/dC
        grad_out_color = torch.zeros(ctx.image_shape, dtype=torch.float32, device=means3D.device)
    view, proj, campos, tanfovx, tanfovy = ctx.camera
    skip = tuple(n for n, t in (("dL_dcolors", colors_precomp), ("dL_dcov3D", cov3Ds_precomp)) if t is None or t.numel() == 0)
    sh_used = sh is not None and sh.numel() != 0
    if exact_pose:
        skip = tuple(n for n in skip if n != "dL_dcov3D" and not (n == "dL_dcolors" and sh_used))
    grad_scale_factors = None
    if ctx.indexed:
        args = (rs.bg, means3D, radii, colors_precomp, scales, scale_factors, rotations, rs.scale_modifier, cov3Ds_precomp, view,
                proj, tanfovx, tanfovy, grad_out_color, sh, rs.sh_degree, campos, geomBuffer, ctx.num_rendered, binningBuffer,
                imgBuffer, rs.debug, sh_indices, g_indices)
        (grad_means2D, grad_colors_precomp, grad_opacities, grad_means3D, grad_cov3Ds_precomp, grad_sh, grad_scales,
         grad_scale_factors, grad_rotations, *grad_axes) = _call_debug(_C.rasterize_gaussians_backward_indexed, args, rs.debug,
                                                                       "snapshot_bw.dump", skip=skip, **maps)
    else:
        args = (rs.bg, means3D, radii, colors_precomp, scales, rotations, rs.scale_modifier, cov3Ds_precomp, view, proj,
                tanfovx, tanfovy, grad_out_color, sh, rs.sh_degree, campos, geomBuffer, ctx.num_rendered, binningBuffer,
                imgBuffer, rs.debug)
        (grad_means2D, grad_colors_precomp, grad_opacities, grad_means3D, grad_cov3Ds_precomp, grad_sh, grad_scales,
         grad_rotations, *grad_axes) = _call_debug(_C.rasterize_gaussians_backward, args, rs.debug, "snapshot_bw.dump", skip=skip,
                                                   **maps)
    if getattr(ctx, "antialiasing", False):
        # behind the whole backward (the depth maps' part included) on the same stream: dL/do' becomes dL/do and the terms through
        # rho are added to the gradients the backward has just written (csrc/aa_opacity.hip)
        present = lambda g, inp: g if (g is not None and inp is not None and inp.numel() != 0) else None
        H, W = ctx.image_size
        by_codebook = present(grad_scales, scales) is not None         # scale factors count only with the codebooks
        _C.aa_opacity_backward(means3D, ctx.saved_tensors[14], radii, scales, rotations, scale_factors, g_indices, cov3Ds_precomp,
                               rs.scale_modifier, view, tanfovx, tanfovy, H, W, grad_opacities, dL_dmeans3D=grad_means3D,
                               dL_dcov3D=present(grad_cov3Ds_precomp, cov3Ds_precomp), dL_dscales=present(grad_scales, scales),
                               dL_drotations=present(grad_rotations, rotations),
                               dL_dscale_factors=present(grad_scale_factors, scale_factors) if by_codebook else None,
                               prefiltered=rs.prefiltered, debug=rs.debug)
    grad_pose = None
    if exact_pose:
        # the indexed entry always carries both index tensors; the library wants each only with what it indexes
        by_codebook = ctx.indexed and scales is not None and scales.numel() != 0
        grad_pose = _C.pose_grad(means3D, grad_means3D, grad_cov3Ds_precomp, grad_colors_precomp if sh_used else None, sh,
                                 rs.sh_degree, sh_indices if sh_used else None, cov3Ds_precomp, scales, rotations,
                                 scale_factors if by_codebook else None, g_indices if by_codebook else None,
                                 rs.scale_modifier, geomBuffer, radii, extrinsic_vector).to(extrinsic_vector.device)
    return SimpleNamespace(pose=grad_pose, means3D=grad_means3D, means2D=grad_means2D, sh=_fit(grad_sh, sh),
                           colors_precomp=_fit(grad_colors_precomp, colors_precomp), opacities=grad_opacities,
                           scales=_fit(grad_scales, scales), scale_factors=_fit(grad_scale_factors, scale_factors),
                           rotations=grad_axes[0] if grad_axes else _fit(grad_rotations, rotations), cov3Ds_precomp=_fit(grad_cov3Ds_precomp, cov3Ds_precomp))


class _RasterizeGaussians(torch.autograd.Function):
    """reference __init__.py:136-323."""

    @staticmethod
    def forward(ctx, means3D, means2D, sh, colors_precomp, opacities, scales, rotations, cov3Ds_precomp, raster_settings,
                extrinsic_vector):
        return _autograd_forward(ctx, False, means3D, sh, None, None, colors_precomp, opacities, scales, None, rotations,
                                 cov3Ds_precomp, raster_settings, extrinsic_vector)

    @staticmethod
    def backward(ctx, grad_out_color, *params):
        g = _autograd_backward(ctx, grad_out_color, map_grads=_map_grads(ctx, params))
        return (g.means3D, g.means2D, g.sh, g.colors_precomp, g.opacities, g.scales, g.rotations, g.cov3Ds_precomp, None, None)


class _RasterizeGaussiansIndexed(torch.autograd.Function):
    """reference __init__.py:326-530."""

    @staticmethod
    def forward(ctx, means3D, means2D, sh, sh_indices, g_indices, colors_precomp, opacities, scales, scale_factors, rotations,
                cov3Ds_precomp, raster_settings, extrinsic_vector):
        return _autograd_forward(ctx, True, means3D, sh, sh_indices, g_indices, colors_precomp, opacities, scales,
                                 scale_factors, rotations, cov3Ds_precomp, raster_settings, extrinsic_vector)

    @staticmethod
    def backward(ctx, grad_out_color, *params):
        g = _autograd_backward(ctx, grad_out_color, map_grads=_map_grads(ctx, params))
        return (g.means3D, g.means2D, g.sh, None, None, g.colors_precomp, g.opacities, g.scales, g.scale_factors, g.rotations,
                g.cov3Ds_precomp, None, None)


def camera_pose_jacobian_sum(means3D, intrinsic, extrinsic_vector, du, dv):
    """grad_mat[7] of the reference's _RasterizeGaussiansIndexedCamera.backward (__init__.py:674-844):
    sum_i grad_params[i,p,0]*du_i + grad_params[i,p,1]*dv_i, with the reference's closed-form
    grad_params written in factored form.  With
        numU, numV, den   the reference's three repeated polynomials in (X,Y,Z,q,t),
    every entry is  A_p * num/den^2 + B_p/den ; the A_p are shared by the u and v columns."""
    X, Y, Z = means3D[:, 0], means3D[:, 1], means3D[:, 2]
    fx, fy = intrinsic[0, 0].to(means3D.device), intrinsic[1, 1].to(means3D.device)
    qx, qy, qz, qw, tx, ty, tz = extrinsic_vector.to(means3D.device)
    ix, iy = 1.0 / torch.tan(fx / 2), 1.0 / torch.tan(fy / 2)
    # constants of the reference's znear=0.01 / zfar=100 projection: zfar/(zfar-znear) etc.
    a1, a2, a4 = 1.000100010001, 2.000200020002, 4.000400040004
    b1, b2, b4 = 0.01000100010001, 0.02000200020002, 0.04000400040004
    Xs, Ys = X * ix, Y * iy
    numU = (Xs * (2.0 * qx ** 2 - 4.0 * qx * qy - 2.0 * qz ** 2 + 1.0) + Ys * (-2.0 * qw * qz + 2.0 * qx * qy)
            + Z * (a2 * qw * qy + a2 * qx * qz + tx) - b2 * qw * qy - b2 * qx * qz)
    numV = (Xs * (2.0 * qw * qz + 2.0 * qx * qy) + Ys * (-4.0 * qx * qy + 2.0 * qy ** 2 - 2.0 * qz ** 2 + 1.0)
            + Z * (-a2 * qw * qx + a2 * qy * qz + ty) + b2 * qw * qx - b2 * qy * qz)
    den = (Xs * (-2.0 * qw * qy + 2.0 * qx * qz) + Ys * (2.0 * qw * qx + 2.0 * qy * qz)
           + Z * (-a4 * qx * qy + tz + a1) + b4 * qx * qy - b1)
    inv = 1.0 / den
    ru, rv = numU * inv * inv, numV * inv * inv
    zero = torch.zeros_like(X)
    A = [2.0 * Xs * qy - 2.0 * Ys * qx,
         -2.0 * Xs * qz - 2.0 * Ys * qw + a4 * Z * qy - b4 * qy,
         2.0 * Xs * qw - 2.0 * Ys * qz + a4 * Z * qx - b4 * qx,
         -2.0 * Xs * qx - 2.0 * Ys * qy,
         zero, zero, -Z]
    Bu = [-2.0 * Ys * qz + a2 * Z * qy - b2 * qy,
          Xs * (4.0 * qx - 4.0 * qy) + 2.0 * Ys * qy + a2 * Z * qz - b2 * qz,
          -4.0 * Xs * qx + 2.0 * Ys * qx + a2 * Z * qw - b2 * qw,
          -4.0 * Xs * qz - 2.0 * Ys * qw + a2 * Z * qx - b2 * qx,
          Z, zero, zero]
    Bv = [2.0 * Xs * qz - a2 * Z * qx + b2 * qx,
          2.0 * Xs * qy - 4.0 * Ys * qy - a2 * Z * qw + b2 * qw,
          2.0 * Xs * qx + Ys * (-4.0 * qx + 4.0 * qy) + a2 * Z * qz - b2 * qz,
          2.0 * Xs * qw - 4.0 * Ys * qz + a2 * Z * qy - b2 * qy,
          zero, Z, zero]
    out = torch.zeros(7, dtype=torch.float32, device=means3D.device)
    for p in range(7):
        gu = A[p] * ru + Bu[p] * inv
        gv = A[p] * rv + Bv[p] * inv
        if p == 5:
            gu = zero                      # reference sets grad_params[:,5,0] = 0 and [:,4,1] = 0 explicitly
        if p == 4:
            gv = zero
        out[p] = (gu * du + gv * dv).sum()
    return out


class _RasterizeGaussiansIndexedCamera(torch.autograd.Function):
    """reference __init__.py:537-866: the indexed rasterizer plus the analytic camera-pose gradient.
    The pose gradient is only evaluated when extrinsic_vector requires grad (in finetune.py it does
    not, and the reference computes and discards it)."""

    @staticmethod
    def forward(ctx, means3D, means2D, sh, sh_indices, g_indices, colors_precomp, opacities, scales, scale_factors, rotations,
                cov3Ds_precomp, raster_settings, extrinsic_vector):
        return _autograd_forward(ctx, True, means3D, sh, sh_indices, g_indices, colors_precomp, opacities, scales,
                                 scale_factors, rotations, cov3Ds_precomp, raster_settings, extrinsic_vector)

    @staticmethod
    def backward(ctx, grad_out_color, *params):
        g = _autograd_backward(ctx, grad_out_color)
        grad_mat = None
        if ctx.needs_input_grad[12]:
            extrinsic_vector, _, means3D = ctx.saved_tensors[:3]
            grad_mat = camera_pose_jacobian_sum(means3D, ctx.raster_settings.intrinsic, extrinsic_vector,
                                                g.means2D[:, 0], g.means2D[:, 1]).to(extrinsic_vector.device)
        return (g.means3D, g.means2D, g.sh, None, None, g.colors_precomp, g.opacities, g.scales, g.scale_factors, g.rotations,
                g.cov3Ds_precomp, None, grad_mat)


class _RasterizeGaussiansCameraExact(torch.autograd.Function):
    """_RasterizeGaussians plus the exact pose gradient (csrc/pose_grad.hip); no reference counterpart. Evaluated only when
    extrinsic_vector requires grad: otherwise the backward is _RasterizeGaussians', launch for launch."""

    @staticmethod
    def forward(ctx, means3D, means2D, sh, colors_precomp, opacities, scales, rotations, cov3Ds_precomp, raster_settings,
                extrinsic_vector):
        return _autograd_forward(ctx, False, means3D, sh, None, None, colors_precomp, opacities, scales, None, rotations,
                                 cov3Ds_precomp, raster_settings, extrinsic_vector)

    @staticmethod
    def backward(ctx, grad_out_color, *params):
        g = _autograd_backward(ctx, grad_out_color, exact_pose=ctx.needs_input_grad[9])
        return (g.means3D, g.means2D, g.sh, g.colors_precomp, g.opacities, g.scales, g.rotations, g.cov3Ds_precomp, None, g.pose)


class _RasterizeGaussiansIndexedCameraExact(torch.autograd.Function):
    """_RasterizeGaussiansIndexedCamera with the exact pose gradient in place of the reference's formula."""

    @staticmethod
    def forward(ctx, means3D, means2D, sh, sh_indices, g_indices, colors_precomp, opacities, scales, scale_factors, rotations,
                cov3Ds_precomp, raster_settings, extrinsic_vector):
        return _autograd_forward(ctx, True, means3D, sh, sh_indices, g_indices, colors_precomp, opacities, scales,
                                 scale_factors, rotations, cov3Ds_precomp, raster_settings, extrinsic_vector)

    @staticmethod
    def backward(ctx, grad_out_color, *params):
        g = _autograd_backward(ctx, grad_out_color, exact_pose=ctx.needs_input_grad[12])
        return (g.means3D, g.means2D, g.sh, None, None, g.colors_precomp, g.opacities, g.scales, g.scale_factors, g.rotations,
                g.cov3Ds_precomp, None, g.pose)


def rasterize_gaussians(means3D, means2D, sh, colors_precomp, opacities, scales, rotations, cov3Ds_precomp, raster_settings,
                        extrinsic_vector):
    return _RasterizeGaussians.apply(means3D, means2D, sh, colors_precomp, opacities, scales, rotations, cov3Ds_precomp,
                                     raster_settings, extrinsic_vector)


def rasterize_gaussians_indexed(means3D, means2D, sh, sh_indices, g_indices, colors_precomp, opacities, scales, scale_factors,
                                rotations, cov3Ds_precomp, raster_settings, extrinsic_vector):
    return _RasterizeGaussiansIndexed.apply(means3D, means2D, sh, sh_indices, g_indices, colors_precomp, opacities, scales,
                                            scale_factors, rotations, cov3Ds_precomp, raster_settings, extrinsic_vector)


def rasterize_gaussians_indexed_camera(means3D, means2D, sh, sh_indices, g_indices, colors_precomp, opacities, scales,
                                       scale_factors, rotations, cov3Ds_precomp, raster_settings, extrinsic_vector):
    _check_depth_grad_camera(raster_settings, True)
    _check_antialiasing_camera(raster_settings, True)
    return _RasterizeGaussiansIndexedCamera.apply(means3D, means2D, sh, sh_indices, g_indices, colors_precomp, opacities,
                                                  scales, scale_factors, rotations, cov3Ds_precomp, raster_settings,
                                                  extrinsic_vector)


def rasterize_gaussians_camera_exact(means3D, means2D, sh, colors_precomp, opacities, scales, rotations, cov3Ds_precomp,
                                     raster_settings, extrinsic_vector):
    _check_depth_grad_camera(raster_settings, True)
    _check_antialiasing_camera(raster_settings, True)
    return _RasterizeGaussiansCameraExact.apply(means3D, means2D, sh, colors_precomp, opacities, scales, rotations,
                                                cov3Ds_precomp, raster_settings, extrinsic_vector)


def rasterize_gaussians_indexed_camera_exact(means3D, means2D, sh, sh_indices, g_indices, colors_precomp, opacities, scales,
                                             scale_factors, rotations, cov3Ds_precomp, raster_settings, extrinsic_vector):
    _check_depth_grad_camera(raster_settings, True)
    _check_antialiasing_camera(raster_settings, True)
    return _RasterizeGaussiansIndexedCameraExact.apply(means3D, means2D, sh, sh_indices, g_indices, colors_precomp, opacities,
                                                       scales, scale_factors, rotations, cov3Ds_precomp, raster_settings,
                                                       extrinsic_vector)


def _check_depth_grad_camera(raster_settings, optimize_camera):
    """`depth_grad` with a pose gradient is not covered yet: the maps' gradient does not reach the pose"""
    if optimize_camera is not False and getattr(raster_settings, "depth_grad", False):
        raise ValueError("depth_grad=True cannot be combined with optimize_camera: the gradient to the camera pose through the "
                         "depth and alpha maps is not implemented")
    if optimize_camera is not False and getattr(raster_settings, "distortion", False) is not False:
        raise ValueError("distortion cannot be combined with optimize_camera: the gradient to the camera pose through the "
                         "depth, alpha and distortion maps is not implemented")
    if optimize_camera is not False and getattr(raster_settings, "normal", False):
        raise ValueError("normal=True cannot be combined with optimize_camera: the gradient to the camera pose through the "
                         "depth, alpha and normal maps is not implemented")


def _distortion_setting(value):
    """False | True | (near, far) of GaussianRasterizationSettings(distortion=), checked and normalised"""
    if value is None or value is False:
        return False
    if value is True:
        return True
    return _near_far(value)


def _check_antialiasing_camera(raster_settings, optimize_camera):
    """`antialiasing` with a pose gradient is not covered: the opacity factor's dependence on the pose is not differentiated"""
    if optimize_camera is not False and getattr(raster_settings, "antialiasing", False):
        raise ValueError("antialiasing=True cannot be combined with optimize_camera: the gradient to the camera pose through the "
                         "opacity compensation is not implemented")


def _check_optimize_camera(value):
    """False | True (the reference's pose gradient) | "exact" (csrc/pose_grad.hip)"""
    if value is True or value is False or value == "exact":
        return value
    raise ValueError(f'optimize_camera must be False, True or "exact", not {value!r}')


# ----------------------------------------------------------------------------- public modules
class _SettingsFields(NamedTuple):
    """reference __init__.py:868-878, plus `depth` (last, optional)."""
    intrinsic: torch.Tensor
    extrinsic_vector: torch.Tensor
    bg: torch.Tensor
    scale_modifier: float
    sh_degree: int
    prefiltered: bool
    debug: bool
    clamp_color: bool
    # True: the rasterizers return (color, radii, depth, alpha, median) -- see _C.render_depth. Forward-only: the three extra
    # maps are non-differentiable, no gradient flows through them. False: (color, radii), the same launches as ever.
    depth: bool = False


class GaussianRasterizationSettings(_SettingsFields):
    """The settings tuple above plus `contrib`, the last constructor argument (optional, by keyword or as the tenth positional).
    True: the rasterizers append (weight_sum, weight_max, hits), each [P] -- see _C.render_contrib -- behind the outputs they
    return otherwise: (color, radii, weight_sum, weight_max, hits), or with `depth` (color, radii, depth, alpha, median,
    weight_sum, weight_max, hits). Forward-only and non-differentiable. False: no launch.
    `contrib` is an attribute beside the tuple's elements, not one of them: the tuple keeps the length, order and `_fields` that
    callers who unpack or index it rely on (`depth` stays its last element). `_replace` carries it (and accepts it); what
    works on the tuple's elements alone does not see it: `==`, `hash`, `_asdict`, `_make` and pickling compare, list or rebuild the
    nine elements only, and two settings that differ in `contrib` alone compare equal.
    `error_target` (keyword only, default None) is a second such attribute: a [3, H, W] fp32 tensor on the device, the view's
    ground truth. With it the rasterizers queue _C.error_map_l1(color, error_target) and _C.render_error behind the forward and
    append (err_sum,), [P], behind whatever `depth` and `contrib` added; forward-only and non-differentiable, the backward is
    unchanged. A wrong shape, dtype or device raises RuntimeError. None: no launch.
    `depth_grad` (keyword only, default False) is a third such attribute. True implies the outputs of `depth=True`, in the same
    position -- (color, radii, depth, alpha, median, ...) with the forward's bits -- and makes `depth` and `alpha` differentiable
    outputs: a loss on them reaches every input the image reaches (csrc/render_maps_backward.hip: one blend replay and one small
    fold added to the backward). `median` (piecewise constant) and `radii` stay non-differentiable. When neither map receives a
    gradient the backward issues the plain backward's launches. The gradient to the camera pose through the maps is not covered
    yet: with `depth_grad`, `optimize_camera` other than False raises ValueError.
    `antialiasing` (keyword only, default False) is a fourth such attribute. True: every Gaussian's opacity is multiplied by
    rho = sqrt(max(0.000025, det Sigma2D / det(Sigma2D + 0.3 I))) in front of the rasterizer (csrc/aa_opacity.hip: one
    per-Gaussian launch in front of the forward, one behind the backward, which chains dL/d(opacity rho) to the opacity, the mean,
    the covariance, scales, rotations and scale factors), so that a splat smaller than a pixel is not drawn with the energy of
    the low-passed one. Radii, tile keys and conics are the plain render's; every output, the extra ones included, sees the
    compensated opacity. False: the plain rasterizer's launches and bits. The gradient to the camera pose through rho is not
    covered: with `antialiasing`, `optimize_camera` other than False raises ValueError.
    `distortion` (keyword only, default False) is a fifth such attribute: False, True (raw mode: s = the view-space depth z) or
    a pair (near, far) with 0 < near < far (s = far / (far - near) (1 - near / z), 2DGS's mapping; anything else raises
    ValueError). Not False: the rasterizers return depth_grad's outputs in their positions, differentiable as there, and append
    the depth-distortion map sum_i sum_j w_i w_j |s_i - s_j| of every pixel's blended entries, [H, W], as the LAST element of the
    tuple (csrc/render_distortion.hip, one more forward replay), a differentiable output as well: a loss on it reaches every input
    the depth map reaches, through ONE blend replay in the backward for the three maps (csrc/render_maps_backward.hip, in
    the place of the depth maps' replay). When it receives no gradient the backward is depth_grad's. With `distortion`,
    `optimize_camera` other than False raises ValueError, as with `depth_grad`.
    `normal` (keyword only, default False) is a sixth such attribute. True: the rasterizers return depth_grad's outputs in their
    positions, differentiable as there, and append the normal map N[3, H, W] = sum_k w_k n_k of every pixel's blended entries as
    the LAST element of the tuple, behind `distortion` when both are set (csrc/normals.hip, csrc/render_normal.hip: one
    per-Gaussian launch and one more forward replay). n is the Gaussian's shortest axis in VIEW space (x right, y down, z
    forward), unit length and facing the camera (_C.gaussian_normals says how it is chosen); N is not normalised and has no
    background term, like `depth`. It is a differentiable output: a loss on it reaches the opacities, means and covariances
    through w, and the rotations through n as well, through ONE blend replay in the backward for every map of the call
    (csrc/render_maps_backward.hip, in the place of the other two) and one more fold. When it receives no gradient the backward
    is what the other settings give. A precomputed covariance has no axes: with `normal`, `cov3D_precomp` alone raises ValueError.
    A caller that blends a covariance it has built from scales and rotations (a filtered one) passes the pair BESIDE it: the
    rasterizer sees the covariance, the normals are made from the pair, and the rotations receive the normals' gradient.
    `optimize_camera` other than False raises ValueError."""
    contrib = False
    error_target = None
    depth_grad = False
    antialiasing = False
    distortion = False
    normal = False

    def __new__(cls, *args, contrib=False, error_target=None, depth_grad=False, antialiasing=False, distortion=False, normal=False,
                **kwargs):
        n = len(cls._fields)
        if len(args) == n + 1:
            args, contrib = args[:n], args[n]
        self = super().__new__(cls, *args, **kwargs)
        self.contrib = bool(contrib)
        self.error_target = error_target
        self.depth_grad = bool(depth_grad)
        self.antialiasing = bool(antialiasing)
        self.distortion = _distortion_setting(distortion)
        self.normal = bool(normal)
        return self

    def _replace(self, **kwargs):
        contrib = kwargs.pop("contrib", self.contrib)
        error_target = kwargs.pop("error_target", self.error_target)
        depth_grad = kwargs.pop("depth_grad", self.depth_grad)
        antialiasing = kwargs.pop("antialiasing", self.antialiasing)
        distortion = kwargs.pop("distortion", self.distortion)
        normal = kwargs.pop("normal", self.normal)
        new = super()._replace(**kwargs)
        new.contrib = bool(contrib)
        new.error_target = error_target
        new.depth_grad = bool(depth_grad)
        new.antialiasing = bool(antialiasing)
        new.distortion = _distortion_setting(distortion)
        new.normal = bool(normal)
        return new


def _check_exclusive(shs, colors_precomp, scales, rotations, cov3D_precomp, axes_beside_covariance=False):
    """`axes_beside_covariance` (settings.normal): a scale / rotation pair NEXT TO a precomputed covariance is accepted; the
    rasterizer blends the covariance and the normals are made from the pair"""
    if (shs is None and colors_precomp is None) or (shs is not None and colors_precomp is not None):
        raise Exception("Please provide excatly one of either SHs or precomputed colors!")
    if axes_beside_covariance and cov3D_precomp is not None and scales is not None and rotations is not None:
        return
    if ((scales is None or rotations is None) and cov3D_precomp is None) or (
            (scales is not None or rotations is not None) and cov3D_precomp is not None):
        raise Exception("Please provide exactly one of either scale/rotation pair or precomputed 3D covariance!")


def _empty():
    return torch.Tensor([])


def _absent_to_empty(*tensors):
    """The reference's `if x is None: x = torch.Tensor([])` for the optional inputs of a module's forward."""
    return [_empty() if t is None else t for t in tensors]


class _Rasterizer(nn.Module):
    """What the module classes of both packages share."""

    def __init__(self, raster_settings):
        super().__init__()
        self.raster_settings = raster_settings

    def markVisible(self, positions, extrinsic_vector):
        """A 7-element pose on the GPU takes the one-launch path; a 4x4 matrix (or CPU tensors) the general one."""
        with torch.no_grad():
            present = _mark_visible_from_pose(positions, extrinsic_vector)
            if present is not None:
                return present
            view, proj = camera_matrices(self.raster_settings.intrinsic, extrinsic_vector, positions.device)[:2]
            return _C.mark_visible(positions, view, proj)


class GaussianRasterizer(_Rasterizer):
    """reference __init__.py:881-948. `forward` accepts the pose as `extrinsic_vector=` (what the reference's own
    caller passes, scene/gaussian_model.py:874) and, for compatibility with the declared signature, `extrinsic=`.
    `optimize_camera="exact"`: a 7-element pose that requires grad receives the exact gradient of the render
    (rasterize_gaussians_camera_exact). False (the default, the reference's behaviour): no pose gradient. The reference has no
    pose formula for this path, so True is not accepted."""

    def __init__(self, raster_settings, optimize_camera=False):
        super().__init__(raster_settings)
        if optimize_camera is True:
            raise ValueError('GaussianRasterizer: optimize_camera must be False or "exact" (the reference formula exists for '
                             'the indexed rasterizer only)')
        self.optimize_camera = _check_optimize_camera(optimize_camera)
        _check_depth_grad_camera(raster_settings, self.optimize_camera)
        _check_antialiasing_camera(raster_settings, self.optimize_camera)

    def forward(self, means3D, means2D, opacities, shs=None, colors_precomp=None, scales=None, rotations=None,
                cov3D_precomp=None, extrinsic_vector=None, extrinsic=None):
        _check_depth_grad_camera(self.raster_settings, self.optimize_camera)
        _check_antialiasing_camera(self.raster_settings, self.optimize_camera)
        _check_exclusive(shs, colors_precomp, scales, rotations, cov3D_precomp, bool(getattr(self.raster_settings, "normal", False)))
        if extrinsic_vector is None:
            extrinsic_vector = extrinsic if extrinsic is not None else self.raster_settings.extrinsic_vector
        shs, colors_precomp, scales, rotations, cov3D_precomp = _absent_to_empty(shs, colors_precomp, scales, rotations,
                                                                                 cov3D_precomp)
        fn = rasterize_gaussians_camera_exact if self.optimize_camera == "exact" else rasterize_gaussians
        return fn(means3D, means2D, shs, colors_precomp, opacities, scales, rotations, cov3D_precomp, self.raster_settings,
                  extrinsic_vector)


class GaussianRasterizerIndexed(_Rasterizer):
    """reference __init__.py:951-1046. `optimize_camera`: False; True, the reference's pose gradient (camera_pose_jacobian_sum,
    dL/dmeans2D through a projection formula); or "exact", the gradient of the render itself (rasterize_gaussians_indexed_camera_exact)."""

    def __init__(self, raster_settings, optimize_camera=False):
        super().__init__(raster_settings)
        self.optimize_camera = optimize_camera
        _check_depth_grad_camera(raster_settings, bool(optimize_camera))
        _check_antialiasing_camera(raster_settings, bool(optimize_camera))

    def forward(self, means3D, means2D, opacities, sh_indices, g_indices, shs=None, colors_precomp=None, scales=None,
                scale_factors=None, rotations=None, cov3D_precomp=None, extrinsic_vector=None):
        _check_depth_grad_camera(self.raster_settings, bool(self.optimize_camera))
        _check_antialiasing_camera(self.raster_settings, bool(self.optimize_camera))
        _check_exclusive(shs, colors_precomp, scales, rotations, cov3D_precomp, bool(getattr(self.raster_settings, "normal", False)))
        if extrinsic_vector is None:
            extrinsic_vector = self.raster_settings.extrinsic_vector
        shs, colors_precomp, scales, scale_factors, rotations, cov3D_precomp = _absent_to_empty(
            shs, colors_precomp, scales, scale_factors, rotations, cov3D_precomp)
        fn = (rasterize_gaussians_indexed_camera_exact if self.optimize_camera == "exact" else
              rasterize_gaussians_indexed_camera if self.optimize_camera else rasterize_gaussians_indexed)
        return fn(means3D, means2D, shs, sh_indices, g_indices, colors_precomp, opacities, scales, scale_factors, rotations,
                  cov3D_precomp, self.raster_settings, extrinsic_vector)
