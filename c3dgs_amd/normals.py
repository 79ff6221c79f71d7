"""Normals from a depth map, and the normal-consistency term of 2DGS / PGSR-style training (csrc/normals.hip).

    depth_to_normal(z, intrinsic)                         the normal of the surface a map of view-space depths describes
    normal_consistency(depth, alpha, normal, intrinsic)   the term that ties the rasterizer's blended normal map to it

All normals are in VIEW space: x right, y down, z forward, the frame of the rasterizer's view matrix and of the `normal` map
GaussianRasterizationSettings(normal=True) appends. The stencil and its backward are one HIP launch each; there is no CPU path.
"""
import torch

from . import _lib
from ._lib import ptr as _ptr, stream as _stream


def _tan_fov(intrinsic):
    from .rasterizer import _intrinsic_scalars
    return _intrinsic_scalars(intrinsic)[0][:2]


def _check(t, shape, what):
    if not isinstance(t, torch.Tensor) or not t.is_cuda:
        raise RuntimeError(f"c3dgs_amd: {what} must be a GPU tensor (there is no CPU path)")
    if t.dtype != torch.float32:
        raise RuntimeError(f"c3dgs_amd: {what} must be float32, not {t.dtype}")
    if shape is not None and tuple(t.shape) != tuple(shape):
        raise RuntimeError(f"c3dgs_amd: {what} must have shape {tuple(shape)}, not {tuple(t.shape)}")


class _DepthToNormal(torch.autograd.Function):
    @staticmethod
    def forward(ctx, z, tan_fovx, tan_fovy):
        _check(z, None, "z")
        if z.dim() != 2 or z.numel() == 0:
            raise RuntimeError(f"c3dgs_amd: z must have shape (H, W), not {tuple(z.shape)}")
        z = z.detach().contiguous()
        H, W = (int(v) for v in z.shape)
        with torch.cuda.device(z.device):
            out = torch.empty((3, H, W), dtype=torch.float32, device=z.device)
            rc = _lib.lib().c3dgs_depth_to_normal(W, H, _ptr(z), tan_fovx, tan_fovy, _ptr(out), _stream(z.device))
        _lib.check(rc)
        ctx.save_for_backward(z)
        ctx.tan_fov = (tan_fovx, tan_fovy)
        return out

    @staticmethod
    def backward(ctx, grad):
        (z,) = ctx.saved_tensors
        H, W = (int(v) for v in z.shape)
        grad = grad.to(torch.float32).contiguous()
        with torch.cuda.device(z.device):
            dz = torch.empty((H, W), dtype=torch.float32, device=z.device)
            rc = _lib.lib().c3dgs_depth_to_normal_backward(W, H, _ptr(z), _ptr(grad), *ctx.tan_fov, _ptr(dz), _stream(z.device))
        _lib.check(rc)
        return dz, None, None


def depth_to_normal(z, intrinsic):
    """z: [H, W] fp32 on the GPU, view-space depths (for a rasterizer's maps: depth / alpha). -> [3, H, W], the unit normal of the
    surface P(x, y) = z(x, y) ((x + 0.5 - W / 2) / fx, (y + 0.5 - H / 2) / fy, 1), fx = W / (2 tan_fovx), fy = H / (2 tan_fovy)
    (the rasterizer's own pixel centres: the inverse of its ndc -> pixel map), at the interior pixels:
        normalize(cross(P(x, y + 1) - P(x, y - 1), P(x + 1, y) - P(x - 1, y))),   normalize(c) = c / max(|c|, 1e-12)
    so a fronto-parallel plane gives (0, 0, -1): towards the camera, like the rasterizer's normals. The one-pixel border is the
    zero vector (an image with W < 3 or H < 3 is all zero). `intrinsic` is the rasterizer settings' (its field of view is what is
    read). Differentiable in z: the backward gathers, per pixel, the at most four stencils that read it (one launch, no atomics)."""
    tan_fovx, tan_fovy = _tan_fov(intrinsic)
    return _DepthToNormal.apply(z, float(tan_fovx), float(tan_fovy))


def normal_consistency(depth, alpha, normal, intrinsic):
    """2DGS's normal-consistency term on a rasterizer's maps (GaussianRasterizationSettings(normal=True) / render(normal=True)):
        z  = depth / alpha.clamp_min(1e-6)                      the expected view-space depth of what the pixel shows
        Ns = depth_to_normal(z, intrinsic) * alpha.detach()     the surface's normal, weighted like the blended one
        -> mean over the pixels of (1 - sum_c normal_c Ns_c)
    a scalar that is 0 where every blended Gaussian's normal is the surface's. Gradients flow to `normal`, and through z to `depth`
    and `alpha`. The divide, the product and the mean are torch ops; the stencil is HIP."""
    _check(depth, None, "depth")
    _check(alpha, depth.shape, "alpha")
    _check(normal, (3,) + tuple(depth.shape), "normal")
    z = depth / alpha.clamp_min(1e-6)
    surface = depth_to_normal(z, intrinsic) * alpha.detach()
    return (1.0 - (normal * surface).sum(0)).mean()
