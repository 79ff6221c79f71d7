"""The 3D smoothing filter of Mip-Splatting (not in the reference): every Gaussian carries a world-space low-pass `filter_3D`
sized by the highest sampling rate (focal / depth) at which any training camera sees it, and is rendered with

    Sigma' = Sigma + (scale_modifier f)^2 I,    o' = o sqrt(prod_k s_k^2 / (s_k^2 + f^2))

so that no Gaussian can become smaller than what the training views resolve. The compressed model cannot bake a per-Gaussian
minimum size into its shared scale codebook; the filter is carried next to the model and applied at render time.

    table = camera_table(cameras, device)             # [C, 16] fp32: rows 0..2 of world -> camera, fx, fy, W, H
    filter_3D, seen = compute(xyz, table)             # csrc/filter3d.hip: one lane per Gaussian loops over the table
    cov3D, opacity = apply(opacities, scales, rotations, filter_3D, ...)   # differentiable; feeds cov3D_precomp / opacities

The mathematics is the contract of include/c3dgs_hip.h ("3D smoothing filter"). compute() is bitwise reproducible; the
codebook-sized gradients of apply() on the indexed form are added with fp32 atomics and are not. GPU tensors only."""
import math

import numpy as np
import torch

from . import _lib
from ._lib import ptr as _ptr
from ._lib import stream as _stream


def camera_table(cameras, device):
    """[C, 16] fp32 on `device`, one row per camera, read from `intrinsic` ([0,0] = FoVx, [1,1] = FoVy, [0,2] = W, [1,2] = H) and
    `extrinsic_vector` (qx, qy, qz, qw, tx, ty, tz, or the transposed 4x4 world -> camera matrix) the way
    rasterizer.camera_matrices reads them: entries 0..11 the rows 0..2 of the world -> camera matrix, then
    fx = W / (2 tan(FoVx / 2)) and fy (evaluated in double, rounded once), W, H. The principal point is the image centre."""
    from .rasterizer import _intrinsic_scalars, quat_to_mat
    cameras = list(cameras)
    if not cameras:
        raise ValueError("filter3d.camera_table: at least one camera is needed")
    rows = np.empty((len(cameras), 16), np.float32)
    for k, cam in enumerate(cameras):
        (_, _, H, W, _, _), vals, _ = _intrinsic_scalars(cam.intrinsic)
        pose = cam.extrinsic_vector
        view_t = pose.detach().float().cpu().numpy() if pose.dim() == 2 else quat_to_mat(pose).numpy()    # transposed
        rows[k, :12] = np.ascontiguousarray(view_t.T[:3, :]).reshape(-1)
        rows[k, 12] = W / (2.0 * math.tan(float(vals[0]) * 0.5))
        rows[k, 13] = H / (2.0 * math.tan(float(vals[4]) * 0.5))
        rows[k, 14], rows[k, 15] = W, H
    return torch.from_numpy(rows).to(device)


def compute(xyz, table):
    """-> (filter_3D f32 [P], seen bool [P]) of the positions `xyz` [P, 3] over `table` (camera_table): c3dgs_filter3d_compute on
    the current stream, no host read."""
    x = _lib.gpu_tensor(xyz.detach(), "filter3d.compute: xyz")
    t = _lib.gpu_tensor(table, "filter3d.compute: table")
    if x.dim() != 2 or x.shape[1] != 3:
        raise RuntimeError("filter3d.compute: xyz must be [P, 3]")
    if t.dim() != 2 or t.shape[1] != 16 or t.shape[0] == 0 or t.device != x.device:
        raise RuntimeError("filter3d.compute: table must be [C, 16] with C >= 1 on xyz's device")
    P, dev = int(x.shape[0]), x.device
    out = torch.empty(P, dtype=torch.float32, device=dev)
    seen = torch.empty(P, dtype=torch.uint8, device=dev)
    if P:
        lib = _lib.lib()
        with torch.cuda.device(dev):
            ws = _lib.workspace("filter3d", dev, int(lib.c3dgs_filter3d_workspace_bytes(P)))
            _lib.check(lib.c3dgs_filter3d_compute(P, int(t.shape[0]), x.data_ptr(), t.data_ptr(), out.data_ptr(), seen.data_ptr(),
                                                  ws.data_ptr(), ws.numel(), _stream(dev)))
    return out, seen.bool()


def _rows(opacities, scales, rotations, filter_3D, scale_modifier, scale_factors, g_indices, visible, rank, cov3d=None):
    """the Filter3DRows of the two apply entries and the tensors it points into"""
    t = dict(opacities=_lib.gpu_tensor(opacities.detach(), "filter3d.apply: opacities"),
             scales=_lib.gpu_tensor(scales.detach(), "filter3d.apply: scales"),
             filter_3D=_lib.gpu_tensor(filter_3D.detach(), "filter3d.apply: filter_3D"))
    n = int(t["opacities"].numel())
    if cov3d is not None:
        t["cov3D_precomp"] = _lib.gpu_tensor(cov3d.detach(), "filter3d.apply: cov3d")
        if t["cov3D_precomp"].numel() != 6 * n:
            raise RuntimeError(f"filter3d.apply: cov3d must be [{n}, 6]")
        if rotations is None:                               # not read with a caller's covariance
            rotations = t["scales"].new_zeros((t["scales"].numel() // 3, 4))
    t["rotations"] = _lib.gpu_tensor(rotations.detach(), "filter3d.apply: rotations")
    indexed = g_indices is not None and g_indices.numel() != 0
    if indexed:
        if scale_factors is None:
            raise RuntimeError("filter3d.apply: g_indices need scale_factors")
        t["g_indices"] = _lib.gpu_tensor(g_indices, "filter3d.apply: g_indices", torch.int64)
        t["scale_factors"] = _lib.gpu_tensor(scale_factors.detach(), "filter3d.apply: scale_factors")
        if t["g_indices"].numel() != n or t["scale_factors"].numel() != n:
            raise RuntimeError(f"filter3d.apply: g_indices and scale_factors must have {n} elements")
    elif t["scales"].numel() != 3 * n or t["rotations"].numel() != 4 * n:
        raise RuntimeError(f"filter3d.apply: scales and rotations must be [{n}, 3] and [{n}, 4]")
    if t["scales"].numel() % 3 or t["rotations"].numel() % 4 or t["scales"].numel() // 3 != t["rotations"].numel() // 4:
        raise RuntimeError("filter3d.apply: scales [G, 3] and rotations [G, 4] must have the same number of rows")
    P_model = 0
    if visible is not None:
        if rank is None:
            raise RuntimeError("filter3d.apply: visible and rank come as a pair")
        t["visible"] = visible.contiguous()
        t["rank"] = _lib.gpu_tensor(rank, "filter3d.apply: rank", torch.int32)
        P_model = int(t["filter_3D"].numel())
        if t["visible"].dtype not in (torch.uint8, torch.bool) or t["visible"].numel() != P_model or t["rank"].numel() != P_model:
            raise RuntimeError(f"filter3d.apply: visible (bytes) and rank (int32) must have the filter's {P_model} rows")
    elif t["filter_3D"].numel() != n:
        raise RuntimeError(f"filter3d.apply: filter_3D must have {n} elements, not {t['filter_3D'].numel()}")
    dev = t["opacities"].device
    if any(v.device != dev for v in t.values()):
        raise RuntimeError("filter3d.apply: all tensors must be on one device")
    r = _lib.Filter3DRows(n=n, P_model=P_model, scale_modifier=float(scale_modifier),
                          **{k: (v.data_ptr() if v.numel() else None) for k, v in t.items()})
    return r, t, indexed


class _Apply(torch.autograd.Function):
    @staticmethod
    def forward(ctx, opacities, scales, rotations, scale_factors, cov3d, filter_3D, g_indices, visible, rank, scale_modifier):
        r, t, indexed = _rows(opacities, scales, rotations, filter_3D, scale_modifier, scale_factors, g_indices, visible, rank, cov3d)
        dev = t["opacities"].device
        cov = torch.empty((r.n, 6), dtype=torch.float32, device=dev)
        opac = torch.empty_like(t["opacities"])
        if r.n:
            with torch.cuda.device(dev):
                _lib.check(_lib.lib().c3dgs_filter3d_apply(r, cov.data_ptr(), opac.data_ptr(), _stream(dev)))
        ctx.args = (filter_3D, g_indices, visible, rank, scale_modifier)
        ctx.save_for_backward(opacities, scales, rotations, scale_factors, cov3d)
        return cov, opac

    @staticmethod
    def backward(ctx, d_cov, d_opac):
        opacities, scales, rotations, scale_factors, cov3d = ctx.saved_tensors
        filter_3D, g_indices, visible, rank, scale_modifier = ctx.args
        r, t, indexed = _rows(opacities, scales, rotations, filter_3D, scale_modifier, scale_factors, g_indices, visible, rank, cov3d)
        dev = t["opacities"].device
        need = ctx.needs_input_grad
        g = _lib.Filter3DGrads()
        keep = []
        for name, d in (("dL_dcov3D", d_cov), ("dL_dopacity_out", d_opac)):
            if d is not None:
                keep.append(_lib.gpu_tensor(d.detach(), "filter3d.apply: " + name))
                setattr(g, name, keep[-1].data_ptr() if keep[-1].numel() else None)
        # rows without a gradient are not written by the kernel, and the codebook rows are added to: zeros
        outs = [torch.zeros_like(t[k]) if want else None
                for k, want in (("opacities", need[0]), ("scales", need[1]), ("rotations", need[2] and cov3d is None))]
        outs.append(torch.zeros_like(t["scale_factors"]) if indexed and need[3] else None)
        if r.n and any(o is not None for o in outs):
            for name, o in zip(("dL_dopacity", "dL_dscales", "dL_drotations", "dL_dscale_factors"), outs):
                setattr(g, name, _ptr(o))
            with torch.cuda.device(dev):
                _lib.check(_lib.lib().c3dgs_filter3d_apply_backward(r, g, _stream(dev)))
        # a caller's covariance enters Sigma' unchanged: its gradient is dL/dSigma' itself
        return (*outs, d_cov if (cov3d is not None and need[4]) else None, None, None, None, None, None)


def apply(opacities, scales, rotations, filter_3D, scale_modifier=1.0, scale_factors=None, g_indices=None, visible=None, rank=None,
          cov3d=None):
    """-> (cov3D' [n, 6], o' shaped like `opacities`) for the rasterizer's `cov3D_precomp` and `opacities` inputs, differentiable
    with respect to opacities, scales, rotations and scale_factors (csrc/filter3d.hip; filter_3D is a constant). `scales` and
    `rotations` are [n, 3] / [n, 4] rows or, with `g_indices` [n] and `scale_factors` [n], the codebooks the rows index.
    `visible` (bytes [P]) and `rank` (int32 [P]): the n rows are the visible subset of a model of P Gaussians (row rank[i] for
    visible[i]) and `filter_3D` [P] is read through them by the kernel; without them filter_3D has n rows.
    `cov3d` [n, 6]: a caller's covariance; cov3D' = cov3d + (scale_modifier f)^2 I with gradient to cov3d, the scales then serve the
    opacity factor alone and `rotations` may be None."""
    return _Apply.apply(opacities, scales, rotations, scale_factors, cov3d, filter_3D, g_indices, visible, rank, scale_modifier)
