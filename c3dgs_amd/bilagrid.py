"""Per-image colour correction (not in the reference): one bilateral grid per training camera, a small 3-D lattice of 3x4 affine
colour transforms that is sliced at (x, y, luma) for every pixel of the render before the loss sees it (gsplat's lib_bilagrid /
fused_bilagrid). A grid of shape (1, 1, 1) is upstream 3DGS's per-image 3x4 `exposure`: ExposureModel.

    grids = BilateralGrid(num_cameras, shape=(8, 16, 16))      # identity at every vertex
    image = grids.slice(render, camera_index)                  # differentiable w.r.t. the grid and the render
    loss = l1_ssim_loss(image, gt) + 10.0 * grids.tv_loss()

The mathematics is the contract of include/c3dgs_hip.h ("bilateral grid"); the kernels are csrc/bilagrid.hip: one launch for
the slice, a gather by vertex plus a fold (and a per-pixel launch for the image gradient, skipped when the image needs none)
for its backward, no float atomics anywhere, so every result is bitwise reproducible. GPU tensors only: there is no CPU path."""
import numpy as np
import torch

from . import _lib
from ._lib import stream as _stream


def _shape3(shape):
    shape = tuple(int(v) for v in shape)
    if len(shape) != 3 or min(shape) < 1:
        raise ValueError(f"bilagrid: shape must be three positive sizes (L, Hg, Wg), not {shape!r}")
    return shape


def _workspace(device, H, W, L, Hg, Wg):
    n = _lib.lib().c3dgs_bilagrid_workspace_bytes(H, W, L, Hg, Wg)
    if n == 0:
        _lib.check(1)
    return _lib.workspace("bilagrid", device, n)


class _Slice(torch.autograd.Function):
    @staticmethod
    def forward(ctx, grids, image, camera_index):
        g = _lib.gpu_tensor(grids.detach(), "bilagrid: grids")
        x = _lib.gpu_tensor(image.detach(), "bilagrid: image")
        if x.dim() != 3 or x.shape[0] != 3:
            raise RuntimeError("bilagrid: the image must be [3, H, W]")
        if x.device != g.device:
            raise RuntimeError("bilagrid: the image and the grids must be on the same device")
        _, H, W = x.shape
        _, _, L, Hg, Wg = g.shape
        out = torch.empty_like(x)
        with torch.cuda.device(x.device):
            _lib.check(_lib.lib().c3dgs_bilagrid_slice(H, W, L, Hg, Wg, g[camera_index].data_ptr(), x.data_ptr(), out.data_ptr(),
                                                       _stream(x.device)))
        ctx.camera_index = camera_index
        ctx.save_for_backward(g, x)
        return out

    @staticmethod
    def backward(ctx, grad_out):
        g, x = ctx.saved_tensors
        _, H, W = x.shape
        _, _, L, Hg, Wg = g.shape
        d = _lib.gpu_tensor(grad_out.detach(), "bilagrid: the output's gradient")
        d_grids = torch.zeros_like(g)
        d_image = torch.empty_like(x) if ctx.needs_input_grad[1] else None
        with torch.cuda.device(x.device):
            ws = _workspace(x.device, H, W, L, Hg, Wg)
            _lib.check(_lib.lib().c3dgs_bilagrid_slice_backward(
                H, W, L, Hg, Wg, g[ctx.camera_index].data_ptr(), x.data_ptr(), d.data_ptr(), d_grids[ctx.camera_index].data_ptr(),
                _lib.ptr(d_image), ws.data_ptr(), _stream(x.device)))
        return d_grids, d_image, None


class _TV(torch.autograd.Function):
    @staticmethod
    def forward(ctx, grids):
        g = _lib.gpu_tensor(grids.detach(), "bilagrid: grids")
        C, _, L, Hg, Wg = g.shape
        out = torch.empty(1, dtype=torch.float32, device=g.device)
        with torch.cuda.device(g.device):
            ws = _workspace(g.device, 1, 1, L, Hg, Wg)
            _lib.check(_lib.lib().c3dgs_bilagrid_tv(C, L, Hg, Wg, g.data_ptr(), ws.data_ptr(), out.data_ptr(), _stream(g.device)))
        ctx.save_for_backward(g)
        return out.reshape(())

    @staticmethod
    def backward(ctx, grad_out):
        g, = ctx.saved_tensors
        C, _, L, Hg, Wg = g.shape
        d = grad_out.detach().reshape(1).to(device=g.device, dtype=torch.float32).contiguous()
        out = torch.empty_like(g)
        with torch.cuda.device(g.device):
            _lib.check(_lib.lib().c3dgs_bilagrid_tv_backward(C, L, Hg, Wg, g.data_ptr(), d.data_ptr(), out.data_ptr(),
                                                             _stream(g.device)))
        return out


class BilateralGrid(torch.nn.Module):
    """`grids`: nn.Parameter [num_cameras, 12, L, Hg, Wg], fp32, the identity affine at every vertex. Camera k of the training
    list owns row k."""

    def __init__(self, num_cameras, shape=(8, 16, 16), device="cuda"):
        super().__init__()
        if int(num_cameras) < 1:
            raise ValueError("bilagrid: num_cameras must be positive")
        L, Hg, Wg = _shape3(shape)
        if not torch.device(device).type == "cuda":
            raise RuntimeError("c3dgs_amd: bilateral grids live on a GPU (there is no CPU path)")
        eye = torch.eye(3, 4, dtype=torch.float32, device=device).reshape(1, 12, 1, 1, 1)
        self.grids = torch.nn.Parameter(eye.repeat(int(num_cameras), 1, L, Hg, Wg).contiguous())
        self.image_names = [""] * int(num_cameras)

    @property
    def shape(self):
        return tuple(self.grids.shape[2:])

    @property
    def num_cameras(self):
        return self.grids.shape[0]

    def slice(self, image, camera_index):
        """image [3, H, W] on the grids' device -> the corrected image. Differentiable w.r.t. `grids` (only row `camera_index` of
        the gradient is non-zero) and, where it requires a gradient, the image."""
        camera_index = int(camera_index)
        if not 0 <= camera_index < self.grids.shape[0]:
            raise IndexError(f"bilagrid: camera_index {camera_index} is outside the {self.grids.shape[0]} cameras")
        return _Slice.apply(self.grids, image, camera_index)

    def tv_loss(self):
        """The total variation of all grids (the definition of include/c3dgs_hip.h); 0 for a shape of one vertex."""
        return _TV.apply(self.grids)

    def set_cameras(self, cameras):
        """Remember the cameras' `image_name`s ("" where a camera has none), in order: what save() writes and load() compares."""
        names = [str(getattr(c, "image_name", "") or "") for c in cameras]
        if len(names) != self.grids.shape[0]:
            raise ValueError(f"bilagrid: {len(names)} cameras for {self.grids.shape[0]} grids")
        self.image_names = names
        return self

    def save(self, path):
        """An .npz with the grids and the cameras' image_name list."""
        with open(path, "wb") as f:
            np.savez(f, grids=self.grids.detach().cpu().numpy(), image_names=np.array(self.image_names, dtype=str))

    def load(self, path):
        """Fill the grids from save()'s file, bit for bit. ValueError if the file's shape or its image names are not this
        object's: the rows would correct the wrong images."""
        with np.load(path, allow_pickle=False) as z:
            grids, saved = z["grids"], [str(s) for s in z["image_names"]]
        if grids.dtype != np.float32 or tuple(grids.shape) != tuple(self.grids.shape):
            raise ValueError(f"bilagrid.load: {path} holds {grids.dtype} {tuple(grids.shape)}, not float32 {tuple(self.grids.shape)}")
        if saved != self.image_names:
            raise ValueError(f"bilagrid.load: the image names saved in {path} are not this object's")
        with torch.no_grad():
            self.grids.copy_(torch.from_numpy(grids))
        return self


class ExposureModel(BilateralGrid):
    """One global 3x4 affine per camera: the bilateral grid of shape (1, 1, 1)."""

    def __init__(self, num_cameras, device="cuda"):
        super().__init__(num_cameras, shape=(1, 1, 1), device=device)
