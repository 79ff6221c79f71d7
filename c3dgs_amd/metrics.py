"""Image metrics and the evaluation pass of the compression run (hot loop D of SURVEY.md 3.1) on the MI355X C-ABI library.

    psnr(img1, img2)                                     utils/image_utils.py:17-19
    ssim(img1, img2, window_size=11, size_average=True)  utils/loss_utils.py:33-63, on [C,H,W] and [N,C,H,W]
    image_metrics(img, gt)                               [N, 3] float64 rows {mse, mean ssim_map, mean |img - gt|}
    render_and_eval(gaussians, cameras, pipe, bg, ...)   compress.py:121-163

One forward-only kernel pass (csrc/metrics.hip) yields MSE, SSIM and L1 of every image of a batch, with a deterministic
two-kernel reduction. Nothing here carries a gradient: the differentiable SSIM / L1 are c3dgs_amd.loss.ssim / l1_loss /
l1_ssim_loss. No CPU path."""
import os

import torch

from . import _lib
from ._lib import stream as _stream


def _check(img1, img2):
    if img1.shape != img2.shape:
        raise RuntimeError(f"c3dgs_amd.metrics: shape mismatch {tuple(img1.shape)} vs {tuple(img2.shape)}")
    if img1.dim() not in (3, 4):
        raise RuntimeError("c3dgs_amd.metrics: expected [C,H,W] or [N,C,H,W] tensors")
    if not img1.is_cuda or not img2.is_cuda:
        raise RuntimeError("c3dgs_amd: metric inputs must be GPU tensors (there is no CPU path)")
    return img1.detach().contiguous().float(), img2.detach().contiguous().float()


def _launch(x, y, out):
    """x, y: contiguous fp32 [N,C,H,W] on one device; out: [N,3] float64 rows (may be a slice of a larger table)."""
    L = _lib.lib()
    N, Cc, H, W = x.shape
    if out.dtype != torch.float64 or out.shape != (N, 3) or not out.is_contiguous() or out.device != x.device:
        raise RuntimeError("c3dgs_amd.metrics: out must be a contiguous float64 [N,3] tensor on the inputs' device")
    nbytes = int(L.c3dgs_image_metrics_ws_bytes(N, Cc, H, W))
    ws = torch.empty(max(nbytes, 8), dtype=torch.uint8, device=x.device)     # tile partials; the allocator orders reuse
    with torch.cuda.device(x.device):
        _lib.check(L.c3dgs_image_metrics(N, Cc, H, W, x.data_ptr(), y.data_ptr(), ws.data_ptr(), ws.numel(), out.data_ptr(),
                                         _stream(x.device)))
    return out


def image_metrics(img, gt, out=None):
    """[N,C,H,W] (or [C,H,W], as N = 1) pair -> [N,3] float64 device rows {mse, mean ssim_map, mean |img - gt|}, means over
    C*H*W. `out`: optional contiguous float64 [N,3] destination, e.g. rows of a larger per-view table. Deterministic:
    row n is bit-identical to image n passed alone. No gradient."""
    x, y = _check(img, gt)
    if x.dim() == 3:
        x, y = x.unsqueeze(0), y.unsqueeze(0)
    if out is None:
        out = torch.empty((x.shape[0], 3), dtype=torch.float64, device=x.device)
    return _launch(x, y, out)


def _psnr_of_mse(mse):
    return (20 * torch.log10(1.0 / torch.sqrt(mse))).float()


def psnr(img1, img2):
    """utils/image_utils.py:17-19: 20 * log10(1 / sqrt(mse)) per row of dim 0, as fp32 [rows, 1] ([N,1] for [N,C,H,W],
    [C,1] for [C,H,W]); identical rows give inf. Detached, on the device: it carries no gradient."""
    x, y = _check(img1, img2)
    if x.dim() == 3:                       # one row per channel: each channel is its own 1-channel image
        x, y = x.unsqueeze(1), y.unsqueeze(1)
    rows = _launch(x, y, torch.empty((x.shape[0], 3), dtype=torch.float64, device=x.device))
    return _psnr_of_mse(rows[:, 0:1])


def ssim(img1, img2, window_size=11, size_average=True):
    """utils/loss_utils.py:33-63 on [C,H,W] or [N,C,H,W]: size_average=True -> the fp32 scalar mean of the SSIM map,
    False -> the per-image means [N] (the reference's .mean(1).mean(1).mean(1), which a [C,H,W] input cannot take).
    Detached, on the device: it carries no gradient; the differentiable SSIM is c3dgs_amd.loss.ssim."""
    if window_size != 11:
        raise NotImplementedError("c3dgs_amd.metrics.ssim implements window_size=11")
    x, y = _check(img1, img2)
    if x.dim() == 3:
        if not size_average:
            raise IndexError("ssim(size_average=False) needs [N,C,H,W] inputs: a [C,H,W] map has no dimension 1 left "
                             "for the third mean")
        x, y = x.unsqueeze(0), y.unsqueeze(0)
    rows = _launch(x, y, torch.empty((x.shape[0], 3), dtype=torch.float64, device=x.device))
    return rows[:, 1].mean().float() if size_average else rows[:, 1].float()


def _save_png(img, path):
    """torchvision.utils.save_image of one [C,H,W] image: x * 255 + 0.5 clamped to [0, 255], truncated to uint8, HWC."""
    from PIL import Image
    if img.shape[0] == 1:                  # make_grid turns one channel into three
        img = torch.cat((img, img, img), 0)
    q = img.mul(255).add_(0.5).clamp_(0, 255).permute(1, 2, 0).to(torch.uint8).cpu().numpy()
    Image.fromarray(q).save(path)


def render_and_eval(gaussians, cameras, pipeline_params, background, out_dir=None, lpips_fn=None):
    """compress.py:121-163: renders every view of `cameras` without gradients (GaussianModel.render(view, pipe,
    background)["render"]), scores it against `view.original_image` and returns
    {"SSIM": mean over views, "PSNR": mean over views of the per-view PSNR, "LPIPS": mean of lpips_fn or None}.

    The per-view rows go into a [V,3] device table and the means are taken on the device: one device-to-host read per
    call. `lpips_fn(render[1,C,H,W], gt[1,C,H,W]) -> tensor` (optional) is called once per view; the reference's
    LPIPS-VGG is not bundled (its weights are fetched by URL). With `out_dir`, writes out_dir/renders/{idx:05d}.png and
    out_dir/gt/{idx:05d}.png as torchvision.utils.save_image would. No gradient."""
    views = list(cameras)
    if not views:
        raise ValueError("render_and_eval: no cameras")
    if out_dir is not None:
        render_path, gts_path = os.path.join(out_dir, "renders"), os.path.join(out_dir, "gt")
        os.makedirs(render_path, exist_ok=True)
        os.makedirs(gts_path, exist_ok=True)
    with torch.no_grad():
        table = None
        lpipss = []
        for idx, view in enumerate(views):
            rendering = gaussians.render(view, pipeline_params, background)["render"]
            gt = view.original_image.to(rendering.device)
            if out_dir is not None:
                _save_png(rendering, os.path.join(render_path, f"{idx:05d}.png"))
                _save_png(gt, os.path.join(gts_path, f"{idx:05d}.png"))
            if table is None:
                table = torch.empty((len(views), 3), dtype=torch.float64, device=rendering.device)
            image_metrics(rendering.unsqueeze(0), gt.unsqueeze(0), out=table[idx:idx + 1])
            if lpips_fn is not None:
                lpipss.append(torch.as_tensor(lpips_fn(rendering.unsqueeze(0), gt.unsqueeze(0))).detach()
                              .to(device=table.device, dtype=torch.float64).mean())
        means = [table[:, 1].mean(), _psnr_of_mse(table[:, 0]).double().mean()]
        if lpipss:
            means.append(torch.stack(lpipss).mean())
        vals = torch.stack(means).tolist()          # the one device-to-host read of the pass
    return {"SSIM": vals[0], "PSNR": vals[1], "LPIPS": vals[2] if lpipss else None}
