"""Image metrics and the evaluation pass of the compression run (hot loop D of SURVEY.md 3.1) on the MI355X C-ABI library.

    psnr(img1, img2)                                     utils/image_utils.py:17-19
    ssim(img1, img2, window_size=11, size_average=True)  utils/loss_utils.py:33-63, on [C,H,W] and [N,C,H,W]
    image_metrics(img, gt)                               [N, 3] float64 rows {mse, mean ssim_map, mean |img - gt|}
    render_and_eval(gaussians, cameras, pipe, bg, ...)   compress.py:121-163
    geometry_metrics(points, reference, thresholds=...)  accuracy / completeness / Chamfer / precision / recall / F-score
    mesh_metrics(vertices, faces, reference, density)    the same for a mesh, sampled at `density` points per unit area
    reference_spacing(reference)                         the sampling distance of a reference cloud

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


# ---- geometry: accuracy / completeness / Chamfer as DTU reports them, precision / recall / F-score as Tanks and Temples does
MAX_THRESHOLDS = 8            # C3DGS_GEOMETRY_MAX_THRESHOLDS


def _reduce_direction(d2, points, bounds, max_dist, thresholds, out):
    """one row {count, sum of d, counts below the thresholds} of `out` (float64, on the device) from one direction's distances"""
    import ctypes as C
    L = _lib.lib()
    N, T = int(d2.numel()), len(thresholds)
    ws = torch.empty(int(L.c3dgs_geometry_reduce_workspace_bytes(N)), dtype=torch.uint8, device=d2.device)
    tau = (C.c_float * max(T, 1))(*thresholds)
    box = None if bounds is None else (C.c_float * 6)(*bounds)
    with torch.cuda.device(d2.device):
        _lib.check(L.c3dgs_geometry_reduce(N, _lib.ptr(d2), None if bounds is None else _lib.ptr(points), box, float(max_dist), T, tau,
                                           ws.data_ptr(), ws.numel(), out.data_ptr(), _stream(d2.device)))


def _flat_bounds(bounds):
    if bounds is None:
        return None
    lo, hi = bounds
    flat = [float(v) for v in lo] + [float(v) for v in hi]
    if len(flat) != 6:
        raise ValueError("geometry_metrics: bounds must be (lo [3], hi [3])")
    return flat


def geometry_metrics(points, reference, thresholds=(), max_dist=float("inf"), bounds=None, points_sort=None):
    """Distances between two point sets, [N,3] and [M,3] finite GPU tensors, by exact nearest-neighbour search in both directions
    (knn.NearestIndex), reduced on the device; ONE host read of the two result rows. With d = sqrt(squared distance) in fp32:

        accuracy        mean d from `points` to their nearest point of `reference`
        completeness    mean d from `reference` to their nearest point of `points`
        chamfer         (accuracy + completeness) / 2, DTU's convention
        n_accuracy, n_completeness   how many distances entered each mean
        precision[tau], recall[tau]  the fraction of those with d < tau, per threshold (at most 8)
        fscore[tau]     2 P R / (P + R), and 0 when P + R == 0

    An element enters a mean iff it has a neighbour, d <= `max_dist` and, with `bounds` = (lo [3], hi [3]), its OWN coordinates lie
    in the box (each set is filtered by its own points). A mean over zero elements is NaN, and so are precision and recall then
    (fscore is 0). Sums are fp64 and bitwise reproducible. `points_sort`: NearestIndex.query's `sort` for the search FROM `points`
    (it changes the time, never the result)."""
    from . import knn
    taus = [float(t) for t in thresholds]
    if len(taus) > MAX_THRESHOLDS:
        raise ValueError(f"geometry_metrics: at most {MAX_THRESHOLDS} thresholds")
    box = _flat_bounds(bounds)
    ref_index, pts_index = knn.NearestIndex(reference), knn.NearestIndex(points)
    if ref_index.device != pts_index.device:
        raise RuntimeError("geometry_metrics: points and reference must be on one device")
    rows = torch.empty((2, 2 + MAX_THRESHOLDS), dtype=torch.float64, device=ref_index.device)
    _reduce_direction(ref_index.query(pts_index.points, sort=points_sort)[1], pts_index.points, box, max_dist, taus, rows[0])
    _reduce_direction(pts_index.query(ref_index.points)[1], ref_index.points, box, max_dist, taus, rows[1])
    acc, comp = rows[:, :2 + len(taus)].tolist()                 # the one device-to-host read
    nan = float("nan")
    out = {"accuracy": acc[1] / acc[0] if acc[0] else nan, "completeness": comp[1] / comp[0] if comp[0] else nan,
           "n_accuracy": int(acc[0]), "n_completeness": int(comp[0]), "precision": {}, "recall": {}, "fscore": {}}
    out["chamfer"] = 0.5 * (out["accuracy"] + out["completeness"])
    for t, tau in enumerate(taus):
        p = acc[2 + t] / acc[0] if acc[0] else nan
        r = comp[2 + t] / comp[0] if comp[0] else nan
        out["precision"][tau], out["recall"][tau] = p, r
        out["fscore"][tau] = 2.0 * p * r / (p + r) if p + r > 0 else 0.0
    return out


def mesh_metrics(vertices, faces, reference, density, seed=0, thresholds=(), max_dist=float("inf"), bounds=None):
    """geometry_metrics of mesh.sample_surface(vertices, faces, density, seed) against `reference`, plus "samples": the number of
    sampled points. Two host reads: the sample count and the result rows."""
    from . import knn, mesh
    points, _ = mesh.sample_surface(vertices, faces, density, seed)
    out = geometry_metrics(points, reference, thresholds=thresholds, max_dist=max_dist, bounds=bounds,
                           points_sort=knn.SORT_FACE_ORDERED_QUERIES)
    out["samples"] = int(points.size(0))
    return out


def reference_spacing(reference):
    """sqrt of the median squared distance of a reference point to its nearest OTHER point (knn.knn3's first column): the
    sampling distance of the cloud. tools/eval_mesh.py samples the mesh at 1 / spacing^2 points per unit area by default, the
    cloud's own density on a surface; nobody has tuned that default. One host read."""
    from . import knn
    d2 = knn.knn3(reference)[1][:, 0]
    if d2.numel() < 2:
        raise ValueError("reference_spacing: at least two points are needed")
    return float(torch.sqrt(d2.median()))
