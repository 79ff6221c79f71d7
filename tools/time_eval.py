"""Times the evaluation pass (hot loop D) at 1080p on one GPU, with device events after warm-up:

    python tools/time_eval.py [--views 50] [--P 3000000] [--reps 3] [--out FILE.json]

  eval      metrics.render_and_eval over the 3M indexed bench scene (synth-v1, `--views` poses, GT = render + noise)
  render    the render-only loop over the same views (GaussianModel.render under no_grad)
  kernel    c3dgs_image_metrics alone on [N,3,1080,1920], N = 1 and 8, against the fused loss forward
            (c3dgs_l1_ssim_forward with and without its three derivative maps) and the 8 us floor of reading both images
  torch     the same PSNR + SSIM written as plain torch ops (grouped conv2d), forward only, N = 1 and 8
Prints one JSON object (and writes it to --out)."""
import argparse
import ctypes as C
import json
import math
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import torch  # noqa: E402
import torch.nn.functional as F  # noqa: E402

from c3dgs_amd import _lib, metrics  # noqa: E402
from c3dgs_amd import model as gm  # noqa: E402
from tests import synth  # noqa: E402

HBM_COPY_TBS = 6.3          # measured device-to-device copy rate of the MI355X (profiles/README.md)


def torch_psnr_ssim(img, gt):
    """psnr per image and mean SSIM with torch ops: separable Gaussian as one 11 x 11 grouped conv2d per moment."""
    Cc = img.shape[1]
    g = torch.tensor([math.exp(-(i - 5) ** 2 / 4.5) for i in range(11)], dtype=torch.float32, device=img.device)
    g = g / g.sum()
    w = torch.outer(g, g).expand(Cc, 1, 11, 11).contiguous()
    conv = lambda t: F.conv2d(t, w, padding=5, groups=Cc)          # noqa: E731
    m1, m2 = conv(img), conv(gt)
    v1, v2, v12 = conv(img * img) - m1 * m1, conv(gt * gt) - m2 * m2, conv(img * gt) - m1 * m2
    smap = (2 * m1 * m2 + 1e-4) * (2 * v12 + 9e-4) / ((m1 * m1 + m2 * m2 + 1e-4) * (v1 + v2 + 9e-4))
    mse = ((img - gt) ** 2).flatten(1).mean(1)
    return -10 * torch.log10(mse), smap.flatten(1).mean(1)


def timed(fn, reps, inner=1):
    """median over `reps` of the device-event time of `inner` calls, in ms per call (after one warm-up call)."""
    fn()
    torch.cuda.synchronize()
    out = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(inner):
            fn()
        b.record()
        b.synchronize()
        out.append(a.elapsed_time(b) / inner)
    return sorted(out)[len(out) // 2]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--views", type=int, default=50)
    ap.add_argument("--P", type=int, default=3_000_000)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    assert torch.cuda.is_available(), "time_eval.py measures on the GPU; there is no CPU path"
    dev = torch.device("cuda", 0)
    torch.cuda.set_device(dev)
    W, H, focal = 1920, 1080, 1200.0
    L = _lib.lib()
    res = {"W": W, "H": H, "P": a.P, "views": a.views}

    # ---- the metric kernel alone
    g = torch.Generator(device=dev).manual_seed(3)
    for N in (1, 8):
        gt = torch.rand(N, 3, H, W, device=dev, generator=g)
        img = (gt + 0.1 * torch.randn(N, 3, H, W, device=dev, generator=g)).clamp(0, 1)
        out = torch.empty(N, 3, dtype=torch.float64, device=dev)
        ws = torch.empty(int(L.c3dgs_image_metrics_ws_bytes(N, 3, H, W)), dtype=torch.uint8, device=dev)
        s = C.c_void_p(torch.cuda.current_stream(dev).cuda_stream)
        call = lambda: _lib.check(L.c3dgs_image_metrics(N, 3, H, W, img.data_ptr(), gt.data_ptr(), ws.data_ptr(),  # noqa: E731
                                                        ws.numel(), out.data_ptr(), s))
        ms = timed(call, a.reps, 50)
        floor_ms = 2 * img.numel() * 4 / (HBM_COPY_TBS * 1e12) * 1e3
        res[f"kernel_N{N}_ms"] = ms
        res[f"kernel_N{N}_floor_ms"] = floor_ms
        res[f"kernel_N{N}_fraction_of_floor"] = floor_ms / ms
        res[f"torch_ops_N{N}_ms"] = timed(lambda: torch_psnr_ssim(img, gt), a.reps, 5)
        p_t, s_t = torch_psnr_ssim(img, gt)
        rows = out.clone()
        res[f"torch_vs_kernel_N{N}_max_abs_diff"] = {"psnr_db": float((p_t.double() - (-10 * torch.log10(rows[:, 0]))).abs().max()),
                                                   "ssim": float((s_t.double() - rows[:, 1]).abs().max())}
        if N == 1:
            sums = torch.empty(128, dtype=torch.float64, device=dev)
            dmaps = torch.empty(3, 3, H, W, device=dev)
            for name, dm in (("loss_forward_with_maps_ms", dmaps.data_ptr()), ("loss_forward_no_maps_ms", None)):
                res[name] = timed(lambda: _lib.check(L.c3dgs_l1_ssim_forward(3, H, W, img.data_ptr(), gt.data_ptr(), dm,
                                                                             sums.data_ptr(), s)), a.reps, 50)
        del img, gt

    # ---- the evaluation pass over the 3M indexed bench scene
    sc = synth.scene(a.P, W, H, focal, seed=1234, sh_degree=3)
    m = gm.GaussianModel(3, quantization=True, device=dev).set_tensors(**synth.raw_params(synth.index_scene(sc)))
    del sc
    pipe, bg = gm.PipelineParams(), torch.zeros(3, device=dev)

    class Cam:
        pass
    cams = []
    for k in range(a.views):
        intr, ev = synth.camera(W, H, focal, extrinsic_vector=(0.02 * math.sin(k), 0.02 * math.cos(k), 0.01 * (k % 5),
                                                                   1.0, 0.0, 0.0, 0.0))
        c = Cam()
        c.intrinsic, c.extrinsic_vector = intr.to(dev), ev.to(dev)
        cams.append(c)
    with torch.no_grad():
        for k, c in enumerate(cams):
            r = m.render(c, pipe, bg)["render"]
            c.original_image = (r + 0.02 * torch.randn(r.shape, device=dev, generator=g)).clamp(0, 1)

    def render_only():
        with torch.no_grad():
            for c in cams:
                m.render(c, pipe, bg)["render"]

    box = {}

    def evaluate():
        box["m"] = metrics.render_and_eval(m, cams, pipe, bg)

    t_eval = timed(evaluate, a.reps)
    t_render = timed(render_only, a.reps)
    res["eval_ms"] = t_eval
    res["render_only_ms"] = t_render
    res["eval_views_per_s"] = a.views / t_eval * 1e3
    res["render_only_views_per_s"] = a.views / t_render * 1e3
    res["eval_over_render_only"] = t_render / t_eval
    res["eval_metrics"] = box["m"]
    print(json.dumps(res))
    if a.out:
        os.makedirs(os.path.dirname(a.out) or ".", exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
