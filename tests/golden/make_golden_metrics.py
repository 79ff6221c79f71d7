#!/usr/bin/env python3
"""Generates tests/golden/metrics.npz by RUNNING the reference's psnr (utils/image_utils.py:17-19) and ssim
(utils/loss_utils.py:33-63) on CPU tensors, in fp32 and in fp64.

    python tests/golden/make_golden_metrics.py REFERENCE_TREE      (CPU only; never runs on the GPU box)

Inputs lie on 8-bit levels (k / 255), except in the out-of-range case. Only arrays are stored (allow_pickle=False): per
case `<tag>_img`, `<tag>_gt` (fp32 inputs) and the reference's outputs
  <tag>_psnr32 / _psnr64      psnr per row of dim 0 ([N,1], or [C,1] for the 3-D case)
  <tag>_ssim32 / _ssim64      ssim(size_average=True)
  <tag>_ssimN32 / _ssimN64    ssim(size_average=False), per image (4-D cases only)
  <tag>_mse64, <tag>_l164     per-image mean (x - y)^2 and |x - y| in fp64 (4-D cases only)
"""
import importlib.util
import os
import sys

import numpy as np
import torch

OUT = os.path.dirname(os.path.abspath(__file__))


def _load(ref, rel, name):
    spec = importlib.util.spec_from_file_location(name, os.path.join(ref, rel))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def cases():
    g = torch.Generator().manual_seed(2024)
    q = lambda t: torch.round(t * 255) / 255                         # noqa: E731  8-bit levels: a small fixture
    r = lambda *s: q(torch.rand(*s, generator=g))                    # noqa: E731
    out = {}
    out["rand"] = (r(1, 3, 37, 53), r(1, 3, 37, 53))
    gt = r(3, 3, 16, 16)
    out["batch"] = (q((gt + 0.1 * torch.randn(3, 3, 16, 16, generator=g)).clamp(0, 1)), gt)
    out["gray"] = (r(1, 1, 9, 40), r(1, 1, 9, 40))
    out["tiny"] = (r(1, 3, 5, 7), r(1, 3, 5, 7))                     # smaller than the window
    out["chw"] = (r(3, 20, 30), r(3, 20, 30))                        # 3-D: psnr per channel
    out["range"] = (1.5 * torch.randn(1, 3, 24, 31, generator=g) + 0.5, torch.full((1, 3, 24, 31), 0.3))
    x = r(1, 3, 12, 14)
    out["same"] = (x, x.clone())                                     # psnr inf, ssim 1
    return out


def main(ref):
    iu = _load(ref, "utils/image_utils.py", "ref_image_utils")
    lu = _load(ref, "utils/loss_utils.py", "ref_loss_utils")
    d = {}
    for tag, (img, gt) in cases().items():
        img, gt = img.float().contiguous(), gt.float().contiguous()
        d[f"{tag}_img"], d[f"{tag}_gt"] = img.numpy(), gt.numpy()
        for bits, dt in (("32", torch.float32), ("64", torch.float64)):
            a, b = img.to(dt), gt.to(dt)
            d[f"{tag}_psnr{bits}"] = iu.psnr(a, b).numpy()
            d[f"{tag}_ssim{bits}"] = np.array(float(lu.ssim(a, b)), dtype=np.float64)
            if img.dim() == 4:
                d[f"{tag}_ssimN{bits}"] = lu.ssim(a, b, size_average=False).numpy()
        if img.dim() == 4:
            a, b = img.double(), gt.double()
            d[f"{tag}_mse64"] = iu.mse(a, b).reshape(-1).numpy()
            d[f"{tag}_l164"] = (a - b).abs().reshape(a.shape[0], -1).mean(1).numpy()
    path = os.path.join(OUT, "metrics.npz")
    np.savez_compressed(path, **d)
    print(path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    if len(sys.argv) != 2:
        sys.exit(__doc__)
    main(sys.argv[1])
