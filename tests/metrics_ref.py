"""numpy float64 restatement of the evaluation metrics (test checker, not product code).

    window()              gaussian(11, 1.5) normalised in fp32, outer product in fp32 (the reference's 2-D window)
    ssim_rows(x, y)       per-image mean of the SSIM map, [N,C,H,W] float64 -> [N]
    mse_rows / l1_rows    per-image mean (x - y)^2 / |x - y|
    psnr_rows(x, y)       20 log10(1 / sqrt(mse)) per row of dim 0

Everything after the window is float64: the 11 x 11 window is applied directly (121 shifted products, zero padding 5,
per channel), the SSIM map is evaluated with C1 = 0.01^2, C2 = 0.03^2. tests/test_metrics_cpu.py pins it to the
reference's fp64 values in tests/golden/metrics.npz."""
import math

import numpy as np

R = 5


def window(running_fp32_sum=False):
    """The reference's window: fp32 taps over their correctly rounded fp32 sum (what torch's sum gives here).
    running_fp32_sum=True: the taps over a left-to-right fp32 sum, 1 ulp lower -- the window of csrc/loss.hip."""
    g = np.array([math.exp(-(x - R) ** 2 / float(2 * 1.5 ** 2)) for x in range(2 * R + 1)], dtype=np.float32)
    if running_fp32_sum:
        s = np.float32(0)
        for t in g:
            s = np.float32(s + t)
    else:
        s = np.float32(g.astype(np.float64).sum())
    g = g / s
    return np.outer(g, g).astype(np.float64)               # fp32 products, then used in float64


def _filter(a, w):
    """zero-padded 'same' correlation of every [H,W] plane of a [..., H, W] float64 array with the 11 x 11 window."""
    H, W = a.shape[-2:]
    p = np.zeros(a.shape[:-2] + (H + 2 * R, W + 2 * R), dtype=np.float64)
    p[..., R:R + H, R:R + W] = a
    out = np.zeros_like(a)
    for dy in range(2 * R + 1):
        for dx in range(2 * R + 1):
            out += w[dy, dx] * p[..., dy:dy + H, dx:dx + W]
    return out


def ssim_map(x, y, w=None):
    x, y = np.asarray(x, np.float64), np.asarray(y, np.float64)
    w = window() if w is None else w
    mu1, mu2 = _filter(x, w), _filter(y, w)
    s1 = _filter(x * x, w) - mu1 * mu1
    s2 = _filter(y * y, w) - mu2 * mu2
    s12 = _filter(x * y, w) - mu1 * mu2
    C1, C2 = 0.01 ** 2, 0.03 ** 2
    return ((2 * mu1 * mu2 + C1) * (2 * s12 + C2)) / ((mu1 * mu1 + mu2 * mu2 + C1) * (s1 + s2 + C2))


def _rows(a):
    return a.reshape(a.shape[0], -1).mean(1)


def ssim_rows(x, y, w=None):
    """[N,C,H,W] -> [N] per-image means of the SSIM map."""
    return _rows(ssim_map(x, y, w))


def mse_rows(x, y):
    d = np.asarray(x, np.float64) - np.asarray(y, np.float64)
    return _rows(d * d)


def l1_rows(x, y):
    return _rows(np.abs(np.asarray(x, np.float64) - np.asarray(y, np.float64)))


def psnr_rows(x, y):
    with np.errstate(divide="ignore"):
        return 20 * np.log10(1.0 / np.sqrt(mse_rows(x, y)))
