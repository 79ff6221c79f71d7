"""The reference's L1 + SSIM formula (utils/loss_utils.py:17-63) in torch on the CPU, at a chosen precision -- TEST
INFRASTRUCTURE. The 2-D 11 x 11 window goes through torch.nn.functional.conv2d(groups=C, padding=5) and the gradient comes
from torch autograd, exactly as the reference runs it.

    torch_loss(img, gt, l1_coeff, ssim_coeff, const, dtype) -> (value, gradient)
        value = l1_coeff * mean|x - y| + ssim_coeff * mean(ssim_map(x, y)) + const

In float32 this is "the reference's own fp32 evaluation": its distance from the float64 truth (oracle.l1_ssim) is what the
content-class tests of tests/test_loss_gpu.py measure the kernel against. In float64 it is pinned to the oracle by
tests/test_loss_ref_cpu.py. The window is the one csrc/loss.hip and the oracle use (fp32 taps over their running fp32 sum),
so that the distance is rounding error only."""
import torch

from tests import metrics_ref


def torch_loss(img, gt, l1_coeff, ssim_coeff, const, dtype=torch.float32):
    x = torch.as_tensor(img).detach().to(dtype).clone().requires_grad_()
    y = torch.as_tensor(gt).detach().to(dtype)
    C = x.shape[0]
    w = torch.from_numpy(metrics_ref.window(running_fp32_sum=True)).to(dtype).expand(C, 1, 11, 11).contiguous()
    conv = lambda a: torch.nn.functional.conv2d(a[None], w, padding=5, groups=C)[0]
    mu1, mu2 = conv(x), conv(y)
    mu1_sq, mu2_sq, mu1_mu2 = mu1.pow(2), mu2.pow(2), mu1 * mu2
    s1 = conv(x * x) - mu1_sq
    s2 = conv(y * y) - mu2_sq
    s12 = conv(x * y) - mu1_mu2
    C1, C2 = 0.01 ** 2, 0.03 ** 2
    ssim_map = ((2 * mu1_mu2 + C1) * (2 * s12 + C2)) / ((mu1_sq + mu2_sq + C1) * (s1 + s2 + C2))
    value = l1_coeff * (x - y).abs().mean() + ssim_coeff * ssim_map.mean() + const
    value.backward()
    return float(value.detach().double()), x.grad.detach().double().numpy()


def coeffs(kind, lam=0.2):
    """(l1_coeff, ssim_coeff, const) of c3dgs_amd.loss.{l1_ssim_loss, ssim, l1_loss}."""
    return {"loss": (1.0 - lam, -lam, lam), "ssim": (0.0, 1.0, 0.0), "l1": (1.0, 0.0, 0.0)}[kind]
