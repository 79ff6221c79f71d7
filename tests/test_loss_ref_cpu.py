"""CPU: tests/loss_ref.py (the reference's conv2d + autograd formula) in float64 equals the oracle's float64 direct sums,
value and gradient, for each of the three losses; and in float32 it is the formula the issue's figures were measured with."""
import numpy as np
import pytest
import torch

from tests import loss_ref


@pytest.mark.parametrize("shape", [(3, 1, 1), (3, 5, 7), (1, 23, 33), (4, 40, 40), (3, 66, 96)])
def test_float64_formula_equals_oracle(orc, shape):
    g = torch.Generator().manual_seed(shape[2])
    gt = torch.rand(*shape, generator=g)
    img = (gt + 0.1 * torch.randn(*shape, generator=g)).clamp(0, 1)
    for kind, lam in (("loss", 0.2), ("ssim", 1.0), ("l1", 0.0)):
        lo, l1, ss, gr = orc.l1_ssim(img.numpy(), gt.numpy(), lam)
        want = {"loss": lo, "ssim": ss, "l1": l1}[kind]
        want_grad = -gr.astype(np.float64) if kind == "ssim" else gr.astype(np.float64)      # lam = 1: loss = 1 - ssim
        val, grad = loss_ref.torch_loss(img, gt, *loss_ref.coeffs(kind), dtype=torch.float64)
        assert abs(val - want) < 1e-12, (kind, val, want)
        assert np.abs(want_grad).max() > 0
        assert np.abs(grad - want_grad).max() <= 1e-7 * np.abs(want_grad).max(), kind         # the oracle stores fp32 gradients


def test_fp32_formula_loses_accuracy_on_flat_content(orc):
    """The premise of the content-class bars: the reference's own fp32 evaluation is an order of magnitude further from the
    truth on a flat image than on noise (sigma = E[x^2] - mu^2 cancels)."""
    g = torch.Generator().manual_seed(1)
    shape = (3, 131, 203)
    gt = torch.rand(*shape, generator=g)
    noise = (gt + 0.1 * torch.randn(*shape, generator=g)).clamp(0, 1)
    flat_gt = torch.ones(*shape)
    flat = flat_gt.clone()
    flat[:, 40:80, 50:120] = torch.rand(3, 40, 70, generator=g)
    dev = {}
    for name, (a, b) in {"noise": (noise, gt), "flat": (flat, flat_gt)}.items():
        lo, _, _, gr = orc.l1_ssim(a.numpy(), b.numpy(), 0.2)
        val, grad = loss_ref.torch_loss(a, b, *loss_ref.coeffs("loss"))
        dev[name] = (abs(val - lo), np.abs(grad - gr).max() / np.abs(gr).max())
    assert dev["noise"][0] < 2e-7 and dev["noise"][1] < 1e-5, dev
    assert dev["flat"][1] > 3 * dev["noise"][1], dev
