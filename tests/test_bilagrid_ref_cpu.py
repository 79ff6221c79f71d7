"""CPU: pins the reference of the bilateral-grid tests (tests/bilagrid_ref.py). The contract's direct formula and its closed-form
backward against the grid_sample form with autograd, values and both gradients, in float64; the total variation and its
closed-form gradient against autograd. These run NO product code and pass without the feature: they make sure that what the GPU
tests compare the kernels with is the mathematics of include/c3dgs_hip.h."""
import numpy as np
import pytest
import torch

from tests import bilagrid_ref as ref

CASES = [((1, 1, 1), (9, 7)), ((8, 16, 16), (33, 40)), ((3, 2, 5), (17, 33)), ((2, 2, 2), (3, 5)), ((1, 4, 3), (16, 16)),
         ((4, 1, 1), (1, 1))]


@pytest.mark.parametrize("shape,hw", CASES, ids=lambda v: "x".join(map(str, v)))
def test_direct_formula_is_the_grid_sample_form(shape, hw):
    G = ref.make_grid(*shape, seed=3)
    rgb = ref.make_image(*hw, shape[0], seed=5)
    assert not ref.offenders(rgb, shape[0]).any()
    dout = ref.hashed((3,) + hw, 7) - 0.5
    out, dG, drgb = ref.slice_grid_sample(G, rgb, dout)
    assert np.abs(ref.slice_direct(G, rgb) - out).max() < 1e-13
    dG_d, drgb_d, mag = ref.slice_backward_direct(G, rgb, dout)
    assert np.abs(dG_d - dG).max() < 1e-12 * max(1.0, mag.max())
    assert np.abs(drgb_d - drgb).max() < 1e-12
    assert (np.abs(dG_d) <= mag + 1e-15).all() and ((mag == 0) <= (dG_d == 0)).all()


def test_the_images_clamp_at_both_ends():
    rgb = ref.make_image(17, 33, 8, seed=5)
    luma = np.tensordot(ref.LUMA, rgb.astype(np.float64), 1)
    assert (luma < 0).any() and (luma > 1).any() and ((luma > 0) & (luma < 1)).sum() > luma.size // 2


def test_identity_grid_is_the_identity():
    rgb = ref.make_image(5, 6, 4, seed=2)
    assert np.array_equal(ref.slice_direct(ref.make_grid(1, 1, 1, seed=1, noise=0.0), rgb), rgb.astype(np.float64))
    G = ref.make_grid(4, 3, 2, seed=1, noise=0.0)                 # the hat weights of a cell add up to 1 within a rounding
    assert np.abs(ref.slice_direct(G, rgb) - rgb).max() < 1e-15


@pytest.mark.parametrize("C", [1, 3])
@pytest.mark.parametrize("shape", ref.SHAPES, ids=lambda v: "x".join(map(str, v)))
def test_tv_and_its_gradient(shape, C):
    X = np.stack([ref.make_grid(*shape, seed=11 + c) for c in range(C)])
    x = X.astype(np.float64)
    want = 0.0
    for axis in (2, 3, 4):                                   # the definition, spelled out
        if x.shape[axis] >= 2:
            d = np.diff(x, axis=axis)
            want += (d ** 2).sum() / (12 * d[0, 0].size)
    want /= C
    assert abs(ref.tv(X) - want) <= 1e-14 * max(want, 1.0)
    grad, mag = ref.tv_backward_direct(X)
    assert np.abs(grad - ref.tv_backward_autograd(X)).max() <= 1e-14
    assert (np.abs(grad) <= mag + 1e-18).all()
    if max(shape) == 1:
        assert ref.tv(X) == 0.0 and not grad.any()
    assert torch.is_tensor(ref.tv_torch(torch.zeros(C, 12, *shape)))
