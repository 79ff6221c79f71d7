"""CPU: tests/adam_ref.py (the references of the fused-Adam GPU tests) pinned to torch.optim.Adam in float64, its numpy and
torch forms pinned to each other, and the bars it states checked against the op-by-op fp32 restatement -- including that
the bars are tight enough to reject the defects they are meant to reject."""
import math

import numpy as np
import pytest
import torch

from tests import adam_ref as R


def _state(n, seed, decades=12):
    rng = np.random.default_rng(seed)
    mag = lambda: (10.0 ** rng.uniform(-decades / 2, decades / 2, n)) * rng.choice([-1.0, 1.0], n)
    p, g, m = (mag().astype(np.float32) for _ in range(3))
    v = (mag() ** 2).astype(np.float32)
    return p, g, m, v


@pytest.mark.parametrize("betas,eps", [((0.9, 0.999), 1e-15), ((0.3, 0.9), 1e-8), ((0.0, 0.0), 1e-15), ((0.5, 0.99), 1e-3)])
def test_float64_helper_equals_torch_adam_in_float64(betas, eps):
    """The formula: chained over 12 steps with the exact (unrounded) scalars, per group lr / betas / eps."""
    g = torch.Generator().manual_seed(3)
    shapes, lrs = [(1,), (5,), (1025,), (33, 7)], [0.01, 0.0025, 0.05, 1e-4]
    params = [torch.randn(s, generator=g, dtype=torch.float64).requires_grad_() for s in shapes]
    opt = torch.optim.Adam([{"params": [p], "lr": lr} for p, lr in zip(params, lrs)], lr=0.0, betas=betas, eps=eps, foreach=False)
    mine = [(p.detach().numpy().copy(), np.zeros(s), np.zeros(s)) for p, s in zip(params, shapes)]
    for t in range(1, 13):
        for k, p in enumerate(params):
            grad = torch.randn(p.shape, generator=g, dtype=torch.float64) * 10.0 ** ((t % 5) - 3)
            if t == 4:
                grad.view(-1)[::2] = 0
            p.grad = grad
            s = R.Scalars(lrs[k], betas[0], betas[1], eps, t, rounded=False)
            pp, m, v = mine[k]
            m2, v2 = R.moments64(grad.numpy(), m, v, s)
            p2, _ = R.param64(pp, m2, v2, s)
            mine[k] = (p2, m2, v2)
        opt.step()
    for k, p in enumerate(params):
        st = opt.state[p]
        np.testing.assert_allclose(mine[k][0], p.detach().numpy(), rtol=1e-12, atol=1e-15)
        np.testing.assert_allclose(mine[k][1], st["exp_avg"].numpy(), rtol=1e-12, atol=1e-300)
        np.testing.assert_allclose(mine[k][2], st["exp_avg_sq"].numpy(), rtol=1e-12, atol=1e-300)


def test_numpy_and_torch_forms_agree():
    p, g, m, v = _state(10_001, 0)
    s = R.Scalars(0.01, 0.9, 0.999, 1e-15, 7)
    p2, m2, v2 = R.step32(p, g, m, v, s)
    a = R.moments64(g, m, v, s) + R.param64(p, m2, v2, s)
    tt = lambda x: torch.from_numpy(x)
    b = R.moments64(tt(g), tt(m), tt(v), s) + R.param64(tt(p), tt(m2), tt(v2), s)
    for x, y in zip(a, b):
        np.testing.assert_allclose(x, y.numpy(), rtol=1e-14, atol=0)
    ea = R.excess64(p, g, m, v, p2, m2, v2, s)
    eb = R.excess64(tt(p), tt(g), tt(m), tt(v), tt(p2), tt(m2), tt(v2), s)
    assert ea == pytest.approx(eb, rel=1e-12)


@pytest.mark.parametrize("betas", [(0.9, 0.999), (0.3, 0.9), (0.0, 0.0), (0.5, 0.5)])
@pytest.mark.parametrize("t", [1, 7, 30_000])
def test_fp32_restatement_is_inside_the_float64_bars(betas, t):
    """With at::lerp's choice of form (measured here: m' <= 1.2u, v' <= 2.9u, p' <= 4.4u). The form at::lerp does NOT pick
    multiplies the rounding error of g - m by a weight >= 0.5 twice and lands at 2.0u - 3.6u: the float64 bar on m' already
    sees most of a wrong form; the bit-exact comparison of the GPU tests sees all of it."""
    p, g, m, v = _state(400_000, t)
    g[::17] = 0
    s = R.Scalars(0.01, betas[0], betas[1], 1e-15, t)
    p2, m2, v2 = R.step32(p, g, m, v, s)
    em, ev, ep = R.excess64(p, g, m, v, p2, m2, v2, s)
    assert em <= 2 and ev <= 4 and ep <= 8, (em, ev, ep)
    assert (s.w1 < 0.5) == (betas[0] > 0.5)                   # which form at::lerp picks: 1 - beta1 < 0.5 -> the first
    natural = 1 if s.w1 < 0.5 else 2
    assert np.array_equal(R.step32(p, g, m, v, s, lerp_form=natural)[1], m2)


@pytest.mark.parametrize("betas", [(0.9, 0.999), (0.3, 0.9), (0.0, 0.0)])
def test_torch_fp32_moments_equal_the_numpy_restatement_bit_for_bit(betas):
    p, g, m, v = _state(200_003, 11)
    g[::5] = 0
    s = R.Scalars(0.01, betas[0], betas[1], 1e-15, 3)
    _, m2, v2 = R.step32(p, g, m, v, s)
    tm, tv = R.moments32_torch(torch.from_numpy(g), torch.from_numpy(m), torch.from_numpy(v), s)
    assert np.array_equal(tm.numpy().view(np.int32), m2.view(np.int32))
    assert np.array_equal(tv.numpy().view(np.int32), v2.view(np.int32))
    p2 = R.step32(p, g, m, v, s)[0]
    tp = R.param32_torch(torch.from_numpy(p), tm, tv, s)
    assert np.array_equal(tp.numpy().view(np.int32), p2.view(np.int32))


def test_bars_reject_the_defects_they_are_meant_to_reject():
    p, g, m, v = _state(400_000, 5, decades=6)
    s = R.Scalars(0.01, 0.9, 0.999, 1e-15, 7)
    good = R.step32(p, g, m, v, s)
    # 1 - beta2 formed in float: 1.3e-5 relative on the w2 g^2 term
    bad = R.Scalars(0.01, 0.9, 0.999, 1e-15, 7)
    bad.w2 = np.float32(1.0) - np.float32(0.999)
    _, _, v_bad = R.step32(p, g, m, v, bad)
    assert R.excess64(p, g, m, v, good[0], good[1], v_bad, s)[1] > 4
    # a skipped element
    p_skip = good[0].copy()
    p_skip[-1] = p[-1]
    assert R.excess64(p, g, m, v, p_skip, good[1], good[2], s)[2] > 8
    # the wrong bias correction (t - 1)
    wrong = R.Scalars(0.01, 0.9, 0.999, 1e-15, 6)
    p_wrong, _, _ = R.step32(p, g, m, v, wrong)
    assert R.excess64(p, g, m, v, p_wrong, good[1], good[2], s)[2] > 8
    # the two lerp forms differ in bits somewhere, though both are inside the float64 bar
    s2 = R.Scalars(0.01, 0.3, 0.9, 1e-15, 7)
    assert not np.array_equal(R.step32(p, g, m, v, s2, lerp_form=1)[1], R.step32(p, g, m, v, s2, lerp_form=2)[1])
    # NaN is reported, not swallowed by a comparison that is false for NaN
    p_nan = good[0].copy()
    p_nan[3] = np.nan
    assert R.excess64(p, g, m, v, p_nan, good[1], good[2], s)[2] == math.inf


def test_zero_gradient_with_zero_moments_does_not_move_the_parameter():
    p = np.linspace(-3, 3, 1001, dtype=np.float32)
    z = np.zeros_like(p)
    s = R.Scalars(0.05, 0.9, 0.999, 1e-15, 1)
    p2, m2, v2 = R.step32(p, z, z, z, s)
    assert np.array_equal(p2, p) and not m2.any() and not v2.any()
    assert R.excess64(p, z, z, z, p2, m2, v2, s) == (0.0, 0.0, 0.0)


def test_ulp_diff():
    a = np.array([1.0, -1.0, 0.0, 1e-45], np.float32)
    assert list(R.ulp_diff(a, a)) == [0, 0, 0, 0]
    assert list(R.ulp_diff(a, np.nextafter(a, np.float32(np.inf)))) == [1, 1, 1, 1]
    assert R.ulp_diff(np.float32([-1e-45]), np.float32([1e-45]))[0] == 2
