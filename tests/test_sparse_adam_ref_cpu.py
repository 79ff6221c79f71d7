"""CPU: tests/sparse_adam_ref.py (the reference of the sparse-Adam GPU tests) pinned to torch.optim.Adam in float64 run on the
gathered rows, its select to np.flatnonzero's meaning for each mask dtype, and its fp32 form to adam_ref.step32."""
import numpy as np
import pytest
import torch

from tests import adam_ref as R
from tests import sparse_adam_ref as S


def _mask(P, rng, frac=0.3):
    return rng.random(P) < frac


def test_select_lists_what_each_mask_kind_lists():
    m = np.array([0, 3, -2, 0, 1, -2**31, 2**31 - 1, 0], np.int32)
    assert list(S.select(m)[0]) == [1, 4, 6] and S.select(m)[1] == 3
    u = np.array([0, 1, 255, 0, 2], np.uint8)
    assert list(S.select(u)[0]) == [1, 2, 4]
    b = np.array([True, False, False, True])
    assert list(S.select(b)[0]) == [0, 3]
    assert S.select(np.zeros(0, np.uint8))[1] == 0 and S.select(np.zeros(7, np.int32))[1] == 0
    with pytest.raises(TypeError):
        S.select(np.zeros(4, np.float32))


@pytest.mark.parametrize("row_shape", [(), (3,), (15, 3)])
@pytest.mark.parametrize("betas,eps", [((0.9, 0.999), 1e-15), ((0.3, 0.9), 1e-8)])
def test_float64_form_equals_torch_adam_in_float64_on_the_gathered_rows(row_shape, betas, eps):
    """Six steps with a new mask each: a row's state advances only in the steps that list it, but with the GLOBAL step count in
    the bias correction. torch side: per step, an Adam over the gathered rows whose state is loaded from the full arrays with
    step = t - 1, run once, scattered back."""
    rng = np.random.default_rng(5)
    P, lr = 37, 0.01
    shape = (P,) + row_shape
    p, m, v = rng.standard_normal(shape), np.zeros(shape), np.zeros(shape)
    tp, tm, tv = p.copy(), m.copy(), v.copy()
    for t in range(1, 7):
        g = rng.standard_normal(shape) * 10.0 ** (t % 3 - 1)
        mask = _mask(P, rng)
        g[~mask] = np.nan                                          # never read
        s = R.Scalars(lr, betas[0], betas[1], eps, t, rounded=False)
        p, m, v = S.step64(p, g, m, v, mask, s)
        rows = np.flatnonzero(mask)
        if rows.size:
            q = torch.from_numpy(tp[rows]).requires_grad_()
            q.grad = torch.from_numpy(g[rows])
            opt = torch.optim.Adam([q], lr=lr, betas=betas, eps=eps, foreach=False)
            opt.state[q] = {"step": torch.tensor(float(t - 1)), "exp_avg": torch.from_numpy(tm[rows]),
                            "exp_avg_sq": torch.from_numpy(tv[rows])}
            opt.step()
            tp[rows], tm[rows], tv[rows] = q.detach().numpy(), opt.state[q]["exp_avg"].numpy(), opt.state[q]["exp_avg_sq"].numpy()
        np.testing.assert_allclose(p, tp, rtol=1e-12, atol=1e-15)
        np.testing.assert_allclose(m, tm, rtol=1e-12, atol=1e-300)
        np.testing.assert_allclose(v, tv, rtol=1e-12, atol=1e-300)
    assert np.isfinite(p).all()


@pytest.mark.parametrize("kind", ["bool", "uint8", "int32"])
def test_fp32_form_is_adam_ref_on_the_listed_rows_and_a_copy_elsewhere(kind):
    rng = np.random.default_rng(1)
    P, rl = 1025, 45
    p, g, m = (rng.standard_normal((P, rl)).astype(np.float32) for _ in range(3))
    v = (rng.standard_normal((P, rl)) ** 2).astype(np.float32)
    want = _mask(P, rng, 0.1)
    mask = {"bool": want, "uint8": want.astype(np.uint8) * 7, "int32": np.where(want, 5, rng.integers(-3, 1, P)).astype(np.int32)}[kind]
    assert np.array_equal(S.listed(mask), want)
    g[~want] = np.nan
    m[~want] = np.float32(np.inf)                                  # a sentinel the step must not touch
    s = R.Scalars(0.0025, 0.9, 0.999, 1e-15, 3)
    p2, m2, v2 = S.step32(p, g, m, v, mask, s)
    rp, rm, rv = R.step32(p[want], g[want], m[want], v[want], s)
    for got, ref, old in ((p2, rp, p), (m2, rm, m), (v2, rv, v)):
        assert np.array_equal(got[want].view(np.int32), ref.view(np.int32))
        assert np.array_equal(got[~want].view(np.int32), old[~want].view(np.int32))
    assert max(S.excess64(p, g, m, v, p2, m2, v2, mask, s)) <= 8
    assert S.excess64(p, g, m, v, p2, m2, v2, np.zeros(P, np.uint8), s) == (0.0, 0.0, 0.0)
    # a step that touched an unlisted row, or skipped a listed one, is seen
    skipped = p2.copy()
    skipped[np.flatnonzero(want)[0]] = p[np.flatnonzero(want)[0]]
    assert S.excess64(p, g, m, v, skipped, m2, v2, mask, s)[2] > 8
