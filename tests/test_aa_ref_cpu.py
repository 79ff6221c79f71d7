"""CPU: the mathematics of the antialiased mode's opacity factor as tests/aa_ref.py restates it, and the yardstick of the GPU bars.

  guards     every case of aa_ref.aa_case is what it claims to be (rows at the floor, clamped and still on screen, behind the
             near plane, cancelling needles, shared codebook rows, rho on the remaining rows from below 0.2 to above 0.9)
  gradcheck  torch.autograd.gradcheck of rho in float64 on 16 visible rows of each case away from the floor and the clamp edge
  zeros      rows with rho = 1 (behind the plane) and rows at the floor give exactly zero gradient, to every leaf
  closed     the derivatives of r the kernel uses, dr/da0 = (c0 D1 - D0 (c0 + h)) / D1^2, dr/dc0 likewise, dr/db = -2 b (D1 - D0)
             / D1^2, against autograd
  deviation  per case, for rho and for the VJP of sum o rho g to every leaf under a hashed cotangent: how far aa_ref in
             float32 lands from aa_ref in float64. Reference against reference; printed, and what tests/test_aa_gpu.py scales
             its bars from (aa_ref.f32_deviation).
All of this passes without the kernels."""
import numpy as np
import pytest
import torch

from tests import aa_ref


@pytest.mark.parametrize("name", aa_ref.AA_CASES)
def test_case_guards(name):
    c = aa_ref.aa_case(name)
    P = c["inp"]["means3D"].shape[0]
    assert P <= 4000 and (c["cam"]["W"], c["cam"]["H"]) == (200, 136)
    print(f"aa case {name}:", c["guard"])
    assert c["guard"]["visible"] >= 1000
    # floor rows are visible all the same: the low-pass alone gives them a radius
    if name == "floor":
        rows = c["t"]["floor"] & (c["radii"] > 0)
        assert int(c["radii"][rows].min()) >= 1


@pytest.mark.parametrize("name", aa_ref.AA_CASES)
def test_gradcheck_float64(name):
    rows = aa_ref.interior_rows(name, 16)
    inp, cam = aa_ref.sub_case(name, rows)
    lv = aa_ref.leaves_of(inp)
    keys = tuple(k for k in lv if k != "opacities")

    def f(*xs):
        return aa_ref.rho(dict(zip(keys, xs)), inp, cam)
    with torch.no_grad():
        t = aa_ref.terms(lv, inp, cam)
    assert bool(t["valid"].all()) and not bool(t["floor"].any())
    assert torch.autograd.gradcheck(f, tuple(lv[k] for k in keys), eps=1e-7, atol=1e-6, rtol=1e-4, nondet_tol=0.0)


@pytest.mark.parametrize("name", ["floor", "behind"])
def test_constant_rows_give_exactly_zero_gradient(name):
    c = aa_ref.aa_case(name)
    mask = c["t"]["floor"] if name == "floor" else c["t"]["behind"]
    assert int(mask.sum()) >= 10
    lv = aa_ref.leaves_of(c["inp"])
    rh = aa_ref.rho(lv, c["inp"], c["cam"])
    want = float(np.sqrt(aa_ref.R_FLOOR)) if name == "floor" else 1.0
    assert bool((rh.detach()[torch.as_tensor(mask)] == want).all())
    w = torch.as_tensor(aa_ref.hashed(len(mask), 3)) * torch.as_tensor(mask)
    (rh * w).sum().backward()
    for k, v in lv.items():
        assert v.grad is None or not bool(v.grad.any()), k


def test_closed_form_of_dr():
    g = torch.Generator().manual_seed(5)
    a0, c0 = (torch.rand(64, generator=g, dtype=torch.float64) * 3 + 0.01).requires_grad_(), \
        (torch.rand(64, generator=g, dtype=torch.float64) * 3 + 0.01).requires_grad_()
    b = ((torch.rand(64, generator=g, dtype=torch.float64) * 2 - 1) * (a0 * c0).sqrt().detach() * 0.99).requires_grad_()
    h = aa_ref.H_LOWPASS
    D0, D1 = a0 * c0 - b * b, (a0 + h) * (c0 + h) - b * b
    (D0 / D1).sum().backward()
    D0, D1 = D0.detach(), D1.detach()
    a, bb, c = a0.detach(), b.detach(), c0.detach()
    np.testing.assert_allclose(a0.grad, (c * D1 - D0 * (c + h)) / D1 ** 2, rtol=1e-12, atol=1e-14)
    np.testing.assert_allclose(c0.grad, (a * D1 - D0 * (a + h)) / D1 ** 2, rtol=1e-12, atol=1e-14)
    np.testing.assert_allclose(b.grad, -2 * bb * (D1 - D0) / D1 ** 2, rtol=1e-12, atol=1e-14)


@pytest.mark.parametrize("name", aa_ref.AA_CASES)
def test_float32_restatement_deviation(name):
    d = aa_ref.f32_deviation(name)
    print(f"aa_ref float32 against float64, {name}:", {k: "%.3e" % v for k, v in d.items()})
    assert all(np.isfinite(v) for v in d.values())
    assert set(d) >= {"rho", "means3D", "opacities"}
    # two evaluations of one formula: not the same number, and not far apart where nothing cancels
    assert d["rho"] > 0
    if name != "needles":
        assert d["rho"] < 1e-5 and max(d.values()) < 1e-4, d
