"""-m gpu: fused Adam (csrc/adam.hip, c3dgs_amd/optim.py) against torch.optim.Adam on the same device, the optimizer
the reference builds for the QAT loop (scene/gaussian_model.py:296-308: param groups with their own lr, eps=1e-15)."""
import pytest
import torch

pytestmark = pytest.mark.gpu


def _groups(tensors, lrs):
    return [{"params": [t], "lr": lr} for t, lr in zip(tensors, lrs)]


def test_fused_adam_follows_torch_adam_over_many_steps():
    from c3dgs_amd.optim import Adam
    g = torch.Generator(device="cuda").manual_seed(0)
    shapes = [(100_003, 3), (5000, 1, 3), (5000, 15, 3), (100_003, 1), (7001, 3), (7001, 4), (100_003, 1), (17,)]
    lrs = [0.00016, 0.0025, 0.0025 / 20, 0.05, 0.005, 0.001, 0.005, 0.01]
    a = [torch.randn(s, device="cuda", generator=g).requires_grad_() for s in shapes]
    b = [t.detach().clone().requires_grad_() for t in a]
    ours = Adam(_groups(a, lrs), lr=0.0, eps=1e-15)
    ref = torch.optim.Adam(_groups(b, lrs), lr=0.0, eps=1e-15)
    for step in range(25):
        for x, y in zip(a, b):
            grad = torch.randn(x.shape, device="cuda", generator=g) * (10.0 ** ((step % 5) - 3))
            if step == 3:
                grad[::2] = 0                                      # v stays tiny: exercises eps = 1e-15
            x.grad, y.grad = grad.clone(), grad.clone()
        ours.step()
        ref.step()
    for x, y, sh in zip(a, b, shapes):
        assert torch.allclose(x, y, rtol=2e-5, atol=1e-7), (sh, float((x - y).abs().max()))
        so, sr = ours.state[x], ref.state[y]
        assert float(so["step"]) == float(sr["step"]) == 25.0
        # the moments cancel through zero: compare against their scale (1-ulp differences of the lerp / fma contraction)
        assert float((so["exp_avg"] - sr["exp_avg"]).abs().max()) <= 2e-6 * float(sr["exp_avg"].abs().max())
        assert float((so["exp_avg_sq"] - sr["exp_avg_sq"]).abs().max()) <= 2e-6 * float(sr["exp_avg_sq"].abs().max())
    # state dicts are interchangeable
    ref2 = torch.optim.Adam(_groups([t.detach().clone().requires_grad_() for t in a], lrs), lr=0.0, eps=1e-15)
    ref2.load_state_dict(ours.state_dict())


def test_fused_adam_skips_parameters_without_grad_and_rejects_cpu():
    from c3dgs_amd.optim import Adam
    p, q = torch.ones(10, device="cuda", requires_grad=True), torch.ones(10, device="cuda", requires_grad=True)
    opt = Adam([p, q], lr=0.1)
    p.grad = torch.ones(10, device="cuda")
    opt.step()
    assert torch.equal(q, torch.ones(10, device="cuda")) and float(p[0]) == pytest.approx(0.9, rel=1e-5)
    c = torch.ones(4, requires_grad=True)
    c.grad = torch.ones(4)
    with pytest.raises(RuntimeError, match="no CPU path"):
        Adam([c], lr=0.1).step()
    with pytest.raises(RuntimeError, match="plain Adam"):
        Adam([p], weight_decay=0.1)


# ---------------------------------------------------------------------------------------------------------------------
# Edges of adam_kernel / abs_accumulate_kernel: ragged tails, misaligned bases (the all-scalar path), the 16384-block cap,
# both at::lerp forms, more than 16 tensors, mixed hyper-parameters. References: tests/adam_ref.py (float64 stage-wise bars
# 2u / 4u / 8u, and the op-by-op fp32 restatement for bit equality), pinned on the CPU by tests/test_adam_ref_cpu.py.
#
# p' goes through sqrtf and two divisions. They are correctly rounded in this build, so p' is asserted bit for bit as
# well (the ulp histogram is printed first); the 8u float64 bar is asserted next to it.
import ctypes as C          # noqa: E402
import math                 # noqa: E402

import numpy as np          # noqa: E402

from tests import adam_ref as R   # noqa: E402

SENTINEL = 0x4B5A5A5A       # guard words around every tensor a kernel writes
GUARD = 16                  # floats of guard in front (64 bytes: the view behind it is 16-byte aligned) and at least as many behind
ADAM_CAP_N = 4 * 1024 * 16384 + 5          # one ragged tail past the 16384-block cap of launch_adam
ALIGNMENTS = {"aligned": (0, 0, 0, 0), "param_off": (1, 0, 0, 0), "grad_off": (0, 1, 0, 0), "all_off": (1, 1, 1, 1)}


def _guarded(n, off=0):
    """-> (buffer, view): n floats starting GUARD + off floats into a sentinel-filled allocation. off = 1 gives the contiguous
    `[1:]` view of an aligned buffer: 4-byte aligned, not 16."""
    buf = torch.full((n + 2 * GUARD + 4,), SENTINEL, dtype=torch.int32, device="cuda").view(torch.float32)
    view = buf[GUARD + off:GUARD + off + n]
    assert view.data_ptr() % 16 == (4 * off) % 16 and view.is_contiguous()
    return buf, view


def _guards_intact(buf, view):
    lo = (view.data_ptr() - buf.data_ptr()) // 4
    ib = buf.view(torch.int32)
    return bool((ib[:lo] == SENTINEL).all()) and bool((ib[lo + view.numel():] == SENTINEL).all())


def _spread(n, gen, lo, hi):
    """Magnitudes 10^lo .. 10^hi, log-uniform, random sign."""
    mag = torch.pow(10.0, torch.rand(n, device="cuda", generator=gen) * (hi - lo) + lo)
    return mag * (torch.randint(0, 2, (n,), device="cuda", generator=gen).float() * 2 - 1)


def _fill_state(p, g, m, v, seed):
    """Gradients 1e-8 .. 1e4 with planted exact zeros, moments of matching spread, all in place (the views keep their guards)."""
    gen = torch.Generator(device="cuda").manual_seed(seed)
    n = p.numel()
    p.copy_(_spread(n, gen, -3, 2))
    g.copy_(_spread(n, gen, -8, 4))
    m.copy_(_spread(n, gen, -8, 4))
    v.copy_(_spread(n, gen, -8, 4) ** 2)
    g[3::7] = 0
    if n > 2:
        g[-2] = 0                                                  # a zero in the tail, a non-zero in the last element


def _bits(t):
    return t.view(torch.int32)


def _check_step(old, new, s, what, chunk=1 << 24):
    """old = (p, g, m, v) before the step, new = (p', m', v') after it (GPU tensors). Asserts the float64 bars and bit equality
    of all three outputs with the fp32 restatement, over every element, evaluated on the device in chunks; the head and the
    tail are compared with the numpy restatement as well (which also yields the printed ulp histogram of p')."""
    p0, g, m0, v0 = old
    p1, m1, v1 = new
    n = p0.numel()
    worst = [0.0, 0.0, 0.0]
    for lo in range(0, n, chunk):
        sl = slice(lo, min(n, lo + chunk))
        e = R.excess64(p0[sl], g[sl], m0[sl], v0[sl], p1[sl], m1[sl], v1[sl], s)
        worst = [max(a, b) for a, b in zip(worst, e)]
        rm, rv = R.moments32_torch(g[sl], m0[sl], v0[sl], s)
        assert torch.equal(_bits(rm), _bits(m1[sl])), f"{what}: exp_avg differs in bits from the fp32 restatement"
        assert torch.equal(_bits(rv), _bits(v1[sl])), f"{what}: exp_avg_sq differs in bits from the fp32 restatement"
        # p' in full as well (sqrt and / through float64, see adam_ref.param32_torch)
        rp = R.param32_torch(p0[sl], m1[sl], v1[sl], s)
        assert torch.equal(_bits(rp), _bits(p1[sl])), f"{what}: param differs in bits from the fp32 restatement"
    print(f"adam {what}: n={n} m' {worst[0]:.2f}u (bar 2)  v' {worst[1]:.2f}u (bar 4)  p' {worst[2]:.2f}u (bar 8)")
    assert worst[0] <= 2 and worst[1] <= 4 and worst[2] <= 8, (what, worst)
    for sl in ([slice(0, n)] if n <= 8192 else [slice(0, 4096), slice(n - 4101, n)]):      # numpy: all three, p' included
        c = lambda t: t[sl].cpu().numpy()
        rp, rm, rv = R.step32(c(p0), c(g), c(m0), c(v0), s)
        assert np.array_equal(rm.view(np.int32), c(m1).view(np.int32)), what
        assert np.array_equal(rv.view(np.int32), c(v1).view(np.int32)), what
        ulps = R.ulp_diff(c(p1), rp)
        hist = np.bincount(np.minimum(ulps, 4))
        print(f"adam {what}: p' ulp histogram vs fp32 restatement (0, 1, 2, 3, >=4): {hist.tolist()}")
        assert ulps.max() == 0, (what, hist.tolist())


def _adam_raw(rows, betas, eps):
    """rows: [(p, g, m, v, Scalars)] -> one c3dgs_adam_step launch with exactly these pointers and scalars."""
    from c3dgs_amd import _lib
    arr = (_lib.AdamTensor * len(rows))()
    for a, (p, g, m, v, s) in zip(arr, rows):
        a.param, a.grad, a.exp_avg, a.exp_avg_sq, a.n = p.data_ptr(), g.data_ptr(), m.data_ptr(), v.data_ptr(), p.numel()
        a.step_size, a.bias_correction2_sqrt = float(s.step_size), float(s.bc2_sqrt)
    _lib.check(_lib.lib().c3dgs_adam_step(len(rows), arr, betas[0], betas[1], eps,
                                          C.c_void_p(torch.cuda.current_stream().cuda_stream)))
    torch.cuda.synchronize()


@pytest.mark.parametrize("align", list(ALIGNMENTS))
@pytest.mark.parametrize("n", [1, 2, 3, 4, 5, 255, 1023, 1024, 1025, ADAM_CAP_N])
def test_adam_step_ragged_sizes_and_misaligned_bases(hip, n, align):
    """One step through c3dgs_adam_step itself: every n % 4, block edges, one tail past the block cap; each pointer aligned or
    the `[1:]` view of an aligned buffer (any misaligned pointer sends the whole tensor down the scalar path)."""
    lr, betas, eps, t = 0.0025, (0.9, 0.999), 1e-15, 7
    s = R.Scalars(lr, betas[0], betas[1], eps, t)
    bufs, views = zip(*[_guarded(n, off) for off in ALIGNMENTS[align]])
    p, g, m, v = views
    _fill_state(p, g, m, v, seed=n % 1000 + len(align))
    g_bits = _bits(g).clone()
    old = (p.clone(), g.clone(), m.clone(), v.clone())
    _adam_raw([(p, g, m, v, s)], betas, eps)
    _check_step(old, (p, m, v), s, f"n={n} {align}")
    assert all(_guards_intact(b, w) for b, w in zip(bufs, views)), "a word outside the tensor was written"
    assert torch.equal(_bits(g), g_bits), "the gradient is read-only"


@pytest.mark.parametrize("betas", [(0.9, 0.999), (0.3, 0.9), (0.0, 0.0), (0.5, 0.5)])
@pytest.mark.parametrize("t", [1, 7, 30_000])
def test_adam_lerp_forms_and_bias_correction(hip, betas, t):
    """1 - beta1 >= 0.5 takes at::lerp's second form (beta1 = 0.3, 0.0, and 0.5 exactly on the boundary); the step count
    goes through optim.Adam's state["step"]; bit equality with the fp32 restatement tells the forms apart."""
    from c3dgs_amd.optim import Adam
    n, lr, eps = 100_003, 0.01, 1e-15
    bufs, views = zip(*[_guarded(n) for _ in range(4)])
    p, g, m, v = views
    _fill_state(p, g, m, v, seed=t)
    param = p.requires_grad_()
    param.grad = g
    opt = Adam([param], lr=lr, betas=betas, eps=eps)
    opt.state[param] = {"step": torch.tensor(float(t - 1)), "exp_avg": m, "exp_avg_sq": v}
    old = tuple(x.detach().clone() for x in (p, g, m, v))
    opt.step()
    torch.cuda.synchronize()
    assert float(opt.state[param]["step"]) == float(t)
    s = R.Scalars(lr, betas[0], betas[1], eps, t)
    _check_step(old, (p.detach(), m, v), s, f"betas={betas} t={t}")
    assert all(_guards_intact(b, w.detach()) for b, w in zip(bufs, views))
    other = R.step32(*(x[:4096].cpu().numpy() for x in old), s, lerp_form=1 if s.w1 >= 0.5 else 2)[1]
    assert not np.array_equal(other, m[:4096].cpu().numpy()), "this input cannot tell the two lerp forms apart"


def _optimizer_case(shapes, groups_of, hyper, seed, t=3):
    """Parameters, gradients and moments each inside a guarded buffer; groups_of[k] = group of tensor k; hyper[group] =
    dict(lr, betas, eps). -> (optimizer, per-tensor records)."""
    from c3dgs_amd.optim import Adam
    recs, groups = [], [dict(params=[], **h) for h in hyper]
    for k, shape in enumerate(shapes):
        n = int(np.prod(shape))
        bufs, views = zip(*[_guarded(n) for _ in range(4)])
        p, g, m, v = views
        _fill_state(p, g, m, v, seed=seed + k)
        param = p.view(shape).requires_grad_()
        param.grad = g.view(shape)
        groups[groups_of[k]]["params"].append(param)
        recs.append(dict(param=param, bufs=bufs, views=(p, g, m, v), group=groups_of[k], shape=shape,
                         old=tuple(x.detach().clone() for x in (p, g, m, v))))
    opt = Adam(groups, lr=0.0)
    for r in recs:
        _, _, m, v = r["views"]
        opt.state[r["param"]] = {"step": torch.tensor(float(t - 1)), "exp_avg": m.view(r["shape"]), "exp_avg_sq": v.view(r["shape"])}
    return opt, recs


def _check_optimizer_case(recs, hyper, t, what):
    for k, r in enumerate(recs):
        h = hyper[r["group"]]
        s = R.Scalars(h["lr"], h["betas"][0], h["betas"][1], h["eps"], t)
        p, g, m, v = (x.detach() for x in r["views"])
        _check_step(r["old"], (p, m, v), s, f"{what} tensor {k}")
        assert all(_guards_intact(b, w.detach()) for b, w in zip(r["bufs"], r["views"])), (what, k)


@pytest.mark.parametrize("count", [17, 33])
def test_adam_more_than_sixteen_tensors_take_several_launches(hip, count):
    sizes = [1, 2, 3, 5, 255, 1025, 4099, 70_001]
    shapes = [(sizes[k % len(sizes)] + k,) for k in range(count)]
    hyper = [dict(lr=0.005, betas=(0.9, 0.999), eps=1e-15)]
    opt, recs = _optimizer_case(shapes, [0] * count, hyper, seed=count)
    opt.step()
    torch.cuda.synchronize()
    _check_optimizer_case(recs, hyper, 3, f"{count} tensors")


def test_adam_groups_with_different_betas_and_eps_flush_between_launches(hip):
    """Two tensors per group, groups interleaved in hyper-parameters: (0.9, 0.999, 1e-15) / (0.3, 0.9, 1e-8) / back to the
    first: every key change flushes the batch; each tensor must be stepped with ITS group's scalars."""
    hyper = [dict(lr=0.005, betas=(0.9, 0.999), eps=1e-15), dict(lr=0.02, betas=(0.3, 0.9), eps=1e-8),
             dict(lr=0.001, betas=(0.9, 0.999), eps=1e-15), dict(lr=0.001, betas=(0.9, 0.999), eps=1e-3)]
    shapes = [(1025,), (7, 3), (100_003,), (5,), (4096,), (333, 1, 3), (9,), (70_001,)]
    opt, recs = _optimizer_case(shapes, [0, 0, 1, 1, 2, 2, 3, 3], hyper, seed=77)
    opt.step()
    torch.cuda.synchronize()
    _check_optimizer_case(recs, hyper, 3, "mixed groups")


@pytest.mark.parametrize("n", [1, 3, 1025, 100_003])
def test_adam_zero_gradient_with_zero_moments_leaves_the_parameter_alone(hip, n):
    """v == 0: denom == eps == 1e-15, m == 0: the update is 0 / 1e-15 = 0, not NaN; from step 1 and at a later step."""
    from c3dgs_amd.optim import Adam
    for t in (1, 9):
        bufs, views = zip(*[_guarded(n) for _ in range(4)])
        p, g, m, v = views
        p.copy_(torch.linspace(-3, 3, n, device="cuda"))
        g.zero_(); m.zero_(); v.zero_()
        before = _bits(p).clone()
        param = p.requires_grad_()
        param.grad = g
        opt = Adam([param], lr=0.05, eps=1e-15)
        opt.state[param] = {"step": torch.tensor(float(t - 1)), "exp_avg": m, "exp_avg_sq": v}
        opt.step()
        torch.cuda.synchronize()
        assert torch.equal(_bits(p.detach()), before), "the parameter moved"
        assert not _bits(m).any() and not _bits(v).any(), "the moments must stay +0"
        assert all(_guards_intact(b, w.detach()) for b, w in zip(bufs, views))


def test_adam_production_sized_tensor_next_to_small_ones_in_one_launch(hip):
    """_features_rest of a non-indexed 3M-Gaussian model (3M x 15 x 3 = 135M floats, past the 16384-block cap: every thread
    walks its grid-stride loop several times) in ONE launch with tensors of 1, 5 and 1025 floats; checked in full on the device."""
    lr, betas, eps, t = 0.0025 / 20, (0.9, 0.999), 1e-15, 1
    s = R.Scalars(lr, betas[0], betas[1], eps, t)
    rows, keep = [], []
    for k, n in enumerate([5, 3_000_000 * 15 * 3, 1, 1025]):
        bufs, views = zip(*[_guarded(n) for _ in range(4)])
        p, g, m, v = views
        if n > 1 << 24:                                            # the big one starts from zero moments: nothing to clone but p
            gen = torch.Generator(device="cuda").manual_seed(9)
            for lo in range(0, n, 1 << 24):
                hi = min(n, lo + (1 << 24))
                p[lo:hi] = _spread(hi - lo, gen, -3, 2)
                g[lo:hi] = _spread(hi - lo, gen, -8, 4)
            g[3::7] = 0
            m.zero_(); v.zero_()
            old = (p.clone(), g, torch.zeros(1, device="cuda").expand(n), torch.zeros(1, device="cuda").expand(n))
        else:
            _fill_state(p, g, m, v, seed=k)
            old = (p.clone(), g.clone(), m.clone(), v.clone())
        rows.append((p, g, m, v, s))
        keep.append((bufs, views, old))
    _adam_raw(rows, betas, eps)
    for k, (bufs, views, old) in enumerate(keep):
        p, g, m, v = views
        _check_step(old, (p, m, v), s, f"production launch tensor {k}")
        assert all(_guards_intact(b, w) for b, w in zip(bufs, views)), k


ABS_BIG = 3_000_000 * 48
ABS_CASES = [(n, a) for n in (1, 3, 4, 5, 1023, 1025, ABS_BIG) for a in ("aligned",)] + \
            [(n, a) for n in (1, 3, 4, 5, 1023, 1025, (1 << 20) + 1) for a in ("g_off", "acc_off", "both_off")] + \
            [((1 << 23) + 3, "both_off")]      # past the 16384-block cap of the scalar path: its loop takes a second pass


@pytest.mark.parametrize("n,align", ABS_CASES)
def test_abs_accumulate_ragged_sizes_and_misaligned_bases(hip, n, align):
    """acc += |g| is a single fp32 add per element: bit-exact against float64 acc + |g| rounded once. A misaligned base takes
    the scalar grid-stride path (every element), an aligned one float4 plus an n % 4 tail."""
    from c3dgs_amd import _lib
    offs = {"aligned": (0, 0), "g_off": (1, 0), "acc_off": (0, 1), "both_off": (1, 1)}[align]
    (gb, g), (ab, acc) = _guarded(n, offs[0]), _guarded(n, offs[1])
    gen = torch.Generator(device="cuda").manual_seed(n % 999)
    for lo in range(0, n, 1 << 24):
        hi = min(n, lo + (1 << 24))
        g[lo:hi] = _spread(hi - lo, gen, -8, 4)
        acc[lo:hi] = _spread(hi - lo, gen, -6, 3).abs()
    g[::5] = 0
    g[-1] = -3.25                                                  # the last element (tail) carries a non-zero, negative gradient
    g_bits, acc0 = _bits(g).clone(), acc.clone()
    _lib.check(_lib.lib().c3dgs_abs_accumulate(n, g.data_ptr(), acc.data_ptr(), C.c_void_p(torch.cuda.current_stream().cuda_stream)))
    torch.cuda.synchronize()
    for lo in range(0, n, 1 << 24):
        sl = slice(lo, min(n, lo + (1 << 24)))
        want = (acc0[sl].double() + g[sl].double().abs()).float()
        assert torch.equal(_bits(want), _bits(acc[sl])), (n, align, lo)
    assert float(acc[-1]) == float(acc0[-1] + 3.25)
    assert _guards_intact(gb, g) and _guards_intact(ab, acc) and torch.equal(_bits(g), g_bits)
