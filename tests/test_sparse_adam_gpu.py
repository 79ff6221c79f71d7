"""-m gpu: sparse Adam (csrc/sparse_adam.hip, c3dgs_amd.optim.SparseGaussianAdam / visible_rows, GaussianModel.training_setup's
optimizer_type, pipeline.train's optimizer_type / optimizer_visibility).

select: rows[:count] against torch.nonzero at the block, wave and scan-sweep edges, for the three mask dtypes.
step:   the listed rows against tests/adam_ref.py's float64 bars (2u / 4u / 8u) AND bit for bit against c3dgs_adam_step run on the
        same rows gathered into dense tensors (both kernels inline adam_common.hpp's adam_one under -ffp-contract=off); the
        unlisted rows as int32 views against their bits before, with NaN / inf planted in their gradients and a sentinel in
        their moments; guard words around every buffer.
Shapes are the smallest at which the kernels change path: wave (64) and block (256) edges of the select, 65,537 rows (257
block totals: a scan thread with a ragged slice of its 16), 4,194,305 rows (16,385 totals: every wave of the scan workgroup
and its second sweep), and for the step more flattened elements than one 1024-element trip, than one workgroup and than the 4096
workgroups a tensor gets at most."""
import ctypes as C

import numpy as np
import pytest
import torch

from tests import adam_ref as R
from tests import test_optim_gpu as TO          # its guarded buffers, value spreads and the raw dense launch

pytestmark = pytest.mark.gpu

DEV = "cuda"
PS = [0, 1, 63, 64, 65, 255, 256, 257, 1025, 65_537]
P_SECOND_SWEEP = 16_384 * 256 + 1               # one row past what one sweep of the block-total scan covers
MASKS = ["none", "all", "first", "last", "alternating", "run300", "random10"]
ROW_LENS = [1, 3, 4, 45, 48]
NAN_BITS, SENTINEL_M, SENTINEL_V = 0x7FC12345, 0x7FA5A5A5, 0x4B3C3C3C


def _mask_bool(name, P, seed=0):
    m = torch.zeros(P, dtype=torch.bool, device=DEV)
    if P == 0 or name == "none":
        return m
    if name == "all":
        m[:] = True
    elif name == "first":
        m[0] = True
    elif name == "last":
        m[-1] = True
    elif name == "alternating":
        m[::2] = True
    elif name == "run300":
        lo = max(0, min(P - 300, 201))              # crosses a block edge where P allows
        m[lo:lo + 300] = True
    elif name == "random10":
        g = torch.Generator(device=DEV).manual_seed(seed + P)
        m = torch.rand(P, device=DEV, generator=g) < 0.1
    return m


def _as_kind(m, kind, seed=0):
    """The bool mask as the dtype `kind`; int32 carries 0 AND negative entries on the unlisted rows, and radii-like values on the others."""
    if kind == "bool":
        return m
    if kind == "uint8":
        g = torch.Generator(device=DEV).manual_seed(seed)
        return m.to(torch.uint8) * torch.randint(1, 256, m.shape, device=DEV, generator=g, dtype=torch.int32).to(torch.uint8)
    g = torch.Generator(device=DEV).manual_seed(seed + 1)
    pos = torch.randint(1, 2**31 - 1, m.shape, device=DEV, generator=g, dtype=torch.int64).to(torch.int32)
    neg = -torch.randint(0, 3, m.shape, device=DEV, generator=g, dtype=torch.int64).to(torch.int32)     # 0, -1, -2
    out = torch.where(m, pos, neg)
    if m.numel() > 2 and not bool(m[1]):
        out[1] = -2**31
    return out


def _stream():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


# ------------------------------------------------------------------------------------------------------------ select
@pytest.mark.parametrize("P", PS + [P_SECOND_SWEEP])
def test_select_lists_the_rows_of_every_mask_kind_in_order(hip, P):
    from c3dgs_amd import optim
    for name in MASKS:
        want_mask = _mask_bool(name, P)
        want = torch.nonzero(want_mask).flatten().to(torch.int32)
        for kind in ("bool", "uint8", "int32"):
            mask = _as_kind(want_mask, kind, seed=P)
            rows, count = optim.visible_rows(mask)
            assert rows.dtype == count.dtype == torch.int32 and rows.shape == (P,) and count.shape == (1,)
            n = int(count)
            assert n == want.numel(), (P, name, kind, n, want.numel())
            assert torch.equal(rows[:n], want), (P, name, kind)


def test_select_reads_a_mask_that_starts_at_any_byte(hip):
    """A contiguous slice of a bool tensor starts at an odd address: the mask is read byte by byte."""
    from c3dgs_amd import optim
    base = _mask_bool("random10", 1030, seed=3)
    for off in (1, 2, 3, 5):
        m = base[off:]
        assert m.is_contiguous() and m.data_ptr() % 4 == (base.data_ptr() + off) % 4
        rows, count = optim.visible_rows(m)
        assert torch.equal(rows[:int(count)], torch.nonzero(m).flatten().to(torch.int32))


# ------------------------------------------------------------------------------------------------------------ step
def _state(P, rl, listed, off, seed):
    """Four guarded [P * rl] buffers (each `off` floats past 16-byte alignment). Listed rows: tests/test_optim_gpu.py's spread
    of magnitudes with planted zero gradients. Unlisted rows: NaN / inf gradients, sentinel bit patterns in the moments."""
    n = P * rl
    if n == 0:                                                         # nothing to guard: four empty tensors
        views = tuple(torch.empty(0, device=DEV) for _ in range(4))
        return views, views
    bufs, views = zip(*[TO._guarded(n, off) for _ in range(4)])
    p, g, m, v = views
    if n:
        TO._fill_state(p, g, m, v, seed=seed)
        un = (~listed).repeat_interleave(rl)
        gi, mi, vi = (x.view(torch.int32) for x in (g, m, v))
        gi[un] = NAN_BITS
        g.view(P, rl)[(~listed).nonzero().flatten()[::2]] = float("inf")
        mi[un] = SENTINEL_M
        vi[un] = SENTINEL_V
    return bufs, views


def _sparse_raw(tensors, P, mask, betas, eps):
    """tensors: [(p, g, m, v, row_len, Scalars)] -> select + one c3dgs_sparse_adam_step launch with exactly these pointers."""
    from c3dgs_amd import _lib, optim
    ws = optim._select(mask)
    arr = (_lib.SparseAdamTensor * len(tensors))()
    for a, (p, g, m, v, rl, s) in zip(arr, tensors):
        a.param, a.grad, a.exp_avg, a.exp_avg_sq, a.n, a.row_len = p.data_ptr(), g.data_ptr(), m.data_ptr(), v.data_ptr(), p.numel(), rl
        a.step_size, a.bias_correction2_sqrt = float(s.step_size), float(s.bc2_sqrt)
    _lib.check(_lib.lib().c3dgs_sparse_adam_step(len(tensors), arr, P, ws.data_ptr(), betas[0], betas[1], eps, _stream()))
    torch.cuda.synchronize()


def _check(old, new, g_now, listed, rl, s, betas, eps, what):
    """old = clones of (p, g, m, v) before, new = (p, m, v) after, all flat [P * rl]; listed bool [P]."""
    P = listed.numel()
    if P * rl == 0:
        return
    rows = listed.nonzero().flatten()
    two = lambda x: x.view(P, rl)
    bits = lambda x: x.view(torch.int32)
    assert torch.equal(bits(g_now), bits(old[1])), f"{what}: the gradient is read-only"
    for name, a, b in zip(("param", "exp_avg", "exp_avg_sq"), (old[0], old[2], old[3]), new):
        assert torch.equal(two(bits(a))[~listed], two(bits(b))[~listed]), f"{what}: an unlisted row of {name} changed"
    if rows.numel() == 0:
        return
    gp, gg, gm, gv = (two(x)[rows].contiguous().view(-1) for x in old)
    before = (gp.clone(), gg.clone(), gm.clone(), gv.clone())
    TO._adam_raw([(gp, gg, gm, gv, s)], betas, eps)                     # the dense kernel on the gathered rows, same scalars
    got = [two(x)[rows].contiguous().view(-1) for x in new]
    e = R.excess64(*before, *got, s)
    assert e[0] <= 2 and e[1] <= 4 and e[2] <= 8, (what, e)
    for name, a, b in zip(("param", "exp_avg", "exp_avg_sq"), (gp, gm, gv), got):
        if not torch.equal(bits(a), bits(b)):
            ulps = R.ulp_diff(a.cpu().numpy(), b.cpu().numpy())
            hist = np.bincount(np.minimum(ulps, 4)).tolist()
            raise AssertionError(f"{what}: {name} of the listed rows differs from c3dgs_adam_step; ulp histogram (0, 1, 2, 3, >=4): {hist}")
    rm, rv = R.moments32_torch(before[1], before[2], before[3], s)      # and the fp32 restatement itself
    assert torch.equal(bits(rm), bits(got[1])) and torch.equal(bits(rv), bits(got[2])), what


# every (alignment, t, beta1) the issue names; a case takes the combination its index selects, so each row length meets all twelve
COMBOS = [(off, t, b1) for off in (0, 1) for t in (1, 2, 1000) for b1 in (0.9, 0.3)]


@pytest.mark.parametrize("rl", ROW_LENS)
def test_step_updates_listed_rows_like_the_dense_kernel_and_leaves_the_rest(hip, rl):
    k = rl
    for P in PS:
        for name in MASKS:
            listed = _mask_bool(name, P, seed=rl)
            mask = _as_kind(listed, ("bool", "uint8", "int32")[k % 3], seed=k)
            off, t, b1 = COMBOS[k % len(COMBOS)]
            k += 1
            betas, eps = (b1, 0.999 if b1 > 0.5 else 0.9), 1e-15
            s = R.Scalars(0.0025, betas[0], betas[1], eps, t)
            bufs, (p, g, m, v) = _state(P, rl, listed, off, seed=k)
            old = tuple(x.clone() for x in (p, g, m, v))
            _sparse_raw([(p, g, m, v, rl, s)], P, mask, betas, eps)
            _check(old, (p, m, v), g, listed, rl, s, betas, eps, f"rl={rl} P={P} {name} off={off} t={t} beta1={b1}")
            assert all(TO._guards_intact(b, w) for b, w in zip(bufs, (p, g, m, v))), (rl, P, name)


@pytest.mark.parametrize("off,t,b1", COMBOS)
def test_step_every_alignment_step_count_and_lerp_form_at_every_row_length(hip, off, t, b1):
    """The full cross at one size: 257 rows (two select blocks, and with 45 / 48 floats per row several trips), 10 % and all listed."""
    P = 257
    betas, eps = (b1, 0.999 if b1 > 0.5 else 0.9), 1e-15
    s = R.Scalars(0.01, betas[0], betas[1], eps, t)
    for rl in ROW_LENS + [7]:                                              # 7: a row length the kernel has no constant for
        for name in ("random10", "all", "alternating"):
            listed = _mask_bool(name, P, seed=t)
            bufs, (p, g, m, v) = _state(P, rl, listed, off, seed=rl + t)
            old = tuple(x.clone() for x in (p, g, m, v))
            _sparse_raw([(p, g, m, v, rl, s)], P, _as_kind(listed, "int32", seed=rl), betas, eps)
            _check(old, (p, m, v), g, listed, rl, s, betas, eps, f"rl={rl} {name} off={off} t={t} beta1={b1}")
            assert all(TO._guards_intact(b, w) for b, w in zip(bufs, (p, g, m, v)))


def test_step_past_the_block_cap_and_the_scan_sweep(hip):
    """4,194,305 rows of 3 floats, half of them listed: 6.3M flattened elements = 6144 trips over the 4096 workgroups a tensor
    gets at most (every workgroup walks its stride loop, some twice), and a list built by the two-sweep scan."""
    P, rl = P_SECOND_SWEEP, 3
    listed = _mask_bool("alternating", P)
    listed[-1] = True
    betas, eps = (0.9, 0.999), 1e-15
    s = R.Scalars(0.00016, betas[0], betas[1], eps, 7)
    bufs, (p, g, m, v) = _state(P, rl, listed, 0, seed=5)
    old = tuple(x.clone() for x in (p, g, m, v))
    _sparse_raw([(p, g, m, v, rl, s)], P, listed, betas, eps)
    _check(old, (p, m, v), g, listed, rl, s, betas, eps, "second sweep")
    assert all(TO._guards_intact(b, w) for b, w in zip(bufs, (p, g, m, v)))


# ------------------------------------------------------------------------------------------------------------ the optimizer class
def _optimizer_case(shapes, flagged, hyper, groups_of, listed, t=3, seed=0):
    """SparseGaussianAdam over guarded tensors; flagged[group] -> "per_gaussian". -> (optimizer, records)."""
    from c3dgs_amd.optim import SparseGaussianAdam
    recs, groups = [], [dict(params=[], **h, **({"per_gaussian": True} if f else {})) for h, f in zip(hyper, flagged)]
    for k, shape in enumerate(shapes):
        P, rl = shape[0], int(np.prod(shape[1:]))
        sparse = flagged[groups_of[k]]
        bufs, views = _state(P, rl, listed if sparse else torch.ones(P, dtype=torch.bool, device=DEV), 0, seed=seed + k)
        p, g, m, v = views
        param = p.view(shape).requires_grad_()
        param.grad = g.view(shape)
        groups[groups_of[k]]["params"].append(param)
        recs.append(dict(param=param, bufs=bufs, views=views, group=groups_of[k], shape=shape, sparse=sparse,
                         old=tuple(x.detach().clone() for x in views)))
    opt = SparseGaussianAdam(groups, lr=0.0)
    for r in recs:
        _, _, m, v = r["views"]
        opt.state[r["param"]] = {"step": torch.tensor(float(t - 1)), "exp_avg": m.view(r["shape"]), "exp_avg_sq": v.view(r["shape"])}
    return opt, recs


def _check_optimizer_case(opt, recs, hyper, listed, t, what):
    for k, r in enumerate(recs):
        h = hyper[r["group"]]
        s = R.Scalars(h["lr"], h["betas"][0], h["betas"][1], h["eps"], t)
        p, g, m, v = (x.detach() for x in r["views"])
        assert float(opt.state[r["param"]]["step"]) == float(t)
        if r["sparse"]:
            _check(r["old"], (p, m, v), g, listed, int(np.prod(r["shape"][1:])), s, h["betas"], h["eps"], f"{what} tensor {k}")
        else:
            TO._check_step(r["old"], (p, m, v), s, f"{what} dense tensor {k}")
        assert all(TO._guards_intact(b, w.detach()) for b, w in zip(r["bufs"], r["views"])), (what, k)


def test_more_than_sixteen_flagged_tensors_take_several_launches(hip):
    P = 300
    listed = _mask_bool("random10", P, seed=8)
    rls = [1, 3, 4, 45, 48, 2, 7]
    shapes = [(P, rls[k % len(rls)]) for k in range(35)]
    hyper = [dict(lr=0.005, betas=(0.9, 0.999), eps=1e-15)]
    opt, recs = _optimizer_case(shapes, [True], hyper, [0] * 35, listed)
    opt.step(_as_kind(listed, "int32"))
    torch.cuda.synchronize()
    _check_optimizer_case(opt, recs, hyper, listed, 3, "35 tensors")


def test_flagged_and_unflagged_groups_with_their_own_betas_and_eps_in_one_call(hip):
    """Sparse and dense tensors interleaved, three sets of hyper-parameters: each tensor is stepped by ITS kernel with ITS
    group's scalars; the unflagged ones move in every row (their length need not be P), a [P,15,3] tensor has 45-float rows."""
    P = 1025
    listed = _mask_bool("random10", P, seed=2)
    hyper = [dict(lr=0.005, betas=(0.9, 0.999), eps=1e-15), dict(lr=0.02, betas=(0.3, 0.9), eps=1e-8),
             dict(lr=0.001, betas=(0.9, 0.999), eps=1e-15), dict(lr=0.001, betas=(0.3, 0.9), eps=1e-3)]
    flagged = [True, False, True, True]
    shapes = [(P, 3), (P, 15, 3), (777, 5), (P,), (P, 1, 3), (P, 4), (P, 1), (P, 16, 3)]
    opt, recs = _optimizer_case(shapes, flagged, hyper, [0, 0, 1, 1, 2, 2, 3, 3], listed, seed=40)
    opt.step(listed)
    torch.cuda.synchronize()
    _check_optimizer_case(opt, recs, hyper, listed, 3, "mixed groups")


def _pair(shapes, per_gaussian=True, seed=0, cls=None):
    """-> (SparseGaussianAdam or `cls` over fresh parameters with gradients, the parameters)"""
    from c3dgs_amd.optim import SparseGaussianAdam
    g = torch.Generator(device=DEV).manual_seed(seed)
    params = [torch.randn(s, device=DEV, generator=g).requires_grad_() for s in shapes]
    groups = [{"params": [p], "lr": 0.01 * (k + 1)} for k, p in enumerate(params)]
    if per_gaussian and cls is None:
        for gr in groups:
            gr["per_gaussian"] = True
    return (cls or SparseGaussianAdam)(groups, lr=0.0, eps=1e-15), params


def _grads(params, seed):
    g = torch.Generator(device=DEV).manual_seed(seed)
    for p in params:
        p.grad = torch.randn(p.shape, device=DEV, generator=g)


def _bits_of(opt, params):
    out = []
    for p in params:
        st = opt.state[p]
        out += [p.detach().view(torch.int32).clone(), st["exp_avg"].view(torch.int32).clone(), st["exp_avg_sq"].view(torch.int32).clone()]
    return out


def test_all_true_mask_and_no_mask_equal_the_dense_optimizer_bit_for_bit(hip):
    from c3dgs_amd.optim import Adam
    shapes = [(1025, 3), (1025, 15, 3), (1025, 1), (1025, 4)]
    a, pa = _pair(shapes, seed=1)
    b, pb = _pair(shapes, seed=1, cls=Adam)
    c, pc = _pair(shapes, seed=1)
    everything = torch.ones(1025, dtype=torch.bool, device=DEV)
    for step in range(3):
        for ps in (pa, pb, pc):
            _grads(ps, 10 + step)
        a.step(everything)
        b.step()
        c.step()                                                          # visibility=None: the dense step
    for x, y, z in zip(_bits_of(a, pa), _bits_of(b, pb), _bits_of(c, pc)):
        assert torch.equal(x, y) and torch.equal(z, y)


def test_all_false_mask_changes_nothing_but_the_step_count(hip):
    opt, params = _pair([(300, 3), (300, 45)], seed=2)
    _grads(params, 1)
    opt.step(torch.ones(300, dtype=torch.uint8, device=DEV))
    before = _bits_of(opt, params)
    _grads(params, 2)
    opt.step(torch.zeros(300, dtype=torch.int32, device=DEV))
    for x, y in zip(before, _bits_of(opt, params)):
        assert torch.equal(x, y)
    assert all(float(opt.state[p]["step"]) == 2.0 for p in params)


def test_parameters_without_grad_are_skipped_and_bad_masks_raise(hip):
    opt, params = _pair([(300, 3), (300, 45)], seed=3)
    params[0].grad = torch.ones_like(params[0])
    kept = params[1].detach().clone()
    opt.step(torch.ones(300, dtype=torch.bool, device=DEV))
    assert torch.equal(params[1].detach(), kept) and len(opt.state[params[1]]) == 0 and float(opt.state[params[0]]["step"]) == 1.0
    _grads(params, 4)
    with pytest.raises(ValueError, match="301"):                          # the stale mask of another scene length
        opt.step(torch.ones(301, dtype=torch.bool, device=DEV))
    with pytest.raises(RuntimeError, match="no CPU path"):
        opt.step(torch.ones(300, dtype=torch.bool))
    with pytest.raises(ValueError, match="contiguous"):
        opt.step(torch.ones(600, dtype=torch.bool, device=DEV)[::2])
    with pytest.raises(ValueError, match="contiguous"):
        opt.step(torch.ones(300, 1, dtype=torch.bool, device=DEV))
    with pytest.raises(ValueError, match="bool, uint8 or int32"):
        opt.step(torch.ones(300, device=DEV))
    with pytest.raises(ValueError, match="bool, uint8 or int32"):
        opt.step(torch.ones(300, dtype=torch.int64, device=DEV))
    assert float(opt.state[params[0]]["step"]) == 1.0, "a refused call must not advance the step count"
    opt.step(torch.ones(300, dtype=torch.bool, device=DEV))
    assert float(opt.state[params[0]]["step"]) == 2.0 and float(opt.state[params[1]]["step"]) == 1.0


def test_state_dict_round_trip_through_torch_adam(hip):
    import copy
    shapes = [(300, 3), (300, 15, 3)]
    opt, params = _pair(shapes, seed=5)
    mask = _mask_bool("random10", 300, seed=5)
    for step in range(3):
        _grads(params, step)
        opt.step(mask)
    ref = torch.optim.Adam([{"params": [p.detach().clone().requires_grad_()], "lr": 0.01 * (k + 1)} for k, p in enumerate(params)],
                           lr=0.0, eps=1e-15)
    ref.load_state_dict(copy.deepcopy(opt.state_dict()))
    twin, tparams = _pair(shapes, seed=5)
    twin.load_state_dict(copy.deepcopy(ref.state_dict()))
    assert twin.param_groups[0].get("per_gaussian") is True
    for p, q in zip(params, tparams):
        q.data.copy_(p.data)
        for key in ("exp_avg", "exp_avg_sq"):
            assert torch.equal(opt.state[p][key], twin.state[q][key])
        assert float(twin.state[q]["step"]) == 3.0
    _grads(params, 9)
    _grads(tparams, 9)
    opt.step(mask)
    twin.step(mask)
    for x, y in zip(_bits_of(opt, params), _bits_of(twin, tparams)):
        assert torch.equal(x, y)


def test_two_identical_runs_give_identical_bits(hip):
    runs = []
    for _ in range(2):
        opt, params = _pair([(65_537, 3), (65_537, 15, 3), (65_537, 1)], seed=6)
        for step in range(3):
            _grads(params, step)
            opt.step(_mask_bool("random10", 65_537, seed=step))
        runs.append(_bits_of(opt, params))
    for x, y in zip(*runs):
        assert torch.equal(x, y)


def test_ten_steps_allocate_nothing(hip):
    opt, params = _pair([(20_001, 3), (20_001, 15, 3), (20_001, 1)], seed=7)
    masks = [_as_kind(_mask_bool("random10", 20_001, seed=k), ("bool", "uint8", "int32")[k % 3]) for k in range(12)]
    _grads(params, 0)
    for k in range(2):                                                    # warm-up: state tensors, the workspace
        opt.step(masks[k])
    torch.cuda.synchronize()
    allocated, calls = torch.cuda.memory_allocated(), torch.cuda.memory_stats()["num_device_alloc"]
    for k in range(2, 12):
        opt.step(masks[k])
    torch.cuda.synchronize()
    assert torch.cuda.memory_allocated() == allocated
    assert torch.cuda.memory_stats()["num_device_alloc"] == calls


# ------------------------------------------------------------------------------------------------------------ the model
def _two_view_model(optimizer_type, P=600):
    """tests/train_scene.py's toy model and two cameras yawed 28.5 degrees either way: each sees one half of the scene."""
    from c3dgs_amd.pipeline import OptimizationParams
    from tests import synth, train_scene
    W, H, focal = 160, 112, 150.0
    m, _ = train_scene.teacher_model(P, W, H, focal, DEV)
    m.spatial_lr_scale = 1.0
    m.training_setup(OptimizationParams(), optimizer_type=optimizer_type)
    cams = []
    for sign in (1.0, -1.0):
        a = sign * np.radians(28.5) / 2
        intr, ev = synth.camera(W, H, focal, extrinsic_vector=(0.0, np.sin(a), 0.0, np.cos(a), 0.0, 0.0, 0.0))
        cams.append(train_scene.Cam(intr, ev, DEV))
    return m, cams


def _view_step(m, cam, sparse):
    from c3dgs_amd import loss
    from c3dgs_amd.model import PipelineParams
    bg = torch.zeros(3, device=DEV)
    pkg = m.render(cam, PipelineParams(), bg, gather_visible=False)
    target = torch.full_like(pkg["render"], 0.5)
    loss.l1_ssim_loss(pkg["render"], target, 0.2).backward()
    radii = pkg["radii"]
    assert radii.dtype == torch.int32 and radii.shape == (m._xyz.shape[0],)
    if sparse:
        m.optimizer.step(radii)
    else:
        m.optimizer.step()
    m.optimizer.zero_grad(set_to_none=True)
    return radii


def _model_bits(m):
    out = {}
    for group in m.optimizer.param_groups:
        p = group["params"][0]
        st = m.optimizer.state.get(p, {})
        if st:
            out[group["name"]] = tuple(x.detach().view(torch.int32).clone() for x in (p, st["exp_avg"], st["exp_avg_sq"]))
    return out


def test_rows_a_view_does_not_see_keep_their_bits_under_sparse_adam_and_move_under_default(hip):
    from c3dgs_amd.optim import Adam, SparseGaussianAdam
    results = {}
    for kind in ("sparse_adam", "default"):
        m, (cam_a, cam_b) = _two_view_model(kind)
        assert type(m.optimizer) is (SparseGaussianAdam if kind == "sparse_adam" else Adam)
        assert all(bool(g.get("per_gaussian")) == (kind == "sparse_adam") for g in m.optimizer.param_groups)
        radii_a = _view_step(m, cam_a, kind == "sparse_adam")
        snap = _model_bits(m)
        radii_b = _view_step(m, cam_b, kind == "sparse_adam")
        now = _model_bits(m)
        unseen_b = radii_b == 0
        moved_by_a = unseen_b & (radii_a > 0)
        assert int((radii_a > 0).sum()) > 50 and int((radii_b > 0).sum()) > 50 and int(moved_by_a.sum()) > 50
        # the tensors view A gave a gradient (f_rest has none while the active SH degree is 0)
        live = [name for name in snap if bool(snap[name][1].view(torch.float32)[moved_by_a].ne(0).any())]
        assert {"xyz", "f_dc", "opacity", "scaling", "rotation"} <= set(live), live
        results[kind] = {name: [bool(torch.equal(x[unseen_b], y[unseen_b])) for x, y in zip(snap[name], now[name])] for name in live}
        if kind == "sparse_adam":                                        # every tensor with a state, live or not
            for name in snap:
                assert all(torch.equal(x[unseen_b], y[unseen_b]) for x, y in zip(snap[name], now[name])), name
        else:                                                            # momentum from view A drags them along
            for name in live:
                changed = (snap[name][0] != now[name][0]).view(now[name][0].shape[0], -1).any(1)
                assert bool(changed[moved_by_a].any()), name
    assert all(all(v) for v in results["sparse_adam"].values()), results["sparse_adam"]
    assert not any(any(v) for v in results["default"].values()), results["default"]


def test_training_setup_reads_the_option_and_refuses_indexed_models(hip):
    from c3dgs_amd.optim import Adam, SparseGaussianAdam
    from c3dgs_amd.pipeline import OptimizationParams
    m, _ = _two_view_model("default", P=64)
    assert OptimizationParams().optimizer_type == "default"
    m.training_setup(OptimizationParams(optimizer_type="sparse_adam"))
    assert type(m.optimizer) is SparseGaussianAdam
    m.training_setup(OptimizationParams(optimizer_type="sparse_adam"), optimizer_type="default")
    assert type(m.optimizer) is Adam
    with pytest.raises(ValueError, match="optimizer_type"):
        m.training_setup(OptimizationParams(), optimizer_type="sparse")
    m._gaussian_indices = torch.zeros(64, dtype=torch.int64, device=DEV)
    with pytest.raises(NotImplementedError, match="non-indexed"):
        m.training_setup(OptimizationParams(), optimizer_type="sparse_adam")


def test_density_control_moves_the_state_of_the_sparse_optimizer_like_the_default_ones(hip):
    """densify_and_prune finds the moments through optimizer.state whatever the class: a sparse and a default model with the same
    state come out of it with the same bits; then a step with the new-length radii works and the old-length mask is refused."""
    models = []
    for kind in ("sparse_adam", "default"):
        m, cams = _two_view_model(kind, P=600)
        for p in m.parameters():
            p.grad = torch.full_like(p, 1e-3)
        m.optimizer.step()
        m.optimizer.zero_grad(set_to_none=True)
        g = torch.Generator().manual_seed(6)
        P = m._xyz.shape[0]
        m.denom = torch.randint(0, 4, (P, 1), generator=g).float().to(DEV)
        m.xyz_gradient_accum = (torch.rand(P, 1, generator=g) * 0.0008).to(DEV) * m.denom.clamp(min=1)
        m.max_radii2D = torch.zeros(P, device=DEV)
        torch.manual_seed(0)
        m.densify_and_prune(0.0002, 0.005, 1.5, 20)
        models.append((m, cams, P))
    (ms, cams, P_old), (md, _, _) = models
    P_new = ms._xyz.shape[0]
    assert P_new != P_old and md._xyz.shape[0] == P_new
    bs, bd = _model_bits(ms), _model_bits(md)
    assert set(bs) == set(bd) and len(bs) >= 6
    for name in bs:
        for x, y in zip(bs[name], bd[name]):
            assert x.shape[0] == P_new and torch.equal(x, y), name
    assert all(g.get("per_gaussian") for g in ms.optimizer.param_groups)
    radii = _view_step(ms, cams[0], True)
    assert radii.shape == (P_new,)
    for p in ms.parameters():
        assert bool(torch.isfinite(p).all())
    for p in ms.parameters():
        p.grad = torch.zeros_like(p)
    steps = [float(ms.optimizer.state[p]["step"]) for p in ms.parameters()]
    with pytest.raises(ValueError, match=str(P_old)):
        ms.optimizer.step(torch.ones(P_old, dtype=torch.int32, device=DEV))
    assert steps == [float(ms.optimizer.state[p]["step"]) for p in ms.parameters()]


def test_toy_training_with_sparse_adam_runs_to_the_end_and_lowers_the_loss(hip, tmp_path):
    from c3dgs_amd import loss, pipeline
    from c3dgs_amd.model import PipelineParams
    from c3dgs_amd.optim import SparseGaussianAdam
    from tests import train_scene
    student, cams, extent = train_scene.make(tmp_path, DEV)

    def mean_loss():
        bg = torch.zeros(3, device=DEV)
        with torch.no_grad():
            return sum(float(loss.l1_ssim_loss(student.render(c, PipelineParams(), bg)["render"], c.original_image, 0.2)) for c in cams) / len(cams)

    class Scene:
        gaussians = student
        cameras_extent = extent

        def getTrainCameras(self):
            return cams

    start = mean_loss()
    events = []
    torch.manual_seed(0)
    n = pipeline.train(Scene(), None, train_scene.schedule(400), PipelineParams(), camera_stride=1, degree_up_iter=80,
                       log=lambda e, i: events.append(i), optimizer_type="sparse_adam")
    assert n == 400 and type(student.optimizer) is SparseGaussianAdam
    assert sum(1 for i in events if i["densified"] is not None) >= 3
    for p in student.parameters():
        assert bool(torch.isfinite(p).all())
    end = mean_loss()
    print(f"sparse_adam toy training: mean loss {start:.4f} -> {end:.4f}, rows {events[0]['N']} -> {student._xyz.shape[0]}")
    assert end < start
    with pytest.raises(ValueError, match="optimizer_visibility"):
        pipeline.train(Scene(), None, train_scene.schedule(400), PipelineParams(), optimizer_visibility="seen")


def test_blended_visibility_steps_by_contrib_hits(hip, tmp_path, monkeypatch):
    """Two epochs of train(optimizer_visibility="blended"): the mask is the int32 contrib_hits of the view's own render, and
    with optimizer_visibility=None the sparse optimizer is stepped without a mask."""
    from c3dgs_amd import pipeline
    from c3dgs_amd.model import PipelineParams
    from c3dgs_amd.optim import SparseGaussianAdam
    from tests import train_scene
    student, cams, extent = train_scene.make(tmp_path, DEV)

    class Scene:
        gaussians = student
        cameras_extent = extent

        def getTrainCameras(self):
            return cams

    masks = []
    real = SparseGaussianAdam.step

    def step(self, visibility=None, closure=None):
        masks.append(visibility)
        return real(self, visibility, closure)

    monkeypatch.setattr(SparseGaussianAdam, "step", step)
    opt = train_scene.schedule(16, densify=False)
    n = pipeline.train(Scene(), None, opt, PipelineParams(), camera_stride=1, optimizer_type="sparse_adam", optimizer_visibility="blended")
    P = student._xyz.shape[0]
    assert n == 16 and len(masks) == 16
    for m in masks:
        assert m.dtype == torch.int32 and m.shape == (P,), (m.dtype, m.shape, P)
        assert int((m > 0).sum()) > 0 and int(m.min()) >= 0
    del masks[:]
    pipeline.train(Scene(), None, opt, PipelineParams(), camera_stride=1, optimizer_type="sparse_adam", optimizer_visibility=None)
    assert masks == [None] * 16
    del masks[:]
    pipeline.train(Scene(), None, opt, PipelineParams(), camera_stride=1, optimizer_type="sparse_adam")
    assert len(masks) == 16 and all(m.dtype == torch.int32 and m.shape == (P,) for m in masks)
    for p in student.parameters():
        assert bool(torch.isfinite(p).all())
