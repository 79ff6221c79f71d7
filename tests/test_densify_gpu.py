"""-m gpu: adaptive density control (csrc/densify.hip, GaussianModel.densify_and_prune & co., pipeline.train).

1  the decision kernels (classify + plan) against tests/densify_ref.py on the same device tensors, exactly
2  every case of tests/golden/densify.npz (recorded from the reference itself); 2b the children's arithmetic alone
3  optimizer continuity; the separate methods in sequence against the staged restatement
4  the per-iteration stats kernel: bit-equal to the torch lines, no allocation
5  one host read, one apply launch, no nonzero / cat / index
6  training from a point cloud end to end
"""
import copy
import ctypes as C

import numpy as np
import pytest
import torch

from tests import densify_ref as dr

pytestmark = pytest.mark.gpu
DEV = "cuda"
CASES = dr.load_fixture()
ATTR = {"xyz": "_xyz", "f_dc": "_features_dc", "f_rest": "_features_rest", "opacity": "_opacity", "scaling": "_scaling",
        "rotation": "_rotation", "scaling_factor": "_scaling_factor"}
QA = ("opacity", "scaling", "scaling_factor")


def _stream():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def _ptr(t):
    return None if t is None else t.data_ptr()


def _classify(accum, denom, sc, ss, sps, spc, op, max_grad, dense, min_op, big):
    from c3dgs_amd import _lib
    P = accum.shape[0]
    code = torch.full((P,), 255, dtype=torch.uint8, device=DEV)
    _lib.check(_lib.lib().c3dgs_densify_classify(P, _ptr(accum), _ptr(denom), _ptr(sc), _ptr(ss), _ptr(sps), _ptr(spc), _ptr(op),
                                                 max_grad, dense, min_op, big, _ptr(code), _stream()))
    return code


def _plan(code, N):
    """c3dgs_rows_plan in one call with the largest possible capacity; rows beyond P_new must stay untouched."""
    from c3dgs_amd import _lib
    L = _lib.lib()
    P = code.shape[0]
    cap = P * (2 + N) + 3
    ws = torch.empty(max(L.c3dgs_rows_plan_workspace_bytes(P), 256), dtype=torch.uint8, device=DEV)
    totals = torch.full((4,), -7, dtype=torch.int32, device=DEV)
    src = torch.full((cap,), -5, dtype=torch.int32, device=DEV)
    kind = torch.full((cap,), 99, dtype=torch.uint8, device=DEV)
    draw = torch.full((cap,), -5, dtype=torch.int32, device=DEV)
    _lib.check(L.c3dgs_rows_plan(P, _ptr(code), N, cap, _ptr(src), _ptr(kind), _ptr(draw), _ptr(totals), _ptr(ws), _stream()))
    K, Cn, S, CK = totals.tolist()
    n = K + Cn + N * CK
    assert bool((src[n:] == -5).all()) and bool((kind[n:] == 99).all()) and bool((draw[n:] == -5).all())
    return src[:n], kind[:n], draw[:n], (K, Cn, S, CK)


def _decision_inputs(P, seed, mode):
    """Activated inputs with rows exactly at every threshold, 0/0, x/0, inf and NaN. Thresholds are the reference's Python
    doubles (0.0002, 0.005, 0.01 * extent, 0.1 * extent: none is an fp32 number)."""
    g = torch.Generator().manual_seed(seed)
    thr, min_op, extent = 0.0002, 0.005, 1.3
    dense, big = 0.01 * extent, 0.1 * extent
    f32 = lambda v: float(torch.tensor(v, dtype=torch.float32))     # noqa: E731
    denom = torch.randint(0, 4, (P,), generator=g).float()
    accum = torch.rand(P, generator=g) * 0.0012 * denom.clamp(min=1)
    accum[torch.rand(P, generator=g) < 0.05] *= -1
    zero = denom == 0
    accum[zero] *= (torch.rand(P, generator=g)[zero] > 0.5).float()                 # 0/0 and x/0
    sc = torch.rand(P, 3, generator=g) * 0.03
    ss = sc * (1 + 0.05 * torch.randn(P, 3, generator=g))
    sps = torch.rand(P, 3, generator=g) * 0.2
    spc = sps / 1.6
    op = torch.rand(P, generator=g) * 0.05
    special = torch.randperm(P, generator=g)[:min(P, 64)]
    for n, i in enumerate(special.tolist()):
        k = n % 16
        if k < 4:            # |g| exactly at / one ulp either side of the fp32 threshold, by an exact division
            accum[i] = torch.nextafter(torch.tensor(f32(thr)), torch.tensor([0.0, f32(thr), 1.0, f32(thr)][k])) * 2 * (-1 if k == 3 else 1)
            denom[i] = 2.0
        elif k < 7:          # max(scale) at / around dense_extent
            v = torch.nextafter(torch.tensor(f32(dense)), torch.tensor([0.0, f32(dense), 1.0][k - 4]))
            sc[i] = torch.tensor([v * 0.5, v, v * 0.25])
            ss[i] = sc[i]
            accum[i], denom[i] = 0.01, 1.0
        elif k < 10:         # opacity at / around min_opacity
            op[i] = torch.nextafter(torch.tensor(f32(min_op)), torch.tensor([0.0, f32(min_op), 1.0][k - 7]))
        elif k < 13:         # world size at / around big_extent
            v = torch.nextafter(torch.tensor(f32(big)), torch.tensor([0.0, f32(big), 1.0][k - 10]))
            sps[i] = torch.tensor([v, v * 0.5, v * 0.1])
            spc[i] = torch.tensor([v * 0.1, v * 0.5, v])
        elif k == 13:
            accum[i], denom[i] = float("inf"), 1.0
        elif k == 14:
            accum[i], denom[i] = float("nan"), 1.0
        else:
            sc[i, 1] = float("nan")
    if mode == "all_keep":
        accum.zero_(); denom.fill_(1.0); op.fill_(0.5); sps.fill_(0.01); spc.fill_(0.01)
    elif mode == "all_prune":
        op.fill_(0.001)
    elif mode == "all_clone":
        accum.fill_(1.0); denom.fill_(1.0); sc.fill_(0.001); ss.fill_(0.001); op.fill_(0.5); sps.fill_(0.01); spc.fill_(0.01)
    elif mode == "all_split":
        accum.fill_(1.0); denom.fill_(1.0); sc.fill_(0.5); ss.fill_(0.5); op.fill_(0.5); sps.fill_(0.01); spc.fill_(0.01)
    t = [x.to(DEV).contiguous() for x in (accum, denom, sc, ss, sps, spc, op)]
    return t, (thr, dense, min_op, big)


@pytest.mark.parametrize("P,mode", [(1, "mixed"), (63, "mixed"), (64, "mixed"), (65, "mixed"), (100_003, "mixed"), (3_000_000, "mixed"),
                                    (1, "all_split"), (1, "all_prune"), (100_003, "all_keep"), (100_003, "all_prune"),
                                    (100_003, "all_clone"), (100_003, "all_split")])
@pytest.mark.parametrize("screen", [False, True])
def test_decision_logic_is_exact(P, mode, screen):
    (accum, denom, sc, ss, sps, spc, op), thr = _decision_inputs(P, 11 + P % 97, mode)
    if not screen:
        sps = spc = None
    code = _classify(accum, denom, sc, ss, sps, spc, op, *thr)
    want = dr.classify_ref(accum.clone(), denom, sc, ss, sps, spc, op, *thr)
    assert torch.equal(code, want), (code != want).nonzero()[:10].tolist()
    for N in (2, 3):
        src, kind, draw, totals = _plan(code, N)
        wsrc, wkind, wdraw, wtotals = dr.plan_ref(want, N)
        assert totals == wtotals
        assert torch.equal(src.long(), wsrc) and torch.equal(kind.long(), wkind) and torch.equal(draw.long(), wdraw)
    if mode == "all_keep":
        assert totals == (P, 0, 0, 0)
    if mode == "all_prune" and not screen:
        assert totals[0] == totals[1] == totals[3] == 0
    if mode == "all_clone":
        assert totals == (P, P, 0, 0)
    if mode == "all_split":
        assert totals == (0, 0, P, P)


# ------------------------------------------------------------------------------------------------ the fixture
def _model_from_case(case, with_optimizer=True):
    from c3dgs_amd.model import GaussianModel
    from c3dgs_amd.pipeline import OptimizationParams
    params, moments = dr.case_tensors(case, DEV)
    quant, factor = bool(case["quantization"][0]), bool(case["use_factor_scaling"][0])
    m = GaussianModel(3, quantization=quant, use_factor_scaling=factor, device=DEV)
    m.set_tensors(xyz=params["xyz"], features_dc=params["f_dc"], features_rest=params["f_rest"], scaling=params["scaling"],
                  rotation=params["rotation"], opacity=params["opacity"], scaling_factor=params["scaling_factor"])
    m.spatial_lr_scale = 1.0
    if with_optimizer:
        m.training_setup(OptimizationParams(percent_dense=float(case["percent_dense"][0])))
        for k, attr in ATTR.items():
            p = getattr(m, attr)
            if p is not None:
                m.optimizer.state[p] = {"step": torch.tensor(3.0), "exp_avg": moments[k][0].clone(), "exp_avg_sq": moments[k][1].clone()}
    else:
        m.percent_dense = float(case["percent_dense"][0])
    m.xyz_gradient_accum = torch.from_numpy(case["accum"].copy()).to(DEV)
    m.denom = torch.from_numpy(case["denom"].copy()).to(DEV)
    m.max_radii2D = torch.from_numpy(case["max_radii2D"].copy()).to(DEV)
    for k in QA:
        if "qa_before_" + k in case:
            row = m._modules_qa[k]._row
            row[:3] = torch.from_numpy(case["qa_before_" + k].copy()).to(DEV)
            row[3:4].view(torch.int32)[0] = int(case["qa_before_" + k + "_zp"][0])
    return m, params, moments


def _check_qa(m, case, tag):
    for k in QA:
        if tag + k not in case:
            continue
        row = m._modules_qa[k]._row
        np.testing.assert_allclose(row[:3].cpu().numpy(), case[tag + k], rtol=3e-7, atol=0, err_msg=tag + k)
        assert int(row[3:4].view(torch.int32)[0]) == int(case[tag + k + "_zp"][0]), tag + k


def _child_bound(z, std, parent_xyz, rot_raw):
    """float64 children and the arithmetic bound 16 * 2^-24 * (|x| + sum_j |z_j std_j|) per component."""
    zz, sd = z.double(), std.double()
    q = rot_raw.double()
    q = q / q.norm(dim=1, keepdim=True)
    w, x, y, zq = q[:, 0], q[:, 1], q[:, 2], q[:, 3]
    R = torch.stack([1 - 2 * (y * y + zq * zq), 2 * (x * y - w * zq), 2 * (x * zq + w * y),
                     2 * (x * y + w * zq), 1 - 2 * (x * x + zq * zq), 2 * (y * zq - w * x),
                     2 * (x * zq - w * y), 2 * (y * zq + w * x), 1 - 2 * (x * x + y * y)], dim=1).reshape(-1, 3, 3)
    want = torch.bmm(R, (zz * sd).unsqueeze(-1)).squeeze(-1) + parent_xyz.double()
    spread = (zz * sd).abs().sum(1, keepdim=True)
    return want, 16 * 2.0 ** -24 * (want.abs() + spread), spread


@pytest.mark.parametrize("with_optimizer", [True, False])
@pytest.mark.parametrize("name", list(CASES))
def test_against_the_reference_fixture(name, with_optimizer):
    case = CASES[name]
    m, params, moments = _model_from_case(case, with_optimizer)
    N = int(case["N"][0])
    z = torch.from_numpy(case["z"].copy()).to(DEV)
    stats = (m.xyz_gradient_accum.clone(), m.denom.clone(), m.max_radii2D.clone())
    src, kind, draw_row, totals = dr.run_case_method(m, case, name, z)
    np.testing.assert_array_equal(src.cpu().numpy(), case["src"])
    np.testing.assert_array_equal(kind.cpu().numpy(), case["kind"])
    assert totals[2] * N == len(case["z"])
    src, kind = src.long(), kind.long()
    child, orig = kind >= 2, kind == 0
    n = len(src)
    for k, attr in ATTR.items():
        p = getattr(m, attr)
        if params[k] is None:
            assert p is None
            continue
        assert p.is_leaf and p.requires_grad and p.shape[0] == n, k
        rows = ~child if k in ("xyz", "scaling") else torch.ones_like(child)
        assert torch.equal(p.detach()[rows], params[k][src[rows]]), k                  # bit-equal copies
        if with_optimizer:
            group = [g for g in m.optimizer.param_groups if g["name"] == k][0]
            assert group["params"][0] is p and len(m.optimizer.state) == len(m.optimizer.param_groups)
            st = m.optimizer.state[p]
            assert float(st["step"]) == 3.0, k
            for got, had in ((st["exp_avg"], moments[k][0]), (st["exp_avg_sq"], moments[k][1])):
                assert got.shape == p.shape and torch.equal(got[orig], had[src[orig]]), k
                assert float(got[~orig].abs().sum()) == 0.0, k
    if name == "prune":
        assert torch.equal(m.xyz_gradient_accum, stats[0][src]) and torch.equal(m.denom, stats[1][src])
        assert torch.equal(m.max_radii2D, stats[2][src])
    else:
        assert tuple(m.xyz_gradient_accum.shape) == (n, 1) and tuple(m.denom.shape) == (n, 1) and tuple(m.max_radii2D.shape) == (n,)
        assert float(m.xyz_gradient_accum.abs().sum() + m.denom.abs().sum() + m.max_radii2D.abs().sum()) == 0.0
    _check_qa(m, case, "qa_after_")
    if bool(child.any()):
        np.testing.assert_array_equal(draw_row[child].cpu().numpy(), case["draw_row"])
        # child _scaling: rtol 3e-6 (what tests/test_model_gpu.py grants get_scaling_factor, the exp it comes from) + one ulp
        # for x / 1.6 against x * (1 / 1.6)
        got = m._scaling.detach()[child].cpu().numpy().astype(np.float64)
        want = case["child_scaling"].astype(np.float64)
        tol = 3e-6 * np.abs(want) + np.spacing(np.abs(case["child_scaling"])).astype(np.float64)
        err = np.abs(got - want)
        print(f"{name}: child scaling max err / tol = {(err / tol).max():.3f}")
        assert (err <= tol).all(), float((err / tol).max())
        # child xyz: the arithmetic bound of the kernel (test 2b) + 3e-6 * sum_j |z_j std_j| for the same tolerance on std
        par = src[child]
        std = torch.from_numpy(case["child_scaling"].copy()).to(DEV).double()
        std = (std.exp() if not bool(case["use_factor_scaling"][0]) else std) * (0.8 * N)
        parent = params["xyz"][par]
        if bool(case["quantization"][0]):
            parent = parent.half().float()
        _, bound, spread = _child_bound(z[draw_row[child].long()], std, parent, params["rotation"][par])
        err = (m._xyz.detach()[child].double() - torch.from_numpy(case["child_xyz"].copy()).to(DEV).double()).abs()
        tol = bound + 3e-6 * spread
        print(f"{name}: child xyz max err / tol = {float((err / tol).max()):.3f}")
        assert bool((err <= tol).all()), float((err / tol).max())
    if "reset_opacity" in case:
        m.reset_opacity()
        _check_qa(m, case, "qa_after_reset_")
        got, want = m._opacity.detach().cpu().numpy(), case["reset_opacity"]
        assert m._opacity.is_leaf and m._opacity.requires_grad
        # log(m / (1 - m)) of min(fake-quantised sigmoid, 0.01): a lattice value or 0.01 exactly, up to the scale's 3e-7 and
        # two roundings of the logit; rows at the lattice value 0 give -inf on both sides
        assert np.array_equal(np.isneginf(got), np.isneginf(want))
        fin = np.isfinite(want)
        np.testing.assert_allclose(got[fin], want[fin], rtol=2e-6, atol=0)
        if with_optimizer:
            st = m.optimizer.state[m._opacity]
            assert float(st["step"]) == 3.0 and float(st["exp_avg"].abs().sum() + st["exp_avg_sq"].abs().sum()) == 0.0


def test_child_arithmetic_alone():
    """c3dgs_rows_apply called directly: explicit std, z, raw rotations (unnormalised, norms from 1e-3 to 1e3) and parents;
    children against float64 with 16 * 2^-24 * (|x| + sum_j |z_j std_j|) per component; both scaling forms; moments zero."""
    from c3dgs_amd import _lib
    L = _lib.lib()
    g = torch.Generator().manual_seed(5)
    P, N = 20_011, 2
    xyz = (torch.randn(P, 3, generator=g) * 5).to(DEV)
    rot = (torch.randn(P, 4, generator=g) * torch.exp(torch.randn(P, 1, generator=g) * 2.5)).to(DEV)
    rot[:50] *= 1e-3
    rot[50:100] *= 1e3
    std = torch.exp(torch.randn(P, 3, generator=g) - 3).to(DEV)
    other = torch.randn(P, 3, generator=g).to(DEV)
    code = torch.full((P,), 12, dtype=torch.uint8, device=DEV)                       # every row split, children kept
    code[::7] = 1
    src, kind, draw, (K, Cn, S, CK) = _plan(code, N)
    z = torch.randn(N * S, 3, generator=g).to(DEV)
    n = K + Cn + N * CK
    for log_scaling in (0, 1):
        for half in (0, 1):
            outs = [torch.full((n, 3), 7.0, device=DEV) for _ in range(6)]
            mom = [torch.rand(P, 3, generator=g).to(DEV) for _ in range(4)]
            tab = (_lib.RowsTensor * 2)()
            tab[0].in_param, tab[0].out_param, tab[0].row_floats, tab[0].role = xyz.data_ptr(), outs[0].data_ptr(), 3, _lib.ROLE_XYZ
            tab[0].in_exp_avg, tab[0].in_exp_avg_sq = mom[0].data_ptr(), mom[1].data_ptr()
            tab[0].out_exp_avg, tab[0].out_exp_avg_sq = outs[1].data_ptr(), outs[2].data_ptr()
            tab[1].in_param, tab[1].out_param, tab[1].row_floats, tab[1].role = other.data_ptr(), outs[3].data_ptr(), 3, _lib.ROLE_SCALING
            tab[1].in_exp_avg, tab[1].in_exp_avg_sq = mom[2].data_ptr(), mom[3].data_ptr()
            tab[1].out_exp_avg, tab[1].out_exp_avg_sq = outs[4].data_ptr(), outs[5].data_ptr()
            _lib.check(L.c3dgs_rows_apply(P, n, _ptr(src), _ptr(kind), _ptr(draw), 2, tab, N, N * S, _ptr(rot), _ptr(std), _ptr(z),
                                          log_scaling, half, _stream()))
            s, child = src.long(), kind >= 2
            assert torch.equal(outs[0][~child], xyz[s[~child]]) and torch.equal(outs[3][~child], other[s[~child]])
            assert torch.equal(outs[1][~child], mom[0][s[~child]]) and torch.equal(outs[5][~child], mom[3][s[~child]])
            assert float(outs[1][child].abs().sum() + outs[2][child].abs().sum() + outs[4][child].abs().sum()) == 0.0
            par = s[child]
            parent = xyz[par].half().float() if half else xyz[par]
            want, bound, _ = _child_bound(z[draw[child].long()], std[par], parent, rot[par])
            err = (outs[0][child].double() - want).abs()
            print(f"log {log_scaling} half {half}: child xyz max err / bound = {float((err / bound).max()):.3f}")
            assert bool((err <= bound).all()), float((err / bound).max())
            sc = std[par].double() / (0.8 * N)
            sc = sc.log() if log_scaling else sc
            got = outs[3][child]
            tol = 3e-6 * sc.abs() + torch.from_numpy(np.spacing(got.abs().cpu().numpy())).to(DEV)   # as for the fixture's child _scaling
            err = (got.double() - sc).abs()
            print(f"log {log_scaling}: child scaling max err / tol = {float((err / tol).max()):.3f}")
            assert bool((err <= tol).all())


# ------------------------------------------------------------------------------------------------ optimizer, sequence
def test_optimizer_continues_after_densify_and_prune():
    """5 more steps of the fused Adam on seeded gradients against torch.optim.Adam loaded from the state dict taken right
    after the call; tolerances of tests/test_optim_gpu.py."""
    case = CASES["factor_qat_screen"]
    m, _, _ = _model_from_case(case)
    dr.run_case_method(m, case, "factor_qat_screen", torch.from_numpy(case["z"].copy()).to(DEV))
    ours = m.optimizer
    twins = [[p.detach().clone().requires_grad_()] for g in ours.param_groups for p in g["params"]]
    ref = torch.optim.Adam([{"params": t, "lr": g["lr"], "name": g["name"]} for t, g in zip(twins, ours.param_groups)], lr=0.0, eps=1e-15)
    ref.load_state_dict(copy.deepcopy(ours.state_dict()))      # load_state_dict keeps tensors that need no cast: copy first
    gen = torch.Generator(device=DEV).manual_seed(3)
    for g in ours.param_groups:
        g["lr"] = max(g["lr"], 1e-4)
    for g, go in zip(ref.param_groups, ours.param_groups):
        g["lr"] = go["lr"]
    for step in range(5):
        for go, gr in zip(ours.param_groups, ref.param_groups):
            grad = torch.randn(go["params"][0].shape, device=DEV, generator=gen) * (10.0 ** ((step % 3) - 3))
            go["params"][0].grad, gr["params"][0].grad = grad.clone(), grad.clone()
        ours.step()
        ref.step()
    for go, gr in zip(ours.param_groups, ref.param_groups):
        x, y = go["params"][0].detach(), gr["params"][0].detach()
        print(f"{go['name']}: max |ours - torch| {float((x - y).abs().max()):.3e}, max |x| {float(x.abs().max()):.3e}")
    for go, gr in zip(ours.param_groups, ref.param_groups):
        x, y = go["params"][0], gr["params"][0]
        assert torch.allclose(x, y, rtol=2e-5, atol=1e-7), (go["name"], float((x - y).abs().max()))
        so, sr = ours.state[x], ref.state[y]
        assert float(so["step"]) == float(sr["step"]) == 8.0
        assert float((so["exp_avg"] - sr["exp_avg"]).abs().max()) <= 2e-6 * float(sr["exp_avg"].abs().max())
        assert float((so["exp_avg_sq"] - sr["exp_avg_sq"]).abs().max()) <= 2e-6 * float(sr["exp_avg_sq"].abs().max())
    assert m._xyz is ours.param_groups[0]["params"][0]


def test_separate_methods_in_sequence_follow_the_staged_restatement():
    """prune_points, densify_and_clone, densify_and_split one after the other: the same scene as tests/densify_ref.py builds
    stage by stage on the same device (quantization off: the observers of both sides then only see the opacity, and every
    mask is taken on the same bits)."""
    case = CASES["factor_fp"]
    m, params, moments = _model_from_case(case)
    ref = dr.Staged({k: v.clone() for k, v in params.items() if v is not None}, {k: (a.clone(), b.clone()) for k, (a, b) in moments.items()},
                    m.xyz_gradient_accum.clone(), m.denom.clone(), m.max_radii2D.clone(), quantization=False,
                    percent_dense=m.percent_dense)
    g = torch.Generator().manual_seed(8)
    P = m._xyz.shape[0]
    mask = (torch.rand(P, generator=g) < 0.25).to(DEV)
    thr, extent = float(case["max_grad"][0]), float(case["extent"][0])
    with torch.no_grad():
        m.prune_points(mask)
        ref.prune_points(mask)
        assert torch.equal(m.xyz_gradient_accum, ref.accum) and torch.equal(m.max_radii2D, ref.max_radii2D)
        grads = ref.accum / ref.denom
        grads[grads.isnan()] = 0.0
        m.densify_and_clone(grads, thr, extent)
        ref.densify_and_clone(grads, thr, extent)
        assert m._xyz.shape[0] == ref.p["xyz"].shape[0] > int((~mask).sum())
        n = m._xyz.shape[0]
        grads = (torch.rand(n - 17, 1, generator=g) * 0.0006).to(DEV)                 # shorter than the scene: zero-padded
        scaling = ref.get_scaling
        S = int(((torch.cat([grads.squeeze(1), torch.zeros(17, device=DEV)]) >= thr) & (scaling.max(1).values > m.percent_dense * extent)).sum())
        z = torch.randn(2 * S, 3, generator=g).to(DEV)
        m.densify_and_split(grads, thr, extent, 2, draws=z)
        ref.densify_and_split(grads, thr, extent, 2, draws=z)
    child = ref.kind >= 2
    assert int(child.sum()) == 2 * S > 0
    for k, attr in ATTR.items():
        got, want = getattr(m, attr).detach(), ref.p[k]
        assert got.shape == want.shape, k
        if k in ("xyz", "scaling"):
            assert torch.equal(got[~child], want[~child]), k
            assert torch.allclose(got[child], want[child], rtol=1e-5, atol=1e-6), k   # fp32 evaluation order of R (z std) + x
        else:
            assert torch.equal(got, want), k
        st = m.optimizer.state[getattr(m, attr)]
        assert torch.equal(st["exp_avg"], ref.m[k][0]) and torch.equal(st["exp_avg_sq"], ref.m[k][1]), k


def test_indexed_models_are_rejected():
    from tests import synth
    from c3dgs_amd.model import GaussianModel
    sc = synth.scene(500, W=64, H=64, focal=60.0, seed=1)
    raw = synth.raw_params(synth.index_scene(sc, shs_extra=8, gs_extra=8))
    m = GaussianModel(3, device=DEV)
    m.set_tensors(**raw)
    m.percent_dense = 0.01
    for call in (lambda: m.densify_and_prune(0.0002, 0.005, 1.0, None), lambda: m.prune_points(torch.zeros(500, dtype=torch.bool)),
                 lambda: m.densify_and_clone(torch.zeros(500, 1), 0.0002, 1.0), lambda: m.densify_and_split(torch.zeros(500, 1), 0.0002, 1.0),
                 lambda: m.add_densification_stats(torch.zeros(500, 3), torch.zeros(500, dtype=torch.bool))):
        with pytest.raises(NotImplementedError, match="non-indexed"):
            call()


# ------------------------------------------------------------------------------------------------ stats
def test_densification_stats_equal_the_torch_lines_and_do_not_allocate():
    from c3dgs_amd.model import GaussianModel
    from tests import synth
    P = 50_021
    sc = synth.scene(P, W=320, H=200, focal=300.0, seed=2)
    norm = sc["scales"].norm(dim=1, keepdim=True)
    m = GaussianModel(3, quantization=False, device=DEV)
    m.set_tensors(xyz=sc["means3D"], features_dc=sc["shs"][:, :1], features_rest=sc["shs"][:, 1:], scaling=sc["scales"] / norm,
                  rotation=sc["rotations"], opacity=sc["opacities"], scaling_factor=torch.log(norm))
    g = torch.Generator(device=DEV).manual_seed(4)
    accum, denom, radii_max = torch.zeros(P, 1, device=DEV), torch.zeros(P, 1, device=DEV), torch.zeros(P, device=DEV)
    screen = torch.zeros(P, 3, device=DEV, requires_grad=True)
    calls = []
    for k in range(21):
        grad = torch.randn(P, 3, device=DEV, generator=g) * 10.0 ** ((k % 11) - 8)
        flt = torch.rand(P, device=DEV, generator=g) < 0.1 * (k % 10)
        radii = torch.randint(0, 200, (P,), device=DEV, generator=g, dtype=torch.int32)
        calls.append((grad, flt, radii))
    n0 = None
    for k, (grad, flt, radii) in enumerate(calls):
        screen.grad = grad
        if k == 1:                                              # after the warm-up call
            n0 = torch.cuda.memory_stats()["num_device_alloc"]
        if k % 2:
            m.add_densification_stats(screen, flt, radii)
        else:
            m.add_densification_stats(screen, flt)
    assert torch.cuda.memory_stats()["num_device_alloc"] == n0
    for k, (grad, flt, radii) in enumerate(calls):              # the reference's lines (train.py:105, :1400-1402)
        if k % 2:
            radii_max[flt] = torch.max(radii_max[flt], radii[flt])
        accum[flt] += torch.norm(grad[flt, :2], dim=-1, keepdim=True)
        denom[flt] += 1
    assert torch.equal(m.denom, denom) and torch.equal(m.max_radii2D, radii_max)
    bad = (m.xyz_gradient_accum != accum).sum().item()
    print("stats: accumulators differing from torch:", bad, "of", P)
    assert bad == 0


# ------------------------------------------------------------------------------------------------ one read, one pass
def _big_model(P, seed=6, optimizer=True):
    from c3dgs_amd.model import GaussianModel
    from c3dgs_amd.pipeline import OptimizationParams
    from tests import synth
    sc = synth.scene(P, seed=seed)
    norm = sc["scales"].norm(dim=1, keepdim=True)
    op = sc["opacities"].clamp(1e-6, 1 - 1e-6)
    m = GaussianModel(3, quantization=True, device=DEV)
    m.set_tensors(xyz=sc["means3D"], features_dc=sc["shs"][:, :1], features_rest=sc["shs"][:, 1:], scaling=sc["scales"] / norm,
                  rotation=sc["rotations"], opacity=torch.log(op / (1 - op)), scaling_factor=torch.log(norm))
    m.spatial_lr_scale = 1.0
    if optimizer:
        m.training_setup(OptimizationParams())
        for p in m.parameters():
            p.grad = torch.full_like(p, 1e-3)
        m.optimizer.step()
        m.optimizer.zero_grad(set_to_none=True)
    g = torch.Generator().manual_seed(seed)
    m.denom = torch.randint(0, 4, (P, 1), generator=g).float().to(DEV)
    m.xyz_gradient_accum = (torch.rand(P, 1, generator=g) * 0.0008).to(DEV) * m.denom.clamp(min=1)
    m.max_radii2D = torch.zeros(P, device=DEV)
    return m


class _HostReads(torch.utils._python_dispatch.TorchDispatchMode):
    """Records every ATen call that takes a GPU tensor and hands back host data (a CPU tensor or a Python scalar): copy_ into
    host memory, _to_copy to the CPU, _local_scalar_dense (item), equal, is_nonzero ... On this platform torch serves a small
    non-blocking copy into pinned memory with a copy KERNEL, so the profiler shows no 'Memcpy DtoH' activity for it; the
    dispatcher sees it whatever carries it."""

    def __init__(self):
        super().__init__()
        self.reads = []

    def __torch_dispatch__(self, func, types, args=(), kwargs=None):
        from torch.utils import _pytree as pytree
        out = func(*args, **(kwargs or {}))
        if any(isinstance(a, torch.Tensor) and a.is_cuda for a in pytree.tree_leaves((args, kwargs or {}))):
            for o in pytree.tree_leaves(out):
                if (isinstance(o, torch.Tensor) and not o.is_cuda) or isinstance(o, (bool, int, float)):
                    self.reads.append(str(func))
                    break
        return out


def test_one_host_read_and_one_apply_launch():
    """densify_and_prune at 1M rows: exactly one device->host transfer (counted at the dispatcher, and no memcpy the profiler
    sees is anything but device-to-device), exactly one launch of the apply kernel, no nonzero / cat / index."""
    import collections
    from torch.profiler import ProfilerActivity, profile
    P = 1_000_000
    m = _big_model(P)
    warm = _big_model(20_000, seed=7)
    warm.densify_and_prune(0.0002, 0.005, 1.5, 20)              # code objects loaded, pinned buffer of `warm` only
    torch.cuda.synchronize()
    reads = _HostReads()
    with profile(activities=[ProfilerActivity.CPU, ProfilerActivity.CUDA]) as prof:
        with reads:
            _, _, _, totals = m.densify_and_prune(0.0002, 0.005, 1.5, 20)
        torch.cuda.synchronize()
    events = list(prof.events())
    on_device = [e for e in events if e.device_type == torch.autograd.DeviceType.CUDA]
    names = [e.name for e in events]
    print("totals", totals, "rows", m._xyz.shape[0])
    assert min(totals) > 0 and totals[3] < totals[2]            # every stage did something
    print("host reads:", reads.reads)
    print("device events:", dict(collections.Counter(e.name[:48] for e in on_device)))
    assert len(reads.reads) == 1 and "copy_" in reads.reads[0], reads.reads
    copies = [e.name for e in on_device if "memcpy" in e.name.lower()]
    assert all("dtod" in n.lower() for n in copies), copies
    api_copies = [n for n in names if n.startswith("hipMemcpy")]
    assert len(api_copies) == len(copies), (api_copies, copies)  # every runtime copy call is one of the device-to-device ones
    applies = [e.name for e in on_device if "rows_apply_kernel" in e.name]
    assert len(applies) == 1, applies
    for op in ("aten::nonzero", "aten::cat", "aten::index", "aten::index_select", "aten::masked_select"):
        assert op not in names, op
    for p in m.parameters():
        assert p.shape[0] == m._xyz.shape[0] and bool(torch.isfinite(p).all())


# ------------------------------------------------------------------------------------------------ end to end
def test_training_from_a_point_cloud(tmp_path):
    from c3dgs_amd import pipeline
    from c3dgs_amd.model import PipelineParams
    from tests import train_scene
    student, cams, extent = train_scene.make(tmp_path, DEV)
    P0 = student._xyz.shape[0]
    before = train_scene.mean_psnr(student, cams)
    events = []

    class Scene:
        gaussians = student
        cameras_extent = extent

        def getTrainCameras(self):
            return cams

    def log(epoch, info):
        n = info["N"]
        for p in student.parameters():
            assert p.shape[0] == n
            st = student.optimizer.state.get(p)
            if st:
                assert st["exp_avg"].shape == p.shape and st["exp_avg_sq"].shape == p.shape
        assert student.xyz_gradient_accum.shape == (n, 1) and student.denom.shape == (n, 1) and student.max_radii2D.shape == (n,)
        assert len(student.optimizer.state) <= len(student.optimizer.param_groups)
        events.append((epoch, info))

    torch.manual_seed(0)
    iterations = pipeline.train(Scene(), None, train_scene.schedule(400), PipelineParams(), log=log, camera_stride=1,
                                degree_up_iter=80)
    assert iterations == 400
    dens = [(e, i["densified"]) for e, i in events if i["densified"] is not None]
    resets = [e for e, i in events if i["reset_opacity"]]
    print("densifications (epoch, rows before, (kept, clones, S, parents with children)):", dens)
    print("opacity resets at epochs", resets, "rows", P0, "->", student._xyz.shape[0])
    assert len(dens) >= 3 and len(resets) >= 1
    for p in student.parameters():
        assert bool(torch.isfinite(p).all())
        st = student.optimizer.state.get(p)
        if st:
            assert bool(torch.isfinite(st["exp_avg"]).all()) and bool(torch.isfinite(st["exp_avg_sq"]).all())
    assert student._xyz.shape[0] != P0
    # one call both added rows (clones, children) and removed rows (pruned originals, parents whose children were pruned)
    assert any(t[1] + 2 * t[3] > 0 and (rows - t[2] - t[0]) + (t[2] - t[3]) > 0 for _, (rows, t) in dens)
    after = train_scene.mean_psnr(student, cams)
    print(f"mean PSNR over the training views: {before:.3f} -> {after:.3f} dB")
    assert after > before
    assert student.active_sh_degree == 3
