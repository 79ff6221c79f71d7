"""-m gpu: the job grid of the two apply kernels (csrc/jobs.hpp: JobTable, job_of_block) where the block lookup can go wrong: a
FULL table of 16 tensors, and sizes at which every job is ONE workgroup, so that block b must pick tensor b.

rows_apply:  out = in[src] bit for bit against torch indexing on the host; moments copied for originals, zero for clones, every
             output zero where src is -1.
mcmc_apply:  copy tensors and all moments bit for bit against tests/mcmc_ref.py's apply; the staged opacity and scale under the
             bar of tests/test_mcmc_gpu.py::test_relocation_values_against_float64.
zero width:  a model whose _features_rest is [P, 0, 3] (SH degree 0) goes through prune_points, densify_and_clone and relocate_gs:
             its tensor gets no job, its empty output is installed."""
import numpy as np
import pytest
import torch

from tests import mcmc_ref as ref
from tests.test_mcmc_gpu import _bar

pytestmark = pytest.mark.gpu

DEV = "cuda"
P = 300
ROW_FLOATS = [(1, 3, 4, 45, 48)[k % 5] for k in range(16)]
MIN_OPACITY = 0.005


def _tensors(seed, opacity=None):
    """16 host tensors [P, row_floats], every second one with two moment tensors."""
    g = torch.Generator().manual_seed(seed)
    params = [torch.randn(P, rf, generator=g) for rf in ROW_FLOATS]
    if opacity is not None:
        params[0] = opacity.reshape(P, 1).clone()
    moments = [(torch.randn(P, rf, generator=g), torch.rand(P, rf, generator=g) + 0.1) if k % 2 == 0 else None
               for k, rf in enumerate(ROW_FLOATS)]
    return params, moments


def _table(ins, outs, roles):
    """ins / outs: per tensor (param, exp_avg | None, exp_avg_sq | None) on the device -> the ctypes array."""
    from c3dgs_amd import _lib
    arr = (_lib.RowsTensor * len(ins))()
    for t, i, o, role in zip(arr, ins, outs, roles):
        t.in_param, t.out_param = i[0].data_ptr(), o[0].data_ptr()
        if i[1] is not None:
            t.in_exp_avg, t.in_exp_avg_sq, t.out_exp_avg, t.out_exp_avg_sq = i[1].data_ptr(), i[2].data_ptr(), o[1].data_ptr(), o[2].data_ptr()
        t.row_floats, t.role = int(i[0].shape[1]), role
    return arr


@pytest.mark.parametrize("P_new", [1, 257, 1025])
def test_rows_apply_over_a_full_table(hip, P_new):
    from c3dgs_amd import _lib
    params, moments = _tensors(P_new)
    g = torch.Generator().manual_seed(100 + P_new)
    src = torch.randint(0, P, (P_new,), generator=g, dtype=torch.int32)
    src[torch.rand(P_new, generator=g) < 0.05] = -1
    if P_new > 1:
        src[P_new // 2] = -1
    kind = (torch.rand(P_new, generator=g) < 0.4).to(torch.uint8)              # 0: original, 1: clone
    ins = [tuple(x.to(DEV) for x in (p,) + m) if m else (p.to(DEV), None, None) for p, m in zip(params, moments)]
    outs = [tuple(torch.full((P_new, p.shape[1]), float("nan"), device=DEV) if x is not None else None for x in i) for p, i in zip(params, ins)]
    src_d, kind_d = src.to(DEV), kind.to(DEV)
    arr = _table(ins, outs, [_lib.ROLE_COPY] * 16)
    # draw_row is read for child rows only: any [P_new] int32 buffer serves
    _lib.check(_lib.lib().c3dgs_rows_apply(P, P_new, src_d.data_ptr(), kind_d.data_ptr(), src_d.data_ptr(), 16, arr, 1, 0,
                                           None, None, None, 0, 0, _lib.stream(torch.device(DEV))))
    torch.cuda.synchronize()
    live = (src >= 0)[:, None]
    at = src.clamp(min=0).long()
    for k, (p, m, o) in enumerate(zip(params, moments, outs)):
        assert torch.equal(o[0].cpu(), torch.where(live, p[at], torch.zeros(()))), f"tensor {k} ({p.shape[1]} floats per row)"
        for x, got in zip(m or (), o[1:]):
            want = torch.where(live & (kind == 0)[:, None], x[at], torch.zeros(()))
            assert torch.equal(got.cpu(), want), f"moments of tensor {k} ({p.shape[1]} floats per row)"


@pytest.mark.parametrize("n", [1, 64, 257])
def test_mcmc_apply_over_a_full_table(hip, n):
    from c3dgs_amd import _lib, mcmc
    rng = np.random.default_rng(n)
    o = rng.uniform(0.1, 0.9, P)
    dead = np.zeros(P, dtype=bool)
    dead[rng.permutation(P)[:n]] = True
    opacity = torch.from_numpy(np.log(o / (1 - o)).astype(np.float32))
    params, moments = _tensors(200 + n, opacity)                               # tensor 0: the raw opacity, tensor 1: the raw scale
    roles = [_lib.MCMC_ROLE_OPACITY, _lib.MCMC_ROLE_SCALE] + [_lib.ROLE_COPY] * 14
    dev_t = [tuple(x.to(DEV) for x in (p,) + m) if m else (p.to(DEV), None, None) for p, m in zip(params, moments)]
    dead_d = torch.from_numpy(dead).to(DEV)
    dst = torch.nonzero(dead_d).squeeze(1).to(torch.int32)
    w = mcmc.weights(dev_t[0][0], dead_d)
    sources = mcmc.draw(w, torch.from_numpy(rng.random(n)).to(DEV))
    counts = w.counts.cpu().numpy()
    mcmc.apply(P, n, dst, 0, sources, w.counts, list(_table(dev_t, dev_t, roles)), True, MIN_OPACITY, w.ws, torch.device(DEV))
    torch.cuda.synchronize()
    dst_h, src_h = dst.cpu().numpy(), sources.cpu().numpy()
    assert not dead[src_h].any()
    names = ["opacity", "scale"] + [f"t{k}" for k in range(2, 16)]
    want, want_m = ref.apply({k: p.numpy() for k, p in zip(names, params)},
                             {k: (m[0].numpy(), m[1].numpy()) for k, m in zip(names, moments) if m}, dst_h, src_h, counts, True,
                             "scale", MIN_OPACITY)
    for k, (name, t) in enumerate(zip(names, dev_t)):
        got = t[0].cpu().numpy()
        if k >= 2:
            assert np.array_equal(got, want[name].astype(np.float32)), f"copy tensor {k} ({got.shape[1]} floats per row)"
        else:                                                                  # staged values: untouched rows keep their bits
            rest = np.ones(P, dtype=bool)
            rest[dst_h] = rest[src_h] = False
            assert np.array_equal(got[rest], params[k].numpy()[rest]) and np.array_equal(got[dst_h], got[src_h]), name
        if name in want_m:
            for a, b in zip(t[1:], want_m[name]):
                assert np.array_equal(a.cpu().numpy(), b), f"moments of tensor {k}"
    rows, on, c = ref.values(params[0].numpy(), counts, MIN_OPACITY)
    assert np.array_equal(rows, np.unique(src_h))
    got_op, got_sc = dev_t[0][0].cpu().numpy().astype(np.float64), dev_t[1][0].cpu().numpy().astype(np.float64)
    for a, i in enumerate(rows):
        op64, sc64 = ref.write_back(on[a:a + 1], c[a:a + 1], params[1].numpy()[i:i + 1])
        op32, sc32 = ref.write_back(on[a:a + 1], c[a:a + 1], params[1].numpy()[i:i + 1], np.float32)
        d_op = float(np.abs(got_op[i:i + 1] - op64.reshape(1, 1)).max() / np.abs(op64).max())
        d_sc = float(np.abs(got_sc[i:i + 1] - sc64).max() / np.abs(sc64).max())
        assert d_op <= _bar(op32, op64), (int(i), int(counts[i]), d_op, _bar(op32, op64))
        assert d_sc <= _bar(sc32, sc64), (int(i), int(counts[i]), d_sc, _bar(sc32, sc64))


# ------------------------------------------------------------------------------------------------ zero floats per row
P0 = 65


def _sh0_model(optimizer, seed):
    from c3dgs_amd.model import GaussianModel
    from c3dgs_amd.pipeline import OptimizationParams
    g = torch.Generator().manual_seed(seed)
    r = lambda *s: torch.randn(*s, generator=g)      # noqa: E731
    opacity = torch.where(torch.arange(P0) % 5 == 0, -8.0, 0.5).reshape(P0, 1) + 0.1 * r(P0, 1)     # every fifth row is dead
    m = GaussianModel(0, quantization=False, use_factor_scaling=True, device=DEV)
    m.set_tensors(xyz=r(P0, 3), features_dc=r(P0, 1, 3), features_rest=torch.zeros(P0, 0, 3), scaling=r(P0, 3).abs() + 0.1,
                  rotation=r(P0, 4), opacity=opacity, scaling_factor=r(P0, 1) * 0.5 - 3.0)
    m.spatial_lr_scale = 1.0
    if optimizer:
        m.training_setup(OptimizationParams())
        for g_ in m.optimizer.param_groups:
            g_["lr"] = 1e-3
        for p in m.parameters():
            p.grad = torch.randn(p.shape, generator=g).to(DEV)
        m.optimizer.step()
        m.optimizer.zero_grad(set_to_none=True)
    return m


_ATTRS = ("_xyz", "_features_dc", "_opacity", "_scaling", "_rotation", "_scaling_factor")


def _check_rows(m, before, rows, is_new, what):
    """Every parameter is before[rows], its moments too, but zero on the rows of `is_new`; _features_rest is [n, 0, 3]."""
    n = rows.shape[0]
    assert tuple(m._features_rest.shape) == (n, 0, 3) and m._features_rest.requires_grad, what
    for attr in _ATTRS:
        p = getattr(m, attr)
        assert torch.equal(p.detach(), before[attr][0][rows]), (what, attr)
        if m.optimizer is not None:
            st = m.optimizer.state[p]
            for got, old in zip((st["exp_avg"], st["exp_avg_sq"]), before[attr][1:]):
                want = torch.where(is_new.reshape([n] + [1] * (old.dim() - 1)), torch.zeros((), device=DEV), old[rows])
                assert torch.equal(got, want) and bool(want.any()), (what, attr)
    if m.optimizer is not None:
        st = m.optimizer.state[m._features_rest]
        assert tuple(st["exp_avg"].shape) == (n, 0, 3) and tuple(st["exp_avg_sq"].shape) == (n, 0, 3), what
        assert any(g["params"][0] is m._features_rest for g in m.optimizer.param_groups), what


def _before(m):
    out = {}
    for attr in _ATTRS:
        p = getattr(m, attr)
        st = m.optimizer.state[p] if m.optimizer is not None else None
        out[attr] = (p.detach().clone(),) + ((st["exp_avg"].clone(), st["exp_avg_sq"].clone()) if st else ())
    return out


@pytest.mark.parametrize("optimizer", [False, True])
def test_a_model_without_higher_sh_bands_is_rebuilt(hip, optimizer):
    m = _sh0_model(optimizer, 7)
    # prune_points
    before = _before(m)
    mask = (torch.arange(P0, device=DEV) % 3 == 1)
    m.prune_points(mask)
    kept = torch.nonzero(~mask).squeeze(1)
    _check_rows(m, before, kept, torch.zeros_like(kept, dtype=torch.bool), "prune_points")
    # densify_and_clone with an explicit mask: every original, then the selected rows with zero moments
    before, n = _before(m), m._xyz.shape[0]
    sel = torch.arange(n, device=DEV) % 4 == 2
    m.densify_and_clone(selected_pts_mask=sel)
    rows = torch.cat((torch.arange(n, device=DEV), torch.nonzero(sel).squeeze(1)))
    _check_rows(m, before, rows, torch.arange(rows.shape[0], device=DEV) >= n, "densify_and_clone")
    # relocate_gs: in place; the copy tensors of a destination are its source's
    before, n = _before(m), m._xyz.shape[0]
    dead = torch.sigmoid(m._opacity.detach().reshape(-1)) <= MIN_OPACITY
    n_dead = int(dead.sum())
    assert 0 < n_dead < n
    from c3dgs_amd import mcmc
    draws = torch.rand(n_dead, dtype=torch.float64, generator=torch.Generator().manual_seed(8)).to(DEV)
    w = mcmc.weights(m._opacity, dead)
    sources = mcmc.draw(w, draws).long()
    assert m.relocate_gs(dead, MIN_OPACITY, draws) == n_dead
    assert tuple(m._features_rest.shape) == (n, 0, 3)
    rows = torch.arange(n, device=DEV)
    rows[dead] = sources
    for attr in ("_xyz", "_features_dc", "_scaling", "_rotation"):
        assert torch.equal(getattr(m, attr).detach(), before[attr][0][rows]), ("relocate_gs", attr)
        if optimizer:
            st = m.optimizer.state[getattr(m, attr)]
            touched = dead.clone()
            touched[sources] = True
            keep = (~touched).reshape([n] + [1] * (before[attr][1].dim() - 1))
            assert torch.equal(st["exp_avg"], torch.where(keep, before[attr][1], torch.zeros((), device=DEV))), ("relocate_gs", attr)
