"""-m gpu: prune, codebook compaction and representation switches of INDEXED models (csrc/index_plan.hip,
GaussianModel.prune_points_indexed / compact_codebooks / to_indexed / to_unindexed, pipeline.finetune(prune_interval=...)).

1  c3dgs_index_plan against tests/index_ref.py on the same device tensors, exactly: sizes either side of a block and of K > P,
   four index distributions, three pruned fractions, keep == NULL, one index space absent; capacities; bad indices
2  the model methods against tests/golden/index_prune.npz (recorded from the reference itself), with and without an optimizer
3  empty and degenerate models; round trips; rendering; one host read per rebuild
4  the fine-tuning driver with prune_interval

Everything but the rendered images is integer- or bit-exact."""
import ctypes as C
import random

import numpy as np
import pytest
import torch

from tests import index_ref as ir

pytestmark = pytest.mark.gpu
DEV = "cuda"
CASES = ir.load_fixture()
ATTR = {"xyz": "_xyz", "f_dc": "_features_dc", "f_rest": "_features_rest", "opacity": "_opacity", "scaling": "_scaling",
        "rotation": "_rotation", "scaling_factor": "_scaling_factor"}
COLOR, GEOMETRY = ("f_dc", "f_rest"), ("scaling", "rotation")


def _stream():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def _ptr(t):
    return None if t is None else t.data_ptr()


# ------------------------------------------------------------------------------------------------ the plan
def _plan(keep, idx0, K0, idx1, K1, P, caps=None):
    """c3dgs_index_plan in ONE call into sentinel-filled outputs. keep: bool [P] or None. -> outputs cut to their totals,
    totals; asserts that nothing at or beyond min(total, capacity) was written."""
    from c3dgs_amd import _lib
    L = _lib.lib()
    K0, K1 = (K0 if idx0 is not None else 0), (K1 if idx1 is not None else 0)
    cap = caps or (P + 3, K0 + 3, K1 + 3)
    ws = torch.empty(max(L.c3dgs_index_plan_workspace_bytes(P, K0, K1), 256), dtype=torch.uint8, device=DEV)
    ws.fill_(0xA5)                                                  # the library clears what it needs itself
    totals = torch.full((4,), -7, dtype=torch.int32, device=DEV)
    src = torch.full((cap[0],), -5, dtype=torch.int32, device=DEV)
    new0 = torch.full((cap[0],), -5, dtype=torch.int64, device=DEV)
    new1 = torch.full((cap[0],), -5, dtype=torch.int64, device=DEV)
    cb0 = torch.full((cap[1],), -5, dtype=torch.int32, device=DEV)
    cb1 = torch.full((cap[2],), -5, dtype=torch.int32, device=DEV)
    k8 = None if keep is None else keep.contiguous().view(torch.uint8)
    _lib.check(L.c3dgs_index_plan(P, _ptr(k8), _ptr(idx0), K0, _ptr(idx1), K1, *cap, _ptr(src), _ptr(new0), _ptr(new1), _ptr(cb0),
                                  _ptr(cb1), _ptr(totals), _ptr(ws), _stream()))
    Pn, K0n, K1n, bad = totals.tolist()
    n, n0, n1 = min(Pn, cap[0]), min(K0n, cap[1]), min(K1n, cap[2])
    assert bool((src[n:] == -5).all()) and bool((cb0[n0:] == -5).all()) and bool((cb1[n1:] == -5).all())
    assert bool((new0[n if idx0 is not None else 0:] == -5).all()) and bool((new1[n if idx1 is not None else 0:] == -5).all())
    return src[:n], new0[:n], new1[:n], cb0[:n0], cb1[:n1], (Pn, K0n, K1n, bad)


def _indices(P, K, dist, g):
    if dist == "uniform":
        return torch.randint(0, K, (P,), generator=g, dtype=torch.int64)
    if dist == "one_row":
        return torch.full((P,), K // 2, dtype=torch.int64)
    if dist == "identity":
        return torch.arange(P, dtype=torch.int64) % K
    return torch.full((P,), K - 1, dtype=torch.int64)               # only the last row


def _check_against_ref(keep, idx0, K0, idx1, K1, P):
    got = _plan(keep, idx0, K0, idx1, K1, P)
    k = keep if keep is not None else torch.ones(P, dtype=torch.bool, device=DEV)
    wsrc, wnew0, wnew1, wcb0, wcb1 = ir.plan_ref(k, idx0, K0, idx1, K1)
    src, new0, new1, cb0, cb1, totals = got
    assert totals == (len(wsrc), 0 if wcb0 is None else len(wcb0), 0 if wcb1 is None else len(wcb1), 0)
    assert torch.equal(src.long(), wsrc)
    if idx0 is not None:
        assert torch.equal(new0, wnew0) and torch.equal(cb0.long(), wcb0)
    if idx1 is not None:
        assert torch.equal(new1, wnew1) and torch.equal(cb1.long(), wcb1)
    return totals


@pytest.mark.parametrize("dist", ["uniform", "one_row", "identity", "last_row"])
@pytest.mark.parametrize("K", [1, 2, 300, 70_003])
@pytest.mark.parametrize("P", [1, 255, 256, 257, 70_001])
def test_plan_equals_the_restatement(P, K, dist):
    g = torch.Generator().manual_seed(P * 7 + K)
    idx0 = _indices(P, K, dist, g).to(DEV)
    K1 = 300
    idx1 = _indices(P, K1, "uniform", g).to(DEV)
    for frac in (0.0, 0.4, 1.0):
        keep = (torch.rand(P, generator=g) >= frac).to(DEV)
        totals = _check_against_ref(keep, idx0, K, idx1, K1, P)
        if frac == 0.0:
            assert totals[0] == P
            _check_against_ref(None, idx0, K, idx1, K1, P)          # keep == NULL: all survive
        if frac == 1.0:
            assert totals[:3] == (0, 0, 0)
        _check_against_ref(keep, idx0, K, None, 0, P)               # one index space absent
        _check_against_ref(keep, None, 0, idx0, K, P)
    _check_against_ref(None, None, 0, None, 0, P)                   # neither: the identity map of the rows


def test_rows_beyond_the_capacities_stay_untouched():
    P, K0, K1 = 5003, 700, 300
    g = torch.Generator().manual_seed(3)
    idx0, idx1 = _indices(P, K0, "uniform", g).to(DEV), _indices(P, K1, "uniform", g).to(DEV)
    keep = (torch.rand(P, generator=g) >= 0.4).to(DEV)
    wsrc, wnew0, wnew1, wcb0, wcb1 = ir.plan_ref(keep, idx0, K0, idx1, K1)
    for caps in ((1000, 100, 50), (1, 1, 1), (0, 0, 0), (len(wsrc) - 1, len(wcb0) - 1, len(wcb1) - 1)):
        src, new0, new1, cb0, cb1, totals = _plan(keep, idx0, K0, idx1, K1, P, caps=caps)     # asserts the sentinels
        assert totals == (len(wsrc), len(wcb0), len(wcb1), 0)       # the totals do not depend on the capacities
        assert torch.equal(src.long(), wsrc[:caps[0]]) and torch.equal(new0, wnew0[:caps[0]]) and torch.equal(new1, wnew1[:caps[0]])
        assert torch.equal(cb0.long(), wcb0[:caps[1]]) and torch.equal(cb1.long(), wcb1[:caps[2]])


def test_totals_only_call_writes_nothing_else():
    from c3dgs_amd import _lib
    L = _lib.lib()
    P, K = 1000, 77
    g = torch.Generator().manual_seed(4)
    idx = _indices(P, K, "uniform", g).to(DEV)
    keep = (torch.rand(P, generator=g) >= 0.5).to(DEV)
    ws = torch.empty(L.c3dgs_index_plan_workspace_bytes(P, K, K), dtype=torch.uint8, device=DEV)
    totals = torch.full((4,), -7, dtype=torch.int32, device=DEV)
    _lib.check(L.c3dgs_index_plan(P, _ptr(keep.view(torch.uint8)), _ptr(idx), K, _ptr(idx), K, 0, 0, 0, None, None, None, None, None,
                                  _ptr(totals), _ptr(ws), _stream()))
    cb, _ = ir.remap_ref(keep, idx, K)
    assert totals.tolist() == [int(keep.sum()), len(cb), len(cb), 0]
    _lib.check(L.c3dgs_index_plan(0, None, None, 0, None, 0, 0, 0, 0, None, None, None, None, None, _ptr(totals), _ptr(ws), _stream()))
    assert totals.tolist() == [0, 0, 0, 0]                          # P == 0


def test_bad_indices_are_counted_and_never_dereferenced():
    P, K0, K1 = 4099, 50, 60
    g = torch.Generator().manual_seed(5)
    idx0, idx1 = _indices(P, K0, "uniform", g), _indices(P, K1, "uniform", g)
    bad0 = torch.randperm(P, generator=g)[:40]
    bad1 = torch.randperm(P, generator=g)[:30]
    idx0[bad0] = torch.tensor([-1, K0, K0 + 1, -(2 ** 40), 2 ** 40, 2 ** 31, -(2 ** 31), 2 ** 32 + 3])[torch.arange(40) % 8]
    idx1[bad1] = torch.tensor([K1, -7, 2 ** 33])[torch.arange(30) % 3]
    idx0, idx1 = idx0.to(DEV), idx1.to(DEV)
    keep = (torch.rand(P, generator=g) >= 0.4).to(DEV)
    src, new0, new1, cb0, cb1, totals = _plan(keep, idx0, K0, idx1, K1, P)
    assert totals[3] == 70 and totals[0] == int(keep.sum())         # counted over all rows, kept or not
    for idx, K, new, cb in ((idx0, K0, new0, cb0), (idx1, K1, new1, cb1)):
        ok = (idx >= 0) & (idx < K)
        wcb, wnew = ir.remap_ref(keep & ok, idx, K)                 # the rows whose index is in range
        assert torch.equal(cb.long(), wcb)
        sel = ok[src.long()]
        assert torch.equal(new[sel], wnew) and bool((new[~sel] == -1).all())
    # the model refuses, and is left as it was
    m = _model(P, K0, K1, idx0, idx1, True, seed=6)
    before = {k: getattr(m, a).detach().clone() for k, a in ATTR.items()}
    with pytest.raises(RuntimeError, match="outside"):
        m.prune_points_indexed(~keep)
    with pytest.raises(RuntimeError, match="outside"):
        m.compact_codebooks()
    assert all(torch.equal(getattr(m, a).detach(), before[k]) for k, a in ATTR.items())
    assert torch.equal(m._feature_indices, idx0) and torch.equal(m._gaussian_indices, idx1)


# ------------------------------------------------------------------------------------------------ the model
def _model(P, C, G, idx0, idx1, with_optimizer, seed, quantization=True):
    """Seeded model with C colour rows and G geometry rows (C = P / G = P for a half that is not indexed) and, with an
    optimizer, step 3 and random non-zero moments on every parameter."""
    from c3dgs_amd.model import GaussianModel
    from c3dgs_amd.pipeline import OptimizationParams
    g = torch.Generator().manual_seed(seed)
    r = lambda *s: torch.randn(*s, generator=g)                     # noqa: E731
    m = GaussianModel(3, quantization=quantization, device=DEV)
    m.set_tensors(xyz=r(P, 3) * 2, features_dc=r(C, 1, 3) * 0.3, features_rest=r(C, 15, 3) * 0.05,
                  scaling=torch.rand(G, 3, generator=g) + 0.05, rotation=r(G, 4), opacity=r(P, 1) * 3 - 2.0,
                  scaling_factor=torch.log(torch.rand(P, 1, generator=g) * 0.2 + 1e-3), feature_indices=idx0, gaussian_indices=idx1)
    m.spatial_lr_scale = 1.0
    if with_optimizer:
        m.training_setup(OptimizationParams())
        for p in m.parameters():
            m.optimizer.state[p] = {"step": torch.tensor(3.0), "exp_avg": r(*p.shape).to(DEV) * 1e-3,
                                    "exp_avg_sq": torch.rand(p.shape, generator=g).to(DEV) * 1e-6}
    return m


def _snapshot(m):
    params = {k: getattr(m, a).detach().clone() for k, a in ATTR.items()}
    moments = None
    if m.optimizer is not None:
        moments = {k: (m.optimizer.state[getattr(m, a)]["exp_avg"].clone(), m.optimizer.state[getattr(m, a)]["exp_avg_sq"].clone())
                   for k, a in ATTR.items()}
    return params, moments


def _check_gathered(m, params, moments, maps, step=3.0):
    """Every parameter is before[map], a leaf that requires grad; its group points at it; moments are the gathers; step kept."""
    for k, a in ATTR.items():
        p = getattr(m, a)
        assert p.is_leaf and p.requires_grad and torch.equal(p.detach(), params[k][maps[k]]), k
        if moments is not None:
            group = [gr for gr in m.optimizer.param_groups if gr["name"] == k][0]
            assert group["params"][0] is p and len(m.optimizer.state) == len(m.optimizer.param_groups), k
            st = m.optimizer.state[p]
            assert float(st["step"]) == step, k
            assert torch.equal(st["exp_avg"], moments[k][0][maps[k]]) and torch.equal(st["exp_avg_sq"], moments[k][1][maps[k]]), k


@pytest.mark.parametrize("with_optimizer", [True, False])
@pytest.mark.parametrize("name", ["both", "color", "geometry"])
def test_model_against_the_reference_fixture(name, with_optimizer):
    case = CASES[name]
    P = 200
    dev = lambda k: torch.from_numpy(case[k].copy()).to(DEV)        # noqa: E731
    idx0 = dev("idx0") if "idx0" in case else None
    idx1 = dev("idx1") if "idx1" in case else None
    m = _model(P, 64 if idx0 is not None else P, 48 if idx1 is not None else P, idx0, idx1, with_optimizer, seed=11)
    m.xyz_gradient_accum, m.denom, m.max_radii2D = dev("accum_in"), dev("denom_in"), dev("max_radii2D_in")
    _ = m.get_opacity, m.get_scaling                                # observers as a render leaves them
    fq = m._fq_state.clone()
    params, moments = _snapshot(m)
    src, cb0, cb1, totals = m.prune_points_indexed(dev("mask"))
    assert torch.equal(m._fq_state.view(torch.int32), fq.view(torch.int32))         # no getter ran: no observer moved
    np.testing.assert_array_equal(src.cpu().numpy(), case["src"])
    maps = {k: src.long() for k in ATTR}
    for tag, idx, cb, new, keys in (("0", idx0, cb0, m._feature_indices, COLOR), ("1", idx1, cb1, m._gaussian_indices, GEOMETRY)):
        if idx is None:
            assert cb is None and new is None
            continue
        np.testing.assert_array_equal(cb.cpu().numpy(), case["cb_src" + tag])
        assert new.dtype == torch.int64 and new.is_contiguous()
        np.testing.assert_array_equal(new.cpu().numpy(), case["new_idx" + tag])
        for k in keys:
            maps[k] = cb.long()
    assert totals == (len(case["src"]), len(case["cb_src0"]) if idx0 is not None else 0,
                      len(case["cb_src1"]) if idx1 is not None else 0, 0)
    assert torch.equal(m.xyz_gradient_accum, dev("accum")) and torch.equal(m.denom, dev("denom"))
    assert torch.equal(m.max_radii2D, dev("max_radii2D"))
    _check_gathered(m, params, moments, maps)
    assert m.is_color_indexed == (idx0 is not None) and m.is_gaussian_indexed == (idx1 is not None)


def test_non_indexed_model_is_pointed_at_prune_points():
    m = _model(50, 50, 50, None, None, False, seed=12)
    with pytest.raises(RuntimeError, match="use prune_points"):
        m.prune_points_indexed(torch.zeros(50, dtype=torch.bool, device=DEV))
    with pytest.raises(RuntimeError, match="use prune_points"):
        m.compact_codebooks()


@pytest.mark.parametrize("with_optimizer", [True, False])
def test_pruning_everything_and_compacting_twice(with_optimizer):
    P, K0, K1 = 300, 40, 30
    g = torch.Generator().manual_seed(13)
    idx0, idx1 = _indices(P, K0, "uniform", g).to(DEV), _indices(P, K1, "uniform", g).to(DEV)
    m = _model(P, K0, K1, idx0, idx1, with_optimizer, seed=14)
    src, cb0, cb1, totals = m.prune_points_indexed(torch.ones(P, dtype=torch.bool, device=DEV))
    assert totals == (0, 0, 0, 0) and len(src) == len(cb0) == len(cb1) == 0
    for k, a in ATTR.items():
        p = getattr(m, a)
        assert p.shape[0] == 0 and p.requires_grad, k
        if with_optimizer:
            st = m.optimizer.state[p]
            assert st["exp_avg"].shape == p.shape and st["exp_avg_sq"].shape == p.shape and float(st["step"]) == 3.0
    assert m._feature_indices.shape == (0,) and m._gaussian_indices.shape == (0,) and m._feature_indices.dtype == torch.int64
    assert m.xyz_gradient_accum.shape == (0, 1) and m.max_radii2D.shape == (0,)
    src, cb0, cb1, totals = m.prune_points_indexed(torch.zeros(0, dtype=torch.bool, device=DEV))   # on the empty model: a no-op
    assert totals == (0, 0, 0, 0) and m._xyz.shape == (0, 3) and m._features_rest.shape == (0, 15, 3)
    # compaction is idempotent
    m = _model(P, K0 + 9, K1 + 9, idx0, idx1, with_optimizer, seed=15)
    _, cb0, cb1, totals = m.compact_codebooks()
    assert totals[0] == P and totals[1] <= K0 and totals[2] <= K1
    assert torch.equal(cb0.long(), torch.unique(idx0)) and torch.equal(cb1.long(), torch.unique(idx1))
    params, moments = _snapshot(m)
    fi, gi = m._feature_indices.clone(), m._gaussian_indices.clone()
    src, cb0b, cb1b, totals_b = m.compact_codebooks()
    ident = lambda n: torch.arange(n, dtype=torch.int32, device=DEV)        # noqa: E731
    assert totals_b == totals and torch.equal(src, ident(P)) and torch.equal(cb0b, ident(totals[1])) and torch.equal(cb1b, ident(totals[2]))
    assert torch.equal(m._feature_indices, fi) and torch.equal(m._gaussian_indices, gi)
    _check_gathered(m, params, moments, {k: slice(None) for k in ATTR})


# ------------------------------------------------------------------------------------------------ round trips, rendering
def _synth_model(indexed, quantization=True, with_optimizer=True, P=500, seed=1):
    from c3dgs_amd.model import GaussianModel
    from c3dgs_amd.pipeline import OptimizationParams
    from tests import synth
    sc = synth.scene(P, W=64, H=64, focal=60.0, seed=seed)
    m = GaussianModel(3, quantization=quantization, device=DEV)
    if indexed:
        m.set_tensors(**synth.raw_params(synth.index_scene(sc, shs_extra=8, gs_extra=8)))
    else:
        norm = sc["scales"].norm(dim=1, keepdim=True)
        op = sc["opacities"].clamp(1e-6, 1 - 1e-6)
        m.set_tensors(xyz=sc["means3D"], features_dc=sc["shs"][:, :1], features_rest=sc["shs"][:, 1:], scaling=sc["scales"] / norm,
                      rotation=sc["rotations"], opacity=torch.log(op / (1 - op)), scaling_factor=torch.log(norm))
    m.spatial_lr_scale = 1.0
    if with_optimizer:
        g = torch.Generator().manual_seed(seed)
        m.training_setup(OptimizationParams())
        for p in m.parameters():
            m.optimizer.state[p] = {"step": torch.tensor(3.0), "exp_avg": torch.randn(p.shape, generator=g).to(DEV) * 1e-3,
                                    "exp_avg_sq": torch.rand(p.shape, generator=g).to(DEV) * 1e-6}
    return m


def test_to_indexed_then_to_unindexed_is_the_identity():
    from c3dgs_amd.model import ColorMode
    m = _synth_model(indexed=False)
    params, moments = _snapshot(m)
    tensors = [getattr(m, a) for a in ATTR.values()]
    m.to_unindexed()                                                # not indexed: a no-op
    assert all(getattr(m, a) is t for a, t in zip(ATTR.values(), tensors))
    m.to_indexed()
    assert all(getattr(m, a) is t for a, t in zip(ATTR.values(), tensors))          # parameters and optimizer untouched
    ident = torch.arange(500, dtype=torch.int64, device=DEV)
    assert torch.equal(m._feature_indices, ident) and torch.equal(m._gaussian_indices, ident)
    assert m.color_index_mode == ColorMode.ALL_INDEXED
    fi = m._feature_indices
    m.to_indexed()                                                  # already indexed: a no-op
    assert m._feature_indices is fi
    m.to_unindexed()
    assert m._feature_indices is None and m._gaussian_indices is None and m.color_index_mode == ColorMode.NOT_INDEXED
    _check_gathered(m, params, moments, {k: slice(None) for k in ATTR})


def test_compact_then_unindex_expands_the_original_codebooks():
    m = _synth_model(indexed=True)
    params, moments = _snapshot(m)
    fi, gi = m._feature_indices.clone(), m._gaussian_indices.clone()
    assert len(torch.unique(fi)) < params["f_dc"].shape[0] or len(torch.unique(gi)) < params["scaling"].shape[0]
    m.compact_codebooks()
    m.to_unindexed()
    rows = torch.arange(500, device=DEV)
    maps = {k: rows for k in ATTR}
    maps.update({k: fi for k in COLOR})
    maps.update({k: gi for k in GEOMETRY})
    _check_gathered(m, params, moments, maps)                       # codebook[indices] of the original, moments alike
    # a half-indexed model expands the half it has
    h = _synth_model(indexed=True)
    h._gaussian_indices = None
    h._scaling, h._rotation = (t.detach()[gi].contiguous().requires_grad_(True) for t in (h._scaling, h._rotation))
    h.optimizer = None
    h.to_unindexed()
    assert h._feature_indices is None and torch.equal(h._features_dc.detach(), params["f_dc"][fi])
    assert torch.equal(h._features_rest.detach(), params["f_rest"][fi]) and torch.equal(h._scaling.detach(), params["scaling"][gi])


def test_fixture_unindexed_case():
    """The reference's to_unindexed gives codebook[indices] (recorded provenance); so does ours on the same index arrays."""
    case = CASES["unindexed"]
    idx0, idx1 = (torch.from_numpy(case[k].copy()).to(DEV) for k in ("idx0", "idx1"))
    m = _model(200, 64, 48, idx0, idx1, True, seed=16)
    params, moments = _snapshot(m)
    m.to_unindexed()
    rows = torch.arange(200, device=DEV)
    maps = {k: rows for k in ATTR}
    for k, a in (("f_dc", "_features_dc"), ("f_rest", "_features_rest"), ("scaling", "_scaling"), ("rotation", "_rotation")):
        maps[k] = torch.from_numpy(case["rows" + a].copy()).to(DEV)
    _check_gathered(m, params, moments, maps)


def test_rendering_survives_compaction_and_expansion():
    """quantization=False: the fused indexed path and the composed non-indexed path hand the rasterizer the same fp32 values
    (codebook[index] is a copy), so the three images are not merely within an image bar of each other but bit-equal."""
    from c3dgs_amd.model import PipelineParams
    from tests import synth
    from tests.train_scene import Cam
    m = _synth_model(indexed=True, quantization=False, with_optimizer=False)
    intr, ev = synth.camera(64, 64, 60.0)
    cam, bg = Cam(intr, ev, DEV), torch.zeros(3, device=DEV)
    with torch.no_grad():
        a = m.render(cam, PipelineParams(), bg)["render"].clone()
        m.compact_codebooks()
        b = m.render(cam, PipelineParams(), bg)["render"].clone()
        m.to_unindexed()
        c = m.render(cam, PipelineParams(), bg)["render"].clone()
    assert float(a.abs().max()) > 0 and bool(torch.isfinite(a).all())
    assert torch.equal(a, b)                                        # compaction changes no value any Gaussian reads
    print(f"indexed vs expanded: max |diff| {float((a - c).abs().max()):.3e}")
    assert torch.equal(a, c)


def test_to_unindexed_gives_zero_rows_for_indices_outside_the_codebook():
    P, K0, K1 = 300, 40, 30
    g = torch.Generator().manual_seed(22)
    idx0, idx1 = _indices(P, K0, "uniform", g), _indices(P, K1, "uniform", g)
    bad = torch.tensor([-1, K0, 2 ** 31, 2 ** 32 + 3, -(2 ** 32) + 5, 2 ** 40])     # the last three narrow to 3, 5 and 0
    idx0[:6] = bad
    idx1[10:16] = bad
    m = _model(P, K0, K1, idx0.to(DEV), idx1.to(DEV), True, seed=23)
    params, moments = _snapshot(m)
    m.to_unindexed()
    for keys, idx, K, rows in ((COLOR, idx0, K0, slice(0, 6)), (GEOMETRY, idx1, K1, slice(10, 16))):
        ok = ((idx >= 0) & (idx < K)).to(DEV)
        assert int((~ok).sum()) == 6
        for k in keys:
            p = getattr(m, ATTR[k])
            st = m.optimizer.state[p]
            assert torch.equal(p.detach()[ok], params[k][idx.to(DEV)[ok]]), k
            for t in (p.detach(), st["exp_avg"], st["exp_avg_sq"]):
                assert t.shape[0] == P and float(t[rows].abs().sum()) == 0.0, k


def test_index_arrays_of_another_length_are_refused():
    P = 100
    g = torch.Generator().manual_seed(24)
    m = _model(P, 20, 20, _indices(P, 20, "uniform", g).to(DEV), _indices(P, 20, "uniform", g).to(DEV), False, seed=25)
    m._gaussian_indices = m._gaussian_indices[:P - 1].contiguous()
    with pytest.raises(RuntimeError, match="_gaussian_indices"):
        m.prune_points_indexed(torch.zeros(P, dtype=torch.bool, device=DEV))
    with pytest.raises(RuntimeError, match="mask"):
        m.prune_points_indexed(torch.zeros(P + 1, dtype=torch.bool, device=DEV))


class _HostReads(torch.utils._python_dispatch.TorchDispatchMode):
    """Records every ATen call that takes a GPU tensor and hands back host data (a CPU tensor or a Python scalar); see
    tests/test_densify_gpu.py."""

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


def test_one_host_read_per_rebuild():
    P, K0, K1 = 100_003, 9000, 20_000
    g = torch.Generator().manual_seed(17)
    idx0, idx1 = _indices(P, K0, "uniform", g).to(DEV), _indices(P, K1, "uniform", g).to(DEV)
    warm = _model(1000, 50, 50, _indices(1000, 50, "uniform", g).to(DEV), _indices(1000, 50, "uniform", g).to(DEV), True, seed=18)
    warm.compact_codebooks()
    m = _model(P, K0, K1, idx0, idx1, True, seed=19)
    _ = m._read_host(torch.zeros(4, dtype=torch.int32, device=DEV))               # the pinned buffer exists
    mask = (torch.rand(P, generator=g) < 0.6).to(DEV)
    torch.cuda.synchronize()
    for call in (lambda: m.prune_points_indexed(mask), lambda: m.compact_codebooks(), lambda: m.to_unindexed()):
        reads = _HostReads()
        with reads:
            call()
        print("host reads:", reads.reads)
        want = 0 if m._feature_indices is None else 1               # to_unindexed needs no size: no read at all
        assert len(reads.reads) == want and all("copy_" in r for r in reads.reads), reads.reads


# ------------------------------------------------------------------------------------------------ the driver
def _finetune_run(tmp_path, iterations, forced=0, **kw):
    """The toy scene's student made indexed with SHARED codebook rows (P / 4 colour rows, P / 3 geometry rows, uniform random
    indices), `forced` opacities at -20. The last row of each codebook is used by the first forced Gaussian alone; the rows of
    the other forced Gaussians are drawn like everybody's, so survivors share them."""
    from c3dgs_amd import pipeline
    from c3dgs_amd.model import PipelineParams
    from tests import train_scene
    student, cams, _ = train_scene.make(tmp_path, DEV)
    P0 = student._xyz.shape[0]
    K0, K1 = P0 // 4, P0 // 3
    g = torch.Generator().manual_seed(21)
    idx0 = torch.randint(0, K0 - 1, (P0,), generator=g, dtype=torch.int64)
    idx1 = torch.randint(0, K1 - 1, (P0,), generator=g, dtype=torch.int64)
    rows = torch.arange(P0)[::max(1, P0 // max(forced, 1))][:forced]
    if forced:
        idx0[rows[0]], idx1[rows[0]] = K0 - 1, K1 - 1
    with torch.no_grad():
        feats = torch.cat((student._features_dc, student._features_rest), dim=1).detach()
        student.set_color_indexed(feats[:K0].clone(), idx0.to(DEV))
        student.set_gaussian_indexed(student._rotation.detach()[:K1].clone(), student._scaling.detach()[:K1].clone(), idx1.to(DEV))
        student._opacity[rows.to(DEV)] = -20.0
    events, snaps = [], []

    class Scene:
        gaussians = student

        def getTrainCameras(self):
            return cams

    def log(iteration, ema):
        st = student
        n = st._xyz.shape[0]
        assert st._feature_indices.shape == (n,) and st._gaussian_indices.shape == (n,)
        events.append((iteration, ema, n, st._features_dc.shape[0], st._scaling.shape[0]))
        snaps.append((st._feature_indices.clone(), st._gaussian_indices.clone()))

    random.seed(3)
    torch.manual_seed(0)
    ema = pipeline.finetune(Scene(), pipeline._Dataset(), pipeline.OptimizationParams(),
                            pipeline.CompressionParams(finetune_iterations=iterations), PipelineParams(), log=log, **kw)
    return dict(student=student, events=events, snaps=snaps, ema=ema, P0=P0, idx=(idx0, idx1), K=(K0, K1), rows=rows)


def test_finetune_prunes_an_indexed_model(tmp_path):
    import math
    forced, k = 7, 5
    run = _finetune_run(tmp_path, 30, forced=forced, prune_interval=k)
    student, events, P0 = run["student"], run["events"], run["P0"]
    print("events (iteration, ema, N, colour rows, geometry rows):", events)
    its = [e[0] for e in events]
    assert its == [5, 10, 10, 15, 20, 20, 25, 30]                   # a log call after every prune, none after the last iteration
    assert P0 > 10 * forced
    # the first prune takes exactly the forced Gaussians; a codebook row goes only if no survivor references it
    keep = torch.ones(P0, dtype=torch.bool)
    keep[run["rows"]] = False
    want = [ir.remap_ref(keep, idx, K) for idx, K in zip(run["idx"], run["K"])]
    assert events[0][2:] == (P0 - forced, len(want[0][0]), len(want[1][0]))
    for (cb, new), idx, K, got in zip(want, run["idx"], run["K"], run["snaps"][0]):
        assert torch.equal(got.cpu(), new)                          # every survivor still names the row it named before
        assert K - 1 not in cb.tolist()                             # the row only a forced Gaussian used is gone
        assert set(idx[run["rows"][1:]].tolist()) & set(cb.tolist())  # rows a forced Gaussian shared with survivors are kept
        assert len(cb) < P0 - forced                                # rows are shared
    sizes = [e[2:] for e in events]
    assert all(all(b <= a for a, b in zip(x, y)) for x, y in zip(sizes, sizes[1:]))   # nothing ever grows
    assert all(math.isfinite(e[1]) for e in events) and math.isfinite(run["ema"])
    n = student._xyz.shape[0]
    assert len(student.optimizer.state) == len(student.optimizer.param_groups) == len(ATTR)
    for name, attr in ATTR.items():
        p = getattr(student, attr)
        st = student.optimizer.state[p]
        assert st["exp_avg"].shape == p.shape and st["exp_avg_sq"].shape == p.shape, name
        assert [gr for gr in student.optimizer.param_groups if gr["name"] == name][0]["params"][0] is p
        assert bool(torch.isfinite(p).all())
    assert student._opacity.shape[0] == n and int(student._feature_indices.max()) < student._features_dc.shape[0]
    assert int(student._gaussian_indices.max()) < student._scaling.shape[0]
    assert all(int(st["step"]) == 29 for st in student.optimizer.state.values())


def test_finetune_without_pruning_is_unchanged(tmp_path):
    a, b = _finetune_run(tmp_path, 20), _finetune_run(tmp_path, 20, prune_interval=0)
    plain, zero, ema_plain, ema_zero = a["events"], b["events"], a["ema"], b["ema"]
    print("logged:", plain)
    assert [e[0] for e in plain] == [10, 20]
    assert plain == zero and ema_plain == ema_zero
