"""-m gpu: GaussianModel.densify_initial (csrc/ray_fill.hip on the neighbour table of knn3) and the explicit form of
densify_and_clone.

1  every case of tests/golden/densify_initial.npz, recorded from the reference itself: plan and new positions bit-equal,
   every other parameter of a new row its source row's, moments, `step`, optimizer groups, accumulators
2  a cloud of 3000 points with outliers against the numpy restatement fed with knn3's own table: thousands of rows, more
   than 64 levels (more than one digit of the level sort); with and without an optimizer; the plan entry's capacity contract
3  what must raise, and leave the model as it was
4  the explicit densify_and_clone against torch.cat of the selected rows
5  the reference drivers' preamble on the small training scene, then one training step
"""
import ctypes as C
import os

import numpy as np
import pytest
import torch

from tests import densify_initial_ref as ref

pytestmark = pytest.mark.gpu
DEV = "cuda"
GOLDEN = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "densify_initial.npz"))
CASES = [str(c) for c in GOLDEN["cases"]]
ATTRS = ("_xyz", "_features_dc", "_features_rest", "_opacity", "_scaling", "_rotation", "_scaling_factor")
NAMES = {"_xyz": "xyz", "_features_dc": "f_dc", "_features_rest": "f_rest", "_opacity": "opacity", "_scaling": "scaling",
         "_rotation": "rotation", "_scaling_factor": "scaling_factor"}


def _model(xyz, quant=True, factor=True, with_optimizer=True, seed=3):
    """Seeded parameters around the given positions, non-zero moments and `step` = 3, used accumulators."""
    from c3dgs_amd.model import GaussianModel
    from c3dgs_amd.pipeline import OptimizationParams
    g = torch.Generator().manual_seed(seed)
    P = len(xyz)
    r = lambda *s: torch.randn(*s, generator=g)                                           # noqa: E731
    m = GaussianModel(3, quantization=quant, use_factor_scaling=factor, device=DEV)
    m.set_tensors(xyz=torch.as_tensor(xyz).clone(), features_dc=r(P, 1, 3) * 0.3, features_rest=r(P, 15, 3) * 0.05,
                  scaling=torch.rand(P, 3, generator=g) + 0.05, rotation=r(P, 4), opacity=r(P, 1),
                  scaling_factor=torch.log(torch.rand(P, 1, generator=g) * 0.2 + 1e-3) if factor else None)
    m.spatial_lr_scale = 1.0
    if with_optimizer:
        m.training_setup(OptimizationParams())
        for a in ATTRS:
            p = getattr(m, a)
            if p is not None:
                m.optimizer.state[p] = {"step": torch.tensor(3.0), "exp_avg": r(*p.shape).to(DEV) * 1e-3,
                                        "exp_avg_sq": (r(*p.shape).to(DEV) * 1e-3) ** 2}
    m.xyz_gradient_accum = torch.rand(P, 1, generator=g).to(DEV)
    m.denom = torch.ones(P, 1, device=DEV)
    m.max_radii2D = torch.rand(P, generator=g).to(DEV) * 40
    return m


def _snapshot(m):
    s = {"params": {a: (getattr(m, a), getattr(m, a).detach().clone()) for a in ATTRS if getattr(m, a) is not None},
         "stats": [(t, t.clone()) for t in (m.xyz_gradient_accum, m.denom, m.max_radii2D)], "moments": {}}
    if m.optimizer is not None:
        for a, (p, _) in s["params"].items():
            st = m.optimizer.state[p]
            s["moments"][a] = (st["exp_avg"], st["exp_avg"].clone(), st["exp_avg_sq"], st["exp_avg_sq"].clone())
    return s


def _assert_untouched(m, s):
    """The same tensor objects with the same contents: nothing was rebuilt, no accumulator reset."""
    for a, (obj, val) in s["params"].items():
        assert getattr(m, a) is obj and torch.equal(obj.detach(), val), a
    for (obj, val), now in zip(s["stats"], (m.xyz_gradient_accum, m.denom, m.max_radii2D)):
        assert now is obj and torch.equal(obj, val)
    for a, (ea, ea_v, es, es_v) in s["moments"].items():
        st = m.optimizer.state[getattr(m, a)]
        assert st["exp_avg"] is ea and st["exp_avg_sq"] is es and torch.equal(ea, ea_v) and torch.equal(es, es_v)
        assert float(st["step"]) == 3.0


def _assert_appended(m, s, src, P):
    """Originals first and unchanged, new rows copies of their sources (xyz apart), moments copied / zero, `step` kept,
    groups re-pointed, accumulators zero at the new length."""
    n = P + len(src)
    src = torch.as_tensor(src).long().to(DEV)
    for a, (_, old) in s["params"].items():
        p = getattr(m, a)
        assert p.is_leaf and p.requires_grad and p.shape[0] == n and p.shape[1:] == old.shape[1:], a
        assert torch.equal(p.detach()[:P], old), a
        if a != "_xyz":
            assert torch.equal(p.detach()[P:], old[src]), a
        if m.optimizer is not None:
            group = [g for g in m.optimizer.param_groups if g["name"] == NAMES[a]][0]
            assert group["params"][0] is p and len(m.optimizer.state) == len(m.optimizer.param_groups)
            st = m.optimizer.state[p]
            assert float(st["step"]) == 3.0, a
            for got, had in ((st["exp_avg"], s["moments"][a][1]), (st["exp_avg_sq"], s["moments"][a][3])):
                assert got.shape == p.shape and torch.equal(got[:P], had) and float(got[P:].abs().sum()) == 0.0, a
    assert tuple(m.xyz_gradient_accum.shape) == (n, 1) and tuple(m.denom.shape) == (n, 1) and tuple(m.max_radii2D.shape) == (n,)
    assert float(m.xyz_gradient_accum.abs().sum() + m.denom.abs().sum() + m.max_radii2D.abs().sum()) == 0.0


def _bits(t):
    return np.ascontiguousarray(t.detach().cpu().numpy() if isinstance(t, torch.Tensor) else t).view(np.uint32)


# ------------------------------------------------------------------------------------------------ 1 the reference's output
@pytest.mark.parametrize("with_optimizer", [True, False])
@pytest.mark.parametrize("name", CASES)
def test_against_the_reference_fixture(name, with_optimizer):
    g = {k.split("/", 1)[1]: GOLDEN[k] for k in GOLDEN.files if k.startswith(name + "/")}
    P = int(g["P"][0])
    m = _model(g["xyz"], bool(g["quantization"][0]), bool(g["use_factor_scaling"][0]), with_optimizer)
    s = _snapshot(m)
    src, slot, level, totals = m.densify_initial(float(g["dist_thr_coeff"][0]))
    assert src.dtype == torch.int32 and slot.dtype == torch.uint8 and level.dtype == torch.int32
    np.testing.assert_array_equal(src.cpu().numpy(), g["src"])
    np.testing.assert_array_equal(slot.cpu().numpy(), g["slot"])
    np.testing.assert_array_equal(level.cpu().numpy(), g["level"])
    assert list(totals) == list(g["totals"])
    if len(g["src"]) == 0:
        _assert_untouched(m, s)
        return
    assert np.array_equal(_bits(m._xyz[P:]), _bits(g["new_xyz"]))
    _assert_appended(m, s, g["src"], P)
    assert tuple(m.xyz_gradient_accum.shape) == tuple(g["xyz_gradient_accum_shape"])
    assert tuple(m.max_radii2D.shape) == tuple(g["max_radii2D_shape"])


# ------------------------------------------------------------------------------------------------ 2 many rows, many levels
COEFF = 0.05


def _outlier_cloud():
    rng = np.random.default_rng(11)
    x = rng.uniform(-1, 1, (3000, 3)).astype(np.float32)
    x[:2400] *= np.float32(0.3)                                  # a dense core in a sparse halo
    far = rng.uniform(-1, 1, (12, 3))                            # twelve lone points 6 to 14 away: they share the high levels,
    far = far / np.linalg.norm(far, axis=1, keepdims=True) * rng.uniform(6, 14, (12, 1))   # the farthest has the quirk's alone
    x[2988:] = far.astype(np.float32)
    return x


_big = {}


def _big_reference():
    """The restatement on knn3's own table, once for the tests that share it."""
    if not _big:
        from c3dgs_amd.knn import knn3
        x = _outlier_cloud()
        idx, d2 = knn3(torch.from_numpy(x).to(DEV))
        idx, d2 = idx.cpu().numpy(), d2.cpu().numpy()
        step = ref.average_step(x, COEFF)
        src, slot, level, totals = ref.plan(d2, step)
        _big.update(x=x, idx=idx, d2=d2, step=step, src=src, slot=slot, level=level, totals=totals,
                    pos=ref.positions(x, idx, d2, step, src, slot, level))
    return _big


@pytest.mark.parametrize("with_optimizer", [True, False])
def test_outlier_cloud_against_the_restatement(with_optimizer):
    w = _big_reference()
    assert len(w["src"]) > 3000 and int(w["level"].max()) > 64 and all(t > 0 for t in w["totals"])
    m = _model(w["x"], quant=False, factor=True, with_optimizer=with_optimizer)
    s = _snapshot(m)
    src, slot, level, totals = m.densify_initial(COEFF)
    np.testing.assert_array_equal(src.cpu().numpy(), w["src"])
    np.testing.assert_array_equal(slot.cpu().numpy(), w["slot"])
    np.testing.assert_array_equal(level.cpu().numpy(), w["level"])
    assert tuple(totals) == tuple(w["totals"])
    assert np.array_equal(_bits(m._xyz[3000:]), _bits(w["pos"]))
    _assert_appended(m, s, w["src"], 3000)


def test_plan_entry_totals_capacity_and_small_workspace():
    """c3dgs_ray_fill_plan directly: the totals-only call writes nothing else; the emitting call writes rows below `capacity`
    and nothing beyond; a workspace sized for fewer rows is refused before anything is written."""
    from c3dgs_amd import _lib
    L = _lib.lib()
    w = _big_reference()
    P, n = len(w["x"]), len(w["src"])
    d2 = torch.from_numpy(w["d2"]).to(DEV)
    stream = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    totals = torch.full((4,), -7, dtype=torch.int32, device=DEV)
    ws0 = torch.empty(L.c3dgs_ray_fill_plan_workspace_bytes(P, 0), dtype=torch.uint8, device=DEV)
    _lib.check(L.c3dgs_ray_fill_plan(P, d2.data_ptr(), w["step"], 0, None, None, None, totals.data_ptr(), ws0.data_ptr(), ws0.numel(),
                                     stream))
    assert totals.tolist() == list(w["totals"]) + [0]
    cap = n - 1000
    src = torch.full((n + 8,), -5, dtype=torch.int32, device=DEV)
    slot = torch.full((n + 8,), 99, dtype=torch.uint8, device=DEV)
    level = torch.full((n + 8,), -5, dtype=torch.int32, device=DEV)
    args = (src.data_ptr(), slot.data_ptr(), level.data_ptr(), totals.data_ptr())
    assert L.c3dgs_ray_fill_plan(P, d2.data_ptr(), w["step"], cap, *args, ws0.data_ptr(), ws0.numel(), stream) == 1
    assert b"workspace too small" in L.c3dgs_last_error() and str(n).encode() in L.c3dgs_last_error()
    assert bool((src == -5).all()) and bool((slot == 99).all())
    ws = torch.empty(L.c3dgs_ray_fill_plan_workspace_bytes(P, n), dtype=torch.uint8, device=DEV)
    _lib.check(L.c3dgs_ray_fill_plan(P, d2.data_ptr(), w["step"], cap, *args, ws.data_ptr(), ws.numel(), stream))
    np.testing.assert_array_equal(src[:cap].cpu().numpy(), w["src"][:cap])
    np.testing.assert_array_equal(slot[:cap].cpu().numpy(), w["slot"][:cap])
    np.testing.assert_array_equal(level[:cap].cpu().numpy(), w["level"][:cap])
    assert bool((src[cap:] == -5).all()) and bool((slot[cap:] == 99).all()) and bool((level[cap:] == -5).all())
    # a step so small that the rows overflow int32: flagged, totals clamped, nothing written
    _lib.check(L.c3dgs_ray_fill_plan(P, d2.data_ptr(), 1e-9, n, *args, ws.data_ptr(), ws.numel(), stream))
    t = totals.tolist()
    assert t[3] == 1 and all(0 < v <= 2**31 - 1 for v in t[:3]) and bool((src[cap:] == -5).all())
    # P = 0 clears the totals and touches nothing else
    _lib.check(L.c3dgs_ray_fill_plan(0, None, 1.0, 0, None, None, None, totals.data_ptr(), None, 0, stream))
    assert totals.tolist() == [0, 0, 0, 0]


def test_positions_entry_rejects_a_bad_plan_without_reading():
    """c3dgs_ray_fill_xyz: rows whose source, slot or neighbour is out of range get zeros."""
    from c3dgs_amd import _lib
    L = _lib.lib()
    x = torch.rand(6, 3, device=DEV) + 1
    idx = torch.tensor([[1, 2, 3], [0, 2, 3], [0, 1, -1], [0, 1, 2], [0, 1, 2], [0, 1, 7]], dtype=torch.int32, device=DEV)
    d2 = torch.full((6, 3), 16.0, device=DEV)
    src = torch.tensor([0, -1, 6, 2, 5, 3], dtype=torch.int32, device=DEV)
    slot = torch.tensor([0, 0, 0, 2, 2, 3], dtype=torch.uint8, device=DEV)
    level = torch.tensor([1, 1, 1, 1, 1, 1], dtype=torch.int32, device=DEV)
    out = torch.full((7, 3), 7.0, device=DEV)
    _lib.check(L.c3dgs_ray_fill_xyz(6, x.data_ptr(), idx.data_ptr(), d2.data_ptr(), 1.0, 6, src.data_ptr(), slot.data_ptr(),
                                    level.data_ptr(), out.data_ptr(), C.c_void_p(torch.cuda.current_stream().cuda_stream)))
    a = np.float32(1.0) / np.float32(4.0)
    want = x[0].cpu().numpy() * (np.float32(1.0) - a) + a * x[1].cpu().numpy()
    assert np.array_equal(_bits(out[0]), _bits(want.astype(np.float32)))
    assert float(out[1:6].abs().sum()) == 0.0 and bool((out[6] == 7.0).all())


# ------------------------------------------------------------------------------------------------ 3 what must raise
def test_errors_leave_the_model_unchanged():
    w = _big_reference()
    m = _model(w["x"], quant=False, factor=True)
    s = _snapshot(m)
    n_new = 3000 + len(w["src"])
    with pytest.raises(ValueError, match=str(n_new)):
        m.densify_initial(COEFF, max_points=n_new - 1)
    _assert_untouched(m, s)
    with pytest.raises(ValueError, match="new rows"):                    # int32 overflow: billions of rows, none allocated
        m.densify_initial(1e-9)
    _assert_untouched(m, s)
    with pytest.raises(ValueError, match="step"):
        m.densify_initial(float("nan"))
    _assert_untouched(m, s)

    three = _model(w["x"][:3])
    s3 = _snapshot(three)
    with pytest.raises(ValueError, match="at least 4 points"):
        three.densify_initial()
    _assert_untouched(three, s3)

    flat = w["x"][:500].copy()
    flat[:, 1] = 0.25                                                    # a planar cloud: zero volume, zero step
    planar = _model(flat)
    sp = _snapshot(planar)
    with pytest.raises(ValueError, match="step"):
        planar.densify_initial()
    _assert_untouched(planar, sp)

    indexed = _model(w["x"][:64], with_optimizer=False)
    indexed.to_indexed()
    xyz = indexed._xyz
    with pytest.raises(NotImplementedError, match="densify_initial"):
        indexed.densify_initial()
    with pytest.raises(NotImplementedError, match="densify_and_clone"):
        indexed.densify_and_clone(selected_pts_mask=torch.zeros(64, dtype=torch.bool, device=DEV))
    assert indexed._xyz is xyz and indexed._xyz.shape[0] == 64


def test_max_points_at_the_exact_count_passes():
    w = _big_reference()
    m = _model(w["x"], quant=False, factor=True, with_optimizer=False)
    m.densify_initial(COEFF, max_points=3000 + len(w["src"]))
    assert m._xyz.shape[0] == 3000 + len(w["src"])


# ------------------------------------------------------------------------------------------------ 4 explicit clone
@pytest.mark.parametrize("form", ["mask", "index", "mask_no_xyz", "empty"])
@pytest.mark.parametrize("with_optimizer", [True, False])
def test_explicit_densify_and_clone_equals_torch_cat(form, with_optimizer):
    P = 301
    g = torch.Generator().manual_seed(9)
    m = _model(torch.randn(P, 3, generator=g), with_optimizer=with_optimizer)
    s = _snapshot(m)
    if form in ("mask", "mask_no_xyz"):
        sel = (torch.rand(P, generator=g) < 0.3).to(DEV)
        rows = torch.nonzero(sel).squeeze(1)
    elif form == "index":
        rows = torch.tensor([5, 300, 5, 0, 17, 299, 5], device=DEV)      # repeats, and not in ascending order
        sel = rows
    else:
        sel = torch.zeros(P, dtype=torch.bool, device=DEV)
        rows = torch.zeros(0, dtype=torch.long, device=DEV)
    new_xyz = None if form == "mask_no_xyz" else torch.randn(len(rows), 3, generator=g).to(DEV)
    src, kind, draw_row = m.densify_and_clone(selected_pts_mask=sel, new_xyz=new_xyz)
    assert torch.equal(src.long(), torch.cat((torch.arange(P, device=DEV), rows)))
    assert torch.equal(kind.long(), torch.cat((torch.zeros(P, device=DEV), torch.ones(len(rows), device=DEV))).long())
    want_xyz = torch.cat((s["params"]["_xyz"][1], s["params"]["_xyz"][1][rows] if new_xyz is None else new_xyz))
    assert torch.equal(m._xyz.detach(), want_xyz)
    _assert_appended(m, s, rows, P)


def test_gradient_form_of_densify_and_clone_keeps_its_positional_signature():
    P = 200
    g = torch.Generator().manual_seed(10)
    m = _model(torch.randn(P, 3, generator=g))
    grads = torch.rand(P, 1, generator=g).to(DEV)
    want = (grads.norm(dim=-1) >= 0.5) & (m.get_scaling.detach().amax(dim=1) <= m.percent_dense * 1000.0)
    src, kind, draw_row, totals = m.densify_and_clone(grads, 0.5, 1000.0)
    assert totals[0] == P and totals[1] == int(want.sum()) > 0
    assert torch.equal(src[P:].long(), torch.nonzero(want).squeeze(1))
    with pytest.raises(ValueError, match="selected_pts_mask"):
        m.densify_and_clone(grads, 0.5, 1000.0, new_xyz=torch.zeros(1, 3))


# ------------------------------------------------------------------------------------------------ 5 the drivers' preamble
def test_preamble_of_the_reference_drivers_then_one_training_step(tmp_path):
    """train_camera.py:26 / train_no_splatting.py:25: densify_initial(); to_indexed(); _sort_morton(); training_setup();
    then one render, loss, backward and optimizer step."""
    from c3dgs_amd import loss as _loss
    from c3dgs_amd.model import PipelineParams
    from tests import train_scene
    student, cams, _ = train_scene.make(tmp_path, DEV, P_teacher=1600, keep_every=8, views=1)
    P = student._xyz.shape[0]
    src, slot, level, totals = student.densify_initial(0.5)
    assert student._xyz.shape[0] == P + sum(totals) > P
    student.to_indexed()
    student._sort_morton()
    student.training_setup(train_scene.schedule(10))
    student.update_learning_rate(1)
    image = student.render(cams[0], PipelineParams(), torch.zeros(3, device=DEV))["render"]
    loss = _loss.l1_ssim_loss(image, cams[0].original_image, 0.2)
    loss.backward()
    before = student._xyz.detach().clone()
    student.optimizer.step()
    assert bool(torch.isfinite(loss)) and float(loss.detach()) > 0
    assert bool(torch.isfinite(student._xyz).all()) and not torch.equal(student._xyz.detach(), before)
