#!/usr/bin/env python3
"""Generates tests/golden/densify_initial.npz by RUNNING the reference's own GaussianModel.densify_initial on the CPU.

    python tests/golden/make_golden_densify_initial.py    (needs the reference checkout, C3DGS_REFERENCE or /root/reference,
                                                           and scikit-learn; never runs on the GPU box)

The model is built as make_golden_densify.py builds its models (same stubs, seeded parameters, three Adam steps so that the
moments are non-zero, seeded accumulators); its positions are then replaced by the case's cloud. Every densify_and_clone call
the reference makes is recorded (the selected rows and the new positions it passes), and the neighbour table of its ball
tree is recorded through a thin wrapper of NearestNeighbors.

Asserted on the reference's own values (a seed that misses a `need` is skipped, the kept seed is recorded):
  * what the case is for: rows are inserted (or none, for the empty case); the outliers are there; at least one level is
    removed by `slot.sum() > 1` where the case asks for it;
  * for every point the four smallest fp32 squared distances to other points are pairwise distinct, and non-zero, with a
    relative gap >= 1e-5, and the ball tree's neighbours ARE the three smallest fp32 (d2, index) pairs: its fp64 order is
    the fp32 order the kernels use;
  * no relative distance lies within 1e-4 of an integer (one ulp of difference cannot add or remove a row);
  * the recorded calls are the level loop's: call k selects exactly the points with rel >= dist + 1 of its (slot, dist);
  * every non-position parameter of a new row is a verbatim copy of its source row (found through a provenance tag in
    _features_dc), moments of the originals are untouched and those of new rows zero, `step` is untouched, the
    accumulators are zeros of the new length.

The file holds per case: the input positions, the step, src / slot / level and the positions of the new rows, the
accumulator shapes, and the flags the model was built with.
"""
import contextlib
import io
import os
import sys

import numpy as np
import sklearn
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))
from make_golden_densify import PARAM_ATTRS, Skip, load_reference, make_model, need   # noqa: E402
import densify_initial_ref as ref                                                       # noqa: E402

DISTINCT_GAP = 1e-5
INTEGER_MARGIN = 1e-4


def cloud(kind, P, seed):
    """[P,3] float32: a uniform cube (too even for a row at dist_thr_coeff >= 1), with far points for the outlier cases (the last rows, so the tag order is plain)."""
    g = torch.Generator().manual_seed(seed)
    x = torch.rand(P, 3, generator=g) * 4 - 2
    if kind == "outliers3":                   # three outliers at different distances and directions
        x[-3] = torch.tensor([7.5, 0.3, -0.4]) + torch.rand(3, generator=g) * 0.2
        x[-2] = torch.tensor([-0.2, -11.0, 0.5]) + torch.rand(3, generator=g) * 0.2
        x[-1] = torch.tensor([0.4, 0.6, 16.0]) + torch.rand(3, generator=g) * 0.2
    elif kind == "halo":                      # a dense core in a sparse halo: the halo's gaps are several steps wide
        core = P - P // 10
        x[:core] = torch.rand(core, 3, generator=g) - 0.5
    elif kind == "outlier1":                  # one far point: the levels only it reaches are the quirk's
        x[-1] = torch.tensor([9.0, 8.0, -7.0]) + torch.rand(3, generator=g) * 0.2
    return x.float().contiguous()


# name, quantization, factor scaling, cloud, points, dist_thr_coeff, expectations
CASES = [
    ("qat_factor_outliers", True, True, "outliers3", 220, 0.3, {"rows": True, "quirk": True}),
    ("fp32_plain", False, False, "halo", 200, 1.0, {"rows": True}),
    ("qat_factor_coarse", True, True, "outliers3", 256, 1.0, {"rows": True}),
    ("fp32_fine", False, True, "uniform", 200, 0.45, {"rows": True}),
    ("nothing", True, True, "uniform", 200, 2.5, {"rows": False}),
    ("quirk", False, False, "outlier1", 240, 0.3, {"rows": True, "quirk": True}),
]


def run_case(gm_module, GaussianModel, opt, name, seed, quant, factor, kind, P, coeff, expect):
    m = make_model(GaussianModel, opt, P, quant, factor, seed)
    with torch.no_grad():
        m._xyz.copy_(cloud(kind, P, seed))
        m._features_dc[:, 0, 0] = torch.arange(P).float()       # the provenance tag
    attrs = [a for a in PARAM_ATTRS if getattr(m, a) is not None]
    before = {a: getattr(m, a).detach().clone() for a in attrs}
    mom = {a: (m.optimizer.state[getattr(m, a)]["exp_avg"].clone(), m.optimizer.state[getattr(m, a)]["exp_avg_sq"].clone())
           for a in attrs}
    steps = {a: float(m.optimizer.state[getattr(m, a)]["step"]) for a in attrs}
    accum_id = (m.xyz_gradient_accum, m.denom, m.max_radii2D)
    x = before["_xyz"].numpy().copy()

    tables, calls = [], []
    real_nn = gm_module["NearestNeighbors"]

    class Recorded(real_nn):
        def kneighbors(self, *a, **k):
            d, i = super().kneighbors(*a, **k)
            tables.append(i.copy())
            return d, i
    cls = type(m)

    class Logged(cls):
        def densify_and_clone(self, grads=None, grad_threshold=None, scene_extent=None, selected_pts_mask=None, new_xyz=None):
            calls.append((selected_pts_mask.clone().numpy(), new_xyz.clone().numpy()))
            return cls.densify_and_clone(self, grads, grad_threshold, scene_extent, selected_pts_mask, new_xyz)
    m.__class__ = Logged
    gm_module["NearestNeighbors"] = Recorded
    try:
        with contextlib.redirect_stdout(io.StringIO()), torch.no_grad():
            m.densify_initial(coeff)
    finally:
        gm_module["NearestNeighbors"] = real_nn
    indices = tables[0]

    # ---- the neighbour table: the ball tree's fp64 order is the fp32 (d2, index) order
    step = ref.average_step(x, coeff)
    need(np.array_equal(indices[:, 0], np.arange(P)), "column 0 of the ball tree is not the point itself")
    d = ((x[None, :, 0] - x[:, None, 0]) ** 2 + (x[None, :, 1] - x[:, None, 1]) ** 2) + (x[None, :, 2] - x[:, None, 2]) ** 2
    assert d.dtype == np.float32
    d[np.arange(P), np.arange(P)] = np.inf
    d4 = np.sort(d, axis=1)[:, :4].astype(np.float64)
    need(d4[:, 0].min() > 0, "coincident points")
    need(((d4[:, 1:] - d4[:, :-1]) / d4[:, 1:]).min() >= DISTINCT_GAP, "two of the four smallest distances of a point too close")
    idx, d2 = ref.knn3_brute(x)
    need(np.array_equal(indices[:, 1:], idx), "ball tree neighbours differ from the fp32 (d2, index) order")
    rel = ref.relative_distance(d2, step)
    need(np.abs(rel - np.round(rel)).min() >= INTEGER_MARGIN, "a relative distance within 1e-4 of an integer")

    # ---- the recorded calls are the level loop's, which names the (slot, level) of every new row
    want = []
    for nb in range(3):
        for dist in range(1, int(rel[:, nb].max())):
            rows = np.nonzero(rel[:, nb] >= dist + 1)[0]
            if rows.size > 1:
                want.append((nb, dist, rows))
    assert len(want) == len(calls), (len(want), len(calls))
    src, slot, level, pos = [], [], [], []
    for (nb, dist, rows), (sel, new_xyz) in zip(want, calls):
        assert np.array_equal(rows, sel)
        src.append(rows), slot.append(np.full(rows.size, nb)), level.append(np.full(rows.size, dist)), pos.append(new_xyz)
    n_new = sum(r.size for r in src)
    if expect["rows"]:
        need(n_new > 0, "nothing inserted")
        src, slot, level, pos = (np.concatenate(v) for v in (src, slot, level, pos))
    else:
        need(n_new == 0, "rows inserted in the empty case")
        src, slot, level, pos = np.zeros(0, np.int64), np.zeros(0, np.int64), np.zeros(0, np.int64), np.zeros((0, 3), np.float32)
    removed = 0
    for nb in range(3):
        r = np.sort(rel[:, nb])
        removed += max(0, int(np.floor(r[-1])) - max(int(np.floor(r[-2])), 1))
    if expect.get("quirk"):
        need(removed > 0, "`slot.sum() > 1` removes no level")
    if kind == "outliers3":
        far = rel[-3:, 0]
        need(len({int(v) for v in far}) == 3 and far.min() >= 2, "the three outliers do not reach three different levels")

    # ---- the reference's output: original rows first, then the recorded rows, everything but xyz a copy of the source
    Pn = P + n_new
    tag = m._features_dc[:, 0, 0].detach().long().numpy()
    assert len(tag) == Pn and np.array_equal(tag[:P], np.arange(P)) and np.array_equal(tag[P:], src)
    assert np.array_equal(m._xyz.detach().numpy()[:P], x) and np.array_equal(m._xyz.detach().numpy()[P:], pos)
    t = torch.from_numpy(tag)
    for a in attrs:
        p = getattr(m, a).detach()
        st = m.optimizer.state[getattr(m, a)]
        assert float(st["step"]) == steps[a], "step is untouched"
        assert torch.equal(st["exp_avg"][:P], mom[a][0]) and torch.equal(st["exp_avg_sq"][:P], mom[a][1])
        assert float(st["exp_avg"][P:].abs().sum()) == 0 and float(st["exp_avg_sq"][P:].abs().sum()) == 0
        if a != "_xyz":
            assert torch.equal(p, before[a][t]), a
    if n_new:
        assert tuple(m.xyz_gradient_accum.shape) == (Pn, 1) and float(m.xyz_gradient_accum.abs().sum()) == 0
        assert tuple(m.denom.shape) == (Pn, 1) and float(m.denom.abs().sum()) == 0
        assert tuple(m.max_radii2D.shape) == (Pn,) and float(m.max_radii2D.abs().sum()) == 0
    else:                                                       # no call, nothing touched: the same objects
        assert all(a is b for a, b in zip(accum_id, (m.xyz_gradient_accum, m.denom, m.max_radii2D)))
    out = {"P": np.array([P]), "seed": np.array([seed]), "quantization": np.array([int(quant)]),
           "use_factor_scaling": np.array([int(factor)]), "dist_thr_coeff": np.array([coeff], np.float64),
           "xyz": x, "step": np.array([step], np.float64), "src": src.astype(np.int32), "slot": slot.astype(np.uint8),
           "level": level.astype(np.int32), "new_xyz": pos.astype(np.float32), "totals": np.array(
               [int((slot == k).sum()) for k in range(3)], np.int64), "levels_removed": np.array([removed]),
           "xyz_gradient_accum_shape": np.array(m.xyz_gradient_accum.shape), "denom_shape": np.array(m.denom.shape),
           "max_radii2D_shape": np.array(m.max_radii2D.shape)}
    return {f"{name}/{k}": v for k, v in out.items()}, (Pn, n_new, int(level.max(initial=0)), removed)


def main():
    GaussianModel, opt = load_reference()
    gm_module = GaussianModel.densify_initial.__globals__      # the namespace scene/gaussian_model.py was executed in
    data, names = {}, []
    for name, quant, factor, kind, P, coeff, expect in CASES:
        for seed in range(1, 200):
            try:
                case, counts = run_case(gm_module, GaussianModel, opt, name, seed, quant, factor, kind, P, coeff, expect)
            except Skip as why:
                print(f"{name}: seed {seed} skipped: {why}")
                continue
            print(f"{name}: seed {seed} kept, rows {P} -> {counts[0]} ({counts[1]} new, {counts[2]} levels, "
                  f"{counts[3]} removed by the quirk)")
            data.update(case)
            names.append(name)
            break
        else:
            raise SystemExit(f"{name}: no seed meets the conditions")
    data["cases"] = np.array(names)
    data["versions"] = np.array([f"numpy {np.__version__}", f"torch {torch.__version__}", f"scikit-learn {sklearn.__version__}"])
    path = os.path.join(HERE, "densify_initial.npz")
    np.savez_compressed(path, **data)
    print(path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
