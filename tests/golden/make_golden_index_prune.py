#!/usr/bin/env python3
"""Generates tests/golden/index_prune.npz by RUNNING the reference's own prune_points (scene/gaussian_model.py:1101-1158) and
to_unindexed (:889-899) on indexed CPU models.

    python tests/golden/make_golden_index_prune.py     (needs the reference checkout, see make_golden_densify.py; never runs
                                                         on the GPU box)

Three prune cases (both halves indexed, colour only, geometry only) at P = 200 Gaussians, 64 colour codebook rows and 48
geometry codebook rows, after three torch.optim.Adam steps (non-zero moments). The index arrays are drawn so that some codebook
rows are unreferenced BEFORE the prune and others become unreferenced BY it; the generator asserts both kinds occur and that the
mask is neither empty nor total.

Every output row is a verbatim copy of a source row, which the generator ASSERTS (every parameter tensor and both its moment
tensors against gather(before, map), `step` untouched, surviving codebook rows in ascending old id, the remapped index naming
the row its Gaussian named before), so the file holds per case only: the index arrays, the mask, src, both cb_src, both
remapped index arrays and the accumulators before and after. The `unindexed` case records the provenance of the reference's
four expanded tensors, asserted to be codebook[indices]."""
import contextlib
import io
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
from make_golden_densify import load_reference  # noqa: E402

P, K_COLOR, K_GEOMETRY = 200, 64, 48
PARAM_ATTRS = ("_xyz", "_features_dc", "_features_rest", "_scaling", "_scaling_factor", "_rotation", "_opacity")
COLOR, GEOMETRY = ("_features_dc", "_features_rest"), ("_scaling", "_rotation")


def draw_indices(K, g):
    """[P] ids over a random 80 % of the K rows, so about a fifth of the codebook is unreferenced from the start."""
    allowed = torch.randperm(K, generator=g)[:int(0.8 * K)]
    return allowed[torch.randint(0, len(allowed), (P,), generator=g)]


def make_model(GaussianModel, opt, color, geometry, seed):
    ColorMode = GaussianModel.to_indexed.__globals__["ColorMode"]
    g = torch.Generator().manual_seed(seed)
    m = GaussianModel(3, quantization=True, use_factor_scaling=True, device="cpu")
    r = lambda *s: torch.randn(*s, generator=g)                                     # noqa: E731
    par = lambda t: torch.nn.Parameter(t.contiguous().requires_grad_(True))         # noqa: E731
    C, G = (K_COLOR if color else P), (K_GEOMETRY if geometry else P)
    m._xyz = par(r(P, 3) * 2)
    m._opacity = par(r(P, 1) * 3 - 2.0)
    m._scaling_factor = par(torch.log(torch.rand(P, 1, generator=g) * 0.2 + 1e-3))
    m._features_dc = par(r(C, 1, 3) * 0.3)
    m._features_rest = par(r(C, 15, 3) * 0.05)
    m._scaling = par(torch.rand(G, 3, generator=g) + 0.05)
    m._rotation = par(r(G, 4))
    idx0 = draw_indices(K_COLOR, g) if color else None
    idx1 = draw_indices(K_GEOMETRY, g) if geometry else None
    if color:
        m._feature_indices = torch.nn.Parameter(idx0.clone(), requires_grad=False)
        m.color_index_mode = ColorMode.ALL_INDEXED
    if geometry:
        m._gaussian_indices = torch.nn.Parameter(idx1.clone(), requires_grad=False)
    m.max_radii2D = torch.zeros(P)
    m.spatial_lr_scale = 1.0
    m.training_setup(opt)
    for _ in range(3):
        for a in PARAM_ATTRS:
            p = getattr(m, a)
            p.grad = torch.randn(p.shape, generator=g) * 1e-3
        m.optimizer.step()
    m.denom = torch.randint(0, 4, (P, 1), generator=g).float()
    m.xyz_gradient_accum = torch.rand(P, 1, generator=g) * 0.0012
    m.max_radii2D = torch.rand(P, generator=g) * 40
    with torch.no_grad():                                       # provenance tags: Gaussian row, colour row, geometry row
        m._xyz[:, 0] = torch.arange(P).float()
        m._features_dc[:, 0, 0] = torch.arange(C).float()
        m._scaling[:, 0] = torch.arange(G).float()
    return m, idx0, idx1, g


def snapshot(m):
    before = {a: getattr(m, a).detach().clone() for a in PARAM_ATTRS}
    mom = {a: (m.optimizer.state[getattr(m, a)]["exp_avg"].clone(), m.optimizer.state[getattr(m, a)]["exp_avg_sq"].clone())
           for a in PARAM_ATTRS}
    steps = {a: float(m.optimizer.state[getattr(m, a)]["step"]) for a in PARAM_ATTRS}
    assert all(float(a.abs().sum()) > 0 and float(b.abs().sum()) > 0 for a, b in mom.values())
    return before, mom, steps


def prune_case(GaussianModel, opt, name, color, geometry, seed):
    m, idx0, idx1, g = make_model(GaussianModel, opt, color, geometry, seed)
    before, mom, steps = snapshot(m)
    accum, denom, max_radii = m.xyz_gradient_accum.clone(), m.denom.clone(), m.max_radii2D.clone()
    mask = torch.rand(P, generator=g) < 0.4
    assert 0 < int(mask.sum()) < P
    with contextlib.redirect_stdout(io.StringIO()), torch.no_grad():
        m.prune_points(mask)
    src = m._xyz[:, 0].detach().long()
    assert torch.equal(src, torch.nonzero(~mask).squeeze(1)), "survivors in source order"
    cb0 = m._features_dc[:, 0, 0].detach().long()
    cb1 = m._scaling[:, 0].detach().long()
    out = {"mask": mask.numpy(), "src": src.numpy().astype(np.int32), "accum_in": accum.numpy(), "denom_in": denom.numpy(),
           "max_radii2D_in": max_radii.numpy(), "accum": m.xyz_gradient_accum.numpy(), "denom": m.denom.numpy(),
           "max_radii2D": m.max_radii2D.numpy()}
    assert torch.equal(m.xyz_gradient_accum, accum[src]) and torch.equal(m.denom, denom[src]) and torch.equal(m.max_radii2D, max_radii[src])
    maps = {a: src for a in PARAM_ATTRS}
    for indexed, attrs, idx, cb, new_idx, K, tag in ((color, COLOR, idx0, cb0, m._feature_indices, K_COLOR, "0"),
                                                    (geometry, GEOMETRY, idx1, cb1, m._gaussian_indices, K_GEOMETRY, "1")):
        if not indexed:
            assert torch.equal(cb, src)
            continue
        new_idx = new_idx.detach()
        assert bool((cb[1:] > cb[:-1]).all()), "surviving codebook rows in ascending old id"
        assert torch.equal(cb[new_idx], idx[src]), "the remapped index names the row its Gaussian named before"
        assert torch.equal(cb, torch.unique(idx[src])), "exactly the referenced rows survive"
        referenced_before = torch.zeros(K, dtype=torch.bool)
        referenced_before[idx] = True
        unref_before = int((~referenced_before).sum())
        unref_by_prune = int(referenced_before.sum()) - len(cb)
        assert unref_before > 0 and unref_by_prune > 0, (name, unref_before, unref_by_prune)
        print(f"{name}: space {tag}: {K} rows, {unref_before} unreferenced before, {unref_by_prune} more by the prune -> {len(cb)}")
        for a in attrs:
            maps[a] = cb
        out["idx" + tag], out["cb_src" + tag], out["new_idx" + tag] = idx.numpy(), cb.numpy().astype(np.int32), new_idx.numpy()
    for a in PARAM_ATTRS:
        p = getattr(m, a)
        st = m.optimizer.state[p]
        assert torch.equal(p.detach(), before[a][maps[a]]), a
        assert torch.equal(st["exp_avg"], mom[a][0][maps[a]]) and torch.equal(st["exp_avg_sq"], mom[a][1][maps[a]]), a
        assert float(st["step"]) == steps[a] == 3.0, "step is untouched"
        assert [gr for gr in m.optimizer.param_groups if gr["params"][0] is p], a
    print(f"{name}: {P} -> {len(src)} Gaussians")
    return {f"{name}/{k}": v for k, v in out.items()}


def unindexed_case(GaussianModel, opt, seed):
    m, idx0, idx1, _ = make_model(GaussianModel, opt, True, True, seed)
    before, _, _ = snapshot(m)
    m.to_unindexed()
    assert m._feature_indices is None and m._gaussian_indices is None
    rows = {}
    for a, idx in (("_features_dc", idx0), ("_features_rest", idx0), ("_scaling", idx1), ("_rotation", idx1)):
        assert torch.equal(getattr(m, a).detach(), before[a][idx]), a          # codebook[indices]
        rows[a] = idx
    assert torch.equal(m._features_dc[:, 0, 0].detach().long(), idx0) and torch.equal(m._scaling[:, 0].detach().long(), idx1)
    out = {"idx0": idx0.numpy(), "idx1": idx1.numpy()}
    out.update({"rows" + a: r.numpy() for a, r in rows.items()})
    return {f"unindexed/{k}": v for k, v in out.items()}


def main():
    GaussianModel, opt = load_reference()
    data = {}
    for seed, (name, color, geometry) in enumerate((("both", True, True), ("color", True, False), ("geometry", False, True)), 1):
        data.update(prune_case(GaussianModel, opt, name, color, geometry, seed))
    data.update(unindexed_case(GaussianModel, opt, 7))
    data["cases"] = np.array(["both", "color", "geometry"])
    path = os.path.join(HERE, "index_prune.npz")
    np.savez_compressed(path, **data)
    print(path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
