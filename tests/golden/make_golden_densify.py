#!/usr/bin/env python3
"""Generates tests/golden/densify.npz by RUNNING the reference's own adaptive density control on the CPU.

    python tests/golden/make_golden_densify.py        (needs the reference checkout, C3DGS_REFERENCE or /root/reference;
                                                        never runs on the GPU box)

scene/gaussian_model.py is loaded by file path (importing the `scene` package would pull cv2) with empty stub modules for its
native extensions. Per case a CPU GaussianModel gets seeded parameters, three torch.optim.Adam steps (non-zero moments),
seeded xyz_gradient_accum / denom (with zeros) / max_radii2D and warmed observers; torch.normal is replaced by
z * std + mean with recorded seeded z; the reference's method runs under no_grad.

Every output row except a child's xyz / _scaling is a verbatim copy of a source row, which the generator ASSERTS (all seven
parameter tensors and their fourteen moment tensors against gather(before, src) / zero, `step` untouched), so the file
holds per case only: the decision-relevant inputs, the draws, the observer states before and after, the provenance
(src, kind) of every output row, the children's xyz / _scaling rows and reset_opacity's result.

Conditions asserted on the reference's own values (a seed that misses one is skipped, the kept seed is recorded):
every stage selects a non-empty, non-total set; no compared quantity lies within relative 1e-3 of
its threshold and no fake-quant input within 1e-4 of a lattice step from a rounding boundary (so one ulp of difference in
exp / sigmoid / a scale between CPU torch and the HIP getters cannot flip a row or move a value by a step); the
reference's fp32 children meet the arithmetic bound of tests/test_densify_gpu.py against a float64 evaluation.
"""
import argparse
import contextlib
import importlib.util
import io
import os
import sys
import types

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
REF = os.environ.get("C3DGS_REFERENCE", "/root/reference")
ROWS = 200
THRESHOLD_MARGIN = 1e-3
LATTICE_MARGIN = 1e-4
ULP_BOUND = 16 * 2.0 ** -24           # tests/test_densify_gpu.py test 2b
MIN_OPACITY = 0.005
PARAM_ATTRS = ("_xyz", "_features_dc", "_features_rest", "_scaling", "_scaling_factor", "_rotation", "_opacity")


def load_reference():
    def stub(name, **attrs):
        m = types.ModuleType(name)
        m.__dict__.update(attrs)
        sys.modules[name] = m
        return m
    sys.path.insert(0, REF)
    stub("plyfile", PlyData=None, PlyElement=None)
    stub("simple_knn")
    stub("simple_knn._C", distCUDA2=None)
    stub("torch_scatter", scatter=None)
    stub("weighted_distance")
    stub("weighted_distance._C", weightedDistance=None)
    stub("diff_gaussian_rasterization_no_camera", GaussianRasterizationSettings=None, GaussianRasterizer=None,
         GaussianRasterizerIndexed=None, getProjectionMatrix=None, quat_to_mat=None)
    try:
        import matplotlib  # noqa: F401
    except Exception:
        stub("matplotlib", pyplot=stub("matplotlib.pyplot"))
    spec = importlib.util.spec_from_file_location("ref_gaussian_model", os.path.join(REF, "scene/gaussian_model.py"))
    gm = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(gm)
    from arguments import OptimizationParams
    return gm.GaussianModel, OptimizationParams(argparse.ArgumentParser())


class Skip(Exception):
    pass


def need(cond, why):
    if not cond:
        raise Skip(why)


def make_model(GaussianModel, opt, P, quant, factor, seed):
    g = torch.Generator().manual_seed(seed)
    m = GaussianModel(3, quantization=quant, use_factor_scaling=factor, device="cpu")
    r = lambda *s: torch.randn(*s, generator=g)                                     # noqa: E731
    u = lambda *s: torch.rand(*s, generator=g)                                      # noqa: E731
    par = lambda t: torch.nn.Parameter(t.contiguous().requires_grad_(True))         # noqa: E731
    m._xyz = par(r(P, 3) * 2)
    m._features_dc = par(r(P, 1, 3) * 0.3)
    m._features_rest = par(r(P, 15, 3) * 0.05)
    if factor:
        m._scaling = par(u(P, 3) + 0.05)
        m._scaling_factor = par(torch.log(u(P, 1) * 0.2 + 1e-3))
    else:
        m._scaling = par(torch.log(u(P, 3) ** 3 * 0.15 + 1e-3))
    m._rotation = par(r(P, 4) * torch.exp(r(P, 1) * 1.5))       # raw quaternions, norms over two decades
    m._opacity = par(r(P, 1) * 3 - 2.0)
    m.max_radii2D = torch.zeros(P)
    m.spatial_lr_scale = 1.0
    m.training_setup(opt)
    for _ in range(3):
        for a in PARAM_ATTRS:
            p = getattr(m, a)
            if p is not None:
                p.grad = torch.randn(p.shape, generator=g) * 1e-3
        m.optimizer.step()
    m.denom = torch.randint(0, 4, (P, 1), generator=g).float()
    m.xyz_gradient_accum = u(P, 1) * 0.0012 * m.denom.clamp(min=1)
    m.xyz_gradient_accum[m.denom[:, 0] == 0] *= (u(P, 1)[m.denom[:, 0] == 0] > 0.5).float()   # 0/0 and x/0 both occur
    m.max_radii2D = u(P) * 40
    with torch.no_grad():                                       # observers as a few renders leave them
        for _ in range(2):
            _ = m.get_scaling
            _ = m.get_opacity
    return m


def qa_modules(m):
    mods = {"opacity": m.opacity_qa, "scaling": m.scaling_qa}
    if m._scaling_factor is not None:
        mods["scaling_factor"] = m.scaling_factor_qa
    return mods


def qa_snapshot(m):
    out = {}
    for k, mod in qa_modules(m).items():
        o = mod.activation_post_process
        out[k] = np.array([float(o.min_val), float(o.max_val), float(mod.scale)], np.float32)
        out[k + "_zp"] = np.array([int(mod.zero_point)], np.int32)
    return out


def run_case(GaussianModel, opt, name, seed, quant, factor, method, screen, extent):
    P, N = ROWS, 2
    m = make_model(GaussianModel, opt, P, quant, factor, seed)
    with torch.no_grad():
        m._features_dc[:, 0, 0] = torch.arange(P).float()       # the provenance tag
    attrs = [a for a in PARAM_ATTRS if getattr(m, a) is not None]
    before = {a: getattr(m, a).detach().clone() for a in attrs}
    mom = {a: (m.optimizer.state[getattr(m, a)]["exp_avg"].clone(), m.optimizer.state[getattr(m, a)]["exp_avg_sq"].clone())
           for a in attrs}
    steps = {a: float(m.optimizer.state[getattr(m, a)]["step"]) for a in attrs}
    accum, denom, max_radii = m.xyz_gradient_accum.clone(), m.denom.clone(), m.max_radii2D.clone()
    out = {"P": np.array([P]), "N": np.array([N]), "seed": np.array([seed]), "quantization": np.array([int(quant)]),
           "use_factor_scaling": np.array([int(factor)]), "extent": np.array([extent], np.float64),
           "max_grad": np.array([opt.densify_grad_threshold], np.float64), "min_opacity": np.array([MIN_OPACITY], np.float64),
           "percent_dense": np.array([opt.percent_dense], np.float64), "max_screen_size": np.array([screen or 0]),
           "accum": accum.numpy(), "denom": denom.numpy(), "max_radii2D": max_radii.numpy()}
    for a in ("_xyz", "_scaling", "_scaling_factor", "_rotation", "_opacity"):
        if a in before:
            out["in" + a] = before[a].numpy()
    for k, v in qa_snapshot(m).items():
        out["qa_before_" + k] = v

    draws, fq_inputs, log = [], [], []
    real_normal, real_fq = torch.normal, torch.fake_quantize_per_tensor_affine

    def normal(mean=None, std=None, **kw):
        z = torch.randn(std.shape, generator=torch.Generator().manual_seed(seed * 7919 + 13))
        draws.append(z)
        return z * std + mean

    def fq(x, scale, zero_point, qmin, qmax):
        fq_inputs.append((x.detach().clone(), float(scale)))
        return real_fq(x, scale, zero_point, qmin, qmax)

    cls = type(m)

    class Logged(cls):                                          # the activated values every decision is taken on
        @property
        def get_scaling(self):
            v = cls.get_scaling.fget(self)
            log.append(("scaling", v.detach().clone()))
            return v

        @property
        def get_opacity(self):
            v = cls.get_opacity.fget(self)
            log.append(("opacity", v.detach().clone()))
            return v
    m.__class__ = Logged

    grads = accum / denom
    grads[grads.isnan()] = 0.0
    thr, dense = opt.densify_grad_threshold, opt.percent_dense * extent
    torch.normal, torch.fake_quantize_per_tensor_affine = normal, fq
    try:
        with contextlib.redirect_stdout(io.StringIO()), torch.no_grad():
            if method == "densify_and_prune":
                m.densify_and_prune(thr, MIN_OPACITY, extent, screen)
            elif method == "densify_and_clone":
                m.densify_and_clone(grads, thr, extent)
            elif method == "densify_and_split":
                m.densify_and_split(grads, thr, extent, N)
            else:
                mask = torch.rand(P, generator=torch.Generator().manual_seed(seed)) < 0.3
                out["prune_mask"] = mask.numpy()
                m.prune_points(mask)
    finally:
        torch.normal = real_normal
    n_fq_main = len(fq_inputs)

    # ---- provenance, and the premise the kernels rest on
    src = m._features_dc[:, 0, 0].detach().long()
    Pn = len(src)
    z = draws[0] if draws else torch.zeros(0, 3)
    is_orig = m.optimizer.state[m._xyz]["exp_avg"].abs().sum(1) > 0
    is_child = (m._xyz.detach() != before["_xyz"][src]).any(1) | (m._scaling.detach() != before["_scaling"][src]).any(1)
    assert not (is_orig & is_child).any()
    K, CH = int(is_orig.sum()), int(is_child.sum())
    Cn = Pn - K - CH
    assert CH % N == 0
    CK = CH // N
    kind = torch.cat([torch.zeros(K), torch.ones(Cn)] + [torch.full((CK,), 2.0 + k) for k in range(N)]).long()
    assert bool(is_orig[:K].all()) and not bool(is_orig[K:].any()) and bool(is_child[K + Cn:].all()) and not bool(is_child[:K + Cn].any())
    for lo, hi in [(0, K), (K, K + Cn)] + [(K + Cn + k * CK, K + Cn + (k + 1) * CK) for k in range(N)]:
        assert bool((src[lo + 1:hi] > src[lo:hi - 1]).all()), "segments are in source order"
    for k in range(1, N):
        assert torch.equal(src[K + Cn:K + Cn + CK], src[K + Cn + k * CK:K + Cn + (k + 1) * CK])
    for a in attrs:
        p = getattr(m, a).detach()
        st = m.optimizer.state[getattr(m, a)]
        assert float(st["step"]) == steps[a], "step is untouched"
        assert torch.equal(st["exp_avg"][:K], mom[a][0][src[:K]]) and torch.equal(st["exp_avg_sq"][:K], mom[a][1][src[:K]])
        assert float(st["exp_avg"][K:].abs().sum()) == 0 and float(st["exp_avg_sq"][K:].abs().sum()) == 0
        rows = slice(0, K + Cn) if a in ("_xyz", "_scaling") else slice(0, Pn)
        assert torch.equal(p[rows], before[a][src[rows]]), a
    if method == "prune_points":
        assert torch.equal(m.xyz_gradient_accum, accum[src]) and torch.equal(m.denom, denom[src]) and \
            torch.equal(m.max_radii2D, max_radii[src])
    else:
        assert tuple(m.xyz_gradient_accum.shape) == (Pn, 1) and float(m.xyz_gradient_accum.abs().sum()) == 0
        assert tuple(m.denom.shape) == (Pn, 1) and float(m.denom.abs().sum()) == 0
        assert tuple(m.max_radii2D.shape) == (Pn,) and float(m.max_radii2D.abs().sum()) == 0

    # ---- conditions on the reference's own values
    scal = [v for k, v in log if k == "scaling"]
    g = grads.squeeze(1)
    margins = []

    def far(values, threshold):
        margins.append((values[torch.isfinite(values)] - threshold).abs().min().item() / abs(threshold))

    S = len(z) // N
    if method in ("densify_and_prune", "densify_and_clone"):
        clone = (g.abs() >= thr) & (scal[0].max(1).values <= dense)
        need(0 < int(clone.sum()) < P, "clone set empty or total")
        far(g.abs(), thr)
        far(scal[0].max(1).values, dense)
    if method in ("densify_and_prune", "densify_and_split"):
        s2 = scal[1] if method == "densify_and_prune" else scal[0]
        far(s2[:P].max(1).values, dense)
        need(0 < S < P, "split set empty or total")
    if method == "densify_and_prune":
        op = [v for k, v in log if k == "opacity"][0].squeeze(1)
        low = op < MIN_OPACITY
        need(0 < int(low.sum()) < len(op), "opacity prune empty or total")
        far(op, MIN_OPACITY)
        n_children = len(z)
        if screen:
            big = scal[2].max(1).values > 0.1 * extent
            far(scal[2].max(1).values, 0.1 * extent)
            need(0 < int((big & ~low).sum()) < len(op), "world-size prune empty or total")
            need(int((big | low)[-n_children:].sum()) > 0, "no child pruned")
        need(0 < CK < S, "children: none pruned or none kept")
    if margins:
        need(min(margins) >= THRESHOLD_MARGIN, f"a compared quantity within {THRESHOLD_MARGIN} of its threshold")
    if method == "densify_and_prune" or method == "densify_and_split":
        # the reference's own fp32 children against float64
        rows = slice(K + Cn, Pn)
        par = src[rows]
        selected = (g >= thr) & (s2[:P].max(1).values > dense)
        assert int(selected.sum()) == S
        draw_row = torch.cat([k * S + (torch.cumsum(selected.long(), 0) - 1)[par[:CK]] for k in range(N)])
        std64 = s2[par].double()
        zz = z[draw_row].double()
        R = _rot64(before["_rotation"][par].double())
        parent = (before["_xyz"][par].half().float() if quant else before["_xyz"][par]).double()
        want = torch.bmm(R, (zz * std64).unsqueeze(-1)).squeeze(-1) + parent
        bound = ULP_BOUND * (want.abs() + (zz * std64).abs().sum(1, keepdim=True))
        err = (m._xyz.detach()[rows].double() - want).abs()
        assert bool((err <= bound).all()), ("the reference's children miss the arithmetic bound", float((err / bound).max()))
        out["child_bound_used"] = np.array([float((err / bound).max())])
        out["draw_row"] = draw_row.numpy().astype(np.int32)

    for k, v in qa_snapshot(m).items():
        out["qa_after_" + k] = v
    out["src"], out["kind"] = src.numpy().astype(np.int32), kind.numpy().astype(np.uint8)
    out["z"] = z.numpy()
    out["child_xyz"] = m._xyz.detach()[K + Cn:].numpy().copy()
    out["child_scaling"] = m._scaling.detach()[K + Cn:].numpy().copy()

    if method == "densify_and_prune":
        torch.fake_quantize_per_tensor_affine = fq
        try:
            with torch.no_grad():
                m.reset_opacity()
        finally:
            torch.fake_quantize_per_tensor_affine = real_fq
        out["reset_opacity"] = m._opacity.detach().numpy().copy()
        assert float(m.optimizer.state[m._opacity]["exp_avg"].abs().sum()) == 0
        for k, v in qa_snapshot(m).items():
            if k.startswith("opacity"):
                out["qa_after_reset_" + k] = v
    lattice = 1.0
    for x, scale in fq_inputs:
        f = x / scale
        lattice = min(lattice, (f - torch.floor(f) - 0.5).abs().min().item())
    need(lattice >= LATTICE_MARGIN, f"a fake-quant input {lattice:.2e} of a step from a rounding boundary")
    out["margin"] = np.array([min(margins) if margins else 1.0, lattice, sum(x.numel() for x, _ in fq_inputs)])
    torch.fake_quantize_per_tensor_affine = real_fq
    assert n_fq_main <= len(fq_inputs)
    return {f"{name}/{k}": v for k, v in out.items()}, (Pn, K, Cn, S, CK)


def _rot64(r):
    q = r / r.norm(dim=1, keepdim=True)
    w, x, y, z = q[:, 0], q[:, 1], q[:, 2], q[:, 3]
    return torch.stack([1 - 2 * (y * y + z * z), 2 * (x * y - w * z), 2 * (x * z + w * y),
                        2 * (x * y + w * z), 1 - 2 * (x * x + z * z), 2 * (y * z - w * x),
                        2 * (x * z - w * y), 2 * (y * z + w * x), 1 - 2 * (x * x + y * y)], dim=1).reshape(-1, 3, 3)


# name, quantization, factor scaling, method, max_screen_size, extent
CASES = [
    ("factor_fp", False, True, "densify_and_prune", None, 1.2),
    ("factor_fp_screen", False, True, "densify_and_prune", 20, 1.2),
    ("factor_qat", True, True, "densify_and_prune", None, 1.2),
    ("factor_qat_screen", True, True, "densify_and_prune", 20, 1.2),
    ("plain_fp_screen", False, False, "densify_and_prune", 20, 1.2),
    ("clone", True, True, "densify_and_clone", None, 5.0),
    ("split", True, True, "densify_and_split", None, 5.0),
    ("prune", True, True, "prune_points", None, 5.0),
]


def main():
    GaussianModel, opt = load_reference()
    data, names = {}, []
    for name, quant, factor, method, screen, extent in CASES:
        for seed in range(1, 200):
            try:
                case, counts = run_case(GaussianModel, opt, name, seed, quant, factor, method, screen, extent)
            except Skip as why:
                print(f"{name}: seed {seed} skipped: {why}")
                continue
            print(f"{name}: seed {seed} kept, rows {ROWS} -> {counts[0]} (kept {counts[1]}, clones {counts[2]}, "
                  f"S {counts[3]}, parents with children {counts[4]})")
            data.update(case)
            names.append(name)
            break
        else:
            raise SystemExit(f"{name}: no seed meets the conditions")
    data["cases"] = np.array(names)
    path = os.path.join(HERE, "densify.npz")
    np.savez_compressed(path, **data)
    print(path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
