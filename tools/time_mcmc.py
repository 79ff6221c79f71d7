#!/usr/bin/env python3
"""Times MCMC density control (csrc/mcmc.hip) in one process and writes profiles/r17_mcmc_time.json (also one JSON line):

  add_position_noise  at 1M / 3M / 6M rows, both scale parameterisations, against upstream's sequence restated in torch ops on
                      the same tensors (build_scaling_rotation, L @ L^T, bmm, gate, add_: two [P,3,3] tensors in memory) and
                      against the streaming floor: the bytes the kernel requests at the rate a 512 MiB device copy reaches here.
  relocate_gs         the whole call, moments attached, 10 % of the rows dead, at 1M / 3M / 6M (SH degree 3: 59 floats per row and
                      as many of each moment), against the torch restatement: torch.multinomial with replacement, bincount, the
                      formula in torch, index_put on every tensor and moment. The stage split comes from the library's stage
                      timers in separate rounds (weights + scan, search + counts, values, apply, and the dead-row selection).
  add_new_gs          3M -> 3.15M, the whole call (the rows are pruned away again between samples).

    python tools/time_mcmc.py [--samples 20] [--warmup 3] [--P 1000000,3000000,6000000] [--out profiles/r17_mcmc_time.json]

Medians of `samples` with min and max after `warmup` unrecorded rounds, between stream events. The expectations (kernel below
the torch sequence) are evaluated and written as booleans, whatever they come to."""
import argparse
import json
import math
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

NOISE_LR, XYZ_LR, MIN_OPACITY = 5e5, 1.6e-4, 0.005


def _event_ms(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b)


def _stats(ms):
    return {"ms": statistics.median(ms), "ms_min_max": [min(ms), max(ms)]}


def _timed(fn, samples, warmup):
    ms = [_event_ms(fn) for _ in range(warmup + samples)]
    return _stats(ms[warmup:])


def copy_rate_gb_s(samples):
    src = torch.empty(512 << 20, dtype=torch.uint8, device="cuda")
    dst = torch.empty_like(src)
    for _ in range(3):
        dst.copy_(src)
    ms = [_event_ms(lambda: dst.copy_(src)) for _ in range(samples)]
    return 2 * src.numel() / (statistics.median(ms) * 1e-3) / 1e9


def torch_noise(xyz, rotation, scaling, factor, opacity, xi, noise_lr, xyz_lr):
    """Upstream's sequence (gsplat inject_noise_to_position) in torch ops."""
    q = torch.nn.functional.normalize(rotation)
    r, x, y, z = q.unbind(1)
    R = torch.stack([1 - 2 * (y * y + z * z), 2 * (x * y - r * z), 2 * (x * z + r * y),
                     2 * (x * y + r * z), 1 - 2 * (x * x + z * z), 2 * (y * z - r * x),
                     2 * (x * z - r * y), 2 * (y * z + r * x), 1 - 2 * (x * x + y * y)], 1).reshape(-1, 3, 3)
    s = torch.exp(scaling) if factor is None else torch.nn.functional.normalize(torch.relu(scaling)) * torch.exp(factor)
    L = R * s[:, None, :]                                   # build_scaling_rotation: R @ diag(s)
    cov = L @ L.transpose(1, 2)
    o = torch.sigmoid(opacity).reshape(-1)
    g = 1 / (1 + torch.exp(-100 * ((1 - o) - 0.995)))
    noise = torch.bmm(cov, (xi * g[:, None] * noise_lr * xyz_lr)[:, :, None]).squeeze(-1)
    xyz.add_(noise)


def time_noise(P, samples, warmup, rate):
    from c3dgs_amd import mcmc
    g = torch.Generator(device="cuda").manual_seed(P)
    r = lambda *s: torch.randn(*s, device="cuda", generator=g)      # noqa: E731
    out = {}
    for name in ("factor", "exp"):
        xyz, rot, xi, op = r(P, 3), r(P, 4), r(P, 3), r(P, 1) * 3 - 3
        scaling, fac = (r(P, 3).abs() + 0.1, r(P, 1) * 0.5 - 3) if name == "factor" else (r(P, 3) * 0.5 - 3, None)
        kernel = _timed(lambda: mcmc.noise(xyz, rot, scaling, fac, op, xi, NOISE_LR, XYZ_LR), samples, warmup)
        restated = _timed(lambda: torch_noise(xyz, rot, scaling, fac, op, xi, NOISE_LR, XYZ_LR), samples, warmup)
        bytes_row = 12 + 16 + 12 + 4 + 12 + 12 + (4 if fac is not None else 0)
        out[name] = {"kernel": kernel, "torch_sequence": restated, "bytes_per_row": bytes_row,
                     "floor_ms": bytes_row * P / (rate * 1e9) * 1e3, "kernel_over_floor": kernel["ms"] / (bytes_row * P / (rate * 1e9) * 1e3),
                     "kernel_below_torch_sequence": kernel["ms"] < restated["ms"]}
        del xyz, rot, xi, op, scaling, fac
        torch.cuda.empty_cache()
    return out


def make_model(P, dead_fraction=0.1):
    from c3dgs_amd.model import GaussianModel
    from c3dgs_amd.pipeline import OptimizationParams
    g = torch.Generator(device="cuda").manual_seed(P + 1)
    r = lambda *s: torch.randn(*s, device="cuda", generator=g)      # noqa: E731
    m = GaussianModel(3, quantization=False, use_factor_scaling=True, device="cuda")
    opacity = r(P, 1) + 1.0
    dead = torch.rand(P, device="cuda", generator=g) < dead_fraction
    opacity[dead] = math.log(0.001 / 0.999)
    m.set_tensors(xyz=r(P, 3), features_dc=r(P, 1, 3), features_rest=r(P, 15, 3), scaling=r(P, 3).abs() + 0.1, rotation=r(P, 4),
                  opacity=opacity, scaling_factor=r(P, 1) * 0.5 - 3)
    m.spatial_lr_scale = 1.0
    m.training_setup(OptimizationParams())
    for p in m.parameters():
        p.grad = torch.randn_like(p)
    m.optimizer.step()                                       # moments attached
    m.optimizer.zero_grad(set_to_none=True)
    return m, dead


_TABLE = None


def _coefficients():
    """A[N-1, k] = (-1)^k / sqrt(k+1) sum_{i=k+1..N} C(i-1, k), float64 [51, 51]: the double sum of eq. 9 as one matrix."""
    global _TABLE
    if _TABLE is None:
        A = torch.zeros(51, 51, dtype=torch.float64)
        for N in range(1, 52):
            for k in range(N):
                A[N - 1, k] = (-1) ** k / math.sqrt(k + 1) * sum(math.comb(i - 1, k) for i in range(k + 1, N + 1))
        _TABLE = A.cuda()
    return _TABLE


def torch_relocate(m, dead):
    """The staged torch restatement of relocate_gs (gsplat's relocate with its compute_relocation in torch ops)."""
    with torch.no_grad():
        dead_idx = dead.nonzero(as_tuple=True)[0]
        alive_idx = (~dead).nonzero(as_tuple=True)[0]
        n = dead_idx.shape[0]
        if n == 0 or alive_idx.shape[0] == 0:
            return 0
        o = torch.sigmoid(m._opacity.detach()).reshape(-1)
        sampled = alive_idx[torch.multinomial(o[alive_idx], n, replacement=True)]
        counts = torch.bincount(sampled, minlength=o.shape[0])
        N = (counts[sampled] + 1).clamp(max=51)
        os_ = o[sampled].double()
        on = (1 - (1 - os_) ** (1.0 / N)).clamp(MIN_OPACITY, 1 - torch.finfo(torch.float32).eps)
        powers = on[:, None] ** torch.arange(1, 52, device="cuda", dtype=torch.float64)[None]
        c = os_ / (powers * _coefficients()[N - 1]).sum(1)
        new_op = torch.log(on / (1 - on)).float()[:, None]
        new_sf = (m._scaling_factor.detach()[sampled].double() + torch.log(c)[:, None]).float()
        for name, attr, _ in m._GROUPS:
            p = getattr(m, attr)
            st = m.optimizer.state[p]
            data = p.detach()
            data[dead_idx] = data[sampled]
            if attr == "_opacity":
                data[sampled] = new_op
                data[dead_idx] = new_op
            elif attr == "_scaling_factor":
                data[sampled] = new_sf
                data[dead_idx] = new_sf
            for key in ("exp_avg", "exp_avg_sq"):
                st[key][sampled] = 0
                st[key][dead_idx] = 0
        return n


def time_relocate(P, samples, warmup):
    from c3dgs_amd import _lib
    m, dead = make_model(P)
    n = int(dead.sum())
    draws = torch.rand(n, dtype=torch.float64, device="cuda")
    kernel = _timed(lambda: m.relocate_gs(dead, MIN_OPACITY, draws), samples, warmup)
    _lib.profile_enable(True)
    _lib.profile_read()
    rounds = 5
    for _ in range(rounds):
        m.relocate_gs(dead, MIN_OPACITY, draws)
    stages = {k: v[0] / rounds for k, v in _lib.profile_read().items() if k.startswith("mcmc_") or k == "sparse_adam_select"}
    _lib.profile_enable(False)
    restated = _timed(lambda: torch_relocate(m, dead), samples, warmup)
    del m
    torch.cuda.empty_cache()
    return {"dead_rows": n, "floats_per_row": 59, "relocate_gs": kernel, "torch_restatement": restated,
            "stage_ms": {"weights_and_scan": stages.get("mcmc_weights"), "dead_row_selection": stages.get("sparse_adam_select"),
                         "search_and_counts": stages.get("mcmc_search"), "values": stages.get("mcmc_values"),
                         "apply": stages.get("mcmc_apply")},
            "relocate_gs_below_torch_restatement": kernel["ms"] < restated["ms"]}


def time_grow(P, samples, warmup):
    m, _ = make_model(P, dead_fraction=0.0)
    cap = int(1.05 * P)
    draws = torch.rand(cap - P, dtype=torch.float64, device="cuda")
    grown = torch.zeros(cap, dtype=torch.bool, device="cuda")
    grown[P:] = True
    ms, clone_ms = [], []
    for k in range(warmup + samples):
        t = _event_ms(lambda: m.add_new_gs(cap, draws))
        assert m._xyz.shape[0] == cap
        m.prune_points(grown)
        rows = torch.randint(0, P, (cap - P,), device="cuda", dtype=torch.int32)
        t2 = _event_ms(lambda: m._append_clones(rows))
        m.prune_points(grown)
        if k >= warmup:
            ms.append(t)
            clone_ms.append(t2)
    del m
    torch.cuda.empty_cache()
    return {"rows_before": P, "rows_after": cap, "add_new_gs": _stats(ms), "append_clones_alone": _stats(clone_ms)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--samples", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--P", default="1000000,3000000,6000000")
    ap.add_argument("--grow-P", type=int, default=3_000_000)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r17_mcmc_time.json"))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("time_mcmc.py needs the GPU; a timing taken anywhere else says nothing")
    rate = copy_rate_gb_s(args.samples)
    out = {"device": torch.cuda.get_device_name(0), "samples": args.samples, "warmup": args.warmup, "copy_rate_gb_s": rate,
           "method": "stream events around each call, medians after warm-up, one process; floor = requested bytes at the copy rate; "
                     "the stage split is the mean of 5 separate rounds under the library's stage timers",
           "noise": {}, "relocate": {}}
    for P in (int(x) for x in args.P.split(",")):
        out["noise"][str(P)] = time_noise(P, args.samples, args.warmup, rate)
        out["relocate"][str(P)] = time_relocate(P, args.samples, args.warmup)
    out["grow"] = time_grow(args.grow_P, min(args.samples, 5), 1)
    out["expectation_noise_below_torch_sequence_everywhere"] = all(v["kernel_below_torch_sequence"] for s in out["noise"].values() for v in s.values())
    out["expectation_relocate_below_torch_restatement_everywhere"] = all(s["relocate_gs_below_torch_restatement"] for s in out["relocate"].values())
    print(json.dumps(out))
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as fh:
            json.dump(out, fh, indent=1)


if __name__ == "__main__":
    main()
