#!/usr/bin/env python3
"""Times GaussianModel.densify_and_prune (one classification pass, one scan, one gather: csrc/densify.hip) against the staged
torch sequence the reference runs (tests/densify_ref.py: clone cat, split cat, the split's prune, the final prune) on the
same device and the same inputs -> profiles/r06_densify_time.json.

    python tools/time_densify.py [--sizes 1000000,3000000,6000000] [--calls 20] [--out profiles/r06_densify_time.json]

synth-v1 parameters at SH degree 3 with Adam moments attached (720 bytes per Gaussian); thresholds picked from the scene's
own quantiles so that roughly 10 % of the rows clone, 10 % split and 10 % are pruned. Every call runs on a fresh clone of the
state; after a warm-up the two alternate in one process and each timing is whole-call wall time between stream
synchronisations (the host read of the row counts is part of the cost). Reported per size: both medians, their ratio, rows
in / out, and the achieved bytes per second of the fused call against the floor of reading and writing each surviving row
once (2 x 720 B x rows out); the apply kernel's own device time and the device-busy time of the whole fused call come from
one extra call under torch.profiler."""
import argparse
import json
import os
import statistics
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from tests import densify_ref, synth  # noqa: E402

DEV = "cuda"
ROW_BYTES = 720            # 60 parameter floats at SH degree 3, times three with the two Adam moments
NAMES = {"xyz": "_xyz", "f_dc": "_features_dc", "f_rest": "_features_rest", "opacity": "_opacity", "scaling": "_scaling",
         "rotation": "_rotation", "scaling_factor": "_scaling_factor"}


def base_state(P, seed=1234):
    sc = synth.scene(P, seed=seed)
    norm = sc["scales"].norm(dim=1, keepdim=True)
    op = sc["opacities"].clamp(1e-6, 1 - 1e-6)
    g = torch.Generator().manual_seed(seed + 1)
    params = {"xyz": sc["means3D"], "f_dc": sc["shs"][:, :1].contiguous(), "f_rest": sc["shs"][:, 1:].contiguous(),
              "opacity": torch.log(op / (1 - op)), "scaling": sc["scales"] / norm, "rotation": sc["rotations"],
              "scaling_factor": torch.log(norm)}
    params = {k: v.float().to(DEV).contiguous() for k, v in params.items()}
    gd = torch.Generator(device=DEV).manual_seed(seed + 2)
    moments = {k: (torch.randn(v.shape, device=DEV, generator=gd) * 1e-3, torch.rand(v.shape, device=DEV, generator=gd) * 1e-6)
               for k, v in params.items()}
    denom = torch.randint(0, 4, (P, 1), generator=g).float().to(DEV)
    accum = (torch.rand(P, 1, generator=g) * 0.001).to(DEV) * denom          # never seen (denom 0) -> 0/0 -> gradient 0
    return params, moments, accum, denom


def thresholds(params, accum, denom, percent_dense):
    """max_grad at the 80 % quantile of the gradients, dense_extent at the median scale of the rows above it, min_opacity at
    the 10 % quantile of the opacities."""
    sub = slice(0, 1_000_000)
    g = (accum / denom).nan_to_num(0.0)[sub, 0]
    max_grad = float(torch.quantile(g, 0.8))
    scale = (torch.exp(params["scaling_factor"]) * params["scaling"]).amax(1)[sub]
    dense = float(torch.quantile(scale[g >= max_grad], 0.5))
    min_opacity = float(torch.quantile(torch.sigmoid(params["opacity"][sub, 0]), 0.1))
    return max_grad, min_opacity, dense / percent_dense


def fused_model(params, moments, accum, denom):
    from c3dgs_amd.model import GaussianModel
    from c3dgs_amd.pipeline import OptimizationParams
    m = GaussianModel(3, quantization=True, device=DEV)
    c = {k: v.clone() for k, v in params.items()}
    m.set_tensors(xyz=c["xyz"], features_dc=c["f_dc"], features_rest=c["f_rest"], scaling=c["scaling"], rotation=c["rotation"],
                  opacity=c["opacity"], scaling_factor=c["scaling_factor"])
    m.spatial_lr_scale = 1.0
    m.training_setup(OptimizationParams())
    for k, attr in NAMES.items():
        m.optimizer.state[getattr(m, attr)] = {"step": torch.tensor(1.0), "exp_avg": moments[k][0].clone(),
                                               "exp_avg_sq": moments[k][1].clone()}
    m.xyz_gradient_accum, m.denom = accum.clone(), denom.clone()
    m.max_radii2D = torch.zeros(accum.shape[0], device=DEV)
    return m


def staged_scene(params, moments, accum, denom, percent_dense):
    return densify_ref.Staged({k: v.clone() for k, v in params.items()}, {k: (a.clone(), b.clone()) for k, (a, b) in moments.items()},
                              accum.clone(), denom.clone(), quantization=True, percent_dense=percent_dense)


def timed(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    out = fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3, out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", default="1000000,3000000,6000000")
    ap.add_argument("--calls", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r06_densify_time.json"))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("time_densify.py measures on the GPU; there is no CPU path")
    percent_dense, screen = 0.01, 20
    results = []
    for P in [int(s) for s in args.sizes.split(",")]:
        params, moments, accum, denom = base_state(P)
        max_grad, min_opacity, extent = thresholds(params, accum, denom, percent_dense)
        fused_ms, staged_ms, rows = [], [], None
        for it in range(args.warmup + args.calls):
            m = fused_model(params, moments, accum, denom)
            with torch.no_grad():
                tf, plan = timed(lambda: m.densify_and_prune(max_grad, min_opacity, extent, screen))
            totals, rows_fused = plan[3], m._xyz.shape[0]
            del m, plan
            s = staged_scene(params, moments, accum, denom, percent_dense)
            with torch.no_grad():
                ts, _ = timed(lambda: s.densify_and_prune(max_grad, min_opacity, extent, screen))
            rows_staged = s.p["xyz"].shape[0]
            del s
            if rows_fused != rows_staged:
                raise SystemExit(f"P={P}: fused gives {rows_fused} rows, staged {rows_staged}")
            rows = rows_fused
            if it >= args.warmup:
                fused_ms.append(tf)
                staged_ms.append(ts)
        fm, sm = statistics.median(fused_ms), statistics.median(staged_ms)
        # device time of the fused call's kernels, from one more call under the profiler (not part of the medians)
        from torch.profiler import ProfilerActivity, profile
        m = fused_model(params, moments, accum, denom)
        torch.cuda.synchronize()
        with profile(activities=[ProfilerActivity.CPU, ProfilerActivity.CUDA]) as prof, torch.no_grad():
            m.densify_and_prune(max_grad, min_opacity, extent, screen)
            torch.cuda.synchronize()
        dev = [e for e in prof.events() if e.device_type == torch.autograd.DeviceType.CUDA]
        apply_ms = sum(e.time_range.elapsed_us() for e in dev if "rows_apply_kernel" in e.name) * 1e-3
        device_ms = sum(e.time_range.elapsed_us() for e in dev) * 1e-3
        del m, prof, dev
        floor_bytes = 2 * ROW_BYTES * rows
        rec = {"rows_in": P, "rows_out": rows, "kept_clones_S_parents_with_children": list(totals),
               "clone_fraction": totals[1] / P, "split_fraction": totals[2] / P,
               "pruned_fraction": ((P - totals[2] - totals[0]) + (totals[2] - totals[3])) / P,
               "fused_ms_median": fm, "staged_ms_median": sm, "ratio": sm / fm, "calls": args.calls,
               "fused_ms_min_max": [min(fused_ms), max(fused_ms)], "staged_ms_min_max": [min(staged_ms), max(staged_ms)],
               "floor_bytes": floor_bytes, "fused_bytes_per_s_of_floor": floor_bytes / (fm * 1e-3),
               "apply_kernel_ms": apply_ms, "apply_kernel_bytes_per_s_of_floor": floor_bytes / (apply_ms * 1e-3) if apply_ms else None,
               "fused_device_busy_ms": device_ms,
               "thresholds": {"max_grad": max_grad, "min_opacity": min_opacity, "extent": extent, "max_screen_size": screen}}
        print(json.dumps(rec), flush=True)
        results.append(rec)
        del params, moments, accum, denom
        torch.cuda.empty_cache()
    out = {"what": "GaussianModel.densify_and_prune (fused) against tests/densify_ref.py Staged.densify_and_prune (staged torch), "
                   "whole-call wall time between stream synchronisations, medians", "device": torch.cuda.get_device_name(0),
           "row_bytes": ROW_BYTES, "sizes": results}
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(out, f, indent=1)
    print("wrote", args.out)


if __name__ == "__main__":
    main()
