#!/usr/bin/env python3
"""Times GaussianModel.prune_points_indexed (flag pass, three scans, one emit pass, at most three gather launches:
csrc/index_plan.hip + the apply kernel of csrc/densify.hip) against the vectorised torch restatement of tests/index_ref.py
followed by torch gathers of the same tensors, on the same device in the same process -> profiles/r07_index_prune_time.json.

    python tools/time_index_prune.py [--sizes 1000000,3000000,6000000] [--calls 20] [--out profiles/r07_index_prune_time.json]

An indexed model at SH degree 3 with Adam moments attached and the codebook sizes of tests/synth.py index_scene's defaults
(4096 + 0.1 P colour rows, 4096 + 0.25 P geometry rows: 754,096 geometry rows at 3M), uniform random indices, random values
drawn on the device (no value is looked at), about 10 % of the Gaussians pruned. Every call runs on a fresh clone of the state;
after a warm-up the two alternate and each timing is the time between two events on the stream around the whole call (the
host read of the totals, and torch's own host reads in nonzero / boolean indexing, are part of the cost). The results of
both are compared once per size.

The reference's own form of the remap, a Python loop with one device write per referenced id (scene/gaussian_model.py:
1110-1113), is timed at a 4096-row codebook ONLY and reported under that name; it is not extrapolated."""
import argparse
import json
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from tests import index_ref  # noqa: E402

DEV = "cuda"
NAMES = {"xyz": "_xyz", "f_dc": "_features_dc", "f_rest": "_features_rest", "opacity": "_opacity", "scaling": "_scaling",
         "rotation": "_rotation", "scaling_factor": "_scaling_factor"}
ROWS, COLOR, GEOMETRY = ("xyz", "opacity", "scaling_factor"), ("f_dc", "f_rest"), ("scaling", "rotation")


def base_state(P, seed=1234):
    g = torch.Generator(device=DEV).manual_seed(seed)
    K0, K1 = min(P, int(4096 + 0.1 * P)), min(P, int(4096 + 0.25 * P))
    shapes = {"xyz": (P, 3), "opacity": (P, 1), "scaling_factor": (P, 1), "f_dc": (K0, 1, 3), "f_rest": (K0, 15, 3),
              "scaling": (K1, 3), "rotation": (K1, 4)}
    params = {k: torch.randn(s, device=DEV, generator=g) for k, s in shapes.items()}
    moments = {k: (torch.randn(s, device=DEV, generator=g) * 1e-3, torch.rand(s, device=DEV, generator=g) * 1e-6) for k, s in shapes.items()}
    idx0 = torch.randint(0, K0, (P,), device=DEV, generator=g, dtype=torch.int64)
    idx1 = torch.randint(0, K1, (P,), device=DEV, generator=g, dtype=torch.int64)
    mask = torch.rand(P, device=DEV, generator=g) < 0.1
    stats = (torch.rand(P, 1, device=DEV, generator=g), torch.rand(P, 1, device=DEV, generator=g), torch.rand(P, device=DEV, generator=g))
    return params, moments, idx0, idx1, mask, stats


def hip_model(params, moments, idx0, idx1, stats):
    from c3dgs_amd.model import GaussianModel
    from c3dgs_amd.pipeline import OptimizationParams
    m = GaussianModel(3, quantization=True, device=DEV)
    c = {k: v.clone() for k, v in params.items()}
    m.set_tensors(xyz=c["xyz"], features_dc=c["f_dc"], features_rest=c["f_rest"], scaling=c["scaling"], rotation=c["rotation"],
                  opacity=c["opacity"], scaling_factor=c["scaling_factor"], feature_indices=idx0.clone(), gaussian_indices=idx1.clone())
    m.spatial_lr_scale = 1.0
    m.training_setup(OptimizationParams())
    for k, attr in NAMES.items():
        m.optimizer.state[getattr(m, attr)] = {"step": torch.tensor(1.0), "exp_avg": moments[k][0].clone(), "exp_avg_sq": moments[k][1].clone()}
    m.xyz_gradient_accum, m.denom, m.max_radii2D = (t.clone() for t in stats)
    return m


def torch_prune(params, moments, idx0, idx1, mask, stats):
    """The whole prune in torch: tests/index_ref.py for the maps, boolean / index gathers for the rows."""
    K0, K1 = params["f_dc"].shape[0], params["scaling"].shape[0]
    src, new0, new1, cb0, cb1 = index_ref.plan_ref(~mask, idx0, K0, idx1, K1)
    out = {}
    for keys, rows in ((ROWS, src), (COLOR, cb0), (GEOMETRY, cb1)):
        for k in keys:
            out[k] = (params[k][rows], moments[k][0][rows], moments[k][1][rows])
    return out, new0, new1, [t[src] for t in stats]


def timed(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    a.record()
    out = fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b), out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", default="1000000,3000000,6000000")
    ap.add_argument("--calls", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r07_index_prune_time.json"))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("time_index_prune.py measures on the GPU; there is no CPU path")
    results = []
    for P in [int(s) for s in args.sizes.split(",")]:
        params, moments, idx0, idx1, mask, stats = base_state(P)
        hip_ms, torch_ms, rec = [], [], None
        for it in range(args.warmup + args.calls):
            m = hip_model(params, moments, idx0, idx1, stats)
            th, (src, cb0, cb1, totals) = timed(lambda: m.prune_points_indexed(mask))
            with torch.no_grad():
                tt, (want, new0, new1, _) = timed(lambda: torch_prune(params, moments, idx0, idx1, mask, stats))
            if it == 0:                                            # the two agree, bit for bit
                for k, attr in NAMES.items():
                    p = getattr(m, attr)
                    st = m.optimizer.state[p]
                    if not (torch.equal(p.detach(), want[k][0]) and torch.equal(st["exp_avg"], want[k][1]) and torch.equal(st["exp_avg_sq"], want[k][2])):
                        raise SystemExit(f"P={P}: {k} differs between the HIP path and the torch restatement")
                if not (torch.equal(m._feature_indices, new0) and torch.equal(m._gaussian_indices, new1)):
                    raise SystemExit(f"P={P}: remapped indices differ")
            rec = {"rows_in": P, "rows_out": totals[0], "color_rows_in": params["f_dc"].shape[0], "color_rows_out": totals[1],
                   "geometry_rows_in": params["scaling"].shape[0], "geometry_rows_out": totals[2]}
            del m, want, new0, new1, src, cb0, cb1
            if it >= args.warmup:
                hip_ms.append(th)
                torch_ms.append(tt)
        hm, tm = statistics.median(hip_ms), statistics.median(torch_ms)
        rec.update({"hip_ms_median": hm, "torch_restatement_ms_median": tm, "ratio_torch_over_hip": tm / hm, "calls": args.calls,
                    "hip_ms_min_max": [min(hip_ms), max(hip_ms)], "torch_restatement_ms_min_max": [min(torch_ms), max(torch_ms)]})
        print(json.dumps(rec), flush=True)
        results.append(rec)
        del params, moments, idx0, idx1, mask, stats
        torch.cuda.empty_cache()
    # the reference's loop over ids, at 4096 codebook rows only
    g = torch.Generator(device=DEV).manual_seed(7)
    idx = torch.randint(0, 4096, (100_000,), device=DEV, generator=g, dtype=torch.int64)
    valid = torch.rand(100_000, device=DEV, generator=g) >= 0.1
    loop_ms = [timed(lambda: index_ref.loop_ref(4096, idx, valid))[0] for _ in range(1 + 3)][1:]
    out = {"what": "GaussianModel.prune_points_indexed (HIP) against tests/index_ref.py plan_ref + torch gathers (torch restatement), "
                   "time between two stream events around the whole call, medians", "device": torch.cuda.get_device_name(0),
           "sizes": results,
           "reference_loop_form_at_4096_rows_only": {"codebook_rows": 4096, "gaussians": 100_000, "ms_median": statistics.median(loop_ms),
                                                     "note": "one index space, the remap alone, no row movement; not extrapolated"}}
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(out, f, indent=1)
    print("wrote", args.out)


if __name__ == "__main__":
    main()
