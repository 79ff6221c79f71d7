#!/usr/bin/env python3
"""Times the per-Gaussian error scores (csrc/render_error.hip, c3dgs_render_error) and the error map (c3dgs_error_map_l1) on the
bench scene -- BASELINE.json configs[2]: 3M Gaussians, 1920x1080, indexed -- and on bench.py's heavy-tailed scene (scale sigma
1.2), next to render_contrib in the same process and against the only route to the same score without the pass: a full
backward, i.e. render_backward + its prep launch (zero_partials) + backward_preprocess. Prints one JSON line and writes
profiles/r12_error_time.json.

    python tools/time_error.py [--samples 20] [--warmup 5] [--P 3000000] [--out profiles/r12_error_time.json]

All figures are the library's stage times (c3dgs_profile_*: two stream events around the launches). One sample = one forward,
one error_map_l1 (the forward's image against a fixed random target), one render_error under that map, one render_contrib and one
backward on one stream; medians of `samples` samples after `warmup` unrecorded ones, with min and max. "render_error" covers
the flag clear and both kernels; "render_error_blend" (A') and "render_error_sum" (B') are the two kernels alone. The two
expectations (render_error below the backward route; not above render_contrib by more than render_contrib's own min-max spread)
are evaluated and written as booleans, whatever they come to."""
import argparse
import json
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from tools.time_contrib import backward, heavy_tail_inputs  # noqa: E402

STAGES = ("render_forward", "error_map_l1", "render_error", "render_error_blend", "render_error_sum", "render_contrib",
          "render_contrib_blend", "render_contrib_sum", "zero_partials", "render_backward", "backward_preprocess")


def time_scene(label, inp, intr, ev, indexed, samples, warmup):
    from c3dgs_amd import _lib, rasterizer
    from oracle import oracle as orc
    from tests import gpu_util
    assert indexed
    cam = orc.camera(intr.numpy(), ev.numpy())
    inp = {k: (v.cuda() if isinstance(v, torch.Tensor) else v) for k, v in inp.items()}     # uploaded once, not per sample
    W, H = cam["W"], cam["H"]
    P = int(inp["means3D"].shape[0])
    dL = torch.ones((3, H, W), dtype=torch.float32, device="cuda")
    target = torch.rand((3, H, W), generator=torch.Generator().manual_seed(1)).cuda()

    def step():
        fw = gpu_util.hip_forward(inp, cam, indexed)
        emap = rasterizer._C.error_map_l1(fw["color"], target)
        err = rasterizer._C.render_error(P, W, H, fw["num_rendered"], fw["geom"], fw["binning"], fw["img"], emap)
        stats = rasterizer._C.render_contrib(P, W, H, fw["num_rendered"], fw["geom"], fw["binning"], fw["img"])
        backward(fw, dL)
        return fw, err, stats

    for _ in range(warmup):
        fw, err, stats = step()
    torch.cuda.synchronize()
    hits = stats[2]
    _lib.profile_enable(True)
    _lib.profile_read()
    t = {k: [] for k in STAGES}
    for _ in range(samples):
        step()
        torch.cuda.synchronize()
        st = _lib.profile_read()
        for k in STAGES:
            assert st[k][1] == 1, (k, st)
            t[k].append(st[k][0])
    _lib.profile_enable(False)
    route = [a + b + c for a, b, c in zip(t["render_backward"], t["zero_partials"], t["backward_preprocess"])]
    out = {"scene": label, "P": P, "W": W, "H": H, "num_rendered": fw["num_rendered"],
           "gaussians_blended": int((hits > 0).sum()), "blended_pairs": int(hits.to(torch.int64).sum()),
           "gaussians_scored": int((err > 0).sum())}
    for k in STAGES:
        out[k + "_ms"] = statistics.median(t[k])
        out[k + "_ms_min_max"] = [min(t[k]), max(t[k])]
    out["backward_route_ms"] = statistics.median(route)
    out["backward_route_ms_min_max"] = [min(route), max(route)]
    out["render_error_over_backward_route"] = out["render_error_ms"] / out["backward_route_ms"]
    out["render_error_over_render_contrib"] = out["render_error_ms"] / out["render_contrib_ms"]
    spread = max(t["render_contrib"]) - min(t["render_contrib"])
    out["expectation_below_backward_route"] = out["render_error_ms"] < out["backward_route_ms"]
    out["expectation_not_above_render_contrib"] = out["render_error_ms"] <= out["render_contrib_ms"] + spread
    del inp, fw, err, stats
    torch.cuda.empty_cache()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--samples", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--P", type=int, default=3_000_000)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r12_error_time.json"))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("time_error.py needs the GPU; a timing taken anywhere else says nothing")
    from tests import fullsize
    scenes = []
    scenes.append(time_scene("bench: BASELINE.json configs[2], synth-v1, indexed", *fullsize.config_inputs("config3_3M_indexed", P=args.P),
                             args.samples, args.warmup))
    scenes.append(time_scene("heavy_tail: synth-v1 with scale = exp(N(log 0.009, 1.2^2)) per axis, indexed",
                             *heavy_tail_inputs(args.P, 1920, 1080, 1200.0), args.samples, args.warmup))
    out = {"device": torch.cuda.get_device_name(0), "samples": args.samples, "warmup": args.warmup,
           "method": "library stage times (stream events around the launches); per sample one forward, error_map_l1, render_error, "
                     "render_contrib and backward on one stream; medians; backward_route = render_backward + zero_partials + "
                     "backward_preprocess; the margin of the render_contrib expectation is render_contrib's own max - min",
           "scenes": scenes}
    print(json.dumps(out))
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as fh:
            json.dump(out, fh, indent=1)


if __name__ == "__main__":
    main()
