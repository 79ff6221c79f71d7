#!/usr/bin/env python3
"""Times the per-Gaussian blend statistics (csrc/render_contrib.hip, c3dgs_render_contrib) on the bench scene -- BASELINE.json
configs[2]: 3M Gaussians, 1920x1080, indexed -- and on bench.py's heavy-tailed scene (scale sigma 1.2), against the cheapest route
to the same weight_sum without it: a full backward, i.e. render_backward + its prep launch (zero_partials) +
backward_preprocess, timed in the same process. Prints one JSON line and writes profiles/r11_contrib_time.json.

    python tools/time_contrib.py [--samples 20] [--warmup 5] [--P 3000000] [--out profiles/r11_contrib_time.json]

All figures are the library's stage times (c3dgs_profile_*: two stream events around the launches). One sample = one forward,
one render_depth, one render_contrib and one backward on one stream; medians of `samples` samples after `warmup` unrecorded
ones. "render_contrib" covers the flag clear and both kernels; "render_contrib_blend" (A) and "render_contrib_sum" (B) are the
two kernels alone."""
import argparse
import json
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

STAGES = ("render_forward", "render_depth", "render_contrib", "render_contrib_blend", "render_contrib_sum", "zero_partials",
          "render_backward", "backward_preprocess")


def heavy_tail_inputs(P, W, H, focal):
    """bench.py:bench_heavy_tail's scene as the inputs dict of tests/fullsize.py:config_inputs"""
    from tests import synth
    intr, ev = synth.camera(W, H, focal)
    ix = synth.index_scene(synth.scene(P, W, H, focal, seed=1234, sh_degree=3, scale_sigma=1.2))
    inp = dict(bg=torch.zeros(3), means3D=ix["means3D"], opacities=ix["opacities"], shs=ix["shs"], colors_precomp=None,
               scales=ix["scales"], rotations=ix["rotations"], cov3D_precomp=None, scale_factors=ix["scale_factors"],
               sh_indices=ix["sh_indices"], g_indices=ix["g_indices"], degree=3, scale_modifier=1.0, prefiltered=False, clamp_color=True)
    return inp, intr, ev, True


def backward(fw, dL):
    """tests/gpu_util.py:hip_backward for an indexed forward, without the copies to the host"""
    from c3dgs_amd import rasterizer
    (bg, means3D, colors, opac, scales, sf, rot, smod, cov3D, view, proj, tfx, tfy, H, W, sh, deg, campos, shi, gi, pre, dbg, clamp) = fw["args"]
    return rasterizer._C.rasterize_gaussians_backward_indexed(bg, means3D, fw["radii"], colors, scales, sf, rot, smod, cov3D, view, proj, tfx,
                                                              tfy, dL, sh, deg, campos, fw["geom"], fw["num_rendered"], fw["binning"],
                                                              fw["img"], False, shi, gi)


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

    def step():
        fw = gpu_util.hip_forward(inp, cam, indexed)
        rasterizer._C.render_depth(P, W, H, fw["num_rendered"], fw["geom"], fw["binning"], fw["img"])
        stats = rasterizer._C.render_contrib(P, W, H, fw["num_rendered"], fw["geom"], fw["binning"], fw["img"])
        backward(fw, dL)
        return fw, stats

    for _ in range(warmup):
        fw, stats = step()
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
           "gaussians_blended": int((hits > 0).sum()), "blended_pairs": int(hits.to(torch.int64).sum())}
    for k in STAGES:
        out[k + "_ms"] = statistics.median(t[k])
        out[k + "_ms_min_max"] = [min(t[k]), max(t[k])]
    out["backward_route_ms"] = statistics.median(route)
    out["backward_route_ms_min_max"] = [min(route), max(route)]
    out["render_contrib_over_backward_route"] = out["render_contrib_ms"] / out["backward_route_ms"]
    del inp, fw, stats
    torch.cuda.empty_cache()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--samples", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--P", type=int, default=3_000_000)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r11_contrib_time.json"))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("time_contrib.py needs the GPU; a timing taken anywhere else says nothing")
    from tests import fullsize
    scenes = []
    scenes.append(time_scene("bench: BASELINE.json configs[2], synth-v1, indexed", *fullsize.config_inputs("config3_3M_indexed", P=args.P),
                             args.samples, args.warmup))
    scenes.append(time_scene("heavy_tail: synth-v1 with scale = exp(N(log 0.009, 1.2^2)) per axis, indexed",
                             *heavy_tail_inputs(args.P, 1920, 1080, 1200.0), args.samples, args.warmup))
    out = {"device": torch.cuda.get_device_name(0), "samples": args.samples, "warmup": args.warmup,
           "method": "library stage times (stream events around the launches); per sample one forward, render_depth, render_contrib "
                     "and backward on one stream; medians; backward_route = render_backward + zero_partials + backward_preprocess",
           "scenes": scenes}
    print(json.dumps(out))
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as fh:
            json.dump(out, fh, indent=1)


if __name__ == "__main__":
    main()
