#!/usr/bin/env python3
"""Times the depth / alpha / median-depth pass (csrc/render_depth.hip, c3dgs_render_depth) on the bench scene -- BASELINE.json
configs[2]: 3M Gaussians, 1920x1080, indexed -- against the yardstick the issue sets for it: render_forward's own stage time in
the same process. Prints one JSON line and writes profiles/r10_depth_time.json.

    python tools/time_depth.py [--samples 20] [--warmup 5] [--P 3000000] [--out profiles/r10_depth_time.json]

Both figures are the library's stage times (c3dgs_profile_*: two stream events around the launch), one forward followed by one
render_depth per sample on one stream, the median of `samples` samples after `warmup` unrecorded ones."""
import argparse
import ctypes
import json
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--samples", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--P", type=int, default=3_000_000)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r10_depth_time.json"))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("time_depth.py needs the GPU; a timing taken anywhere else says nothing")
    from c3dgs_amd import _lib, rasterizer
    from oracle import oracle as orc
    from tests import fullsize, gpu_util
    inp, intr, ev, indexed = fullsize.config_inputs("config3_3M_indexed", P=args.P)
    cam = orc.camera(intr.numpy(), ev.numpy())
    inp = {k: (v.cuda() if isinstance(v, torch.Tensor) else v) for k, v in inp.items()}     # uploaded once, not per sample
    W, H = cam["W"], cam["H"]

    def step():
        fw = gpu_util.hip_forward(inp, cam, indexed)
        maps = rasterizer._C.render_depth(args.P, W, H, fw["num_rendered"], fw["geom"], fw["binning"], fw["img"])
        return fw, maps

    for _ in range(args.warmup):
        fw, maps = step()
    torch.cuda.synchronize()
    il = _lib.ImageLayout()
    _lib.lib().c3dgs_get_image_layout(W, H, ctypes.byref(il))
    alpha_ok = bool(torch.equal(maps[1].reshape(-1), 1.0 - gpu_util._view(fw["img"], il.final_T, W * H, torch.float32)))
    _lib.profile_enable(True)
    _lib.profile_read()
    t_fwd, t_depth = [], []
    for _ in range(args.samples):
        step()
        torch.cuda.synchronize()
        st = _lib.profile_read()
        assert st["render_forward"][1] == 1 and st["render_depth"][1] == 1, st
        t_fwd.append(st["render_forward"][0])
        t_depth.append(st["render_depth"][0])
    _lib.profile_enable(False)
    f, d = statistics.median(t_fwd), statistics.median(t_depth)
    out = {"device": torch.cuda.get_device_name(0), "scene": "BASELINE.json configs[2]: synth-v1, indexed", "P": args.P, "W": W, "H": H,
           "num_rendered": fw["num_rendered"], "samples": args.samples, "warmup": args.warmup,
           "method": "library stage times (stream events around the launch), one forward + one render_depth per sample, median",
           "render_forward_ms": f, "render_forward_ms_min_max": [min(t_fwd), max(t_fwd)],
           "render_depth_ms": d, "render_depth_ms_min_max": [min(t_depth), max(t_depth)],
           "render_depth_over_render_forward": d / f, "alpha_equals_one_minus_final_T": alpha_ok}
    print(json.dumps(out))
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as fh:
            json.dump(out, fh, indent=1)


if __name__ == "__main__":
    main()
