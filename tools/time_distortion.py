#!/usr/bin/env python3
"""Times the depth-distortion map and its backward (csrc/render_distortion.hip, csrc/render_maps_backward.hip) on the bench
scene -- BASELINE.json configs[2]: 3M Gaussians, 1920x1080, indexed -- and on bench.py's heavy-tailed scene (scale sigma 1.2), each
next to its sibling in the same run: render_distortion next to render_depth, the three-map backward replay next to the two-map
one, and the whole backward with the three maps next to the plain one. Prints one JSON line and writes
profiles/distortion_time.json.

    python tools/time_distortion.py [--samples 20] [--warmup 5] [--P 3000000] [--near-far 0.2 100] [--out profiles/distortion_time.json]

All figures are the library's stage times (c3dgs_profile_*: two stream events around the launches), summed per call. One sample =
one forward; render_depth; render_distortion; the plain backward (image gradient only); the backward with the image gradient and
the depth and alpha maps; the backward with the image gradient and all three maps; on one stream, in one process. Medians of
`samples` samples after `warmup` unrecorded ones, with min and max. Nothing is promised: the figures are there to be read."""
import argparse
import json
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

BACKWARD = ("zero_partials", "render_backward", "backward_preprocess")
TWO = ("render_depth_backward", "depth_backward_fold")
THREE = ("render_distortion_backward", "depth_backward_fold")


def time_scene(label, inp, intr, ev, indexed, samples, warmup, near_far):
    from c3dgs_amd import _lib, rasterizer
    from oracle import oracle as orc
    from tests import gpu_util
    from tools.time_depth_backward import backward
    assert indexed
    cam = orc.camera(intr.numpy(), ev.numpy())
    inp = {k: (v.cuda() if isinstance(v, torch.Tensor) else v) for k, v in inp.items()}     # uploaded once, not per sample
    W, H = cam["W"], cam["H"]
    P = int(inp["means3D"].shape[0])
    dL = torch.ones((3, H, W), dtype=torch.float32, device="cuda")
    g = torch.Generator(device="cuda").manual_seed(5)
    gD, gA, gL = (0.25 + 0.75 * torch.rand((H, W), device="cuda", generator=g) for _ in range(3))

    def total(st):
        return sum(ms for ms, _ in st.values())

    def sample(record):
        fw = gpu_util.hip_forward(inp, cam, indexed)
        bufs = (P, W, H, fw["num_rendered"], fw["geom"], fw["binning"], fw["img"])
        torch.cuda.synchronize()
        _lib.profile_read()
        rasterizer._C.render_depth(*bufs)
        torch.cuda.synchronize()
        depth = _lib.profile_read()
        _, moment = rasterizer._C.render_distortion(*bufs, near_far)
        torch.cuda.synchronize()
        dist = _lib.profile_read()
        backward(fw, dL)
        torch.cuda.synchronize()
        plain = _lib.profile_read()
        backward(fw, dL, dL_ddepth=gD, dL_dalpha=gA)
        torch.cuda.synchronize()
        two = _lib.profile_read()
        backward(fw, dL, dL_ddepth=gD, dL_dalpha=gA, dL_ddistortion=gL, moment=moment, near_far=near_far)
        torch.cuda.synchronize()
        three = _lib.profile_read()
        if record is not None:
            assert set(depth) == {"render_depth"} and set(dist) == {"render_distortion"}, (sorted(depth), sorted(dist))
            assert set(plain) == set(BACKWARD) and set(two) == set(BACKWARD + TWO) and set(three) == set(BACKWARD + THREE), \
                (sorted(plain), sorted(two), sorted(three))
            record["render_depth"].append(total(depth))
            record["render_distortion"].append(total(dist))
            record["render_depth_backward"].append(two["render_depth_backward"][0])
            record["render_distortion_backward"].append(three["render_distortion_backward"][0])
            record["plain_backward"].append(total(plain))
            record["backward_with_two_maps"].append(total(two))
            record["backward_with_three_maps"].append(total(three))
        return fw

    _lib.profile_enable(True)
    for _ in range(warmup):
        fw = sample(None)
    t = {k: [] for k in ("render_depth", "render_distortion", "render_depth_backward", "render_distortion_backward", "plain_backward",
                         "backward_with_two_maps", "backward_with_three_maps")}
    for _ in range(samples):
        fw = sample(t)
    _lib.profile_enable(False)
    out = {"scene": label, "P": P, "W": W, "H": H, "num_rendered": fw["num_rendered"]}
    for k, vals in t.items():
        out[k + "_ms"] = statistics.median(vals)
        out[k + "_ms_min_max"] = [min(vals), max(vals)]
    del inp, fw
    torch.cuda.empty_cache()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--samples", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--P", type=int, default=3_000_000)
    ap.add_argument("--near-far", type=float, nargs=2, default=None, metavar=("NEAR", "FAR"),
                    help="the ndc mode's planes (default: the raw mode)")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "distortion_time.json"))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("time_distortion.py needs the GPU; a timing taken anywhere else says nothing")
    from tests import fullsize
    from tools.time_contrib import heavy_tail_inputs
    near_far = tuple(args.near_far) if args.near_far else None
    scenes = []
    scenes.append(time_scene("bench: BASELINE.json configs[2], synth-v1, indexed", *fullsize.config_inputs("config3_3M_indexed", P=args.P),
                             args.samples, args.warmup, near_far))
    scenes.append(time_scene("heavy_tail: synth-v1 with scale = exp(N(log 0.009, 1.2^2)) per axis, indexed",
                             *heavy_tail_inputs(args.P, 1920, 1080, 1200.0), args.samples, args.warmup, near_far))
    out = {"device": torch.cuda.get_device_name(0), "samples": args.samples, "warmup": args.warmup,
           "mode": "raw" if near_far is None else f"ndc{near_far}",
           "method": "library stage times (stream events around the launches), summed per call; per sample one forward, render_depth, "
                     "render_distortion, the plain backward, the backward with the image gradient and the depth and alpha maps, and "
                     "the backward with the image gradient and all three maps, on one stream; medians; plain_backward = "
                     "zero_partials + render_backward + backward_preprocess; with two maps those + render_depth_backward + "
                     "depth_backward_fold; with three maps those + render_distortion_backward + depth_backward_fold",
           "scenes": scenes}
    print(json.dumps(out))
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as fh:
            json.dump(out, fh, indent=1)


if __name__ == "__main__":
    main()
