#!/usr/bin/env python3
"""Times the backward through the depth and alpha maps (csrc/render_maps_backward.hip, c3dgs_rasterize_gaussians_backward_depth_indexed)
on the bench scene -- BASELINE.json configs[2]: 3M Gaussians, 1920x1080, indexed -- and on bench.py's heavy-tailed scene (scale
sigma 1.2), against the same run's plain backward and against the only route to the same gradients without it: a second
forward with colours (z, 1, 0) and a second full backward. Prints one JSON line and writes profiles/r15_depth_backward_time.json.

    python tools/time_depth_backward.py [--samples 20] [--warmup 5] [--P 3000000] [--out profiles/r15_depth_backward_time.json]

All figures are the library's stage times (c3dgs_profile_*: two stream events around the launches), summed per call. One sample =
one forward; the plain backward (image gradient only); the backward with the image gradient and both maps; the colour-coded
forward and its backward; all on one stream, in one process. Medians of `samples` samples after `warmup` unrecorded ones, with
min and max. The expectation to read the figures against: backward_with_maps < plain_backward + extra_route."""
import argparse
import json
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

BACKWARD = ("zero_partials", "render_backward", "backward_preprocess")
NEW = ("render_depth_backward", "depth_backward_fold")


def backward(fw, dL, **maps):
    """tests/gpu_util.py:hip_backward for an indexed forward, without the copies to the host"""
    from c3dgs_amd import rasterizer
    (bg, means3D, colors, opac, scales, sf, rot, smod, cov3D, view, proj, tfx, tfy, H, W, sh, deg, campos, shi, gi, pre, dbg, clamp) = fw["args"]
    return rasterizer._C.rasterize_gaussians_backward_indexed(bg, means3D, fw["radii"], colors, scales, sf, rot, smod, cov3D, view, proj, tfx,
                                                              tfy, dL, sh, deg, campos, fw["geom"], fw["num_rendered"], fw["binning"],
                                                              fw["img"], False, shi, gi, **maps)


def time_scene(label, inp, intr, ev, indexed, samples, warmup):
    from c3dgs_amd import _lib
    from oracle import oracle as orc
    from tests import gpu_util
    assert indexed
    cam = orc.camera(intr.numpy(), ev.numpy())
    inp = {k: (v.cuda() if isinstance(v, torch.Tensor) else v) for k, v in inp.items()}     # uploaded once, not per sample
    W, H = cam["W"], cam["H"]
    P = int(inp["means3D"].shape[0])
    dL = torch.ones((3, H, W), dtype=torch.float32, device="cuda")
    g = torch.Generator(device="cuda").manual_seed(5)
    gD = 0.25 + 0.75 * torch.rand((H, W), device="cuda", generator=g)
    gA = 0.25 + 0.75 * torch.rand((H, W), device="cuda", generator=g)
    v = torch.from_numpy(cam["viewmatrix"]).cuda().reshape(4, 4)
    m = inp["means3D"]
    z = m[:, 0] * v[0, 2] + m[:, 1] * v[1, 2] + m[:, 2] * v[2, 2] + v[3, 2]
    inp_z = dict(inp, shs=None, sh_indices=None, colors_precomp=torch.stack([z, torch.ones_like(z), torch.zeros_like(z)], 1).contiguous(),
                 bg=torch.zeros(3, device="cuda"))
    dLz = torch.stack([gD, gA, torch.zeros_like(gD)]).contiguous()

    def total(st, names=None):
        return sum(ms for k, (ms, _) in st.items() if names is None or k in names)

    def sample(record):
        fw = gpu_util.hip_forward(inp, cam, indexed)
        torch.cuda.synchronize()
        _lib.profile_read()
        backward(fw, dL)
        torch.cuda.synchronize()
        plain = _lib.profile_read()
        backward(fw, dL, dL_ddepth=gD, dL_dalpha=gA)
        torch.cuda.synchronize()
        maps = _lib.profile_read()
        fz = gpu_util.hip_forward(inp_z, cam, indexed)
        backward(fz, dLz)
        torch.cuda.synchronize()
        extra = _lib.profile_read()
        if record is not None:
            assert set(plain) == set(BACKWARD) and set(maps) == set(BACKWARD + NEW), (sorted(plain), sorted(maps))
            record["plain_backward"].append(total(plain))
            record["backward_with_maps"].append(total(maps))
            record["extra_route"].append(total(extra))
            for k in NEW:
                record[k].append(maps[k][0])
        return fw

    _lib.profile_enable(True)
    for _ in range(warmup):
        fw = sample(None)
    t = {k: [] for k in ("plain_backward", "backward_with_maps", "extra_route") + NEW}
    for _ in range(samples):
        fw = sample(t)
    _lib.profile_enable(False)
    out = {"scene": label, "P": P, "W": W, "H": H, "num_rendered": fw["num_rendered"]}
    for k, vals in t.items():
        out[k + "_ms"] = statistics.median(vals)
        out[k + "_ms_min_max"] = [min(vals), max(vals)]
    out["added_by_the_maps_ms"] = out["backward_with_maps_ms"] - out["plain_backward_ms"]
    out["maps_over_plain_plus_extra_route"] = out["backward_with_maps_ms"] / (out["plain_backward_ms"] + out["extra_route_ms"])
    del inp, inp_z, fw
    torch.cuda.empty_cache()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--samples", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--P", type=int, default=3_000_000)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r15_depth_backward_time.json"))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("time_depth_backward.py needs the GPU; a timing taken anywhere else says nothing")
    from tests import fullsize
    from tools.time_contrib import heavy_tail_inputs
    scenes = []
    scenes.append(time_scene("bench: BASELINE.json configs[2], synth-v1, indexed", *fullsize.config_inputs("config3_3M_indexed", P=args.P),
                             args.samples, args.warmup))
    scenes.append(time_scene("heavy_tail: synth-v1 with scale = exp(N(log 0.009, 1.2^2)) per axis, indexed",
                             *heavy_tail_inputs(args.P, 1920, 1080, 1200.0), args.samples, args.warmup))
    out = {"device": torch.cuda.get_device_name(0), "samples": args.samples, "warmup": args.warmup,
           "method": "library stage times (stream events around the launches), summed per call; per sample one forward, the plain "
                     "backward, the backward with the image gradient and both maps, and the extra route (a forward with colours "
                     "(z, 1, 0) and its backward) on one stream; medians; plain_backward = zero_partials + render_backward + "
                     "backward_preprocess; backward_with_maps = those + render_depth_backward + depth_backward_fold; extra_route "
                     "= every stage of the second forward and backward",
           "scenes": scenes}
    print(json.dumps(out))
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as fh:
            json.dump(out, fh, indent=1)


if __name__ == "__main__":
    main()
