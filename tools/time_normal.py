#!/usr/bin/env python3
"""Times the normal maps (csrc/normals.hip, csrc/render_normal.hip, csrc/render_maps_backward.hip) on the bench scene --
BASELINE.json configs[2]: 3M Gaussians, 1920x1080, indexed -- and on bench.py's heavy-tailed scene (scale sigma 1.2), each next to
its sibling in the same run: gaussian_normals and render_normal next to render_depth, the four-map backward replay next to the
three-map one, the whole backward with the term next to the plain one, the stencil pair next to the same stencil in torch ops, and
the whole feature next to the route it replaces (a second forward + backward with colors_precomp = n). Prints one JSON line and
writes profiles/normal_time.json.

    python tools/time_normal.py [--samples 20] [--warmup 5] [--P 3000000] [--near-far 0.2 100] [--out profiles/normal_time.json]

The rasterizer's figures are the library's stage times (c3dgs_profile_*: two stream events around the launches), summed per call;
the torch stencil and the replaced route, which the library does not time, are stream-event times around the calls, and so is the
HIP stencil pair next to the torch one. One sample = one forward; render_depth; gaussian_normals; render_normal; render_distortion;
the plain backward (image gradient only); the backward with the image gradient and three maps; the one with all four; the two
stencils; the second forward + backward; on one stream, in one process. Medians of `samples` samples after `warmup` unrecorded
ones, with min and max. Nothing is promised: the figures are there to be read."""
import argparse
import json
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

BACKWARD = ("zero_partials", "render_backward", "backward_preprocess")
THREE = ("render_distortion_backward", "depth_backward_fold")
FOUR = ("render_normal_backward", "depth_backward_fold", "normal_backward_fold")
KEYS = ("render_depth", "gaussian_normals", "render_normal", "render_distortion_backward", "render_normal_backward", "plain_backward",
        "backward_with_three_maps", "backward_with_four_maps", "stencil_pair_hip", "stencil_pair_torch", "feature", "replaced_route")


def torch_depth_to_normal(z, tan_fovx, tan_fovy):
    """the same stencil in torch ops (what a user writes without the kernel)"""
    H, W = z.shape
    fx, fy = W / (2.0 * tan_fovx), H / (2.0 * tan_fovy)
    xs = (torch.arange(W, device=z.device, dtype=z.dtype) + 0.5 - W / 2.0) / fx
    ys = (torch.arange(H, device=z.device, dtype=z.dtype) + 0.5 - H / 2.0) / fy
    P = torch.stack([z * xs[None, :], z * ys[:, None], z], -1)
    c = torch.linalg.cross(P[2:, 1:-1] - P[:-2, 1:-1], P[1:-1, 2:] - P[1:-1, :-2])
    n = c / c.norm(dim=-1, keepdim=True).clamp_min(1e-12)
    return torch.nn.functional.pad(n.permute(2, 0, 1), (1, 1, 1, 1))


def _events(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    out = fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b), out


def time_scene(label, inp, intr, ev, indexed, samples, warmup, near_far):
    from c3dgs_amd import _lib, normals, rasterizer
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
    gN = torch.rand((3, H, W), device="cuda", generator=g) - 0.5
    tan_fov = rasterizer._intrinsic_scalars(intr)[0][:2]

    def total(st):
        return sum(ms for ms, _ in st.values())

    def stencil(fn, z0):
        z = z0.clone().requires_grad_()

        def go():
            (fn(z) * gN).sum().backward()
        return _events(go)[0]

    def sample(record):
        fw = gpu_util.hip_forward(inp, cam, indexed)
        a = fw["args"]
        bufs = (P, W, H, fw["num_rendered"], fw["geom"], fw["binning"], fw["img"])
        torch.cuda.synchronize()
        _lib.profile_read()
        depth_map, alpha_map, _ = rasterizer._C.render_depth(*bufs)
        torch.cuda.synchronize()
        depth = _lib.profile_read()
        nb = rasterizer._C.gaussian_normals(a[1], a[4], a[6], a[19], a[9])
        torch.cuda.synchronize()
        per_gaussian = _lib.profile_read()
        rasterizer._C.render_normal(*bufs, nb)
        torch.cuda.synchronize()
        nmap = _lib.profile_read()
        _, moment = rasterizer._C.render_distortion(*bufs, near_far)
        torch.cuda.synchronize()
        _lib.profile_read()
        backward(fw, dL)
        torch.cuda.synchronize()
        plain = _lib.profile_read()
        backward(fw, dL, dL_ddepth=gD, dL_dalpha=gA, dL_ddistortion=gL, moment=moment, near_far=near_far)
        torch.cuda.synchronize()
        three = _lib.profile_read()
        backward(fw, dL, dL_ddepth=gD, dL_dalpha=gA, dL_ddistortion=gL, moment=moment, near_far=near_far, dL_dnormal=gN, normals=nb)
        torch.cuda.synchronize()
        four = _lib.profile_read()
        z = depth_map / alpha_map.clamp_min(1e-6)
        hip_ms = stencil(lambda t: normals.depth_to_normal(t, intr), z)
        torch_ms = stencil(lambda t: torch_depth_to_normal(t, *tan_fov), z)
        _lib.profile_read()

        def second_pass():                                       # the route the feature replaces: the normals as colours
            f2 = gpu_util.hip_forward(dict(inp, shs=None, sh_indices=None, colors_precomp=nb[:, :3].contiguous()), cam, indexed)
            backward(f2, gN)
        route_ms = _events(second_pass)[0]
        _lib.profile_read()
        if record is not None:
            assert set(depth) == {"render_depth"} and set(per_gaussian) == {"gaussian_normals"} and set(nmap) == {"render_normal"}
            assert set(plain) == set(BACKWARD) and set(three) == set(BACKWARD + THREE) and set(four) == set(BACKWARD + FOUR), \
                (sorted(plain), sorted(three), sorted(four))
            record["render_depth"].append(total(depth))
            record["gaussian_normals"].append(total(per_gaussian))
            record["render_normal"].append(total(nmap))
            record["render_distortion_backward"].append(three["render_distortion_backward"][0])
            record["render_normal_backward"].append(four["render_normal_backward"][0])
            record["plain_backward"].append(total(plain))
            record["backward_with_three_maps"].append(total(three))
            record["backward_with_four_maps"].append(total(four))
            record["stencil_pair_hip"].append(hip_ms)
            record["stencil_pair_torch"].append(torch_ms)
            # what the term adds to a step that already has the three maps: two forward launches, the four-map backward in the
            # place of the three-map one, the stencil pair
            record["feature"].append(total(per_gaussian) + total(nmap) + (total(four) - total(three)) + hip_ms)
            record["replaced_route"].append(route_ms + torch_ms)
        return fw

    _lib.profile_enable(True)
    for _ in range(warmup):
        fw = sample(None)
    t = {k: [] for k in KEYS}
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
                    help="the distortion map's ndc planes (default: the raw mode)")
    ap.add_argument("--scenes", default="bench,heavy_tail")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "normal_time.json"))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("time_normal.py needs the GPU; a timing taken anywhere else says nothing")
    from tests import fullsize
    from tools.time_contrib import heavy_tail_inputs
    near_far = tuple(args.near_far) if args.near_far else None
    scenes = []
    if "bench" in args.scenes:
        scenes.append(time_scene("bench: BASELINE.json configs[2], synth-v1, indexed", *fullsize.config_inputs("config3_3M_indexed", P=args.P),
                                 args.samples, args.warmup, near_far))
    if "heavy_tail" in args.scenes:
        scenes.append(time_scene("heavy_tail: synth-v1 with scale = exp(N(log 0.009, 1.2^2)) per axis, indexed",
                                 *heavy_tail_inputs(args.P, 1920, 1080, 1200.0), args.samples, args.warmup, near_far))
    out = {"device": torch.cuda.get_device_name(0), "samples": args.samples, "warmup": args.warmup,
           "distortion_mode": "raw" if near_far is None else f"ndc{near_far}",
           "method": "library stage times (stream events around the launches), summed per call, for the rasterizer's stages; stream "
                     "events around the calls for the two stencil pairs (forward + backward under a random gradient) and for the "
                     "replaced route (a second forward + backward with colors_precomp = n, plus the torch stencil); medians; "
                     "plain_backward = zero_partials + render_backward + backward_preprocess; with three maps those + "
                     "render_distortion_backward + depth_backward_fold; with four maps those + render_normal_backward + "
                     "depth_backward_fold + normal_backward_fold; feature = gaussian_normals + render_normal + (four maps - three "
                     "maps) + the HIP stencil pair",
           "scenes": scenes}
    print(json.dumps(out))
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as fh:
            json.dump(out, fh, indent=1)


if __name__ == "__main__":
    main()
