#!/usr/bin/env python3
"""Times the exact pose gradient (csrc/pose_grad.hip, c3dgs_pose_grad) on the bench scene -- BASELINE.json configs[2]: 3M
Gaussians, 1920x1080, indexed -- against the only route to a pose gradient without it, rasterizer.camera_pose_jacobian_sum (the
reference's formula in torch ops) on the same inputs in the same process. Prints one JSON line and writes
profiles/r13_pose_grad_time.json.

    python tools/time_pose_grad.py [--samples 20] [--warmup 5] [--P 3000000] [--out profiles/r13_pose_grad_time.json]

pose_grad, pose_grad_sums (stage A) and pose_grad_fold (stage B) are the library's stage times (c3dgs_profile_*: two stream
events around the launches); the torch route is timed between two stream events as well. One sample = one forward, one backward
with nothing skipped, one pose_grad, one camera_pose_jacobian_sum, and one more backward with dL_dcolors / dL_dcov3D skipped (what
the autograd wrappers do when no exact pose gradient is asked for): the difference of the two backwards is what exact mode adds
to the backward itself. Medians of `samples` samples after `warmup` unrecorded ones, with min and max. The floor is the bytes
stage A actually requests (counted from the gradients' zero pattern) at the rate a device-to-device copy of 512 MiB reaches in
the same process. The expectation (pose_grad below the torch route) is evaluated and written as a boolean, whatever it comes to."""
import argparse
import json
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

STAGES = ("pose_grad", "pose_grad_sums", "pose_grad_fold", "zero_partials", "render_backward", "backward_preprocess")
BWD = ("zero_partials", "render_backward", "backward_preprocess")


def _event_ms(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    out = fn()
    b.record()
    b.synchronize()
    return out, a.elapsed_time(b)


def copy_rate_gb_s(samples):
    src = torch.empty(512 << 20, dtype=torch.uint8, device="cuda")
    dst = torch.empty_like(src)
    for _ in range(3):
        dst.copy_(src)
    ms = [_event_ms(lambda: dst.copy_(src))[1] for _ in range(samples)]
    return 2 * src.numel() / (statistics.median(ms) * 1e-3) / 1e9        # bytes read + bytes written


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--samples", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--P", type=int, default=3_000_000)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r13_pose_grad_time.json"))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("time_pose_grad.py needs the GPU; a timing taken anywhere else says nothing")
    from c3dgs_amd import _lib, rasterizer
    from oracle import oracle as orc
    from tests import fullsize, gpu_util
    inp, intr, ev, indexed = fullsize.config_inputs("config3_3M_indexed", P=args.P)
    assert indexed
    cam = orc.camera(intr.numpy(), ev.numpy())
    inp = {k: (v.cuda() if isinstance(v, torch.Tensor) else v) for k, v in inp.items()}
    intr_d, pose = intr.cuda(), ev.cuda()
    W, H, P = cam["W"], cam["H"], int(inp["means3D"].shape[0])
    dL = torch.ones((3, H, W), dtype=torch.float32, device="cuda")

    def backward(fw, skip):
        (bg, means3D, colors, opac, scales, sf, rot, smod, cov3D, view, proj, tfx, tfy, H_, W_, sh, deg, campos, shi, gi, pre, dbg,
         clamp) = fw["args"]
        return rasterizer._C.rasterize_gaussians_backward_indexed(bg, means3D, fw["radii"], colors, scales, sf, rot, smod, cov3D, view,
                                                                  proj, tfx, tfy, dL, sh, deg, campos, fw["geom"], fw["num_rendered"],
                                                                  fw["binning"], fw["img"], False, shi, gi, skip=skip)

    def pose_grad(fw, g):
        return rasterizer._C.pose_grad(inp["means3D"], g[3], g[4], g[1], inp["shs"], 3, inp["sh_indices"], None, inp["scales"],
                                       inp["rotations"], inp["scale_factors"], inp["g_indices"], 1.0, fw["geom"], fw["radii"], pose)

    def torch_route(g):
        return rasterizer.camera_pose_jacobian_sum(inp["means3D"], intr_d, pose, g[0][:, 0], g[0][:, 1])

    t = {k: [] for k in STAGES + ("torch_route", "backward_skipping", "backward_not_skipping")}
    _lib.profile_enable(True)
    for n in range(args.warmup + args.samples):
        fw = gpu_util.hip_forward(inp, cam, indexed)
        torch.cuda.synchronize()
        _lib.profile_read()
        g = backward(fw, ())
        exact = pose_grad(fw, g)
        torch.cuda.synchronize()
        st = _lib.profile_read()
        ref, ms_ref = _event_ms(lambda: torch_route(g))
        backward(fw, ("dL_dcolors", "dL_dcov3D"))
        torch.cuda.synchronize()
        st_skip = _lib.profile_read()
        if n < args.warmup:
            continue
        for k in STAGES:
            assert st[k][1] == 1, (k, st)
            t[k].append(st[k][0])
        t["torch_route"].append(ms_ref)
        t["backward_not_skipping"].append(sum(st[k][0] for k in BWD))
        t["backward_skipping"].append(sum(st_skip[k][0] for k in BWD))
    _lib.profile_enable(False)

    radii, g3, gcov, gcol = fw["radii"], g[3], g[4], g[1]
    vis = radii > 0
    nz_col = vis & (gcol != 0).any(1)
    nz = vis & ((g3 != 0).any(1) | (gcov != 0).any(1) | (gcol != 0).any(1))
    n_vis, n_nz, n_col = int(vis.sum()), int(nz.sum()), int(nz_col.sum())
    n_rows = (P + 255) // 256
    # radii for all; the three gradient rows of the visible; mean + g_index + scale factor + codebook row (rotation 16, scale 12) of
    # the rows with any gradient; clamp byte + sh_index + 192-byte SH row of those with a colour gradient; the rows written
    bytes_a = 4 * P + 48 * n_vis + (12 + 8 + 4 + 28) * n_nz + (1 + 8 + 192) * n_col + 96 * n_rows
    rate = copy_rate_gb_s(args.samples)
    out = {"device": torch.cuda.get_device_name(0), "samples": args.samples, "warmup": args.warmup,
           "scene": "bench: BASELINE.json configs[2], synth-v1, indexed", "P": P, "W": W, "H": H, "num_rendered": fw["num_rendered"],
           "gaussians_visible": n_vis, "gaussians_with_gradient": n_nz, "gaussians_with_colour_gradient": n_col,
           "method": "library stage times (stream events around the launches) for pose_grad and the backward's stages; the torch route "
                     "(camera_pose_jacobian_sum) between two stream events; medians",
           "pose_grad_exact": [float(v) for v in exact.tolist()], "pose_grad_reference_formula": [float(v) for v in ref.tolist()]}
    for k, v in t.items():
        out[k + "_ms"] = statistics.median(v)
        out[k + "_ms_min_max"] = [min(v), max(v)]
    out["unskip_cost_ms"] = out["backward_not_skipping_ms"] - out["backward_skipping_ms"]
    out["stage_a_bytes"] = bytes_a
    out["copy_rate_gb_s"] = rate
    out["stage_a_floor_ms"] = bytes_a / (rate * 1e9) * 1e3
    out["pose_grad_over_torch_route"] = out["pose_grad_ms"] / out["torch_route_ms"]
    out["exact_total_over_torch_route"] = (out["pose_grad_ms"] + out["unskip_cost_ms"]) / out["torch_route_ms"]
    out["expectation_below_torch_route"] = out["pose_grad_ms"] < out["torch_route_ms"]
    print(json.dumps(out))
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as fh:
            json.dump(out, fh, indent=1)


if __name__ == "__main__":
    main()
