#!/usr/bin/env python3
"""Times the two kernels of the antialiased mode (csrc/aa_opacity.hip: c3dgs_aa_opacity in front of the forward,
c3dgs_aa_opacity_backward behind the backward) on the bench scene -- BASELINE.json configs[2]: 3M Gaussians, 1920x1080, indexed --
and on bench.py's heavy-tailed scene (scale sigma 1.2), against the per-Gaussian stages next to them in the same run. Prints one
JSON line and writes profiles/r16_antialiasing_time.json.

    python tools/time_antialiasing.py [--samples 20] [--warmup 5] [--P 3000000] [--out profiles/r16_antialiasing_time.json]

All figures are the library's stage times (c3dgs_profile_*: two stream events around the launches). One sample = the plain
forward and backward on the raw opacities, then aa_opacity, the forward on o', its backward and aa_opacity_backward, on one stream
in one process. Medians of `samples` samples after `warmup` unrecorded ones, with min and max. The expectation to read the
figures against is derived, not measured: each new kernel does a subset of its neighbour's per-Gaussian work (no SH, no colour,
no conic, no radius), so aa_opacity < preprocess and aa_opacity_backward < backward_preprocess in the same run. Each new kernel's
requested bytes and the time of streaming them at the process's own copy rate are reported beside its time."""
import argparse
import json
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

STAGES = ("aa_opacity", "aa_opacity_backward", "preprocess", "backward_preprocess")


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


def time_scene(label, inp, intr, ev, indexed, samples, warmup, rate):
    from c3dgs_amd import _lib, rasterizer
    from oracle import oracle as orc
    from tests import gpu_util
    assert indexed
    cam = orc.camera(intr.numpy(), ev.numpy())
    inp = {k: (v.cuda() if isinstance(v, torch.Tensor) else v) for k, v in inp.items()}     # uploaded once, not per sample
    W, H = cam["W"], cam["H"]
    P = int(inp["means3D"].shape[0])
    dL = torch.ones((3, H, W), dtype=torch.float32, device="cuda")
    view = torch.from_numpy(cam["viewmatrix"]).cuda()
    proj_in = (inp["scales"], inp["rotations"], inp["scale_factors"], inp["g_indices"], None, float(inp.get("scale_modifier", 1.0)), view,
               cam["tan_fovx"], cam["tan_fovy"], H, W)

    def backward(fw):
        (bg, means3D, colors, opac, scales, sf, rot, smod, cov3D, view_, proj, tfx, tfy, H_, W_, sh, deg, campos, shi, gi, pre, dbg,
         clamp) = fw["args"]
        return rasterizer._C.rasterize_gaussians_backward_indexed(bg, means3D, fw["radii"], colors, scales, sf, rot, smod, cov3D, view_,
                                                                  proj, tfx, tfy, dL, sh, deg, campos, fw["geom"], fw["num_rendered"],
                                                                  fw["binning"], fw["img"], False, shi, gi,
                                                                  skip=("dL_dcolors", "dL_dcov3D"))

    def total(st):
        return sum(ms for ms, _ in st.values())

    t = {k: [] for k in STAGES + ("preprocess_plain", "backward_preprocess_plain", "forward_backward_plain", "forward_backward_antialiased")}
    _lib.profile_enable(True)
    for n in range(warmup + samples):
        torch.cuda.synchronize()
        _lib.profile_read()
        fw = gpu_util.hip_forward(inp, cam, indexed)
        backward(fw)
        torch.cuda.synchronize()
        plain = _lib.profile_read()
        o_aa, _ = rasterizer._C.aa_opacity(inp["means3D"], inp["opacities"], *proj_in, rho=False)
        fa = gpu_util.hip_forward(dict(inp, opacities=o_aa), cam, indexed)
        g = backward(fa)
        rasterizer._C.aa_opacity_backward(inp["means3D"], inp["opacities"], fa["radii"], *proj_in, g[2], dL_dmeans3D=g[3],
                                          dL_dscales=g[6], dL_drotations=g[8], dL_dscale_factors=g[7])
        torch.cuda.synchronize()
        aa = _lib.profile_read()
        if n < warmup:
            continue
        for k in STAGES:
            assert aa[k][1] == 1, (k, aa)
            t[k].append(aa[k][0])
        assert not [k for k in plain if k.startswith("aa_")]
        t["preprocess_plain"].append(plain["preprocess"][0])
        t["backward_preprocess_plain"].append(plain["backward_preprocess"][0])
        t["forward_backward_plain"].append(total(plain))
        t["forward_backward_antialiased"].append(total(aa))
    _lib.profile_enable(False)
    n_vis = int((fa["radii"] > 0).sum())
    # forward, per Gaussian: mean 12 + opacity 4 + g_index 8 + scale factor 4 + codebook row (rotation 16, scale 12) + o' 4
    bytes_fwd = 60 * P
    n_grad = int(((fa["radii"] > 0) & (g[2].reshape(-1) != 0)).sum())        # rho > 0: rho g' is zero where g' was
    # backward: radii for all; dL_dopacity read for the visible; per Gaussian with an opacity gradient the forward's 56 bytes of
    # inputs, dL_dopacity written, dL_dmeans3D and dL_dscale_factors read and written (4 + 24 + 8) and the codebook gradient row
    # added (28)
    bytes_bwd = 4 * P + 4 * n_vis + (56 + 36 + 28) * n_grad
    out = {"scene": label, "P": P, "W": W, "H": H, "num_rendered_plain": fw["num_rendered"], "num_rendered_antialiased": fa["num_rendered"],
           "gaussians_visible": n_vis, "gaussians_with_opacity_gradient": n_grad}
    for k, vals in t.items():
        out[k + "_ms"] = statistics.median(vals)
        out[k + "_ms_min_max"] = [min(vals), max(vals)]
    out["added_by_the_flag_ms"] = out["forward_backward_antialiased_ms"] - out["forward_backward_plain_ms"]
    out["aa_opacity_bytes"], out["aa_opacity_bytes_per_gaussian"] = bytes_fwd, bytes_fwd / P
    out["aa_opacity_floor_ms"] = bytes_fwd / (rate * 1e9) * 1e3
    out["aa_opacity_backward_bytes"], out["aa_opacity_backward_bytes_per_gaussian"] = bytes_bwd, bytes_bwd / P
    out["aa_opacity_backward_floor_ms"] = bytes_bwd / (rate * 1e9) * 1e3
    out["expectation_aa_opacity_below_preprocess"] = out["aa_opacity_ms"] < out["preprocess_ms"]
    out["expectation_aa_opacity_backward_below_backward_preprocess"] = out["aa_opacity_backward_ms"] < out["backward_preprocess_ms"]
    del inp, fw, fa, g
    torch.cuda.empty_cache()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--samples", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--P", type=int, default=3_000_000)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r16_antialiasing_time.json"))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("time_antialiasing.py needs the GPU; a timing taken anywhere else says nothing")
    from tests import fullsize
    from tools.time_contrib import heavy_tail_inputs
    rate = copy_rate_gb_s(args.samples)
    scenes = []
    scenes.append(time_scene("bench: BASELINE.json configs[2], synth-v1, indexed", *fullsize.config_inputs("config3_3M_indexed", P=args.P),
                             args.samples, args.warmup, rate))
    scenes.append(time_scene("heavy_tail: synth-v1 with scale = exp(N(log 0.009, 1.2^2)) per axis, indexed",
                             *heavy_tail_inputs(args.P, 1920, 1080, 1200.0), args.samples, args.warmup, rate))
    out = {"device": torch.cuda.get_device_name(0), "samples": args.samples, "warmup": args.warmup, "copy_rate_gb_s": rate,
           "method": "library stage times (stream events around the launches); per sample the plain forward and backward on the raw "
                     "opacities, then aa_opacity, the forward on its o', the backward and aa_opacity_backward, on one stream; medians; "
                     "preprocess / backward_preprocess are those of the antialiased pass (the *_plain ones of the other); "
                     "forward_backward_* = the sum of every stage of the pass; floors = requested bytes at the process's copy rate",
           "scenes": scenes}
    print(json.dumps(out))
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as fh:
            json.dump(out, fh, indent=1)


if __name__ == "__main__":
    main()
