#!/usr/bin/env python3
"""Times the 3D smoothing filter (csrc/filter3d.hip) in one process with stream events, medians of --samples with min-max,
and writes profiles/r19_filter3d_time.json.

    python tools/time_filter3d.py [--samples 20] [--warmup 5] [--P 3000000] [--out profiles/r19_filter3d_time.json]

compute: c3dgs_filter3d_compute (the library's stage time: the workspace clear and both kernels) at 1M / 3M / 6M rows x 100 and
300 cameras (tests/filter3d_ref.py: ring_scene) next to upstream's per-camera loop restated in torch ops on the same device
(filter3d_ref.upstream_loop; events around the whole loop). Reported: the ratio and the kernel's lane-operations per second
(rows x cameras / time). Expectation, derived and not measured beforehand: below that loop at every size.
apply: on the bench scene (BASELINE.json configs[2]: 3M Gaussians, 1920x1080, indexed) and the heavy-tailed one, per sample a plain
forward + backward through the indexed rasterizer module and then filter3d.apply, the forward on (Sigma', o'), its backward and
filter3d's backward, all as library stage times. Expectation: filter3d_apply below preprocess and filter3d_apply_backward below
backward_preprocess of the same pass (each does a subset of that neighbour's per-Gaussian work)."""
import argparse
import json
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def _event_ms(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b)


def _stat(out, key, vals):
    out[key + "_ms"] = statistics.median(vals)
    out[key + "_ms_min_max"] = [min(vals), max(vals)]


def time_compute(P, C, samples, warmup):
    from c3dgs_amd import _lib, filter3d
    from tests import filter3d_ref as ref
    xyz, table = ref.ring_scene(P, C, seed=1)
    xyz, table = torch.from_numpy(xyz).cuda(), torch.from_numpy(table).cuda()
    kernel, loop = [], []
    _lib.profile_enable(True, only="filter3d_compute")
    for n in range(warmup + samples):
        torch.cuda.synchronize()
        _lib.profile_read()
        f, seen = filter3d.compute(xyz, table)
        torch.cuda.synchronize()
        st = _lib.profile_read()["filter3d_compute"]
        assert st[1] == 1
        if n >= warmup:
            kernel.append(st[0])
    _lib.profile_enable(False)
    for n in range(2 + samples):
        ms = _event_ms(lambda: ref.upstream_loop(xyz, table))
        if n >= 2:
            loop.append(ms)
    up = ref.upstream_loop(xyz, table)
    out = {"P": P, "cameras": C, "seen_fraction": float(seen.float().mean()),
           "max_relative_difference_from_the_loop": float(((f - up).abs() / up).max())}
    _stat(out, "filter3d_compute", kernel)
    _stat(out, "upstream_loop_torch", loop)
    out["loop_over_kernel"] = out["upstream_loop_torch_ms"] / out["filter3d_compute_ms"]
    out["lane_operations_per_s"] = P * C / (out["filter3d_compute_ms"] * 1e-3)
    out["expectation_below_the_loop"] = out["filter3d_compute_ms"] < out["upstream_loop_torch_ms"]
    return out


class _Cam:
    def __init__(self, intrinsic, ev):
        self.intrinsic, self.extrinsic_vector = intrinsic.cuda(), ev.cuda()


def time_apply(label, inp, intr, ev, indexed, samples, warmup):
    import c3dgs_amd as hip
    from c3dgs_amd import _lib, filter3d
    assert indexed
    inp = {k: (v.cuda() if isinstance(v, torch.Tensor) else v) for k, v in inp.items()}
    P = int(inp["means3D"].shape[0])
    W, H = int(intr[0, 2]), int(intr[1, 2])
    rs = hip.GaussianRasterizationSettings(intrinsic=intr.cuda(), extrinsic_vector=ev.cuda(), bg=inp["bg"].cuda(),
                                           scale_modifier=float(inp.get("scale_modifier", 1.0)), sh_degree=int(inp["degree"]),
                                           prefiltered=False, debug=False, clamp_color=bool(inp["clamp_color"]))
    f, seen = filter3d.compute(inp["means3D"], filter3d.camera_table([_Cam(intr, ev)], "cuda"))
    dL = torch.ones((3, H, W), dtype=torch.float32, device="cuda")
    names = ("means3D", "opacities", "shs", "scales", "rotations", "scale_factors")
    rast = hip.GaussianRasterizerIndexed(rs)

    def run(filtered):
        lv = {k: inp[k].detach().clone().requires_grad_() for k in names}
        kw = dict(means3D=lv["means3D"], means2D=torch.zeros_like(lv["means3D"], requires_grad=True), shs=lv["shs"],
                  sh_indices=inp["sh_indices"], g_indices=inp["g_indices"], extrinsic_vector=ev.cuda())
        if filtered:
            cov, o = filter3d.apply(lv["opacities"], lv["scales"], lv["rotations"], f, rs.scale_modifier,
                                    scale_factors=lv["scale_factors"], g_indices=inp["g_indices"])
            out = rast(opacities=o, cov3D_precomp=cov, **kw)
        else:
            out = rast(opacities=lv["opacities"], scales=lv["scales"], rotations=lv["rotations"], scale_factors=lv["scale_factors"], **kw)
        (out[0] * dL).sum().backward()

    total = lambda st: sum(ms for ms, _ in st.values())       # noqa: E731
    keys = ("filter3d_apply", "filter3d_apply_backward", "preprocess", "backward_preprocess", "preprocess_plain",
            "backward_preprocess_plain", "forward_backward_plain", "forward_backward_filtered")
    t = {k: [] for k in keys}
    _lib.profile_enable(True)
    for n in range(warmup + samples):
        torch.cuda.synchronize()
        _lib.profile_read()
        run(False)
        torch.cuda.synchronize()
        plain = _lib.profile_read()
        run(True)
        torch.cuda.synchronize()
        filt = _lib.profile_read()
        if n < warmup:
            continue
        assert not [k for k in plain if k.startswith("filter3d")]
        for k in keys[:4]:
            assert filt[k][1] == 1, (k, filt)
            t[k].append(filt[k][0])
        t["preprocess_plain"].append(plain["preprocess"][0])
        t["backward_preprocess_plain"].append(plain["backward_preprocess"][0])
        t["forward_backward_plain"].append(total(plain))
        t["forward_backward_filtered"].append(total(filt))
    _lib.profile_enable(False)
    out = {"scene": label, "P": P, "W": W, "H": H, "seen_fraction": float(seen.float().mean()), "filter_median": float(f.median())}
    for k, vals in t.items():
        _stat(out, k, vals)
    out["added_by_the_filter_ms"] = out["forward_backward_filtered_ms"] - out["forward_backward_plain_ms"]
    out["expectation_filter3d_apply_below_preprocess"] = out["filter3d_apply_ms"] < out["preprocess_ms"]
    out["expectation_filter3d_apply_backward_below_backward_preprocess"] = out["filter3d_apply_backward_ms"] < out["backward_preprocess_ms"]
    torch.cuda.empty_cache()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--samples", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--P", type=int, default=3_000_000)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r19_filter3d_time.json"))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("time_filter3d.py needs the GPU; a timing taken anywhere else says nothing")
    from tests import fullsize
    from tools.time_contrib import heavy_tail_inputs
    compute = [time_compute(P, C, args.samples, args.warmup) for P in (1_000_000, 3_000_000, 6_000_000) for C in (100, 300)]
    scenes = [time_apply("bench: BASELINE.json configs[2], synth-v1, indexed", *fullsize.config_inputs("config3_3M_indexed", P=args.P),
                         args.samples, args.warmup),
              time_apply("heavy_tail: synth-v1 with scale = exp(N(log 0.009, 1.2^2)) per axis, indexed",
                         *heavy_tail_inputs(args.P, 1920, 1080, 1200.0), args.samples, args.warmup)]
    out = {"device": torch.cuda.get_device_name(0), "samples": args.samples, "warmup": args.warmup,
           "method": "one process; library stage times (stream events around the launches) for every kernel, stream events around the "
                     "whole torch loop for the baseline; medians with min-max. compute: tests/filter3d_ref.py ring_scene, points "
                     "uniform in +-3, cameras on a ring of radius 4. apply: per sample a plain forward + backward through the indexed "
                     "rasterizer module, then the same through filter3d.apply and cov3D_precomp; forward_backward_* = the sum of every "
                     "stage of the pass; the filter is that of the scene's own camera",
           "compute": compute, "apply": scenes}
    print(json.dumps(out))
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as fh:
            json.dump(out, fh, indent=1)


if __name__ == "__main__":
    main()
