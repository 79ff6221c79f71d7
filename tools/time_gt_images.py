#!/usr/bin/env python3
"""Times the ground-truth image kernel (csrc/image_io.hip, c3dgs_image_from_u8) against the same sequence written with torch
ops on the same device from the same device bytes, and, at one size, against the host path a save_memory loop of the
reference's design pays per access. Prints one JSON line and writes profiles/r09_gt_images_time.json.

    python tools/time_gt_images.py [--samples 20] [--reps 10] [--out profiles/r09_gt_images_time.json]

A sample is the time between two stream events around `reps` back-to-back calls, divided by `reps`; the figure of a side is the
median of `samples` samples after a warm-up, and the two sides alternate sample by sample within one run. Kernel bytes/s is
over the algorithmic bytes: the source footprint read once plus 12 B per output pixel. The host figure is measured at one
size only and is not extrapolated to the others."""
import argparse
import json
import os
import statistics
import sys
import tempfile
import time

import numpy as np
import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

# (name, Hs, Ws, C, Hd, Wd)
CASES = (("1600x1063 RGB, same size", 1063, 1600, 3, 1063, 1600),
         ("4946x3286 RGB -> 1600x1063", 3286, 4946, 3, 1063, 1600),
         ("800x800 RGBA, same size", 800, 800, 4, 800, 800))
HOST_CASE = 0


def torch_sequence(src, Hd, Wd, flip=False):
    """to(float) / 255, alpha, flip, permute, bilinear resize (half-pixel centres, no antialiasing), clamp."""
    x = src.to(torch.float32) / 255
    if x.shape[2] == 4:
        x = x[:, :, :3] * x[:, :, 3:4]
    if flip:
        x = x.flip(0, 1)
    x = x.permute(2, 0, 1)[None]
    x = F.interpolate(x, size=(Hd, Wd), mode="bilinear", align_corners=False, antialias=False)
    return x[0].clamp(0.0, 1.0)


def sample(fn, reps):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(reps):
        fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) * 1e3 / reps            # microseconds per call


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--samples", type=int, default=20)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r09_gt_images_time.json"))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("time_gt_images.py needs the GPU; a timing taken anywhere else says nothing")
    from c3dgs_amd import image_io
    from tests import image_ref, scene_fixture
    rows = []
    for k, (name, Hs, Ws, C, Hd, Wd) in enumerate(CASES):
        host = scene_fixture.pattern(Hs, Ws, seed=k, alpha=C == 4)
        src = torch.from_numpy(host).to("cuda")
        out = torch.empty((3, Hd, Wd), dtype=torch.float32, device="cuda")
        fused = lambda: image_io.image_from_u8(src, Hd, Wd, out=out)          # noqa: E731
        eager = lambda: torch_sequence(src, Hd, Wd)                            # noqa: E731
        for _ in range(3):
            fused(), eager()
        torch.cuda.synchronize()
        diff = float((fused() - eager()).abs().max())
        t_fused, t_eager = [], []
        for _ in range(args.samples):                                          # the two sides alternate
            t_fused.append(sample(fused, args.reps))
            t_eager.append(sample(eager, args.reps))
        us_f, us_e = statistics.median(t_fused), statistics.median(t_eager)
        algo = Hs * Ws * C + 12 * Hd * Wd
        row = {"case": name, "src": [Hs, Ws, C], "dst": [Hd, Wd], "algorithmic_bytes": algo,
               "fused_us": us_f, "fused_us_min_max": [min(t_fused), max(t_fused)], "fused_GBps": algo / us_f * 1e-3,
               "torch_us": us_e, "torch_us_min_max": [min(t_eager), max(t_eager)], "torch_over_fused": us_e / us_f,
               "max_abs_diff_fused_vs_torch": diff}
        if k == HOST_CASE:
            with tempfile.TemporaryDirectory() as tmp:
                path = os.path.join(tmp, "view.png")
                scene_fixture.write_png(path, host)
                t = []
                for _ in range(3):
                    t0 = time.perf_counter()
                    img = torch.from_numpy(image_ref.image_from_u8(image_io.decode_u8(path), Hd, Wd)).to("cuda")
                    torch.cuda.synchronize()
                    t.append((time.perf_counter() - t0) * 1e6)
                row["host_decode_numpy_upload_us"] = statistics.median(t)
                row["host_matches_fused_bit_for_bit"] = bool(torch.equal(img, fused()))
        rows.append(row)
    out = {"device": torch.cuda.get_device_name(0), "samples": args.samples, "reps_per_sample": args.reps,
           "method": "median over samples of (stream-event time around reps back-to-back calls) / reps; sides alternate per sample",
           "cases": rows}
    print(json.dumps(out))
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(out, f, indent=1)


if __name__ == "__main__":
    main()
