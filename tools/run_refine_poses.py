#!/usr/bin/env python3
"""Runs c3dgs_amd.pipeline.refine_poses on the toy scene of tests/train_scene.py (tests/pose_ref.py:refine_problem: the teacher
as an indexed model, eight views 160x112, two cameras' poses moved by 0.02 N(0, 1) per element) once with the exact pose
gradient and once with the reference's formula, from the same start, and prints one JSON line: per camera first and last loss,
starting and final distance to the true pose (tests/pose_ref.py:pose_distance: camera centre + scale-free rotation; the raw
7-vector distance, which contains a common scale of R and t that no image can see, is listed beside it), their ratios, and
seconds per run.

    python tools/run_refine_poses.py [--iterations 200] [--lr 1e-3] [--noise 0.02] [--out profiles/r13_refine_poses.json]"""
import argparse
import json
import os
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def run(mode, iterations, lr, noise):
    from c3dgs_amd import pipeline
    from c3dgs_amd.model import PipelineParams
    from tests import pose_ref
    model, cams, true = pose_ref.refine_problem(noise=noise)
    idx = sorted(true)
    start = [pose_ref.pose_distance(cams[k].extrinsic_vector, true[k]) for k in idx]
    raw_start = [float((cams[k].extrinsic_vector - true[k]).norm()) for k in idx]
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    res = pipeline.refine_poses(cams, model, PipelineParams(), torch.zeros(3, device="cuda"), iterations, lr=lr, cameras=idx,
                                pose_grad=mode)
    torch.cuda.synchronize()
    seconds = time.perf_counter() - t0
    end = [pose_ref.pose_distance(cams[k].extrinsic_vector, true[k]) for k in idx]
    raw_end = [float((cams[k].extrinsic_vector.detach() - true[k]).norm()) for k in idx]
    return {"cameras": idx, "loss_first": [r[0] for r in res], "loss_last": [r[1] for r in res],
            "loss_ratio": [r[1] / r[0] for r in res], "pose_distance_start": start, "pose_distance_end": end,
            "pose_distance_ratio": [e / s for e, s in zip(end, start)],
            "raw_7_vector_distance_start": raw_start, "raw_7_vector_distance_end": raw_end, "seconds": seconds}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iterations", type=int, default=200)
    ap.add_argument("--lr", type=float, default=1e-3)
    ap.add_argument("--noise", type=float, default=0.02)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("run_refine_poses.py needs the GPU; there is no CPU path")
    out = {"scene": "tests/pose_ref.py:refine_problem: 4000-Gaussian synth-v1 teacher of tests/train_scene.py, indexed, 8 views 160x112",
           "iterations": args.iterations, "lr": args.lr, "noise": args.noise,
           "exact": run("exact", args.iterations, args.lr, args.noise),
           "reference": run("reference", args.iterations, args.lr, args.noise)}
    print(json.dumps(out))
    if args.out:
        with open(args.out, "w") as f:
            json.dump(out, f, indent=1)


if __name__ == "__main__":
    main()
