#!/usr/bin/env python3
"""Optimises the synthetic point-cloud scene of tests/train_scene.py with c3dgs_amd.pipeline.train, once with adaptive density
control and once with densify_until_iter = 0, and prints one JSON line: Gaussian counts, mean PSNR over the training views
before / after, and seconds per phase.

    python tools/run_train.py [--iterations 400] [--out profiles/r06_train_synth.json]
                              [--densify-by grad|error] [--error-threshold T] [--optimizer default|sparse_adam]
                              [--lambda-depth X] [--lambda-alpha Y]

--densify-by error (with --error-threshold, which has no default) lets the run with density control densify by image error
(pipeline.train(densify_by="error")); the JSON then carries "densify_by" and "error_threshold".
--optimizer sparse_adam runs both with optim.SparseGaussianAdam stepping only the rows with radii > 0
(pipeline.train(optimizer_type="sparse_adam")); the JSON then carries "optimizer".
--lambda-depth X / --lambda-alpha Y (either positive) attach the teacher's own maps to the cameras -- alpha_target = its alpha,
depth_target = its depth / alpha where alpha > 0.5, else 0 -- and run pipeline.train(lambda_depth=X, lambda_alpha=Y); both runs
are then also made WITHOUT the two terms ("without_map_terms"), and every run carries "depth_l1" and "alpha_l1": the mean over
the views of mean |depth - teacher depth| and mean |alpha - teacher alpha| of the trained student (sum alpha T z, not normalised)."""
import argparse
import json
import os
import sys
import tempfile
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from tests import train_scene  # noqa: E402


def teacher_maps(cams):
    """-> [(depth, alpha)] of the teacher per camera (train_scene.make's teacher: the same seed and size)"""
    from c3dgs_amd.model import PipelineParams
    teacher, _ = train_scene.teacher_model(4000, 160, 112, 150.0, "cuda")
    bg = torch.zeros(3, device="cuda")
    with torch.no_grad():
        outs = [teacher.render(cam, PipelineParams(), bg, return_depth=True) for cam in cams]
    return [(o["depth"].clone(), o["alpha"].clone()) for o in outs]


def map_l1(student, cams, maps):
    from c3dgs_amd.model import PipelineParams
    bg = torch.zeros(3, device="cuda")
    d, a = [], []
    with torch.no_grad():
        for cam, (depth, alpha) in zip(cams, maps):
            o = student.render(cam, PipelineParams(), bg, return_depth=True)
            d.append(float((o["depth"] - depth).abs().mean()))
            a.append(float((o["alpha"] - alpha).abs().mean()))
    return sum(d) / len(d), sum(a) / len(a)


def run(iterations, densify, densify_by="grad", error_threshold=None, optimizer="default", lambda_depth=0.0, lambda_alpha=0.0,
        with_maps=False):
    from c3dgs_amd import pipeline
    from c3dgs_amd.model import PipelineParams
    with tempfile.TemporaryDirectory() as tmp:
        t0 = time.perf_counter()
        student, cams, extent = train_scene.make(tmp)
        torch.cuda.synchronize()
        t_setup = time.perf_counter() - t0
    extra = {}
    if with_maps:
        maps = teacher_maps(cams)
        for cam, (depth, alpha) in zip(cams, maps):
            cam.alpha_target, cam.depth_target = alpha, (depth / alpha.clamp(min=1e-6)) * (alpha > 0.5)
        extra = dict(lambda_depth=lambda_depth, lambda_alpha=lambda_alpha)
    rows0, before = student._xyz.shape[0], train_scene.mean_psnr(student, cams)
    events = []

    class Scene:
        gaussians = student
        cameras_extent = extent

        def getTrainCameras(self):
            return cams

    torch.manual_seed(0)
    t0 = time.perf_counter()
    n = pipeline.train(Scene(), None, train_scene.schedule(iterations, densify), PipelineParams(), camera_stride=1, degree_up_iter=80,
                       log=lambda epoch, info: events.append((epoch, info)), densify_by=densify_by, error_threshold=error_threshold,
                       optimizer_type=optimizer, **extra)
    torch.cuda.synchronize()
    t_train = time.perf_counter() - t0
    t0 = time.perf_counter()
    after = train_scene.mean_psnr(student, cams)
    t_eval = time.perf_counter() - t0
    out = {"iterations": n, "gaussians_before": rows0, "gaussians_after": student._xyz.shape[0], "psnr_before": before,
           "psnr_after": after, "densifications": [[e, i["densified"][0], list(i["densified"][1])] for e, i in events if i["densified"]],
           "opacity_resets": [e for e, i in events if i["reset_opacity"]],
           "seconds": {"setup": t_setup, "train": t_train, "eval": t_eval}}
    if with_maps:
        out["depth_l1"], out["alpha_l1"] = map_l1(student, cams, maps)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iterations", type=int, default=400)
    ap.add_argument("--out", default=None)
    ap.add_argument("--densify-by", choices=("grad", "error"), default="grad")
    ap.add_argument("--error-threshold", type=float, default=None)
    ap.add_argument("--optimizer", choices=("default", "sparse_adam"), default="default")
    ap.add_argument("--lambda-depth", type=float, default=0.0)
    ap.add_argument("--lambda-alpha", type=float, default=0.0)
    args = ap.parse_args()
    if args.densify_by == "error" and args.error_threshold is None:
        ap.error("--densify-by error needs --error-threshold (there is no default)")
    if not torch.cuda.is_available():
        raise SystemExit("run_train.py needs the GPU; there is no CPU path")
    out = {"scene": "tests/train_scene.py: 4000-Gaussian synth-v1 teacher, 8 views 160x112, student = every 8th position as a point cloud"}
    terms = args.lambda_depth > 0 or args.lambda_alpha > 0
    kw = dict(lambda_depth=args.lambda_depth, lambda_alpha=args.lambda_alpha, with_maps=True) if terms else {}
    out["with_density_control"] = run(args.iterations, True, args.densify_by, args.error_threshold, args.optimizer, **kw)
    out["densify_until_iter_0"] = run(args.iterations, False, optimizer=args.optimizer, **kw)
    if terms:
        out["lambda_depth"], out["lambda_alpha"] = args.lambda_depth, args.lambda_alpha
        none = dict(lambda_depth=0.0, lambda_alpha=0.0, with_maps=True)
        out["without_map_terms"] = {"with_density_control": run(args.iterations, True, args.densify_by, args.error_threshold,
                                                                args.optimizer, **none),
                                    "densify_until_iter_0": run(args.iterations, False, optimizer=args.optimizer, **none)}
    if args.densify_by != "grad":
        out["densify_by"], out["error_threshold"] = args.densify_by, args.error_threshold
    if args.optimizer != "default":
        out["optimizer"] = args.optimizer
    print(json.dumps(out))
    if args.out:
        with open(args.out, "w") as f:
            json.dump(out, f, indent=1)


if __name__ == "__main__":
    main()
