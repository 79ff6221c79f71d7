#!/usr/bin/env python3
"""Optimises the synthetic point-cloud scene of tests/train_scene.py with c3dgs_amd.pipeline.train, once with adaptive density
control and once with densify_until_iter = 0, and prints one JSON line: Gaussian counts, mean PSNR over the training views
before / after, and seconds per phase.

    python tools/run_train.py [--iterations 400] [--out profiles/r06_train_synth.json]
                              [--densify-by grad|error] [--error-threshold T] [--optimizer default|sparse_adam]
                              [--lambda-depth X] [--lambda-alpha Y] [--antialiasing] [--filter-3d [--filter-3d-interval N]]
                              [--strategy default|mcmc] [--cap-max N] [--noise-lr X]
                              [--bilagrid L HG WG | --exposure] [--bilagrid-lr X] [--bilagrid-tv Y] [--exposure-jitter S]

--densify-by error (with --error-threshold, which has no default) lets the run with density control densify by image error
(pipeline.train(densify_by="error")); the JSON then carries "densify_by" and "error_threshold".
--optimizer sparse_adam runs both with optim.SparseGaussianAdam stepping only the rows with radii > 0
(pipeline.train(optimizer_type="sparse_adam")); the JSON then carries "optimizer".
--lambda-depth X / --lambda-alpha Y (either positive) attach the teacher's own maps to the cameras -- alpha_target = its alpha,
depth_target = its depth / alpha where alpha > 0.5, else 0 -- and run pipeline.train(lambda_depth=X, lambda_alpha=Y); both runs
are then also made WITHOUT the two terms ("without_map_terms"), and every run carries "depth_l1" and "alpha_l1": the mean over
the views of mean |depth - teacher depth| and mean |alpha - teacher alpha| of the trained student (sum alpha T z, not normalised).
--antialiasing makes the run without density control twice, with PipelineParams(antialiasing=False) and (True), at the scene's
resolution, and scores each trained student with metrics.render_and_eval (under the pipe it was trained with) at 0.5x, 1x and 2x
that resolution, same poses, focal length scaled. The targets there are the teacher rendered at 4x the evaluated resolution by
the plain rasterizer and box-filtered down 4 x 4 ("resolution_eval"); "train_views_1x" is the score against the training images
themselves. One run each, nothing tuned; the JSON then carries "antialiasing" in place of the two default runs.
--strategy mcmc --cap-max N [--noise-lr X] makes ONE run with pipeline.train(strategy="mcmc", cap_max=N) (relocation, growth
by 5 % up to N rows, position noise; csrc/mcmc.hip) in place of the two default runs; the JSON carries "strategy", "cap_max",
"noise_lr" and under "mcmc" the run with its (epoch, relocated, added) refinements.
--bilagrid L HG WG (or --exposure, which is --bilagrid 1 1 1) [--bilagrid-lr X] [--bilagrid-tv Y] trains one bilateral grid per
camera next to the model (pipeline.train(bilagrid=(L, HG, WG)); csrc/bilagrid.hip). --exposure-jitter S, for the demonstration
only, replaces every training image by a_k * image + b_k with per-camera, per-channel a in [1 - S, 1 + S] and b in
[-S / 4, S / 4] from a seeded generator (tests/bilagrid_ref.py jitter_exposure). With any of them ONE run is made, without
density control, in place of the two default runs; the JSON carries "bilagrid" (the shape or null), "exposure_jitter" and under
"run" the run: "final_loss" (the mean loss over the last epoch, which every run reports), "psnr_after" as always (the RAW render against the
training images as they were trained on, jittered or not) and, here only, "psnr_vs_clean_images" (the raw render against the
teacher's own images; it carries a global gain ambiguity that only a colour-corrected metric would remove).
--filter-3d [--filter-3d-interval N] makes the run without density control four times -- plain, PipelineParams(antialiasing=True),
pipeline.train(filter_3d=True, filter_3d_interval=N) (the 3D smoothing filter, csrc/filter3d.hip) and both -- and scores each
trained student at 0.5x, 1x and 2x as --antialiasing does (the student keeps its filter for the evaluation). One run each,
nothing tuned; the JSON carries "filter_3d" in place of the two default runs."""
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


def resolution_eval(student, cams, pipe):
    """-> {"0.5x" | "1x" | "2x": render_and_eval's dict against the 4x supersampled, box-filtered teacher, "train_views_1x": against
    the training images}"""
    from c3dgs_amd import metrics
    from c3dgs_amd.model import PipelineParams
    from tests import synth
    W, H, focal = 160, 112, 150.0
    teacher, _ = train_scene.teacher_model(4000, W, H, focal, "cuda")
    bg = torch.zeros(3, device="cuda")
    out = {"train_views_1x": metrics.render_and_eval(student, cams, pipe, bg)}
    for label, s in (("0.5x", 0.5), ("1x", 1.0), ("2x", 2.0)):
        views = []
        for cam in cams:
            ev = tuple(cam.extrinsic_vector.detach().cpu().tolist())
            view = train_scene.Cam(*synth.camera(int(W * s), int(H * s), focal * s, extrinsic_vector=ev), "cuda")
            fine = train_scene.Cam(*synth.camera(int(W * s) * 4, int(H * s) * 4, focal * s * 4, extrinsic_vector=ev), "cuda")
            with torch.no_grad():
                big = teacher.render(fine, PipelineParams(), bg)["render"].clamp(0, 1)
                view.original_image = torch.nn.functional.avg_pool2d(big[None], 4)[0].contiguous()
            views.append(view)
        out[label] = metrics.render_and_eval(student, views, pipe, bg)
    return out


def run(iterations, densify, densify_by="grad", error_threshold=None, optimizer="default", lambda_depth=0.0, lambda_alpha=0.0,
        with_maps=False, antialiasing=None, mcmc=None, bilagrid=None, jitter=0.0, filter_3d=None):
    from c3dgs_amd import pipeline
    from c3dgs_amd.model import PipelineParams
    with tempfile.TemporaryDirectory() as tmp:
        t0 = time.perf_counter()
        student, cams, extent = train_scene.make(tmp)
        torch.cuda.synchronize()
        t_setup = time.perf_counter() - t0
    extra = dict(bilagrid or {}, **(filter_3d or {}))
    clean = [cam.original_image.clone() for cam in cams]
    if jitter:
        from tests import bilagrid_ref
        bilagrid_ref.jitter_exposure(cams, jitter)
    if with_maps:
        maps = teacher_maps(cams)
        for cam, (depth, alpha) in zip(cams, maps):
            cam.alpha_target, cam.depth_target = alpha, (depth / alpha.clamp(min=1e-6)) * (alpha > 0.5)
        extra.update(lambda_depth=lambda_depth, lambda_alpha=lambda_alpha)
    rows0, before = student._xyz.shape[0], train_scene.mean_psnr(student, cams)
    events = []

    class Scene:
        gaussians = student
        cameras_extent = extent

        def getTrainCameras(self):
            return cams

    torch.manual_seed(0)
    t0 = time.perf_counter()
    pipe = PipelineParams(antialiasing=bool(antialiasing))
    n = pipeline.train(Scene(), None, train_scene.schedule(iterations, densify), pipe, camera_stride=1, degree_up_iter=80,
                       log=lambda epoch, info: events.append((epoch, info)), densify_by=densify_by, error_threshold=error_threshold,
                       optimizer_type=optimizer, **extra, **(mcmc or {}))
    torch.cuda.synchronize()
    t_train = time.perf_counter() - t0
    t0 = time.perf_counter()
    after = train_scene.mean_psnr(student, cams)
    t_eval = time.perf_counter() - t0
    out = {"iterations": n, "gaussians_before": rows0, "gaussians_after": student._xyz.shape[0], "psnr_before": before,
           "psnr_after": after, "densifications": [[e, i["densified"][0], list(i["densified"][1])] for e, i in events if i["densified"]],
           "opacity_resets": [e for e, i in events if i["reset_opacity"]],
           "seconds": {"setup": t_setup, "train": t_train, "eval": t_eval}}
    out["final_loss"] = events[-1][1]["epoch_loss"]           # the mean loss over the last epoch
    if bilagrid is not None or jitter:
        trained_on = [cam.original_image for cam in cams]
        for cam, img in zip(cams, clean):
            cam.original_image = img
        out["psnr_vs_clean_images"] = train_scene.mean_psnr(student, cams)
        for cam, img in zip(cams, trained_on):
            cam.original_image = img
    if mcmc:
        out["refinements"] = [[e, i["mcmc"][0], i["mcmc"][1]] for e, i in events if i.get("mcmc")]
    if with_maps:
        out["depth_l1"], out["alpha_l1"] = map_l1(student, cams, maps)
    if antialiasing is not None:
        out["resolution_eval"] = resolution_eval(student, cams, pipe)
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
    ap.add_argument("--antialiasing", action="store_true")
    ap.add_argument("--strategy", choices=("default", "mcmc"), default="default")
    ap.add_argument("--cap-max", type=int, default=None)
    ap.add_argument("--noise-lr", type=float, default=5e5)
    ap.add_argument("--bilagrid", type=int, nargs=3, metavar=("L", "HG", "WG"), default=None)
    ap.add_argument("--exposure", action="store_true")
    ap.add_argument("--bilagrid-lr", type=float, default=2e-3)
    ap.add_argument("--bilagrid-tv", type=float, default=10.0)
    ap.add_argument("--exposure-jitter", type=float, default=0.0)
    ap.add_argument("--filter-3d", action="store_true")
    ap.add_argument("--filter-3d-interval", type=int, default=100)
    args = ap.parse_args()
    if args.exposure and args.bilagrid is not None:
        ap.error("--exposure is --bilagrid 1 1 1; give one of the two")
    if args.densify_by == "error" and args.error_threshold is None:
        ap.error("--densify-by error needs --error-threshold (there is no default)")
    if args.strategy == "mcmc" and args.cap_max is None:
        ap.error("--strategy mcmc needs --cap-max (there is no default)")
    if not torch.cuda.is_available():
        raise SystemExit("run_train.py needs the GPU; there is no CPU path")
    out = {"scene": "tests/train_scene.py: 4000-Gaussian synth-v1 teacher, 8 views 160x112, student = every 8th position as a point cloud"}
    if args.antialiasing and not args.filter_3d:
        out["antialiasing"] = {"off": run(args.iterations, False, optimizer=args.optimizer, antialiasing=False),
                               "on": run(args.iterations, False, optimizer=args.optimizer, antialiasing=True)}
        print(json.dumps(out))
        if args.out:
            with open(args.out, "w") as f:
                json.dump(out, f, indent=1)
        return
    if args.filter_3d:
        f3 = dict(filter_3d=True, filter_3d_interval=args.filter_3d_interval)
        out["filter_3d_interval"] = args.filter_3d_interval
        out["filter_3d"] = {name: run(args.iterations, False, optimizer=args.optimizer, antialiasing=aa, filter_3d=f)
                            for name, aa, f in (("plain", False, None), ("antialiasing", True, None), ("filter_3d", False, f3),
                                                ("antialiasing_and_filter_3d", True, f3))}
        print(json.dumps(out))
        if args.out:
            with open(args.out, "w") as f:
                json.dump(out, f, indent=1)
        return
    shape = (1, 1, 1) if args.exposure else (tuple(args.bilagrid) if args.bilagrid is not None else None)
    if shape is not None or args.exposure_jitter:
        grid = None if shape is None else dict(bilagrid=shape, bilagrid_lr=args.bilagrid_lr, bilagrid_tv=args.bilagrid_tv)
        out["bilagrid"], out["exposure_jitter"] = shape, args.exposure_jitter
        if shape is not None:
            out["bilagrid_lr"], out["bilagrid_tv"] = args.bilagrid_lr, args.bilagrid_tv
        out["run"] = run(args.iterations, False, optimizer=args.optimizer, bilagrid=grid, jitter=args.exposure_jitter)
        print(json.dumps(out))
        if args.out:
            with open(args.out, "w") as f:
                json.dump(out, f, indent=1)
        return
    if args.strategy == "mcmc":
        out["strategy"], out["cap_max"], out["noise_lr"] = "mcmc", args.cap_max, args.noise_lr
        out["mcmc"] = run(args.iterations, True, optimizer=args.optimizer,
                          mcmc=dict(strategy="mcmc", cap_max=args.cap_max, noise_lr=args.noise_lr))
        if args.optimizer != "default":
            out["optimizer"] = args.optimizer
        print(json.dumps(out))
        if args.out:
            with open(args.out, "w") as f:
                json.dump(out, f, indent=1)
        return
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
