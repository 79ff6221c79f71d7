#!/usr/bin/env python3
"""From a dataset on disk to held-out metrics with nothing hand-rolled in between: writes the rendered Blender dataset of
tests/scene_fixture.py to a temporary directory, then c3dgs_amd.scene.Scene -> pipeline.train -> scene.save ->
metrics.render_and_eval on the held-out views, and prints one JSON line.

    python tools/run_scene.py [--iterations 600] [--views 8] [--width 160] [--height 112] [--out profiles/r09_run_scene.json]"""
import argparse
import json
import os
import sys
import tempfile
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from tests import scene_fixture, train_scene  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iterations", type=int, default=600)
    ap.add_argument("--views", type=int, default=8)
    ap.add_argument("--width", type=int, default=160)
    ap.add_argument("--height", type=int, default=112)
    ap.add_argument("--save-memory", action="store_true")
    ap.add_argument("--densify", action="store_true", help="adaptive density control on the scene's camera extent (nearly coincident views: small)")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("run_scene.py needs the GPU; there is no CPU path")
    from c3dgs_amd import metrics, pipeline
    from c3dgs_amd.model import GaussianModel, PipelineParams
    from c3dgs_amd.scene import Scene

    def clock():
        torch.cuda.synchronize()
        return time.perf_counter()

    with tempfile.TemporaryDirectory() as tmp:
        t0 = clock()
        n_points = scene_fixture.rendered_blender(os.path.join(tmp, "data"), views=args.views, hold_every=4, W=args.width,
                                                  H=args.height, focal=150.0 * args.width / 160, P_teacher=4000, keep_every=8)
        t_write = clock() - t0
        model = GaussianModel(3, quantization=True, device="cuda")
        params = pipeline.ModelParams(source_path=os.path.join(tmp, "data"), model_path=os.path.join(tmp, "out"), eval=True).extract()
        t0 = clock()
        scene = Scene(params, model, shuffle=False, save_memory=args.save_memory)
        for cam in scene.getTrainCameras() + scene.getTestCameras():
            cam.original_image                                       # decode + upload + kernel, once per view
        t_scene = clock() - t0
        bg = torch.zeros(3, device="cuda")
        before = metrics.render_and_eval(model, scene.getTestCameras(), PipelineParams(), bg)
        events = []
        torch.manual_seed(0)
        t0 = clock()
        n = pipeline.train(scene, None, train_scene.schedule(args.iterations, args.densify), PipelineParams(), camera_stride=1,
                           degree_up_iter=args.iterations // 5, log=lambda epoch, info: events.append(info))
        t_train = clock() - t0
        scene.save(n)
        saved = os.path.join(tmp, "out", "point_cloud", f"iteration_{n}", "point_cloud.ply")
        t0 = clock()
        after = metrics.render_and_eval(model, scene.getTestCameras(), PipelineParams(), bg)
        t_eval = clock() - t0
        out = {"dataset": f"tests/scene_fixture.py rendered_blender: {args.views} views {args.width}x{args.height}, every 4th held out, "
                          f"{n_points} points", "kind": scene.kind, "train_views": len(scene.getTrainCameras()),
               "test_views": len(scene.getTestCameras()), "cameras_extent": float(scene.cameras_extent), "save_memory": args.save_memory, "densify": args.densify,
               "iterations": n, "gaussians_before": n_points, "gaussians_after": model._xyz.shape[0],
               "held_out_before": {k: before[k] for k in ("PSNR", "SSIM")}, "held_out_after": {k: after[k] for k in ("PSNR", "SSIM")},
               "final_ema_loss": events[-1]["ema_loss"], "saved_ply_bytes": os.path.getsize(saved),
               "seconds": {"write_dataset": t_write, "scene": t_scene, "train": t_train, "eval": t_eval}}
    print(json.dumps(out))
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(out, f, indent=1)


if __name__ == "__main__":
    main()
