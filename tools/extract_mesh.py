#!/usr/bin/env python3
"""From a saved model and its dataset on disk to a mesh: c3dgs_amd.scene.Scene loads the cameras and the saved Gaussians,
mesh.extract_mesh renders every training camera's depth, fuses the maps into a TSDF volume and extracts the surface
(csrc/mesh.hip), ply.write_mesh_ply writes it, and one JSON line reports V, F, the lattice and the seconds per stage.

    python tools/extract_mesh.py --source DATA --model OUT --voxel-size 0.02 [--iteration -1] [--sdf-trunc T] [--depth-mode median]
                                 [--alpha-min 0.5] [--depth-max D] [--batch 8] [--bounds x0 y0 z0 x1 y1 z1] [--out OUT/mesh.ply]

--bounds defaults to the bounding box of the camera centres grown by the scene radius (bounded scenes only)."""
import argparse
import json
import math
import os
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--source", required=True, help="the dataset (COLMAP sparse/ or transforms_train.json)")
    ap.add_argument("--model", required=True, help="the model directory with point_cloud/iteration_*/")
    ap.add_argument("--iteration", type=int, default=-1)
    ap.add_argument("--voxel-size", type=float, required=True)
    ap.add_argument("--sdf-trunc", type=float, default=None, help="default: 4 voxel sizes")
    ap.add_argument("--depth-mode", choices=("median", "expected"), default="median")
    ap.add_argument("--alpha-min", type=float, default=0.5)
    ap.add_argument("--depth-max", type=float, default=math.inf)
    ap.add_argument("--batch", type=int, default=8)
    ap.add_argument("--bounds", type=float, nargs=6, default=None, metavar=("X0", "Y0", "Z0", "X1", "Y1", "Z1"))
    ap.add_argument("--white-background", action="store_true")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("extract_mesh.py needs the GPU; there is no CPU path")
    from c3dgs_amd import mesh, pipeline, ply
    from c3dgs_amd.model import GaussianModel, PipelineParams
    from c3dgs_amd.scene import Scene

    t0 = time.perf_counter()
    model = GaussianModel(3, quantization=True, device="cuda")
    params = pipeline.ModelParams(source_path=args.source, model_path=args.model, white_background=args.white_background).extract()
    scene = Scene(params, model, load_iteration=args.iteration, shuffle=False, save_memory=True)
    t_load = time.perf_counter() - t0
    bg = torch.full((3,), 1.0 if args.white_background else 0.0, device="cuda")
    bounds = None if args.bounds is None else (args.bounds[:3], args.bounds[3:])
    spent = {}
    v, c, f = mesh.extract_mesh(model, scene.getTrainCameras(), PipelineParams(), bg, args.voxel_size, sdf_trunc=args.sdf_trunc,
                                bounds=bounds, depth_mode=args.depth_mode, alpha_min=args.alpha_min, depth_max=args.depth_max,
                                batch=args.batch, timings=spent)
    out_path = args.out or os.path.join(args.model, "mesh.ply")
    t0 = time.perf_counter()
    ply.write_mesh_ply(out_path, v.cpu().numpy(), c.cpu().numpy(), f.cpu().numpy())
    t_write = time.perf_counter() - t0
    dims = spent.pop("dims")
    print(json.dumps({"mesh": out_path, "V": int(v.shape[0]), "F": int(f.shape[0]), "dims": list(dims), "voxel_size": args.voxel_size,
                      "cameras": len(scene.getTrainCameras()), "iteration": scene.loaded_iter,
                      "seconds": {"load": t_load, **spent, "write": t_write}}))


if __name__ == "__main__":
    main()
