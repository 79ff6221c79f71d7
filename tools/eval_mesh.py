#!/usr/bin/env python3
"""A mesh PLY against a reference point-cloud PLY -> one JSON line: accuracy, completeness, Chamfer distance, precision / recall /
F-score per threshold (c3dgs_amd.metrics.mesh_metrics), the sample counts and the seconds per stage.

    python tools/eval_mesh.py mesh.ply reference.ply [--density D] [--threshold T ...] [--max-dist M]
                              [--bounds x0 y0 z0 x1 y1 z1] [--seed 0]

--density: sampled points per unit area of the mesh; default 1 / spacing^2 with spacing = metrics.reference_spacing(reference),
the reference cloud's own density on a surface (nobody has tuned that default). --threshold may be given up to eight times."""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("mesh")
    ap.add_argument("reference")
    ap.add_argument("--density", type=float, default=None)
    ap.add_argument("--threshold", type=float, action="append", default=[])
    ap.add_argument("--max-dist", type=float, default=float("inf"))
    ap.add_argument("--bounds", type=float, nargs=6, default=None, metavar=("X0", "Y0", "Z0", "X1", "Y1", "Z1"))
    ap.add_argument("--seed", type=int, default=0)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("eval_mesh.py needs the GPU (c3dgs_amd has no CPU path)")
    from c3dgs_amd import metrics, ply
    seconds = {}

    def timed(stage, fn):
        t0 = time.perf_counter()
        out = fn()
        torch.cuda.synchronize()
        seconds[stage] = time.perf_counter() - t0
        return out

    def load():
        vertices, _, faces = ply.read_mesh_ply(args.mesh)
        cloud = ply.read_ply(args.reference)
        ref = np.stack([cloud["x"], cloud["y"], cloud["z"]], 1).astype(np.float32)
        return torch.from_numpy(vertices).cuda(), torch.from_numpy(faces).cuda(), torch.from_numpy(ref).cuda()

    vertices, faces, ref = timed("load", load)
    out = {"mesh": args.mesh, "reference": args.reference, "vertices": int(vertices.shape[0]), "faces": int(faces.shape[0]),
           "reference_points": int(ref.shape[0])}
    density = args.density
    if density is None:
        spacing = timed("spacing", lambda: metrics.reference_spacing(ref))
        if not spacing > 0:
            raise SystemExit("eval_mesh.py: the reference cloud's median spacing is 0 (duplicated points); give --density")
        density = 1.0 / spacing ** 2
        out["reference_spacing"] = spacing
    bounds = None if args.bounds is None else (args.bounds[:3], args.bounds[3:])
    m = timed("metrics", lambda: metrics.mesh_metrics(vertices, faces, ref, density, seed=args.seed, thresholds=args.threshold,
                                                      max_dist=args.max_dist, bounds=bounds))
    for k in ("precision", "recall", "fscore"):
        m[k] = {repr(t): v for t, v in m[k].items()}
    out.update(m, density=density, seed=args.seed, seconds=seconds)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
