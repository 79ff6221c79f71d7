#!/usr/bin/env python3
"""Times the geometry evaluation (csrc/nn_query.hip, mesh_sample.hip, geometry_metrics.hip) on the GPU, in one process with stream
events, medians of --samples with min-max.

    python tools/time_geometry.py [--P 1000000] [--N 256] [--sizes 1000000 4000000] [--samples 5] [--warmup 2]
                                  [--out profiles/geometry_time.json]

The mesh: the bench scene (synth-v1) fused from 32 maps into an N^3 volume and extracted, as tools/time_mesh.py does. For each size
S the density is chosen so that sample_surface emits about S points; the reference cloud is a second sampling (another seed) of
about S points, jittered by a tenth of the sample spacing. Timed per size: the index build; the query in both orders (Morton-sorted,
caller's) for both query layouts (the face-ordered samples as sample_surface emits them, and the same points in random order), with
the mean number of leaves scanned per query; sample_surface; the reduction; the whole mesh_metrics call. At the first size only,
next to the query, the same result from torch ops: chunked torch.cdist + min."""
import argparse
import json
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))


def _event_ms(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b)


def _timed(out, key, fn, samples, warmup):
    vals = [_event_ms(fn) for _ in range(warmup + samples)][warmup:]
    out[key + "_ms"] = statistics.median(vals)
    out[key + "_ms_min_max"] = [min(vals), max(vals)]


def bench_mesh(P, N):
    import time_mesh
    from c3dgs_amd import mesh
    table, depth, colour = time_mesh.bench_maps(P, 32)
    h = 10.0 / (N - 1)
    vol = mesh.TSDFVolume((-5.0, -5.0, 2.0), h, (N, N, N), 4 * h, "cuda").integrate(depth, table, colour)
    vertices, _, faces = vol.extract()
    del vol, depth, colour
    torch.cuda.empty_cache()
    return vertices, faces


def torch_nearest(queries, points, chunk=2048):
    """the nearest point by brute force in torch ops: chunked cdist + min -> (idx, squared distance)"""
    idx = torch.empty(queries.shape[0], dtype=torch.int64, device=queries.device)
    d2 = torch.empty(queries.shape[0], dtype=torch.float32, device=queries.device)
    for a in range(0, queries.shape[0], chunk):
        d, i = torch.cdist(queries[a:a + chunk], points).min(dim=1)
        idx[a:a + chunk], d2[a:a + chunk] = i, d * d
    return idx, d2


def time_size(S, vertices, faces, area, samples, warmup, with_torch):
    from c3dgs_amd import knn, mesh, metrics
    density = S / area
    out = {"target": S, "density": density}
    pts, _ = mesh.sample_surface(vertices, faces, density, seed=0)
    ref, _ = mesh.sample_surface(vertices, faces, density, seed=1)
    spacing = density ** -0.5
    ref = ref + (torch.rand_like(ref) - 0.5) * (0.2 * spacing)
    out.update(samples=int(pts.shape[0]), reference=int(ref.shape[0]), spacing=spacing)
    _timed(out, "sample_surface", lambda: mesh.sample_surface(vertices, faces, density, seed=0), samples, warmup)
    _timed(out, "build", lambda: knn.NearestIndex(ref), samples, warmup)
    index = knn.NearestIndex(ref)
    layouts = {"face_ordered": pts, "random_order": pts[torch.randperm(pts.shape[0], device=pts.device)]}
    for name, q in layouts.items():
        r = {}
        for sort in (True, False):
            _timed(r, "sorted" if sort else "caller_order", lambda: index.query(q, sort=sort), samples, warmup)
        _, d2, leaves = index.query(q, sort=True, leaves=True)
        r["mean_leaves_per_query"] = float(leaves.double().mean())
        r["max_leaves_per_query"] = int(leaves.max())
        r["faster"] = "sorted" if r["sorted_ms"] <= r["caller_order_ms"] else "caller_order"
        r["shipped"] = "sorted" if (knn.SORT_FACE_ORDERED_QUERIES if name == "face_ordered" else knn.SORT_QUERIES) else "caller_order"
        r["shipped_is_the_faster"] = r["faster"] == r["shipped"]
        out[name] = r
    if with_torch:
        q = layouts["random_order"]
        t = {}
        ti, td = torch_nearest(q, ref)                                          # also the warm-up of the one timed run
        _timed(t, "torch_cdist_min", lambda: torch_nearest(q, ref), 1, 0)
        gi, gd = index.query(q)
        t["same_index_fraction"] = float((ti == gi.long()).double().mean())     # cdist rounds differently: ties and near-ties may differ
        t["torch_over_kernel"] = t["torch_cdist_min_ms"] / out["random_order"]["sorted_ms" if knn.SORT_QUERIES else "caller_order_ms"]
        t["condition_kernel_faster"] = t["torch_over_kernel"] > 1.0
        out["torch"] = t
    d2 = index.query(pts)[1]
    rows = torch.empty((2, 10), dtype=torch.float64, device="cuda")
    taus = [spacing, 2 * spacing]
    _timed(out, "reduce", lambda: metrics._reduce_direction(d2, pts, None, float("inf"), taus, rows[0]), samples, warmup)
    _timed(out, "reduce_torch_ops", lambda: (torch.sqrt(d2).double().sum(), (torch.sqrt(d2) < taus[0]).sum(),
                                             (torch.sqrt(d2) < taus[1]).sum()), samples, warmup)
    m = {}
    _timed(out, "mesh_metrics", lambda: m.update(metrics.mesh_metrics(vertices, faces, ref, density, thresholds=taus)), samples, warmup)
    out["metrics"] = {k: v for k, v in m.items() if not isinstance(v, dict)}
    out["metrics"]["fscore"] = {str(k): v for k, v in m["fscore"].items()}
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--P", type=int, default=1_000_000)
    ap.add_argument("--N", type=int, default=256)
    ap.add_argument("--sizes", type=int, nargs="+", default=[1_000_000, 4_000_000])
    ap.add_argument("--samples", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "geometry_time.json"))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("time_geometry.py needs the GPU; a timing taken anywhere else says nothing")
    from tests import mesh_ref
    vertices, faces = bench_mesh(args.P, args.N)
    area = float(mesh_ref.triangle_areas(vertices.cpu().numpy(), faces.cpu().numpy()).sum())
    out = {"device": torch.cuda.get_device_name(0), "samples": args.samples, "warmup": args.warmup, "P": args.P,
           "mesh": {"N": args.N, "V": int(vertices.shape[0]), "F": int(faces.shape[0]), "area": area},
           "method": "one process; stream events around each call (allocations included), medians with min-max", "sizes": []}
    for i, S in enumerate(args.sizes):
        out["sizes"].append(time_size(S, vertices, faces, area, args.samples, args.warmup, with_torch=i == 0))
        print(json.dumps(out["sizes"][-1]), flush=True)
    print(json.dumps(out))
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as fh:
            json.dump(out, fh, indent=1)


if __name__ == "__main__":
    main()
