#!/usr/bin/env python3
"""Times the mesh extraction (csrc/mesh.hip) on the GPU, in one process with stream events, medians of --samples with min-max.

    python tools/time_mesh.py [--P 1000000] [--sizes 256 512] [--samples 5] [--warmup 2] [--out profiles/mesh_time.json]

The maps: 32 cameras on a small orbit around the bench scene's camera (synth-v1, 1920x1080, focal 1200), each rendered with
render(return_depth=True); surface_depth's median map and the rendered colours. The volume: a cube of side 10 around the scene
(z in [2, 12]) with N^3 lattice points, sdf_trunc = 4 voxels, colour planes included (20 B per point).
integrate, for K = 1, 8 and 32 maps, per sample ALTERNATED on the same volume: one launch of K maps, then K launches of one map
(the condition: the first must not take longer), and for K = 1 and 8 the same per-camera sequence written in torch ops. Next to
each the streaming floor: the bytes of the planes read once and written once where touched, plus the maps, at 6.3 TB/s.
extract on the fused volume: TSDFVolume.extract() as a whole (four launches and the host read) and its stages, next to the same
marching tetrahedra written in torch ops (a port of tests/mesh_ref.py: extract) and to the floor of its passes' plane and scratch
traffic plus the outputs."""
import argparse
import itertools
import json
import math
import os
import statistics
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

HBM_BYTES_PER_S = 6.3e12          # achievable, not peak
W, H, FOCAL = 1920, 1080, 1200.0


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


class _Cam:
    def __init__(self, intrinsic, ev):
        self.intrinsic, self.extrinsic_vector = intrinsic.cuda(), ev.cuda()
        self.original_image = None


def bench_maps(P, views):
    """-> (table [views, 16], depth [views, H, W], colour [views, 3, H, W]) of the bench scene on the GPU"""
    from c3dgs_amd import filter3d, mesh
    from c3dgs_amd.model import GaussianModel, PipelineParams
    from tests import synth
    sc = synth.scene(P, W, H, FOCAL, seed=1234, sh_degree=3)
    op = sc["opacities"].clamp(1e-4, 1 - 1e-6)
    norm = sc["scales"].norm(dim=1, keepdim=True)
    m = GaussianModel(3, quantization=False, device="cuda")
    m.set_tensors(xyz=sc["means3D"], features_dc=sc["shs"][:, :1], features_rest=sc["shs"][:, 1:], scaling=sc["scales"] / norm,
                  rotation=sc["rotations"], opacity=torch.log(op / (1 - op)), scaling_factor=torch.log(norm))
    cams = []
    for k in range(views):
        a = 2 * math.pi * k / views
        ev = (0.015 * math.sin(a), 0.015 * math.cos(a), 0.0, 1.0, 0.25 * math.cos(a), 0.25 * math.sin(a), 0.0)
        cams.append(_Cam(*synth.camera(W, H, FOCAL, extrinsic_vector=ev)))
    bg = torch.zeros(3, device="cuda")
    depth, colour = [], []
    with torch.no_grad():
        for cam in cams:
            pkg = m.render(cam, PipelineParams(), bg, return_depth=True)
            depth.append(mesh.surface_depth(pkg, "median", 0.5))
            colour.append(pkg["render"].clone())
    return filter3d.camera_table(cams, "cuda"), torch.stack(depth), torch.stack(colour)


def torch_integrate(vol, depth, table, colour, depth_min=0.2, depth_max=math.inf):
    """the integration's contract in torch ops, one camera after the other, on the volume's planes"""
    Nx, Ny, Nz = vol.dims
    dev = vol.tsdf.device
    ax = [vol.origin[a] + torch.arange(n, device=dev, dtype=torch.float32) * vol.voxel_size for a, n in enumerate((Nx, Ny, Nz))]
    pz, py, px = torch.meshgrid(ax[2], ax[1], ax[0], indexing="ij")
    rows = table.cpu().tolist()
    for c, m in enumerate(rows):
        x = m[0] * px + m[1] * py + m[2] * pz + m[3]
        y = m[4] * px + m[5] * py + m[6] * pz + m[7]
        z = m[8] * px + m[9] * py + m[10] * pz + m[11]
        u = m[12] * x / z + 0.5 * m[14]
        v = m[13] * y / z + 0.5 * m[15]
        ok = (z >= depth_min) & (u >= 0) & (u < m[14]) & (v >= 0) & (v < m[15])
        ui = torch.where(ok, u, torch.zeros_like(u)).long()
        vi = torch.where(ok, v, torch.zeros_like(v)).long()
        pix = vi * depth.shape[2] + ui
        d = depth[c].reshape(-1)[pix]
        sdf = d - z
        ok &= (d > 0) & (d <= depth_max) & (sdf >= -vol.sdf_trunc)
        s = torch.clamp_max(sdf / vol.sdf_trunc, 1.0)
        w1 = vol.weight + 1
        vol.tsdf.copy_(torch.where(ok, (vol.tsdf * vol.weight + s) / w1, vol.tsdf))
        for q in range(3):
            vol.color[q].copy_(torch.where(ok, (vol.color[q] * vol.weight + colour[c, q].reshape(-1)[pix]) / w1, vol.color[q]))
        vol.weight.copy_(torch.where(ok, w1, vol.weight))


SLOT_DIR = ((1, 0, 0), (0, 1, 0), (0, 0, 1), (1, 1, 0), (1, 0, 1), (0, 1, 1), (1, 1, 1))


def _shift(a, d):
    Nz, Ny, Nx = a.shape
    p = torch.nn.functional.pad(a, (1, 1, 1, 1, 1, 1))
    return p[1 + d[2]:1 + d[2] + Nz, 1 + d[1]:1 + d[1] + Ny, 1 + d[0]:1 + d[0] + Nx]


def torch_extract(vol):
    """tests/mesh_ref.py's extract in torch ops on the volume's device -> (vertices, colors, faces)"""
    tsdf, weight = vol.tsdf, vol.weight
    Nz, Ny, Nx = tsdf.shape
    dev = tsdf.device
    inside, wpos = tsdf < 0, weight > 0
    cell = torch.ones_like(inside)
    for q in itertools.product((0, 1), repeat=3):
        cell &= _shift(wpos, q)
    edge = []
    for d in SLOT_DIR:
        around = torch.zeros_like(inside)
        for c in itertools.product(*[((0,) if d[a] else (-1, 0)) for a in range(3)]):
            around |= _shift(cell, c)
        edge.append((inside ^ _shift(inside, d)) & around)
    per_point = torch.stack(edge).sum(0).reshape(-1)
    base = (torch.cumsum(per_point, 0) - per_point).reshape(tsdf.shape)
    V = int(per_point.sum())
    ax = [vol.origin[a] + torch.arange(n, device=dev, dtype=torch.float32) * vol.voxel_size for a, n in enumerate((Nx, Ny, Nz))]
    vertices = torch.empty((V, 3), dtype=torch.float32, device=dev)
    colors = torch.empty((V, 3), dtype=torch.float32, device=dev)
    vid, below = [], torch.zeros_like(base)
    for s, d in enumerate(SLOT_DIR):
        vid.append(base + below)
        below = below + edge[s]
        k, j, i = torch.nonzero(edge[s], as_tuple=True)
        at = vid[s][k, j, i]
        va, vb = tsdf[k, j, i], tsdf[k + d[2], j + d[1], i + d[0]]
        t = va / (va - vb)
        for q, idx in enumerate((i, j, k)):
            pa, pb = ax[q][idx], ax[q][idx + d[q]]
            vertices[at, q] = pa + t * (pb - pa)
            ca, cb = vol.color[q][k, j, i], vol.color[q][k + d[2], j + d[1], i + d[0]]
            colors[at, q] = ca + t * (cb - ca)
    slot_of = {d: s for s, d in enumerate(SLOT_DIR)}
    faces = []
    for perm in itertools.permutations(range(3)):
        path = [(0, 0, 0)]
        for a in perm:
            path.append(tuple(path[-1][q] + (1 if q == a else 0) for q in range(3)))
        det = round(float(np.linalg.det(np.array([np.subtract(path[q], path[0]) for q in (1, 2, 3)], float))))
        code = sum(_shift(inside, c).int() << q for q, c in enumerate(path))
        code = torch.where(cell, code, torch.zeros_like(code))
        for m in range(1, 15):
            k, j, i = torch.nonzero(code == m, as_tuple=True)
            if not k.numel():
                continue
            n = bin(m).count("1")
            first = (~m & 15) if n == 3 else m
            L = [q for q in range(4) if (first >> q) & 1] + [q for q in range(4) if not (first >> q) & 1]
            inv = sum(L[a] > L[b] for a in range(4) for b in range(a + 1, 4))
            positive = ((-1) ** inv) * det > 0
            keep = (not positive) if n == 3 else positive

            def vertex(p, q):
                lo, hi = path[min(p, q)], path[max(p, q)]
                return vid[slot_of[tuple(hi[a] - lo[a] for a in range(3))]][k + lo[2], j + lo[1], i + lo[0]]

            if n == 2:
                ac, ad, bd, bc = vertex(L[0], L[2]), vertex(L[0], L[3]), vertex(L[1], L[3]), vertex(L[1], L[2])
                tris = [(ac, ad, bd), (ac, bd, bc)]
            else:
                tris = [(vertex(L[0], L[1]), vertex(L[0], L[2]), vertex(L[0], L[3]))]
            for a, b, c in tris:
                faces.append(torch.stack([a, b, c] if keep else [a, c, b], 1))
    faces = torch.cat(faces).int() if faces else torch.zeros((0, 3), dtype=torch.int32, device=dev)
    return vertices, colors, faces


def time_size(N, table, depth, colour, samples, warmup):
    from c3dgs_amd import _lib, mesh
    h = 10.0 / (N - 1)
    new = lambda: mesh.TSDFVolume((-5.0, -5.0, 2.0), h, (N, N, N), 4 * h, "cuda")       # noqa: E731
    points = N ** 3
    out = {"N": N, "points": points, "voxel_size": h, "plane_bytes": 20 * points, "integrate": []}
    vol = new()
    for K in (1, 8, 32):
        d, t, c = depth[:K].contiguous(), table[:K].contiguous(), colour[:K].contiguous()
        one, many = [], []
        for n in range(warmup + samples):
            a = _event_ms(lambda: vol.integrate(d, t, c))
            b = _event_ms(lambda: [vol.integrate(d[q:q + 1], t[q:q + 1], c[q:q + 1]) for q in range(K)])
            if n >= warmup:
                one.append(a)
                many.append(b)
        probe = new().integrate(d, t, c)
        touched = int((probe.weight > 0).sum())
        del probe
        floor_bytes = 20 * points + 20 * touched + K * W * H * 16
        r = {"K": K, "touched_fraction": touched / points, "floor_ms": floor_bytes / HBM_BYTES_PER_S * 1e3}
        _stat(r, "one_launch_of_K", one)
        _stat(r, "K_launches_of_one", many)
        r["per_camera_ms"] = r["one_launch_of_K_ms"] / K
        r["fraction_of_floor"] = r["floor_ms"] / r["one_launch_of_K_ms"]
        r["condition_one_launch_not_slower"] = r["one_launch_of_K_ms"] <= r["K_launches_of_one_ms"]
        if K <= 8:
            tv = new()
            loop = [_event_ms(lambda: torch_integrate(tv, d, t, c)) for _ in range(1 + min(samples, 3))][1:]
            _stat(r, "torch_ops", loop)
            r["torch_over_kernel"] = r["torch_ops_ms"] / r["one_launch_of_K_ms"]
            del tv
        out["integrate"].append(r)
        torch.cuda.empty_cache()
    # extract on a volume every map went into once
    vol = new().integrate(depth, table, colour)
    whole, stages = [], {k: [] for k in ("mesh_classify", "mesh_scan", "mesh_emit_vertices", "mesh_emit_faces")}
    for n in range(warmup + samples):
        ms = _event_ms(vol.extract)
        if n >= warmup:
            whole.append(ms)
    _lib.profile_enable(True)
    for n in range(samples):
        torch.cuda.synchronize()
        _lib.profile_read()
        v, c, f = vol.extract()
        torch.cuda.synchronize()
        st = _lib.profile_read()
        for k in stages:
            stages[k].append(st[k][0] if k in st else 0.0)
    _lib.profile_enable(False)
    V, F = int(v.shape[0]), int(f.shape[0])
    floor_bytes = points * (8 + 1 + 1 + 4 + 1) + V * 24 + F * 12
    e = {"V": V, "F": F, "floor_ms": floor_bytes / HBM_BYTES_PER_S * 1e3}
    _stat(e, "extract", whole)
    for k, vals in stages.items():
        _stat(e, k, vals)
    e["fraction_of_floor"] = e["floor_ms"] / e["extract_ms"]
    loop = [_event_ms(lambda: torch_extract(vol)) for _ in range(3)][1:]
    _stat(e, "torch_ops", loop)
    e["torch_over_kernel"] = e["torch_ops_ms"] / e["extract_ms"]
    tv, tc, tf = torch_extract(vol)
    e["torch_ops_give_the_same_vertices"] = bool(tv.shape == v.shape and torch.equal(tv, v)) and int(tf.shape[0]) == F
    out["extract"] = e
    del vol, v, c, f, tv, tc, tf
    torch.cuda.empty_cache()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--P", type=int, default=1_000_000)
    ap.add_argument("--sizes", type=int, nargs="+", default=[256, 512])
    ap.add_argument("--samples", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "mesh_time.json"))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("time_mesh.py needs the GPU; a timing taken anywhere else says nothing")
    table, depth, colour = bench_maps(args.P, 32)
    out = {"device": torch.cuda.get_device_name(0), "samples": args.samples, "warmup": args.warmup, "P": args.P,
           "maps": f"32 x {H}x{W}, measured fraction {float((depth > 0).float().mean()):.3f}",
           "method": "one process; stream events around each call, medians with min-max; one launch of K maps and K launches of one "
                     "map alternated per sample; floors at 6.3 TB/s", "sizes": []}
    for N in args.sizes:
        out["sizes"].append(time_size(N, table, depth, colour, args.samples, args.warmup))
        print(json.dumps(out["sizes"][-1]), flush=True)
    print(json.dumps(out))
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as fh:
            json.dump(out, fh, indent=1)


if __name__ == "__main__":
    main()
