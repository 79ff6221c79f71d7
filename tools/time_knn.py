"""Time the 3-NN scale initialiser (c3dgs_amd.knn.distCUDA2, csrc/knn.hip) and PLY IO on the GPU; write one JSON.

    python tools/time_knn.py [--out profiles/r05_knn_time.json] [--reps 5]

Clouds: synth-v1 positions (tests/synth.py scene) at 1M / 3M / 6M, uniform cubes at 1M / 3M, a clustered cloud (1M:
half uniform, half in clusters of 64 points inside 1e-6 cubes) and an all-identical 1M cloud. Per cloud: the call
(device events around distCUDA2, which includes the finiteness check and the workspace allocation) and the kernel stages
knn_sort / knn_bounds / knn_query (events the library records around each stage), after one warm-up call.
Also: save_ply and load_ply of a 3M-Gaussian degree-3 scene (host clock, the file in a temporary directory)."""
import argparse
import json
import os
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import torch  # noqa: E402

from c3dgs_amd import _lib, knn  # noqa: E402
from tests import synth  # noqa: E402


def clouds():
    g = torch.Generator(device="cuda").manual_seed(0)
    for P in (1_000_000, 3_000_000, 6_000_000):
        yield f"synth_{P // 1_000_000}M", lambda P=P: synth.scene(P, sh_degree=0)["means3D"].cuda()
    for P in (1_000_000, 3_000_000):
        yield f"uniform_{P // 1_000_000}M", lambda P=P: torch.rand(P, 3, device="cuda", generator=g)

    def clustered(P=1_000_000, k=64):
        x = torch.rand(P, 3, device="cuda", generator=g)
        n = P // 2 // k
        centres = torch.rand(n, 3, device="cuda", generator=g)
        x[:n * k] = (centres[:, None, :] + 1e-6 * torch.rand(n, k, 3, device="cuda", generator=g)).reshape(-1, 3)
        return x
    yield "clustered_1M", clustered
    yield "identical_1M", lambda: torch.full((1_000_000, 3), 0.375, device="cuda")


def time_cloud(x, reps):
    knn.distCUDA2(x)                                           # warm-up: code objects, sort configuration
    torch.cuda.synchronize()
    _lib.profile_read()
    _lib.profile_enable(True)
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    calls = []
    for _ in range(reps):
        a.record()
        knn.distCUDA2(x)
        b.record()
        b.synchronize()
        calls.append(a.elapsed_time(b))
    _lib.profile_enable(False)
    st = _lib.profile_read()
    stages = {k: st[k][0] / st[k][1] for k in ("knn_sort", "knn_bounds", "knn_query") if k in st}
    return {"P": int(x.shape[0]), "call_ms_median": sorted(calls)[len(calls) // 2], "call_ms_min": min(calls),
            "stages_ms": stages, "stages_sum_ms": sum(stages.values())}


def time_ply(P=3_000_000):
    from c3dgs_amd.model import GaussianModel
    sc = synth.scene(P, seed=5)
    op = sc["opacities"].clamp(1e-4, 1 - 1e-4)
    m = GaussianModel(3, quantization=False, use_factor_scaling=False).set_tensors(
        xyz=sc["means3D"], features_dc=sc["shs"][:, :1], features_rest=sc["shs"][:, 1:], scaling=torch.log(sc["scales"]),
        rotation=sc["rotations"], opacity=torch.log(op / (1 - op)))
    del sc
    with tempfile.TemporaryDirectory() as d:
        path = os.path.join(d, "scene.ply")
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        m.save_ply(path)
        t1 = time.perf_counter()
        size = os.path.getsize(path)
        m2 = GaussianModel(3, quantization=False, use_factor_scaling=False).load_ply(path)
        torch.cuda.synchronize()
        t2 = time.perf_counter()
    assert torch.equal(m2._xyz, m._xyz)
    return {"P": P, "sh_degree": 3, "file_bytes": size, "save_ply_s": t1 - t0, "load_ply_s": t2 - t1}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r05_knn_time.json"))
    ap.add_argument("--reps", type=int, default=5)
    args = ap.parse_args()
    res = {"device": torch.cuda.get_device_name(0), "knn": {}}
    for name, make in clouds():
        x = make()
        res["knn"][name] = time_cloud(x, args.reps)
        print(name, json.dumps(res["knn"][name]), flush=True)
        del x
        torch.cuda.empty_cache()
    res["ply_3M_degree3"] = time_ply()
    print("ply", json.dumps(res["ply_3M_degree3"]), flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
