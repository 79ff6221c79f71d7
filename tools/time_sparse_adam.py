#!/usr/bin/env python3
"""Times sparse Adam (csrc/sparse_adam.hip: c3dgs_sparse_adam_select + c3dgs_sparse_adam_step) against the dense step
(c3dgs_adam_step, csrc/adam.hip) on the same tensors in the same process: the six tensors of a non-indexed model at SH degree 3
(xyz 3, f_dc 3, f_rest 45, opacity 1, scaling 3, rotation 4 = 59 floats per Gaussian) with gradients and both moments, at 3M
Gaussians, and at 1M and 6M for scaling. Prints one JSON line and writes profiles/r14_sparse_adam_time.json.

    python tools/time_sparse_adam.py [--samples 20] [--warmup 5] [--P 3000000,1000000,6000000] [--out profiles/r14_sparse_adam_time.json]

Masks: listed fractions 1, 0.5, 0.25, 0.1, 0.01, each seeded random and as contiguous runs of 4096 rows (what a Morton-ordered
scene gives a view); at the first size also the bench scene's own radii > 0 and contrib_hits > 0 (BASELINE.json configs[2]).
Per mask: medians of `samples` with min and max after `warmup` unrecorded rounds, between stream events, one round = select,
sparse step, dense step, so the three alternate inside one loop. The floor: the distinct 128-byte lines the listed rows touch
in each array, counted on the host from the mask, times 7 line transfers (g read; p, m, v read and written), plus the mask and
the list, at the rate a device-to-device copy of 512 MiB reaches in the same process. The expectations (select + step below
the dense step at every fraction <= 0.25) are evaluated and written as booleans, whatever they come to."""
import argparse
import ctypes as C
import json
import math
import os
import statistics
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

ROW_LENS = (("xyz", 3, 0.00016), ("f_dc", 3, 0.0025), ("f_rest", 45, 0.0025 / 20), ("opacity", 1, 0.05), ("scaling", 3, 0.005),
            ("rotation", 4, 0.001))
FRACTIONS = (1.0, 0.5, 0.25, 0.1, 0.01)
RUN = 4096
BETAS, EPS, T = (0.9, 0.999), 1e-15, 100


def _event_ms(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b)


def copy_rate_gb_s(samples):
    src = torch.empty(512 << 20, dtype=torch.uint8, device="cuda")
    dst = torch.empty_like(src)
    for _ in range(3):
        dst.copy_(src)
    ms = [_event_ms(lambda: dst.copy_(src)) for _ in range(samples)]
    return 2 * src.numel() / (statistics.median(ms) * 1e-3) / 1e9        # bytes read + bytes written


def random_mask(P, fraction, seed):
    if fraction >= 1.0:
        return torch.ones(P, dtype=torch.bool, device="cuda")
    g = torch.Generator(device="cuda").manual_seed(seed)
    return torch.rand(P, device="cuda", generator=g) < fraction


def runs_mask(P, fraction, seed):
    n = (P + RUN - 1) // RUN
    g = torch.Generator(device="cuda").manual_seed(seed)
    pick = torch.randperm(n, device="cuda", generator=g)[:max(1, round(fraction * n))]
    blocks = torch.zeros(n, dtype=torch.bool, device="cuda")
    blocks[pick] = True
    return blocks.repeat_interleave(RUN)[:P].contiguous()


def lines_touched(rows, row_len, base_ptr):
    """Distinct 128-byte lines the rows (ascending int64) of a [P, row_len] float array at `base_ptr` touch."""
    if rows.size == 0:
        return 0
    off = base_ptr % 128
    first = (rows * (4 * row_len) + off) // 128
    last = ((rows + 1) * (4 * row_len) - 1 + off) // 128
    start = first.copy()
    start[1:] = np.maximum(first[1:], last[:-1] + 1)                      # a row's first line may be the row before's last
    return int(np.maximum(last - start + 1, 0).sum())


def bench_scene_masks(P):
    """radii and contrib_hits (both int32 [P]) of the bench scene's own view."""
    from c3dgs_amd import rasterizer
    from oracle import oracle as orc
    from tests import fullsize, gpu_util
    inp, intr, ev, indexed = fullsize.config_inputs("config3_3M_indexed", P=P)
    cam = orc.camera(intr.numpy(), ev.numpy())
    inp = {k: (v.cuda() if isinstance(v, torch.Tensor) else v) for k, v in inp.items()}
    fw = gpu_util.hip_forward(inp, cam, indexed)
    hits = rasterizer._C.render_contrib(int(inp["means3D"].shape[0]), cam["W"], cam["H"], fw["num_rendered"], fw["geom"], fw["binning"],
                                        fw["img"])[2]
    return fw["radii"].contiguous(), hits.contiguous()


def time_size(P, samples, warmup, rate, with_bench_scene):
    from c3dgs_amd import _lib, optim
    L = _lib.lib()
    g = torch.Generator(device="cuda").manual_seed(P)
    tensors = []
    for name, rl, lr in ROW_LENS:
        p, grad = (torch.randn(P, rl, device="cuda", generator=g) for _ in range(2))
        m, v = torch.randn(P, rl, device="cuda", generator=g) * 0.1, torch.rand(P, rl, device="cuda", generator=g) * 0.01
        tensors.append((name, rl, lr, p, grad, m, v))
    dense, sparse = (_lib.AdamTensor * len(tensors))(), (_lib.SparseAdamTensor * len(tensors))()
    for arr in (dense, sparse):
        for a, (name, rl, lr, p, grad, m, v) in zip(arr, tensors):
            a.param, a.grad, a.exp_avg, a.exp_avg_sq, a.n = p.data_ptr(), grad.data_ptr(), m.data_ptr(), v.data_ptr(), p.numel()
            a.step_size, a.bias_correction2_sqrt = lr / (1.0 - BETAS[0] ** T), math.sqrt(1.0 - BETAS[1] ** T)
    for a, t in zip(sparse, tensors):
        a.row_len = t[1]
    stream = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    need = C.c_size_t(0)
    _lib.check(L.c3dgs_sparse_adam_workspace_bytes(P, C.byref(need)))
    ws = torch.zeros(need.value, dtype=torch.uint8, device="cuda")

    masks = [(form, f, fn(P, f, 17)) for f in FRACTIONS for form, fn in (("random", random_mask), ("runs_of_4096", runs_mask))]
    if with_bench_scene:
        radii, hits = bench_scene_masks(P)
        masks += [("bench_scene_radii", None, radii), ("bench_scene_contrib_hits", None, hits)]
    out = []
    for form, fraction, mask in masks:
        kind = optim._MASK_KINDS[mask.dtype]
        t = {"select": [], "step": [], "dense": []}
        for n in range(warmup + samples):
            ms_sel = _event_ms(lambda: _lib.check(L.c3dgs_sparse_adam_select(P, mask.data_ptr(), kind, ws.data_ptr(), stream)))
            ms_step = _event_ms(lambda: _lib.check(L.c3dgs_sparse_adam_step(len(tensors), sparse, P, ws.data_ptr(), BETAS[0], BETAS[1],
                                                                             EPS, stream)))
            ms_dense = _event_ms(lambda: _lib.check(L.c3dgs_adam_step(len(tensors), dense, BETAS[0], BETAS[1], EPS, stream)))
            if n >= warmup:
                t["select"].append(ms_sel)
                t["step"].append(ms_step)
                t["dense"].append(ms_dense)
        listed = (mask > 0) if mask.dtype == torch.int32 else mask
        rows = torch.nonzero(listed).flatten().cpu().numpy().astype(np.int64)
        count = int(ws[:4].view(torch.int32))
        assert count == rows.size, (count, rows.size)
        lines = sum(lines_touched(rows, rl, p.data_ptr()) for _, rl, _, p, _, _, _ in tensors)     # the four arrays are aligned alike
        floor_bytes = 7 * 128 * lines + mask.numel() * mask.element_size() + 4 * count
        rec = {"mask": form, "fraction_asked": fraction, "listed": count, "fraction_listed": count / P,
               "mask_dtype": str(mask.dtype).split(".")[-1]}
        for k, v in t.items():
            rec[k + "_ms"] = statistics.median(v)
            rec[k + "_ms_min_max"] = [min(v), max(v)]
        both = [a + b for a, b in zip(t["select"], t["step"])]
        rec["select_plus_step_ms"] = statistics.median(both)
        rec["select_plus_step_ms_min_max"] = [min(both), max(both)]
        rec["select_plus_step_over_dense"] = rec["select_plus_step_ms"] / rec["dense_ms"]
        rec["lines_touched_per_array"] = lines
        rec["floor_bytes"] = floor_bytes
        rec["floor_ms"] = floor_bytes / (rate * 1e9) * 1e3
        rec["step_over_floor"] = rec["step_ms"] / rec["floor_ms"] if rec["floor_ms"] > 0 else None
        out.append(rec)
    dense_all = [r["dense_ms"] for r in out]
    return {"P": P, "floats_per_gaussian": sum(rl for _, rl, _ in ROW_LENS), "dense_bytes": 28 * P * sum(rl for _, rl, _ in ROW_LENS),
            "dense_ms": statistics.median(dense_all), "dense_ms_min_max_over_masks": [min(dense_all), max(dense_all)], "masks": out}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--samples", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--P", default="3000000,1000000,6000000")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r14_sparse_adam_time.json"))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("time_sparse_adam.py needs the GPU; a timing taken anywhere else says nothing")
    rate = copy_rate_gb_s(args.samples)
    sizes = []
    for k, P in enumerate(int(x) for x in args.P.split(",")):
        sizes.append(time_size(P, args.samples, args.warmup, rate, with_bench_scene=k == 0))
        torch.cuda.empty_cache()
    out = {"device": torch.cuda.get_device_name(0), "samples": args.samples, "warmup": args.warmup, "copy_rate_gb_s": rate,
           "method": "stream events around each library call; one round = select, sparse step, dense step on the same tensors; medians "
                     "after warm-up; floor = 7 x 128 B per distinct line the listed rows touch + mask + list, at the copy rate",
           "tensors": [[name, rl] for name, rl, _ in ROW_LENS], "sizes": sizes}
    exp = {}
    for s in sizes:
        for r in s["masks"]:
            if r["fraction_asked"] is not None and r["fraction_asked"] <= 0.25:
                exp[f"P={s['P']} {r['mask']} {r['fraction_asked']}"] = r["select_plus_step_ms"] < r["dense_ms"]
    out["expectation_select_plus_step_below_dense_at_fractions_up_to_0.25"] = exp
    out["expectation_met_everywhere"] = all(exp.values())
    out["ratio_to_dense_at_fraction_1"] = {f"P={s['P']} {r['mask']}": r["select_plus_step_over_dense"]
                                           for s in sizes for r in s["masks"] if r["fraction_asked"] == 1.0}
    print(json.dumps(out))
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as fh:
            json.dump(out, fh, indent=1)


if __name__ == "__main__":
    main()
