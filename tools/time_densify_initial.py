#!/usr/bin/env python3
"""Times GaussianModel.densify_initial (knn3 -> ray-fill plan -> ONE apply launch -> positions: csrc/knn.hip, csrc/ray_fill.hip,
the apply kernel of csrc/densify.hip) -> profiles/r08_densify_initial_time.json.

    python tools/time_densify_initial.py [--sizes 100000,1000000,3000000] [--calls 20] [--out profiles/r08_densify_initial_time.json]

A sparse cloud (a dense core in a halo twenty times wider, seeded, drawn on the device) as an SH degree 3 model with Adam
moments attached; dist_thr_coeff is picked per size, by bisection on the plan's totals, so that the scene roughly doubles.
Every timing is the time between two events on the stream around the work, host reads included, as a median of `calls`
after a warm-up; every call of the whole method and of the apply stage runs on a fresh clone of the state.

    stages      knn3, the plan (both calls and the read of the totals between them), the apply launch with its allocations
                and the install, the position kernel
    whole       GaussianModel.densify_initial
    baseline    the staged sequence the reference runs (scene/gaussian_model.py:1369-1387), restated with torch ops on the
                same device FROM OUR neighbour table: per neighbour slot and level one boolean selection, the new positions,
                and one torch.cat of every parameter tensor and both its moments (cat_tensors_to_optimizer). Its result is
                compared with the HIP path's once per size: rows, order and moments exactly, positions to 1e-5 with the
                bit-equality recorded (torch's own division and multiply-add decide the last bit there).
    ball tree   scikit-learn's NearestNeighbors(n_neighbors=4, algorithm="ball_tree") fit + kneighbors on the host, which is
                what the reference runs before its loop: at 100k points ONLY, as measured, not extrapolated. Skipped (null)
                where scikit-learn is not installed.
"""
import argparse
import json
import os
import statistics
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

DEV = "cuda"
NAMES = {"xyz": "_xyz", "f_dc": "_features_dc", "f_rest": "_features_rest", "opacity": "_opacity", "scaling": "_scaling",
         "rotation": "_rotation", "scaling_factor": "_scaling_factor"}


def base_state(P, seed=1234):
    g = torch.Generator(device=DEV).manual_seed(seed)
    shapes = {"xyz": (P, 3), "f_dc": (P, 1, 3), "f_rest": (P, 15, 3), "opacity": (P, 1), "scaling": (P, 3), "rotation": (P, 4),
              "scaling_factor": (P, 1)}
    params = {k: torch.randn(s, device=DEV, generator=g) for k, s in shapes.items()}
    x = torch.rand(P, 3, device=DEV, generator=g) * 2 - 1
    x[: P - P // 8] *= 0.05                                         # seven eighths of the points in the core
    params["xyz"] = x.contiguous()
    moments = {k: (torch.randn(s, device=DEV, generator=g) * 1e-3, torch.rand(s, device=DEV, generator=g) * 1e-6) for k, s in shapes.items()}
    return params, moments


def hip_model(params, moments):
    from c3dgs_amd.model import GaussianModel
    from c3dgs_amd.pipeline import OptimizationParams
    m = GaussianModel(3, quantization=True, device=DEV)
    c = {k: v.clone() for k, v in params.items()}
    m.set_tensors(xyz=c["xyz"], features_dc=c["f_dc"], features_rest=c["f_rest"], scaling=c["scaling"], rotation=c["rotation"],
                  opacity=c["opacity"], scaling_factor=c["scaling_factor"])
    m.spatial_lr_scale = 1.0
    m.training_setup(OptimizationParams())
    for k, attr in NAMES.items():
        m.optimizer.state[getattr(m, attr)] = {"step": torch.tensor(1.0), "exp_avg": moments[k][0].clone(), "exp_avg_sq": moments[k][1].clone()}
    return m


def step_of(x, coeff):
    import ctypes
    volume = torch.prod((x.max(dim=0)[0] - x.min(dim=0)[0]).cpu()).item() / x.shape[0]
    return ctypes.c_float(coeff * volume ** (1.0 / 3)).value


def plan(lib_mod, P, d2, step):
    """Both calls of c3dgs_ray_fill_plan with the read of the totals between them, as densify_initial makes them."""
    import ctypes as C
    L = lib_mod.lib()
    s = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    totals = torch.empty(4, dtype=torch.int32, device=DEV)
    ws = torch.empty(int(L.c3dgs_ray_fill_plan_workspace_bytes(P, 0)), dtype=torch.uint8, device=DEV)
    lib_mod.check(L.c3dgs_ray_fill_plan(P, d2.data_ptr(), step, 0, None, None, None, totals.data_ptr(), ws.data_ptr(), ws.numel(), s))
    n0, n1, n2, overflow = totals.tolist()
    n = n0 + n1 + n2
    if overflow or n == 0:
        return n if not overflow else -1, None
    src = torch.empty(n, dtype=torch.int32, device=DEV)
    slot = torch.empty(n, dtype=torch.uint8, device=DEV)
    level = torch.empty(n, dtype=torch.int32, device=DEV)
    ws = torch.empty(int(L.c3dgs_ray_fill_plan_workspace_bytes(P, n)), dtype=torch.uint8, device=DEV)
    lib_mod.check(L.c3dgs_ray_fill_plan(P, d2.data_ptr(), step, n, src.data_ptr(), slot.data_ptr(), level.data_ptr(), totals.data_ptr(),
                                        ws.data_ptr(), ws.numel(), s))
    return n, (src, slot, level)


def totals_only(lib_mod, P, d2, step):
    import ctypes as C
    L = lib_mod.lib()
    totals = torch.empty(4, dtype=torch.int32, device=DEV)
    ws = torch.empty(int(L.c3dgs_ray_fill_plan_workspace_bytes(P, 0)), dtype=torch.uint8, device=DEV)
    lib_mod.check(L.c3dgs_ray_fill_plan(P, d2.data_ptr(), step, 0, None, None, None, totals.data_ptr(), ws.data_ptr(), ws.numel(),
                                        C.c_void_p(torch.cuda.current_stream().cuda_stream)))
    t = totals.tolist()
    return float("inf") if t[3] else sum(t[:3])


def pick_coeff(lib_mod, x, d2):
    """dist_thr_coeff at which the new rows are closest to P: bisection (the row count falls as the step grows)."""
    P = x.shape[0]
    lo, hi = 0.02, 4.0
    for _ in range(24):
        mid = (lo * hi) ** 0.5
        if totals_only(lib_mod, P, d2, step_of(x, mid)) > P:
            lo = mid
        else:
            hi = mid
    return hi


def staged_baseline(params, moments, idx, d2, step):
    """The reference's loop with torch ops on the device, from our neighbour table. -> (params, moments, levels run)."""
    params, moments = dict(params), dict(moments)
    x0 = params["xyz"]
    rel = torch.sqrt(d2) / torch.tensor(step, dtype=torch.float32, device=DEV)
    levels = 0
    for nb in range(3):
        r = rel[:, nb]
        for dist in range(1, int(r.max())):
            slot = r >= dist + 1
            if int(slot.sum()) > 1:
                rows = torch.nonzero(slot).squeeze(1)
                alpha = torch.tensor(float(dist), dtype=torch.float32, device=DEV) / r[rows]
                selected = idx[rows, nb].long()
                coords = x0[rows] * (1.0 - alpha)[:, None] + alpha[:, None] * x0[selected]
                for k in params:
                    new = coords if k == "xyz" else params[k][rows]
                    params[k] = torch.cat((params[k], new), dim=0)
                    moments[k] = (torch.cat((moments[k][0], torch.zeros_like(new)), dim=0),
                                  torch.cat((moments[k][1], torch.zeros_like(new)), dim=0))
                levels += 1
    return params, moments, levels


def timed(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    a.record()
    out = fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b), out


def ball_tree_seconds(x):
    try:
        from sklearn.neighbors import NearestNeighbors
    except ImportError:
        return None
    data = x.cpu().numpy()
    t0 = time.perf_counter()
    NearestNeighbors(n_neighbors=4, algorithm="ball_tree").fit(data).kneighbors(data)
    return time.perf_counter() - t0


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", default="100000,1000000,3000000")
    ap.add_argument("--calls", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r08_densify_initial_time.json"))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("time_densify_initial.py measures on the GPU; there is no CPU path")
    import ctypes as C
    from c3dgs_amd import _lib
    from c3dgs_amd.knn import knn3
    results, tree = [], None
    for P in [int(s) for s in args.sizes.split(",")]:
        params, moments = base_state(P)
        x = params["xyz"]
        idx, d2 = knn3(x)
        coeff = pick_coeff(_lib, x, d2)
        step = step_of(x, coeff)
        ms = {k: [] for k in ("knn3", "plan", "apply", "xyz", "whole", "baseline")}
        rec, xyz_equal, xyz_diff = None, None, None
        for it in range(args.warmup + args.calls):
            t_knn, (idx, d2) = timed(lambda: knn3(x))
            t_plan, (n, (src, slot, level)) = timed(lambda: plan(_lib, P, d2, step))
            m = hip_model(params, moments)
            t_apply, _ = timed(lambda: m._append_clones(src))
            out = m._xyz.detach()[P:]
            t_xyz, _ = timed(lambda: _lib.check(_lib.lib().c3dgs_ray_fill_xyz(
                P, x.data_ptr(), idx.data_ptr(), d2.data_ptr(), step, n, src.data_ptr(), slot.data_ptr(), level.data_ptr(), out.data_ptr(),
                C.c_void_p(torch.cuda.current_stream().cuda_stream))))
            del m, out
            m = hip_model(params, moments)
            t_whole, (wsrc, _, wlevel, totals) = timed(lambda: m.densify_initial(coeff))
            with torch.no_grad():
                t_base, (bp, bm, levels) = timed(lambda: staged_baseline(params, moments, idx, d2, step))
            if it == 0:                                            # the two agree, bit for bit
                if not (torch.equal(wsrc, src) and torch.equal(wlevel, level)):
                    raise SystemExit(f"P={P}: the method's plan differs from the staged plan call")
                for k, attr in NAMES.items():                      # same rows in the same order; positions compared below
                    p = getattr(m, attr)
                    st = m.optimizer.state[p]
                    if k != "xyz" and not torch.equal(p.detach(), bp[k]):
                        raise SystemExit(f"P={P}: {k} differs between the HIP path and the staged torch sequence")
                    if not (torch.equal(st["exp_avg"], bm[k][0]) and torch.equal(st["exp_avg_sq"], bm[k][1])):
                        raise SystemExit(f"P={P}: moments of {k} differ between the HIP path and the staged torch sequence")
                xyz_equal = torch.equal(m._xyz.detach(), bp["xyz"])
                xyz_diff = float((m._xyz.detach() - bp["xyz"]).abs().max())
                if xyz_diff > 1e-5:
                    raise SystemExit(f"P={P}: positions differ by {xyz_diff} between the HIP path and the staged torch sequence")
            rec = {"rows_in": P, "rows_out": P + n, "new_rows_per_slot": list(totals), "dist_thr_coeff": coeff, "step": step,
                   "largest_level": int(level.max()), "non_empty_levels_of_the_baseline": levels,
                   "baseline_positions_bit_equal": xyz_equal, "baseline_positions_max_abs_diff": xyz_diff}
            del m, bp, bm
            if it >= args.warmup:
                for k, v in (("knn3", t_knn), ("plan", t_plan), ("apply", t_apply), ("xyz", t_xyz), ("whole", t_whole), ("baseline", t_base)):
                    ms[k].append(v)
        med = {k: statistics.median(v) for k, v in ms.items()}
        rec.update({"stage_ms_median": {k: med[k] for k in ("knn3", "plan", "apply", "xyz")}, "whole_call_ms_median": med["whole"],
                    "staged_torch_baseline_ms_median": med["baseline"], "ratio_baseline_over_whole": med["baseline"] / med["whole"],
                    "whole_call_ms_min_max": [min(ms["whole"]), max(ms["whole"])],
                    "staged_torch_baseline_ms_min_max": [min(ms["baseline"]), max(ms["baseline"])], "calls": args.calls})
        if P == 100_000:
            tree = {"points": P, "seconds": ball_tree_seconds(x),
                    "note": "host, fit + kneighbors(k=4), one run; what the reference runs before its loop; not extrapolated, not part "
                            "of the baseline above, which starts from our neighbour table"}
        print(json.dumps(rec), flush=True)
        results.append(rec)
        del params, moments, x, idx, d2, src, slot, level
        torch.cuda.empty_cache()
    out = {"what": "GaussianModel.densify_initial (HIP) against the reference's staged sequence restated with torch ops on the same "
                   "device from our neighbour table (one torch.cat of every parameter and moment tensor per non-empty level); time "
                   "between two stream events around the work, host reads included, medians",
           "device": torch.cuda.get_device_name(0), "sizes": results, "scikit_learn_ball_tree_at_100k_only": tree}
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(out, f, indent=1)
    print("wrote", args.out)


if __name__ == "__main__":
    main()
