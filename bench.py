#!/usr/bin/env python3
"""bench.py -- headline benchmark of the hot path on MI355X.

    python bench.py --gpus N --steps K --warmup W [--dump-outputs DIR] [--full]
        N > 1 under torch.distributed.run (WORLD_SIZE set): this process is one rank.
        N > 1 started plainly: the parent starts N rank processes itself (one per GPU, RCCL rendezvous on 127.0.0.1) BEFORE it
        touches the GPU, relays rank 0's JSON line and exits with the worst child code.

Metric (BASELINE.json): raster views/sec, forward+backward, 1920x1080.  The N=1 workload is
BASELINE.json configs[2]: 3M synthetic Gaussians (synth-v1), SH degree 3, the indexed-camera rasterizer the QAT loop
(finetune.py) uses, clamp_color=True.  A step = mark_visible + forward + backward of ONE view through the package's
autograd Function, inputs resident in HBM.  The raster path does not shard a single view ("replicas
only"), so with --gpus N every rank renders its own replica and `value` is the whole-job views/s (weak scaling).

A plain run sets up, warms up, times exactly K steps and prints the headline line (`value`, `ms_per_step` = ms of one timed
step, no event pair inside the timed region).  --dump-outputs DIR then also writes what the last timed step returned to its
caller (dump_outputs).  Everything below is measured only with --full.

Extra objects on the same JSON line (--full):
  roofline      dominant kernel: algorithmic bytes per launch (SURVEY.md 8(d) formula) / live HIP-event duration; `traffic` = HBM
                bytes per launch from two rocprofv3 --pmc passes (FETCH_SIZE, WRITE_SIZE) that THIS invocation runs on a child
                copy of itself (N = 1, no --no-* option; otherwise the committed profiles/traffic_latest.json), `traffic_source` says which
  cpu_baseline  the oracle (CPU restatement, OpenMP) timed on this box's host cores on a bounded sample
  stages        per-stage mean ms from the same HIP events (all kernels of the view)
  parity        HIP vs oracle on THIS workload at full size (integers equal, PSNR, gradient rel-inf; tests/fullsize.py),
                reusing the oracle view the cpu_baseline leg computes (N = 1 only)
  roofline_blend  the roofline object of BOTH blend kernels (render_forward, render_backward)
  sizes         the other sizes / shapes BASELINE.json's metric names, timed in this same invocation: configs[1] = 1M forward-only
                (non-indexed and indexed), 1M and 6M fwd+bwd with the headline's step shape; each with P / V / R
  heavy_tail    robustness (timing only): the 3M scene with scale = exp(N(log 0.009, 1.2^2)) -- R/P, deepest tile, stage times
  vq.slice_step_ms  one rank's Lloyd step (draw -> update, no collective) on a 2^15 / 2^16-point slice of the 2^18 batch
  vq.cov        config 4's covariance codebook loop (D = 6, K = 2048, 2^20-point batches), HBM-bytes roofline per SURVEY 8(d)
  ranks_seen    all-reduce of ones over the job's ranks (must equal n_gpus)
  vq            sensitivity-weighted VQ Lloyd steps/s on config 4's colour shape THROUGH c3dgs_amd.vq_features(group=...)
                itself (batch draws, collectives and EMA update included), sharded over the N ranks (RCCL), its final
                assignment, and (N = 1) vq.cpu_baseline: the reference's PyTorch-CPU loop restated (oracle/vq_torch.py)
  (N = 1 only)  qat_loop: the step + fused L1/SSIM loss; qat_model: the whole QAT view / iteration from raw parameters (fused
                glue + fused Adam next to the reference's torch glue + torch Adam); postvq_index_layout: the headline step with
                the codebook indices laid out as compression/vq.py's join_features produces them
  device_allocs_in_timed_region   hipMalloc calls of torch's caching allocator during the K timed steps (expected 0)
  host_gc_ms                      time Python's cyclic collector ran inside the timed region (expected ~0; see _quiesce)
"""
import argparse
import json
import math
import os
import sys
import time

ROOT = os.path.dirname(os.path.abspath(__file__))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

import torch  # noqa: E402
import torch.distributed as dist  # noqa: E402

HBM_PEAK_GBS = 8000.0          # MI355X_MICROARCH.md: HBM3E 8.0 TB/s spec (6.29 TB/s measured float4 copy)
# Host-side hygiene of the timed regions: a full pass of Python's cyclic collector costs 30-50 ms in this process (torch's
# object graph), i.e. more than a whole 20-step region; it fires after a fixed number of container allocations, wherever the
# program happens to be. Each timed loop therefore starts from an emptied young generation (gc.collect() outside the timing,
# the collector stays ENABLED) and reports the collector time that fell inside it (`host_gc_ms`), so a distorted line shows.
_GC = {"ms": 0.0, "t": 0.0}


def _gc_cb(phase, info):
    if phase == "start":
        _GC["t"] = time.perf_counter()
    else:
        _GC["ms"] += (time.perf_counter() - _GC["t"]) * 1e3


def _quiesce():
    import gc
    if _gc_cb not in gc.callbacks:
        gc.callbacks.append(_gc_cb)
    gc.collect()
    return _GC["ms"]


MFMA_F32_PEAK_TFLOPS = 157.3   # f32-in MFMA dense peak
MFMA_F16_PEAK_TFLOPS = 2500.0  # dense f16 / bf16 MFMA peak (MI355X_MICROARCH.md, Matrix cores)


def alg_bytes(stage, P, V, R, T, N, M, bit, indexed=True):
    """Algorithmic HBM bytes of one launch of `stage` -- the per-term formula of SURVEY.md section 8(d)."""
    G_in = 48 if indexed else 28
    G_out = 4 if indexed else 28
    f = {
        "mark_visible": P * (12 + 1),
        "preprocess": P * (12 + 4 + 4) + V * (4 + 12 * M + G_in) + V * (4 + 8 + 24 + 16 + 12 + 3),
        "scan": 8 * P,
        "duplicate_with_keys": 4 * P + 16 * V + 12 * R,
        "sort": (24 * math.ceil((32 + bit) / 8) + 8) * R,
        "identify_ranges": 8 * R + 8 * T,
        "render_forward": 8 * T + 40 * R + 20 * N,
        "zero_partials": 36 * R,
        "render_backward": 8 * T + 40 * R + 8 * N + 12 * N + 72 * R,
        "backward_preprocess": V * (12 + 4 + 24 + 16 + 24 + 12) + V * (12 + 12 + 12 * M + 3 + G_in + 24 + 12)
                               + V * (12 + 12 * M + G_out),
    }
    return float(f[stage])


def higher_msb(n):
    msb, step = 16, 16
    while step > 1:
        step //= 2
        msb = msb + step if (n >> msb) else msb - step
    return msb + 1 if (n >> msb) else msb


def build_workload(P, W, H, focal, device):
    from tests import synth
    intr, ev = synth.camera(W, H, focal)
    sc = synth.scene(P, W, H, focal, seed=1234, sh_degree=3)
    ix = synth.index_scene(sc)
    t = {k: v.to(device) for k, v in ix.items()}
    dL = synth.grad_image(W, H).to(device)
    return intr, ev, t, dL, ix


def launch_ranks(n, argv):
    """`bench.py --gpus N` started without a launcher: start N rank processes (RANK / LOCAL_RANK / WORLD_SIZE / MASTER_* as
    torch.distributed.run would set them) from a parent that has NOT touched the GPU, relay rank 0's stdout, return the worst
    exit code. Children are ordinary child processes (no exec of a GPU-initialised process anywhere)."""
    import socket
    import subprocess
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    port = s.getsockname()[1]
    s.close()
    import tempfile
    procs = []
    out0 = tempfile.TemporaryFile(mode="w+")
    for r in range(n):
        env = dict(os.environ, RANK=str(r), LOCAL_RANK=str(r), WORLD_SIZE=str(n), LOCAL_WORLD_SIZE=str(n),
                   MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
        env.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")
        procs.append(subprocess.Popen([sys.executable, os.path.abspath(__file__)] + argv, env=env,
                                      stdout=out0 if r == 0 else subprocess.DEVNULL))
    worst = 0
    while any(p.poll() is None for p in procs):
        failed = [p for p in procs if p.poll() not in (None, 0)]
        if failed:                                    # a dead rank leaves the others waiting in a collective: stop them
            worst = max(abs(p.returncode) for p in failed)
            for p in procs:
                if p.poll() is None:
                    p.kill()
            break
        time.sleep(0.1)
    worst = max([worst] + [abs(p.wait()) for p in procs])
    out0.seek(0)
    sys.stdout.write(out0.read())
    sys.stdout.flush()
    return worst


def selftest_launch(backend):
    """Rendezvous + one all-reduce + the JSON line, nothing else: what the CPU test of the launcher runs (gloo)."""
    rank, world = int(os.environ.get("RANK", "0")), int(os.environ.get("WORLD_SIZE", "1"))
    if world > 1:
        os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
        dist.init_process_group(backend)
    ones = torch.ones(1)
    if world > 1:
        dist.all_reduce(ones)
    if rank == 0:
        print(json.dumps({"metric": "launcher self-test", "n_gpus": world, "ranks_seen": int(ones.item()), "selftest": True}))
    if world > 1:
        dist.destroy_process_group()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--gaussians", type=int, default=3_000_000)
    ap.add_argument("--width", type=int, default=1920)
    ap.add_argument("--height", type=int, default=1080)
    ap.add_argument("--no-cpu-baseline", action="store_true")
    ap.add_argument("--no-vq", action="store_true")
    ap.add_argument("--no-extras", action="store_true", help="skip the single-GPU extra lines (qat_loop, qat_model, postvq layout)")
    ap.add_argument("--vq-steps", type=int, default=30)
    ap.add_argument("--no-live-traffic", action="store_true",
                    help="do not run the two rocprofv3 --pmc passes (about 30 s); roofline.traffic then comes from profiles/traffic_latest.json")
    ap.add_argument("--full", action="store_true",
                    help="also run every measurement beyond the headline (stages, roofline, live PMC traffic, other sizes, extras, "
                         "VQ, CPU baselines, parity); the --no-* options select among them")
    ap.add_argument("--dump-outputs", default=None, metavar="DIR",
                    help="write the last timed step's outputs as DIR/<name>.npy (float32; seeded row samples of the large ones)")
    ap.add_argument("--selftest-launch", default=None, metavar="BACKEND", help=argparse.SUPPRESS)
    args = ap.parse_args()

    if "WORLD_SIZE" not in os.environ and args.gpus > 1:
        # no launcher around us: become the launcher (before anything initialises the GPU in this process)
        if args.selftest_launch is None and torch.cuda.device_count() < args.gpus:
            sys.exit(f"bench.py: --gpus {args.gpus} but only {torch.cuda.device_count()} GPU(s) are visible")
        sys.exit(launch_ranks(args.gpus, sys.argv[1:]))
    if args.selftest_launch is not None:
        return selftest_launch(args.selftest_launch)

    rank = int(os.environ.get("RANK", "0"))
    local_rank = int(os.environ.get("LOCAL_RANK", "0"))
    world = int(os.environ.get("WORLD_SIZE", "1"))
    if world != args.gpus and rank == 0:
        print(f"bench.py: --gpus {args.gpus} but the launcher started {world} rank(s); reporting n_gpus = {world}", file=sys.stderr)
    torch.cuda.set_device(local_rank)
    dev = torch.device("cuda", local_rank)
    ranks_seen = 1
    if world > 1:
        os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
        dist.init_process_group("nccl", device_id=dev)
        ones = torch.ones(1, device=dev)
        dist.all_reduce(ones)
        ranks_seen = int(ones.item())

    import c3dgs_amd
    from c3dgs_amd import _lib
    _lib.lib()

    P, W, H, focal = args.gaussians, args.width, args.height, 1200.0
    intr, ev, t, dL, ix_cpu = build_workload(P, W, H, focal, dev)
    rs = c3dgs_amd.GaussianRasterizationSettings(intrinsic=intr, extrinsic_vector=ev.to(dev), bg=torch.zeros(3, device=dev),
                                                 scale_modifier=1.0, sh_degree=3, prefiltered=False, debug=False,
                                                 clamp_color=True)
    rast = c3dgs_amd.GaussianRasterizerIndexed(rs, optimize_camera=True)
    leaves = {k: t[k].clone().requires_grad_() for k in ("means3D", "opacities", "shs", "scales", "scale_factors", "rotations")}
    means2D = torch.zeros_like(leaves["means3D"], requires_grad=True)
    evd = ev.to(dev)
    state = {}

    def step():
        for v in leaves.values():
            v.grad = None
        means2D.grad = None
        visible = rast.markVisible(leaves["means3D"], extrinsic_vector=evd)
        color, radii = rast(means3D=leaves["means3D"], means2D=means2D, opacities=leaves["opacities"],
                            sh_indices=t["sh_indices"], g_indices=t["g_indices"], shs=leaves["shs"], scales=leaves["scales"],
                            scale_factors=leaves["scale_factors"], rotations=leaves["rotations"], extrinsic_vector=evd)
        torch.autograd.backward(color, dL)
        state["color"], state["radii"], state["visible"] = color, radii, visible

    def barrier():
        if world > 1:
            dist.barrier()
        torch.cuda.synchronize()

    # set-up, not warm-up: run until the step time has settled (torch's caching allocator reaches its steady-state
    # block set after ~4 steps; a freshly acquired box can also take a while to ramp clocks / page the libraries in)
    prev = None
    for k in range(40):
        torch.cuda.synchronize()
        tp = time.perf_counter()
        step()
        torch.cuda.synchronize()
        cur = time.perf_counter() - tp
        if k >= 5 and prev is not None and abs(cur - prev) <= 0.05 * min(cur, prev):
            break
        prev = cur
    if args.full:
        # every stage bracketed by HIP events: per-stage means and the dominant kernel (untimed pass; an event pair costs
        # ~10 us of queue time, x11 stages, which does not belong in `value`)
        _lib.profile_enable(True)
        _lib.profile_read()
        for _ in range(max(args.warmup, 3)):
            step()
        torch.cuda.synchronize()
        stages = _lib.profile_read()
        _lib.profile_enable(False)
        raster_names = ("preprocess", "scan", "duplicate_with_keys", "sort", "identify_ranges", "render_forward", "zero_partials",
                        "render_backward", "backward_preprocess", "mark_visible", "depth_sort")
        # the dominant kernel among the stages SURVEY 8(d) gives a byte formula for (the depth sort is part of its one "sort" term)
        dom = max((k for k in stages if k in raster_names and k != "depth_sort"), key=lambda k: stages[k][0] / max(stages[k][1], 1))
    else:
        for _ in range(args.warmup):
            step()
    barrier()
    # timed region: exactly K steps; with --full only the dominant kernel carries an event pair (roofline.achieved is its
    # live average over these same K launches)
    if args.full:
        _lib.profile_enable(True, only=dom)
        _lib.profile_read()
    n_alloc = torch.cuda.memory_stats(dev)["num_device_alloc"]
    gc_ms = _quiesce()
    t0 = time.perf_counter()
    for _ in range(args.steps):
        step()
    torch.cuda.synchronize()
    elapsed = time.perf_counter() - t0
    gc_ms = _GC["ms"] - gc_ms
    n_alloc = torch.cuda.memory_stats(dev)["num_device_alloc"] - n_alloc
    if args.full:
        dom_live = _lib.profile_read()
        _lib.profile_enable(False)
    el = torch.tensor([elapsed], dtype=torch.float64, device=dev)
    if world > 1:
        dist.all_reduce(el, op=dist.ReduceOp.MAX)
    elapsed = float(el.item())
    barrier()
    if args.dump_outputs and rank == 0:
        dump_outputs(args.dump_outputs, state, leaves, means2D)

    out = {
        "metric": "raster views/sec fwd+bwd @1920x1080",
        "value": world * args.steps / elapsed,
        "unit": "views/s",
        "n_gpus": world,
        "ranks_seen": ranks_seen,
        "steps": args.steps,
        "warmup": args.warmup,
        "ms_per_step": 1e3 * elapsed / args.steps,
        "higher_is_better": True,
        "scaling": "weak",
        "vs_baseline": None,
        "dtype": "f32",
        "data": "synthetic",
        "config": {"workload": "BASELINE.json configs[2]: synth-v1 3M Gaussians, SH deg 3, indexed-camera rasterizer "
                               "(QAT inner loop), mark_visible+fwd+bwd, 1 view/step/GPU",
                   "gaussians": P, "width": W, "height": H,
                   "sh_codebook": int(t["shs"].shape[0]), "gaussian_codebook": int(t["scales"].shape[0]),
                   "parallelism": f"replicas x{world}"},
        "device_allocs_in_timed_region": n_alloc,     # hipMalloc calls of the caching allocator (expected: 0)
        "host_gc_ms": round(gc_ms, 3),                # time of Python's cyclic collector inside the timed region (expected: ~0)
    }
    if not args.full:
        return emit(out, rank, world)

    # workload statistics for the roofline
    radii = state["radii"]
    V = int((radii > 0).sum().item())
    from c3dgs_amd import rasterizer as rz
    with torch.no_grad():
        view, proj, campos, tfx, tfy, _, _ = rz.camera_matrices(intr, evd, dev)
        R = rz._C.rasterize_gaussians_indexed(
            rs.bg, t["means3D"], torch.Tensor([]), t["opacities"], t["scales"], t["scale_factors"], t["rotations"], 1.0,
            torch.Tensor([]), view, proj, tfx, tfy, H, W, t["shs"], 3, campos, t["sh_indices"], t["g_indices"], False, False,
            True)[0]
    T = ((W + 15) // 16) * ((H + 15) // 16)
    N = W * H
    bit = higher_msb(T)
    stage_ms = {k: v[0] / max(v[1], 1) for k, v in stages.items()}
    stage_ms[dom] = dom_live[dom][0] / max(dom_live[dom][1], 1)     # the timed region's own measurement
    # the view's algorithmic bytes are those of the REFERENCE's algorithm, whatever stages this build fuses away
    raster_stages = ["mark_visible", "preprocess", "scan", "duplicate_with_keys", "sort", "identify_ranges", "render_forward",
                     "zero_partials", "render_backward", "backward_preprocess"]
    # HBM bytes per launch: rocprofv3 --pmc passes of THIS command (tools/pmc_traffic.sh runs bench.py under the profiler and
    # writes profiles/traffic_latest.json; counters cannot be read from inside the process that is being timed)
    traffic_all, traffic_src = {}, None
    try:
        if P == 3_000_000 and (W, H) == (1920, 1080):
            with open(os.path.join(ROOT, "profiles", "traffic_latest.json")) as f:
                traffic_all = json.load(f)
            traffic_src = "profiles/traffic_latest.json: rocprofv3 --pmc FETCH_SIZE / WRITE_SIZE passes of `python bench.py --full --no-vq " \
                          "--no-cpu-baseline --no-extras` (tools/pmc_traffic.sh; counters cannot be read inside the timed process)"
    except Exception:
        traffic_all = {}
    # ... unless rocprofv3 is at hand: then the two PMC passes (FETCH_SIZE, WRITE_SIZE; MI355X_MICROARCH.md, HBM) are run right
    # here on THIS build and box, each as a child process that profiles this same script on the same workload
    if rank == 0 and world == 1 and not args.no_live_traffic and not args.no_cpu_baseline and "C3DGS_BENCH_CHILD" not in os.environ:
        live = live_pmc_traffic(P, W, H)
        if live:
            traffic_all, traffic_src = live, "live: rocprofv3 --pmc FETCH_SIZE / WRITE_SIZE passes of this script (3 steps each), run by this bench invocation"

    def roofline_of(k):
        b = alg_bytes(k, P, V, R, T, N, 16, bit, indexed=True)
        gbs = b / (stage_ms[k] * 1e-3) / 1e9
        tr = traffic_all.get(k, {}).get("hbm_bytes_per_launch")
        meas = tr / (stage_ms[k] * 1e-3) / 1e9 if tr else None
        # `achieved` / `frac` are ALGORITHMIC bandwidth (SURVEY 8(d) bytes of the reference's algorithm / this kernel's time: how far
        # the kernel is from a byte-bound implementation of that algorithm); `measured_hbm_gbs` / `measured_hbm_frac` are what
        # the HBM actually moved (PMC traffic / the same time) -- the store-and-sum backward moves 0.68x the algorithmic bytes
        return {"bound": "hbm", "kernel": k, "achieved": gbs, "peak": HBM_PEAK_GBS, "unit": "GB/s", "frac": gbs / HBM_PEAK_GBS,
                "achieved_is": "algorithmic bytes per launch (SURVEY 8(d)) / live kernel time",
                "traffic": tr, "measured_hbm_gbs": meas, "measured_hbm_frac": meas / HBM_PEAK_GBS if meas else None,
                "alg_bytes_per_launch": b, "avg_launch_ms": stage_ms[k]}
    view_bytes = sum(alg_bytes(k, P, V, R, T, N, 16, bit, True) for k in raster_stages)

    out["config"].update(visible=V, tile_instances=R)
    out.update({
        "roofline": dict(roofline_of(dom), traffic_source=traffic_src),
        "roofline_blend": {k: roofline_of(k) for k in ("render_forward", "render_backward") if k in stage_ms},
        "stages_ms": {k: round(v, 4) for k, v in sorted(stage_ms.items(), key=lambda kv: -kv[1])},
        # informational: kernels of one step (untimed profiling pass) vs the timed step. A ratio far above 1 means the
        # GPU sat idle waiting for the host during the timed region (seen once on a heavily loaded box: profiles/README.md)
        "step_over_kernel_time": (1e3 * elapsed / args.steps) / max(sum(v for k, v in stage_ms.items() if k in raster_names), 1e-9),
        "view_alg_bytes": view_bytes,
        "view_hbm_frac": view_bytes * (args.steps / elapsed) / 1e9 / HBM_PEAK_GBS,
    })

    # ---- the same step with the fused L1+SSIM loss producing dL/dimage (QAT inner loop of finetune.py:40-49 without the
    # optimizer / FakeQuantize glue): extra, not the headline
    # (single-GPU extras: with N replicas they would only repeat the headline's weak scaling, behind more barriers)
    try:
        if world > 1 or args.no_extras:
            raise _SkipExtra()
        from c3dgs_amd import loss as lossm
        gt = torch.rand(3, H, W, device=dev, generator=torch.Generator(device=dev).manual_seed(5))

        def qat_step():
            for v in leaves.values():
                v.grad = None
            rast.markVisible(leaves["means3D"], extrinsic_vector=evd)
            color, _ = rast(means3D=leaves["means3D"], means2D=means2D, opacities=leaves["opacities"],
                            sh_indices=t["sh_indices"], g_indices=t["g_indices"], shs=leaves["shs"], scales=leaves["scales"],
                            scale_factors=leaves["scale_factors"], rotations=leaves["rotations"], extrinsic_vector=evd)
            lossm.l1_ssim_loss(color, gt, 0.2).backward()

        for _ in range(3):
            qat_step()
        barrier()
        _quiesce()
        tq = time.perf_counter()
        for _ in range(args.steps):
            qat_step()
        torch.cuda.synchronize()
        out["qat_loop"] = {"metric": "views/s render + fused L1+SSIM loss + backward", "value": world * args.steps / (time.perf_counter() - tq)}
    except _SkipExtra:
        pass
    except Exception as e:
        out["qat_loop"] = {"error": repr(e)}

    # ---- the headline step again with the index layout compression/vq.py produces (join_features, vq.py:90-103): most
    # Gaussians point into the 4096-row VQ codebook, the kept ones own one row each, in Gaussian order. synth-v1's indices
    # (the headline) are uniformly random over the whole codebook -- the worst case for the codebook gathers.
    try:
        if world > 1 or args.no_extras:
            raise _SkipExtra()
        out["postvq_index_layout"] = bench_postvq_layout(step, t, P, args.steps, dev, _lib)
    except _SkipExtra:
        pass
    except Exception as e:
        out["postvq_index_layout"] = {"error": repr(e)}

    # ---- the other sizes / shapes of BASELINE.json's metric (1M forward-only = configs[1]; 1M / 6M fwd+bwd) and a heavy-tailed
    # scene (robustness: R / P of real captures), all driver-timed in this same invocation
    try:
        if world > 1 or args.no_extras:
            raise _SkipExtra()
        out["sizes"] = bench_sizes(c3dgs_amd, _lib, dev, args.steps)
    except _SkipExtra:
        pass
    except Exception as e:
        out["sizes"] = {"error": repr(e)}
    try:
        if world > 1 or args.no_extras:
            raise _SkipExtra()
        out["heavy_tail"] = bench_heavy_tail(c3dgs_amd, _lib, dev, args.steps)
    except _SkipExtra:
        pass
    except Exception as e:
        out["heavy_tail"] = {"error": repr(e)}

    # ---- the whole QAT view from the RAW parameters -- getters (activations + FakeQuantize observers +
    # [visible] gathers) + raster + fused loss + backward -- through c3dgs_amd.model.GaussianModel.render (fused glue),
    # next to the reference's composition of the same glue from torch ops / torch.ao modules around the same rasterizer
    try:
        if world > 1 or args.no_extras:
            raise _SkipExtra()
        out["qat_model"] = bench_qat_model(c3dgs_amd, _lib, dev, ix_cpu, intr, evd, W, H, args.steps, barrier, world)
    except _SkipExtra:
        pass
    except Exception as e:
        out["qat_model"] = {"error": repr(e)}

    # ---- VQ (config 4 colour shape), sharded over the ranks with one all-reduce per Lloyd step
    if not args.no_vq:
        try:
            out["vq"] = bench_vq(c3dgs_amd, _lib, dev, rank, world, args.vq_steps, not args.no_cpu_baseline)
        except Exception as e:  # keep the headline line alive
            out["vq"] = {"error": repr(e)}

    # ---- CPU baseline: the oracle on this box's host cores (rank 0, N=1 only) -- and, from the same oracle view, the
    # parity of the HIP path on this very workload
    if rank == 0 and world == 1 and not args.no_cpu_baseline:
        try:
            out["cpu_baseline"], out["parity"] = cpu_baseline_and_parity(ix_cpu, intr, ev, W, H, focal)
        except Exception as e:
            out["cpu_baseline"] = {"error": repr(e)}

    emit(out, rank, world)


def emit(out, rank, world):
    if rank == 0:
        print(json.dumps(out))
    if world > 1:
        dist.destroy_process_group()


DUMP_ROWS = 2 ** 17          # rows kept of a larger per-Gaussian / codebook output
DUMP_SH_ROWS = 2 ** 15       # SH codebook gradient rows are 16 x 3 floats each
DUMP_PIXELS = 2 ** 21        # pixels kept of an image larger than DUMP_IMAGE_BYTES
DUMP_IMAGE_BYTES = 32 * 2 ** 20
DUMP_BUDGET = 64 * 2 ** 20   # bytes of all files together


def _sample_rows(x, n, seed):
    """x, or a fixed seeded sample of n of its rows kept in row order: the same rows for the same shape, whatever the build."""
    if x.shape[0] <= n:
        return x
    import numpy as np
    idx = np.sort(np.random.default_rng(seed).choice(x.shape[0], n, replace=False))
    return x[torch.from_numpy(idx).to(x.device)]


def dump_outputs(d, state, leaves, means2D):
    """--dump-outputs: what the caller of the timed step holds after its last timed step, one float32 DIR/<name>.npy each --
    the image (3 x H x W; a seeded sample of pixel rows [n, 3] when larger than DUMP_IMAGE_BYTES), radii, the visibility flags,
    and the gradient of every input. Outputs longer than DUMP_ROWS rows keep a seeded sample of rows; all per-Gaussian outputs
    share one sample, so their rows line up."""
    import numpy as np
    color = state["color"].detach()
    if color.numel() * 4 > DUMP_IMAGE_BYTES:
        color = _sample_rows(color.reshape(color.shape[0], -1).t(), DUMP_PIXELS, 1)
    arrays = {"color": color, "radii": state["radii"], "visible": state["visible"], "grad_means2D": means2D.grad}
    arrays.update({"grad_" + k: v.grad for k, v in leaves.items()})
    seeds = {"grad_shs": 3, "grad_scales": 4, "grad_rotations": 4}     # codebooks: rows of their own; per-Gaussian outputs: 2
    for k, v in arrays.items():
        if k != "color":
            arrays[k] = _sample_rows(v, DUMP_SH_ROWS if k == "grad_shs" else DUMP_ROWS, seeds.get(k, 2))
    arrays = {k: v.detach().float().cpu().numpy() for k, v in arrays.items()}
    total = sum(a.nbytes for a in arrays.values())
    assert total <= DUMP_BUDGET, f"--dump-outputs: {total} bytes exceed the {DUMP_BUDGET}-byte budget"
    os.makedirs(d, exist_ok=True)
    for k, a in arrays.items():
        np.save(os.path.join(d, k + ".npy"), np.ascontiguousarray(a))


def _scene_step(c3dgs_amd, intr, evd, t, dL, dev, indexed, backward):
    """One view of a scene `t` (device tensors) through the module API: mark_visible + forward (+ backward through autograd),
    the shape of the headline step()."""
    rs = c3dgs_amd.GaussianRasterizationSettings(intrinsic=intr, extrinsic_vector=evd, bg=torch.zeros(3, device=dev), scale_modifier=1.0,
                                                 sh_degree=3, prefiltered=False, debug=False, clamp_color=True)
    names = ("means3D", "opacities", "shs", "scales", "rotations") + (("scale_factors",) if indexed else ())
    leaves = {k: (t[k].clone().requires_grad_() if backward else t[k]) for k in names}
    means2D = torch.zeros_like(t["means3D"], requires_grad=backward)
    rast = c3dgs_amd.GaussianRasterizerIndexed(rs, optimize_camera=True) if indexed else c3dgs_amd.GaussianRasterizer(rs)

    def fwd():
        rast.markVisible(leaves["means3D"], extrinsic_vector=evd)
        if indexed:
            return rast(means3D=leaves["means3D"], means2D=means2D, opacities=leaves["opacities"], sh_indices=t["sh_indices"],
                        g_indices=t["g_indices"], shs=leaves["shs"], scales=leaves["scales"], scale_factors=leaves["scale_factors"],
                        rotations=leaves["rotations"], extrinsic_vector=evd)
        return rast(means3D=leaves["means3D"], means2D=means2D, opacities=leaves["opacities"], shs=leaves["shs"],
                    scales=leaves["scales"], rotations=leaves["rotations"], extrinsic_vector=evd)

    def step():
        if not backward:
            with torch.no_grad():
                return fwd()
        for v in leaves.values():
            v.grad = None
        means2D.grad = None
        color, radii = fwd()
        torch.autograd.backward(color, dL)
        return color, radii
    return step


def _scene_counts(intr, evd, t, dev, indexed, W, H):
    """(V, R, deepest tile list) of a scene from one forward through the C-level entry point."""
    import ctypes as C
    from c3dgs_amd import _lib
    from c3dgs_amd import rasterizer as rz
    E = torch.Tensor([])
    with torch.no_grad():
        view, proj, campos, tfx, tfy, _, _ = rz.camera_matrices(intr, evd, dev)
        bg = torch.zeros(3, device=dev)
        if indexed:
            o = rz._C.rasterize_gaussians_indexed(bg, t["means3D"], E, t["opacities"], t["scales"], t["scale_factors"], t["rotations"], 1.0, E,
                                                  view, proj, tfx, tfy, H, W, t["shs"], 3, campos, t["sh_indices"], t["g_indices"], False, False, True)
        else:
            o = rz._C.rasterize_gaussians(bg, t["means3D"], E, t["opacities"], t["scales"], t["rotations"], 1.0, E, view, proj, tfx, tfy,
                                          H, W, t["shs"], 3, campos, False, False, True)
    il = _lib.ImageLayout()
    _lib.lib().c3dgs_get_image_layout(W, H, C.byref(il))
    T = ((W + 15) // 16) * ((H + 15) // 16)
    rg = o[5][il.ranges:il.ranges + 8 * T].view(torch.int32).view(T, 2).to(torch.int64)
    radii = o[2]
    return int((radii > 0).sum()), int(o[0]), int((rg[:, 1] - rg[:, 0]).max()), radii


def _time_steps(step, steps, warm=3):
    for _ in range(warm):
        step()
    torch.cuda.synchronize()
    gc0 = _quiesce()
    t0 = time.perf_counter()
    for _ in range(steps):
        step()
    torch.cuda.synchronize()
    el = time.perf_counter() - t0
    return {"views_per_s": steps / el, "ms_per_view": 1e3 * el / steps, "steps": steps, "host_gc_ms": round(_GC["ms"] - gc0, 3)}


def bench_sizes(c3dgs_amd, _lib, dev, steps, W=1920, H=1080, focal=1200.0):
    """The other sizes / shapes BASELINE.json's metric names ("1M/3M/6M Gaussians", configs[1] forward-only), driver-timed in the
    same invocation as the headline: configs[1] = 1M synth-v1 forward only (render.py path), non-indexed and indexed; 1M and 6M
    fwd+bwd with the headline's step() shape (indexed QAT path). Each with P / V / R."""
    from tests import synth
    intr, ev = synth.camera(W, H, focal)
    evd = ev.to(dev)
    dL = synth.grad_image(W, H).to(dev)
    out = {}
    n = max(5, min(steps, 20))
    for P in (1_000_000, 6_000_000):
        sc = synth.scene(P, W, H, focal, seed=1234, sh_degree=3)
        ix = synth.index_scene(sc)
        ti = {k: v.to(dev) for k, v in ix.items()}
        V, R, deep, _ = _scene_counts(intr, evd, ti, dev, True, W, H)
        tag = f"{P // 1_000_000}M"
        if P == 1_000_000:
            tn = {k: v.to(dev) for k, v in sc.items()}
            Vn, Rn, _, _ = _scene_counts(intr, evd, tn, dev, False, W, H)
            out["config2_1M_forward_only_non_indexed"] = dict(_time_steps(_scene_step(c3dgs_amd, intr, evd, tn, dL, dev, False, False), n),
                                                              gaussians=P, visible=Vn, tile_instances=Rn)
            out["config2_1M_forward_only_indexed"] = dict(_time_steps(_scene_step(c3dgs_amd, intr, evd, ti, dL, dev, True, False), n),
                                                          gaussians=P, visible=V, tile_instances=R)
            del tn
        out[f"{tag}_fwd_bwd_indexed"] = dict(_time_steps(_scene_step(c3dgs_amd, intr, evd, ti, dL, dev, True, True), n),
                                             gaussians=P, visible=V, tile_instances=R, deepest_tile_list=deep)
        del ti, sc, ix
        torch.cuda.empty_cache()
    return out


def bench_heavy_tail(c3dgs_amd, _lib, dev, steps, P=3_000_000, W=1920, H=1080, focal=1200.0):
    """Robustness line (timing only; parity for screen-filling splats is in tests/test_fuzz_gpu.py): synth-v1 with a HEAVY-TAILED
    scale distribution, scale = exp(N(log 0.009, 1.2^2)) per axis instead of sigma 0.6 -- a per cent of the splats are tens to
    hundreds of pixels wide, R / P rises from 5.5 to the 20-50 of real captures, tile lists get thousands deep. Shows that the
    load-balanced instance emission, the tile sort and the longest-first backward schedule hold up."""
    from tests import synth
    intr, ev = synth.camera(W, H, focal)
    evd = ev.to(dev)
    dL = synth.grad_image(W, H).to(dev)
    sc = synth.scene(P, W, H, focal, seed=1234, sh_degree=3, scale_sigma=1.2)
    ix = synth.index_scene(sc)
    t = {k: v.to(dev) for k, v in ix.items()}
    V, R, deep, radii = _scene_counts(intr, evd, t, dev, True, W, H)
    rq = torch.quantile(radii[radii > 0].float()[:: max(1, V // 1_000_000)], torch.tensor([0.5, 0.9, 0.99, 0.999], device=dev)).tolist()
    step = _scene_step(c3dgs_amd, intr, evd, t, dL, dev, True, True)
    res = dict(_time_steps(step, max(3, min(steps, 8)), warm=2), gaussians=P, visible=V, tile_instances=R, instances_per_gaussian=R / P,
               deepest_tile_list=deep, radius_px_p50_p90_p99_p999=[round(x, 1) for x in rq],
               scene="synth-v1 with scale = exp(N(log 0.009, 1.2^2)) per axis (heavy tail), indexed QAT path, fwd+bwd")
    _lib.profile_enable(True)
    _lib.profile_read()
    for _ in range(3):
        step()
    torch.cuda.synchronize()
    st = _lib.profile_read()
    _lib.profile_enable(False)
    res["stages_ms"] = {k: round(v[0] / max(v[1], 1), 4) for k, v in sorted(st.items(), key=lambda kv: -kv[1][0])}
    del t, sc, ix
    torch.cuda.empty_cache()
    return res


def live_pmc_traffic(P, W, H):
    """HBM bytes per launch of every raster kernel from two rocprofv3 --pmc passes (separate passes for FETCH_SIZE and
    WRITE_SIZE, kernel trace only, units and the gfx950 x2 on FETCH_SIZE as tools/pmc_summarize.py applies them) of a child
    run of this script. None when rocprofv3 is missing or anything goes wrong (the committed profile is used then)."""
    import shutil
    import subprocess
    import tempfile
    if not shutil.which("rocprofv3"):
        return None
    try:
        sys.path.insert(0, os.path.join(ROOT, "tools"))
        import pmc_summarize
        out = tempfile.mkdtemp(prefix="c3dgs_pmc_")
        env = dict(os.environ, TMPDIR="/tmp", C3DGS_BENCH_CHILD="1")
        files = {}
        for counter, tag in (("FETCH_SIZE", "f"), ("WRITE_SIZE", "w")):
            cmd = ["rocprofv3", "--pmc", counter, "--kernel-trace", "--output-format", "csv", "-d", os.path.join(out, tag), "-o", tag, "--",
                   sys.executable, os.path.join(ROOT, "bench.py"), "--full", "--steps", "3", "--warmup", "1", "--no-vq", "--no-cpu-baseline",
                   "--no-extras", "--gaussians", str(P), "--width", str(W), "--height", str(H)]
            subprocess.run(cmd, cwd=ROOT, env=env, stdout=subprocess.DEVNULL, stderr=subprocess.DEVNULL, timeout=150, check=True)
            import glob
            hits = glob.glob(os.path.join(out, tag, "**", "*counter_collection.csv"), recursive=True)
            if not hits:
                return None
            files[tag] = hits[0]
        res = pmc_summarize.summarize(files["f"], files["w"])
        shutil.rmtree(out, ignore_errors=True)
        return res or None
    except Exception:
        return None


def bench_postvq_layout(step, t, P, steps, dev, _lib):
    """Same scene, same codebook sizes; only sh_indices / g_indices change (and so which rows the kernels gather)."""
    g = torch.Generator().manual_seed(17)

    def layout(n_rows, n_vq=4096):
        kept = max(min(n_rows - n_vq, P), 0)                      # rows past the VQ codebook: one per kept Gaussian
        idx = torch.randint(0, min(n_vq, n_rows), (P,), generator=g, dtype=torch.int64)
        if kept:
            who = torch.randperm(P, generator=g)[:kept].sort().values
            idx[who] = n_vq + torch.arange(kept, dtype=torch.int64)
        return idx.to(dev)

    saved = t["sh_indices"], t["g_indices"]
    try:
        t["sh_indices"], t["g_indices"] = layout(t["shs"].shape[0]), layout(t["scales"].shape[0])
        prev = None
        for k in range(40):                                        # until the step time has settled (as for the headline)
            torch.cuda.synchronize()
            tp = time.perf_counter()
            step()
            torch.cuda.synchronize()
            cur = time.perf_counter() - tp
            if k >= 5 and prev is not None and abs(cur - prev) <= 0.05 * min(cur, prev):
                break
            prev = cur
        n_alloc = torch.cuda.memory_stats(dev)["num_device_alloc"]
        gc_ms = _quiesce()
        t0 = time.perf_counter()
        for _ in range(steps):
            step()
        torch.cuda.synchronize()
        el = time.perf_counter() - t0
        gc_ms = _GC["ms"] - gc_ms
        n_alloc = torch.cuda.memory_stats(dev)["num_device_alloc"] - n_alloc
        _lib.profile_enable(True)
        _lib.profile_read()
        for _ in range(5):
            step()
        torch.cuda.synchronize()
        st = _lib.profile_read()
        _lib.profile_enable(False)
    finally:
        t["sh_indices"], t["g_indices"] = saved
    return {"metric": "views/s fwd+bwd, indices as join_features lays them out", "value": steps / el, "ms_per_step": 1e3 * el / steps,
            "device_allocs_in_timed_loop": n_alloc, "host_gc_ms": round(gc_ms, 3),
            "stages_ms": {k: round(v[0] / max(v[1], 1), 4) for k, v in sorted(st.items(), key=lambda kv: -kv[1][0])[:6]}}


class _SkipExtra(Exception):
    pass


def bench_qat_model(c3dgs_amd, _lib, dev, ix_cpu, intr, evd, W, H, steps, barrier, world):
    from c3dgs_amd import loss as lossm
    from c3dgs_amd import model as gm
    from tests import synth
    raw = synth.raw_params(ix_cpu)
    m = gm.GaussianModel(3, quantization=True, device=dev).set_tensors(**raw)

    class Cam:
        intrinsic, extrinsic_vector = intr.to(dev), evd
    cam, pipe, bg = Cam(), gm.PipelineParams(), torch.zeros(3, device=dev)
    gt = torch.rand(3, H, W, device=dev, generator=torch.Generator(device=dev).manual_seed(5))

    def fused_step():
        for p in m.parameters():
            p.grad = None
        lossm.l1_ssim_loss(m.render(cam, pipe, bg)["render"], gt, 0.2).backward()

    # the reference's glue (scene/gaussian_model.py:213-267, 766-886): torch ops + torch.ao modules + boolean gathers
    mods = {k: torch.ao.quantization.FakeQuantize(dtype=torch.qint8).to(dev) for k in gm.SLOTS}
    leaves = {k: v.to(dev).clone().requires_grad_(v.is_floating_point()) for k, v in raw.items()}
    rs = c3dgs_amd.GaussianRasterizationSettings(intrinsic=cam.intrinsic, extrinsic_vector=evd, bg=bg, scale_modifier=1.0,
                                                 sh_degree=3, prefiltered=False, debug=False, clamp_color=True)
    rast = c3dgs_amd.GaussianRasterizerIndexed(rs, optimize_camera=True)
    nz = torch.nn.functional.normalize

    def torch_glue_step():
        for v in leaves.values():
            v.grad = None
        xyz = gm.FakeQuantizationHalf.apply(leaves["xyz"])
        opacity = mods["opacity"](torch.sigmoid(leaves["opacity"]))
        scales = mods["scaling"](nz(torch.relu(leaves["scaling"])))
        rotations = nz(mods["rotation"](leaves["rotation"]))
        sfac = torch.exp(mods["scaling_factor"](leaves["scaling_factor"]))
        shs = torch.cat((mods["features_dc"](leaves["features_dc"]), mods["features_rest"](leaves["features_rest"])), dim=1)
        screen = torch.zeros_like(xyz, requires_grad=True)
        vis = rast.markVisible(xyz, extrinsic_vector=evd)
        color, _ = rast(means3D=xyz[vis], means2D=screen[vis], shs=shs, sh_indices=leaves["feature_indices"][vis],
                        g_indices=leaves["gaussian_indices"][vis], colors_precomp=None, opacities=opacity[vis], scales=scales,
                        scale_factors=sfac[vis], rotations=rotations, cov3D_precomp=None, extrinsic_vector=evd)
        lossm.l1_ssim_loss(color, gt, 0.2).backward()

    # the complete QAT iteration of finetune.py:29-66 incl. optimizer.step(): per-group learning rates of
    # scene/gaussian_model.py:296-308, eps 1e-15
    from c3dgs_amd import optim as optm
    lrs = (0.00016, 0.0025, 0.0025 / 20.0, 0.005, 0.005, 0.001, 0.05)

    def groups(ps):
        return [{"params": [p], "lr": lr} for p, lr in zip(ps, lrs)]
    opt_fused = optm.Adam(groups(m.parameters()), lr=0.0, eps=1e-15)
    opt_torch = torch.optim.Adam(groups([leaves[k] for k in ("xyz", "features_dc", "features_rest", "scaling", "scaling_factor",
                                                               "rotation", "opacity")]), lr=0.0, eps=1e-15)

    def fused_iteration():
        lossm.l1_ssim_loss(m.render(cam, pipe, bg)["render"], gt, 0.2).backward()
        opt_fused.step()
        opt_fused.zero_grad(set_to_none=True)

    def torch_iteration():
        torch_glue_step()
        opt_torch.step()
        opt_torch.zero_grad(set_to_none=True)

    res = {"metric": "views/s of a whole QAT view from raw parameters (getters + raster + L1/SSIM loss + backward)"}
    for name, fn in (("fused_glue", fused_step), ("torch_glue", torch_glue_step), ("iteration_fused_glue_fused_adam", fused_iteration),
                     ("iteration_torch_glue_torch_adam", torch_iteration)):
        for _ in range(4):
            fn()
        barrier()
        gc_ms = _quiesce()
        t0 = time.perf_counter()
        for _ in range(steps):
            fn()
        torch.cuda.synchronize()
        el = time.perf_counter() - t0
        res[name] = {"views_per_s": world * steps / el, "ms_per_view": 1e3 * el / steps, "host_gc_ms": round(_GC["ms"] - gc_ms, 3)}
    _lib.profile_enable(True)                                  # separate, untimed pass for the glue kernels' durations
    _lib.profile_read()
    for _ in range(5):
        fused_step()
    torch.cuda.synchronize()
    st = _lib.profile_read()
    _lib.profile_enable(False)
    res["glue_stages_ms"] = {k: round(v[0] / max(v[1], 1), 4) for k, v in st.items() if k.startswith("qat_")}
    _lib.profile_enable(True, only="adam_step")
    _lib.profile_read()
    for _ in range(5):
        fused_iteration()
    torch.cuda.synchronize()
    st = _lib.profile_read()
    _lib.profile_enable(False)
    res["adam_step_ms"] = round(st["adam_step"][0] / max(st["adam_step"][1], 1), 4) if "adam_step" in st else None
    res["glue_only_ms"] = {"fused": round(sum(res["glue_stages_ms"].values()), 4)}
    return res


def bench_vq(c3dgs_amd, _lib, dev, rank, world, steps, cpu_baseline):
    """Config 4 colour codebook: N=5.4M x 48 features, K=4096, batch 2^18 -- timed THROUGH the product entry point
    c3dgs_amd.vq_features (compression/vq.py:49-87): batch draws, assignment, accumulation, the step's all-reduce over the
    ranks and the EMA update are all inside the timed Lloyd loop; the sharded final assignment is timed separately."""
    from c3dgs_amd import vq as vqm
    g = torch.Generator(device=dev).manual_seed(7)
    N, D, K, B = 5_400_000, 48, 4096, 2 ** 18
    feats = torch.randn(N, D, device=dev, generator=g) * 0.1
    imp = torch.rand(N, device=dev, generator=g).pow(4)
    group = True if world > 1 else None
    torch.manual_seed(11)                                     # the batch draws come from the CPU generator (vq.py:69)

    def run(n_steps, profile_stage=None):
        st = {}
        if profile_stage:
            _lib.profile_enable(True, only=profile_stage)
            _lib.profile_read()
        vqm.vq_features(feats, imp, K, B, n_steps, silent=True, group=group, stats=st)
        if profile_stage:
            st["stage"] = _lib.profile_read().get(profile_stage, (0.0, 0))
            _lib.profile_enable(False)
        return st

    run(3)                                                    # warm-up: RCCL communicators, allocator, pinned draw ring
    first = run(1, "vq_accumulate")                           # the FIRST Lloyd step after uniform_init: every point lands on a
    first_acc_ms = first["stage"][0] / max(first["stage"][1], 1)   # handful of codewords (worst-case contention of the sums)
    if world > 1:
        dist.barrier()
    torch.cuda.synchronize()
    _quiesce()
    st = run(steps)                                           # timed: lloyd_seconds brackets exactly `steps` Lloyd steps
    el = torch.tensor([st["lloyd_seconds"], st["final_assignment_seconds"]], dtype=torch.float64, device=dev)
    if world > 1:
        dist.all_reduce(el, op=dist.ReduceOp.MAX)
    lloyd_s, final_s = float(el[0]), float(el[1])
    prof = run(steps, "weighted_distance")                    # untimed passes for the kernels' own durations
    wd_ms = prof["stage"][0] / max(prof["stage"][1] - 1, 1) if prof["stage"][1] > 1 else 0.0   # (includes the final assignment launch)
    acc = run(steps, "vq_accumulate")["stage"]
    # the assignment launches of the Lloyd steps only: subtract the final assignment's share by timing it alone
    only_final = run(0, "weighted_distance")["stage"]
    wd_step_ms = (prof["stage"][0] - only_final[0]) / max(prof["stage"][1] - only_final[1], 1)
    flops = 2.0 * (B / world) * K * D
    out = {"metric": "vq_lloyd_steps_per_s", "value": steps / lloyd_s, "unit": "steps/s", "ms_per_step": 1e3 * lloyd_s / steps,
           "n_gpus": world, "scaling": "strong", "steps": steps,
           "config": {"workload": "config 4 colour: N=5.4M, D=48, K=4096, batch 2^18 per step split over the ranks; "
                                  "c3dgs_amd.vq_features(group=...) end to end", "batch": B},
           "final_assignment_ms": 1e3 * final_s, "collectives_per_step": 1 if world > 1 else 0,
           "assign_kernel_ms": wd_step_ms, "accumulate_kernel_ms": acc[0] / max(acc[1], 1),
           "accumulate_first_step_ms": first_acc_ms,
           # the search runs on the fp16 matrix cores with every multiply as three fp16 piece products (csrc/vq.hip): `roofline`
           # prices the EXECUTED flops (3 x 2 N K D) against the dense fp16 MFMA peak; `survey_8d` is SURVEY 8(d)'s formula
           # (algorithmic 2 N K D against the fp32 MFMA peak), which this formulation exceeds
           "roofline": {"bound": "mfma", "kernel": "weighted_distance", "achieved": 3 * flops / (wd_step_ms * 1e-3) / 1e12 if wd_step_ms else None,
                        "peak": MFMA_F16_PEAK_TFLOPS, "unit": "TFLOP/s",
                        "frac": 3 * flops / (wd_step_ms * 1e-3) / 1e12 / MFMA_F16_PEAK_TFLOPS if wd_step_ms else None, "traffic": None,
                        "executed": "3 fp16 piece products per multiply (xh ch + xh cl + xl ch), fp32 accumulate; exact re-scan of the ambiguous points included in the time"},
           "survey_8d": {"achieved": flops / (wd_step_ms * 1e-3) / 1e12 if wd_step_ms else None, "peak": MFMA_F32_PEAK_TFLOPS,
                         "unit": "TFLOP/s", "frac": flops / (wd_step_ms * 1e-3) / 1e12 / MFMA_F32_PEAK_TFLOPS if wd_step_ms else None}}
    del wd_ms
    # ---- what ONE rank of a sharded run executes per Lloyd step, without the collective: the same 2^18-point batch is drawn, a
    # 2^15 / 2^16-point slice of it is assigned + accumulated, the update runs -- the fixed per-step part that bounds strong scaling
    if world == 1:
        try:
            out["slice_step_ms"] = {str(n): vq_slice_step(vqm, feats, imp, K, B, n, max(steps, 100), dev) for n in (2 ** 15, 2 ** 16, 2 ** 18)}
            out["slice_step_ms"]["what"] = ("ms per full Lloyd step (batch draw -> update, no collective) when only the first n points of each "
                                            "2^18-point batch are this rank's: n = 2^15 / 2^16 = one of 8 / 4 ranks; launches per step: "
                                            "draws_to_indices, search, exact re-scan, accumulate (+ distance sum), update (+ next split, clears) "
                                            "= 5 kernels, no copy (the conversion kernel reads the raw draws from page-locked host memory; profiles/r03_vq_step_kernel_trace.txt)")
        except Exception as e:
            out["slice_step_ms"] = {"error": repr(e)}
    # ---- config 4's OTHER codebook: normalised covariances, D = 6, K = 2048, batches of 2^20, scale_normalize (compress_covariance,
    # compression/vq.py:149-191). Arithmetic intensity too low for the matrix cores to matter: priced against HBM bytes,
    # assignment N (4 D + 12) + 4 K D per launch (+ the update's B (4 D + 12) + 8 K (D + 1) per step).
    try:
        Nc, Dc, Kc, Bc = 4_500_000, 6, 2048, 2 ** 20
        fc = torch.randn(Nc, Dc, device=dev, generator=g) * 0.1
        fc[:, [0, 3, 5]] = fc[:, [0, 3, 5]].abs() + 0.2
        fc = fc / (fc[:, 0] + fc[:, 3] + fc[:, 5])[:, None]
        ic = torch.rand(Nc, device=dev, generator=g).pow(4)

        def run_cov(n_steps, profile_stage=None):
            stc = {}
            if profile_stage:
                _lib.profile_enable(True, only=profile_stage)
                _lib.profile_read()
            vqm.vq_features(fc, ic, Kc, Bc, n_steps, scale_normalize=True, silent=True, group=group, stats=stc)
            if profile_stage:
                stc["stage"] = _lib.profile_read().get(profile_stage, (0.0, 0))
                _lib.profile_enable(False)
            return stc
        run_cov(2)
        if world > 1:
            dist.barrier()
        torch.cuda.synchronize()
        _quiesce()
        stc = run_cov(steps)
        elc = torch.tensor([stc["lloyd_seconds"], stc["final_assignment_seconds"]], dtype=torch.float64, device=dev)
        if world > 1:
            dist.all_reduce(elc, op=dist.ReduceOp.MAX)
        profc, finc = run_cov(steps, "weighted_distance")["stage"], run_cov(0, "weighted_distance")["stage"]
        wdc_ms = (profc[0] - finc[0]) / max(profc[1] - finc[1], 1)
        bytes_assign = (Bc / world) * (4 * Dc + 12) + 4 * Kc * Dc
        out["cov"] = {"metric": "vq_lloyd_steps_per_s", "value": steps / float(elc[0]), "unit": "steps/s", "ms_per_step": 1e3 * float(elc[0]) / steps,
                      "steps": steps, "n_gpus": world,
                      "config": {"workload": "config 4 covariance: N=4.5M, D=6, K=2048, batch 2^20 per step split over the ranks, "
                                             "scale_normalize; c3dgs_amd.vq_features end to end", "batch": Bc},
                      "final_assignment_ms": 1e3 * float(elc[1]), "assign_kernel_ms": wdc_ms,
                      "roofline": {"bound": "hbm", "kernel": "weighted_distance", "achieved": bytes_assign / (wdc_ms * 1e-3) / 1e9 if wdc_ms else None,
                                   "peak": HBM_PEAK_GBS, "unit": "GB/s", "frac": bytes_assign / (wdc_ms * 1e-3) / 1e9 / HBM_PEAK_GBS if wdc_ms else None,
                                   "traffic": None, "alg_bytes_per_launch": bytes_assign,
                                   "note": "N (4 D + 12) + 4 K D bytes per assignment (SURVEY 8(d)); the search itself is bound by its "
                                           "2 N K D = 25.8 GFLOP of fp16 split-operand MFMA + top-2 vector work, not by these 38 MB"}}
        del fc, ic
    except Exception as e:
        out["cov"] = {"error": repr(e)}
    if cpu_baseline and rank == 0 and world == 1:
        try:
            out["cpu_baseline"] = vq_cpu_baseline(N, D, K, B)
        except Exception as e:
            out["cpu_baseline"] = {"error": repr(e)}
    return out


def vq_slice_step(vqm, feats, imp, K, B, n_slice, steps, dev):
    """The inner loop of c3dgs_amd.vq.vq_features (same objects: _BatchDraws, HipOps.step_sums / step_apply) as ONE rank of a
    sharded run executes it, minus the all-reduce: batch of B draws, the first n_slice of them assigned and accumulated, update."""
    N, D = feats.shape
    model = vqm.VectorQuantize(channels=D, codebook_size=K, decay=0.8).to(dev)
    model.uniform_init(feats)
    err = torch.zeros(steps + 8, dtype=torch.float64, device=dev)
    state = {}

    def loop(n):
        draws = vqm._BatchDraws(N, B, n, dev)
        try:
            for s_ in range(n):
                batch = draws.next_batch(0, n_slice)            # rank 0's slice of the common batch, as vq_features asks for it
                res = vqm.HipOps.step_sums(state, feats, imp, batch, model.codebook.data, err[s_:s_ + 1])
                assert res is not None
                vqm.HipOps.step_apply(state, model.codebook.data, model.entry_importance.data, model.decay, model.eps, False)
        finally:
            draws.finish()
    loop(5)
    torch.cuda.synchronize()
    _quiesce()
    err.zero_()
    t0 = time.perf_counter()
    loop(steps)
    torch.cuda.synchronize()
    return 1e3 * (time.perf_counter() - t0) / steps


def vq_cpu_baseline(N, D, K, B):
    """The reference's PyTorch-CPU VQ loop (compression/vq.py:28-35, 49-87) restated on CPU tensors (oracle/vq_torch.py; the
    reference file does not travel and its two native extensions have no CPU build), all host cores, on a bounded sample:
    the direct-difference search (reference-exact numerics) on 1/32 of a batch, the GEMM-form search on 1/4 of a batch;
    per-step times scaled to the full 2^18-point batch. `value` is the FASTER (GEMM) form."""
    from oracle import vq_torch
    cores = os.cpu_count() or 1
    try:
        cores = len(os.sched_getaffinity(0))
    except Exception:
        pass
    direct = vq_torch.time_lloyd_steps(N // 8, D, K, B, "direct", B // 32, 2, threads=cores)
    gemm = vq_torch.time_lloyd_steps(N // 8, D, K, B, "gemm", B // 4, 3, threads=cores)
    return {"value": 1.0 / gemm["seconds_per_step"], "unit": "steps/s", "cores": gemm["threads"], "kind": "port",
            "sample": f"GEMM-form search: {gemm['steps']} Lloyd steps on {gemm['sample_points']}-point batches "
                      f"({gemm['measured_seconds']:.2f} s), time scaled x{gemm['scale']:.0f} to the 2^18-point batch; "
                      "oracle/vq_torch.py = compression/vq.py:28-35,49-87 on CPU tensors, torch.set_num_threads(all cores)",
            "direct_difference_form": {"value": 1.0 / direct["seconds_per_step"], "unit": "steps/s",
                                       "sample": f"{direct['steps']} steps on {direct['sample_points']}-point batches "
                                                 f"({direct['measured_seconds']:.2f} s), scaled x{direct['scale']:.0f}"}}


def cpu_baseline_and_parity(ix_cpu, intr, ev, W, H, focal):
    """The oracle (`kind: port`, oracle/c3dgs_oracle.c, OpenMP) on this box's host cores: one fwd+bwd view of the SAME
    workload. A 10 % Gaussian subsample is timed first; if that predicts more than ~45 s for the full view the scaled
    subsample figure is reported instead (the sample field says which). The oracle's view is then the checker of the HIP
    path on the same inputs (tests/fullsize.py) -> `parity`."""
    import numpy as np
    from oracle import oracle as orc
    from tests import fullsize, synth
    cam = orc.camera(intr.numpy(), ev.numpy())
    P = ix_cpu["means3D"].shape[0]
    dL = synth.grad_image(W, H).numpy()

    def inputs(n):
        return dict(bg=torch.zeros(3), means3D=ix_cpu["means3D"][:n], opacities=ix_cpu["opacities"][:n], shs=ix_cpu["shs"],
                    colors_precomp=None, scales=ix_cpu["scales"], rotations=ix_cpu["rotations"], cov3D_precomp=None,
                    scale_factors=ix_cpu["scale_factors"][:n], sh_indices=ix_cpu["sh_indices"][:n],
                    g_indices=ix_cpu["g_indices"][:n], degree=3, scale_modifier=1.0, prefiltered=False, clamp_color=True)

    sub = max(1, P // 10)
    inp = inputs(sub)
    st, ref, tf, tb = fullsize.oracle_view(inp, cam, dL)
    n_used, dt = sub, tf + tb
    if dt * (P / sub) <= 45.0:
        inp = inputs(P)
        st, ref, tf, tb = fullsize.oracle_view(inp, cam, dL)
        n_used, dt = P, tf + tb
        base = {"value": 1.0 / dt, "unit": "views/s", "cores": orc.num_threads(), "kind": "port",
                "sample": f"1 full view fwd+bwd, {P} Gaussians at {W}x{H} ({dt:.2f} s, R={st.num_rendered}); "
                          "oracle/c3dgs_oracle.c, OpenMP"}
    else:
        scale = P / sub
        base = {"value": 1.0 / (dt * scale), "unit": "views/s", "cores": orc.num_threads(), "kind": "port",
                "sample": f"1 view fwd+bwd of the first {sub} of {P} Gaussians at {W}x{H} ({dt:.2f} s, R={st.num_rendered}), "
                          f"time scaled x{scale:.0f}; oracle/c3dgs_oracle.c, OpenMP"}
    try:
        parity = fullsize.compare(inp, cam, True, st, ref, dL)
        parity["sample"] = f"HIP (C-ABI front-end) vs oracle, the first {n_used} of {P} Gaussians of the timed workload, fwd+bwd"
        parity["bars"] = ("integers equal; PSNR >= 80 dB; dPSNR <= 0.05 dB; grad rel-inf <= 1e-4 away from flipped pixels, <= 1e-3 overall; "
                          "every flipped pixel proven an fp32 borderline in float64 (flips_outside_band == 0)")
        parity["ok"] = bool(
            parity["num_rendered_equal"] and parity["image_finite"] and parity["psnr_db"] >= 80.0 and parity["delta_psnr_db"] <= 0.05
            and all(parity[k] == 0 for k in ("radii_mismatches", "tiles_touched_mismatches", "sorted_keys_mismatches",
                                             "point_list_mismatches", "ranges_mismatches", "splat_float_bit_mismatches"))
            and parity["grad_rel_inf_excluding_flips_max"] <= 1e-4 and parity["grad_rel_inf_max"] <= 1e-3
            and parity["flips_outside_band"] == 0)
    except Exception as e:
        parity = {"error": repr(e)}
    return base, parity


if __name__ == "__main__":
    main()
