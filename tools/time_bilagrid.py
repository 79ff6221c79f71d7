#!/usr/bin/env python3
"""Times the bilateral-grid kernels (csrc/bilagrid.hip) in one process and writes profiles/r18_bilagrid_time.json (also one
JSON line). At 3 x 1080 x 1920 with the grids (8, 16, 16) and (1, 1, 1):

  slice, slice backward      the calls as BilateralGrid.slice makes them (with dL_drgb), and the backward's stage split from the
                             library's stage timers in separate rounds: gather, fold, rgb
  tv, tv backward            over 100 cameras' grids
  torch route                the same slice + backward as torch ops on the same device: grid_sample, the affine apply, autograd
                             (tests/bilagrid_ref.py's grid_sample form in float32)
  floors                     the bytes each kernel must move at the rate a 512 MiB device copy reaches in this process

    python tools/time_bilagrid.py [--samples 20] [--warmup 3] [--H 1080] [--W 1920] [--out profiles/r18_bilagrid_time.json]

Medians of `samples` with min and max after `warmup` unrecorded rounds, between stream events. The expectation (slice + backward
below the torch route at both shapes) is evaluated and written as a boolean, whatever it comes to."""
import argparse
import json
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

TV_CAMERAS = 100


def _event_ms(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b)


def _stats(ms):
    return {"ms": statistics.median(ms), "ms_min_max": [min(ms), max(ms)]}


def _timed(fn, samples, warmup):
    ms = [_event_ms(fn) for _ in range(warmup + samples)]
    return _stats(ms[warmup:])


def copy_rate_gb_s(samples):
    src = torch.empty(512 << 20, dtype=torch.uint8, device="cuda")
    dst = torch.empty_like(src)
    for _ in range(3):
        dst.copy_(src)
    ms = [_event_ms(lambda: dst.copy_(src)) for _ in range(samples)]
    return 2 * src.numel() / (statistics.median(ms) * 1e-3) / 1e9


def torch_slice(grid, rgb):
    """grid_sample + the affine apply, float32 on the device: the [12, H, W] intermediate and its launches"""
    _, H, W = rgb.shape
    xs = ((torch.arange(W, device=rgb.device, dtype=rgb.dtype) + 0.5) / W)[None, :].expand(H, W)
    ys = ((torch.arange(H, device=rgb.device, dtype=rgb.dtype) + 0.5) / H)[:, None].expand(H, W)
    luma = 0.299 * rgb[0] + 0.587 * rgb[1] + 0.114 * rgb[2]
    u = torch.stack([2 * xs - 1, 2 * ys - 1, 2 * luma - 1], -1)[None, None]
    A = torch.nn.functional.grid_sample(grid[None], u, mode="bilinear", padding_mode="border", align_corners=True)[0, :, 0]
    A = A.reshape(3, 4, H, W)
    return (A[:, :3] * rgb[None]).sum(1) + A[:, 3]


def time_shape(shape, H, W, samples, warmup, rate):
    from c3dgs_amd import _lib
    from c3dgs_amd.bilagrid import BilateralGrid
    gen = torch.Generator(device="cuda").manual_seed(sum(shape))
    grids = BilateralGrid(1, shape)
    with torch.no_grad():
        grids.grids.add_(0.1 * (torch.rand(grids.grids.shape, device="cuda", generator=gen) - 0.5))
    image = (torch.rand(3, H, W, device="cuda", generator=gen) * 1.4 - 0.2).requires_grad_(True)
    dout = torch.rand(3, H, W, device="cuda", generator=gen) - 0.5
    state = {}

    def forward():
        state["out"] = grids.slice(image, 0)

    def backward():
        grids.grids.grad = image.grad = None
        state["out"].backward(dout, retain_graph=True)

    fwd = _timed(forward, samples, warmup)
    bwd = _timed(backward, samples, warmup)
    _lib.profile_read()
    _lib.profile_enable(True)
    rounds = 5
    for _ in range(rounds):
        forward()
        backward()
    torch.cuda.synchronize()
    stages = {k: v[0] / rounds for k, v in _lib.profile_read().items() if k.startswith("bilagrid")}
    _lib.profile_enable(False)

    g32 = grids.grids.detach()[0].clone().requires_grad_(True)
    i32 = image.detach().clone().requires_grad_(True)

    def t_forward():
        state["t_out"] = torch_slice(g32, i32)

    def t_backward():
        g32.grad = i32.grad = None
        state["t_out"].backward(dout, retain_graph=True)

    t_fwd = _timed(t_forward, samples, warmup)
    t_bwd = _timed(t_backward, samples, warmup)
    worst = float((state["t_out"].detach() - state["out"].detach()).abs().max())

    hw, n_grid = H * W, grids.grids[0].numel()
    ws = _lib.lib().c3dgs_bilagrid_workspace_bytes(H, W, *shape)
    floor = lambda nbytes: nbytes / (rate * 1e9) * 1e3      # noqa: E731
    bytes_ = {"slice": 6 * hw * 4 + n_grid * 4,                         # rgb in, out out, the grid once
              "gather": 6 * hw * 4 + ws,                                # rgb and dL_dout once (each pixel is read by 4 vertices: caches), partial rows out
              "fold": ws + n_grid * 4,
              "rgb": 9 * hw * 4 + n_grid * 4}                           # rgb, dL_dout in, dL_drgb out, the grid once
    out = {"slice": fwd, "slice_backward": bwd, "slice_plus_backward_ms": fwd["ms"] + bwd["ms"],
           "stage_ms": {k: stages.get(k) for k in ("bilagrid_slice", "bilagrid_slice_backward", "bilagrid_gather", "bilagrid_fold",
                                                   "bilagrid_rgb_backward")},
           "torch_route": {"forward": t_fwd, "backward": t_bwd, "forward_plus_backward_ms": t_fwd["ms"] + t_bwd["ms"]},
           "max_abs_difference_of_the_two_outputs": worst, "workspace_bytes": ws,
           "floor_ms": {k: floor(v) for k, v in bytes_.items()}, "floor_bytes": bytes_,
           "below_torch_route": fwd["ms"] + bwd["ms"] < t_fwd["ms"] + t_bwd["ms"]}
    many = BilateralGrid(TV_CAMERAS, shape)
    with torch.no_grad():
        many.grids.add_(0.1 * (torch.rand(many.grids.shape, device="cuda", generator=gen) - 0.5))

    def tv_forward():
        state["tv"] = many.tv_loss()

    def tv_backward():
        many.grids.grad = None
        state["tv"].backward(retain_graph=True)

    out["tv"] = dict(_timed(tv_forward, samples, warmup), cameras=TV_CAMERAS, floor_ms=floor(many.grids.numel() * 4))
    out["tv_backward"] = dict(_timed(tv_backward, samples, warmup), cameras=TV_CAMERAS, floor_ms=floor(2 * many.grids.numel() * 4))
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--samples", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--H", type=int, default=1080)
    ap.add_argument("--W", type=int, default=1920)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r18_bilagrid_time.json"))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("time_bilagrid.py needs the GPU; a timing taken anywhere else says nothing")
    rate = copy_rate_gb_s(args.samples)
    out = {"device": torch.cuda.get_device_name(0), "samples": args.samples, "warmup": args.warmup, "copy_rate_gb_s": rate,
           "image": [3, args.H, args.W],
           "method": "stream events around each call as the autograd Functions make it (allocation of the outputs included), medians "
                     "after warm-up, one process; floor = the bytes that must move at the copy rate; the stage split is the mean of 5 "
                     "separate rounds under the library's stage timers",
           "shapes": {}}
    for shape in ((8, 16, 16), (1, 1, 1)):
        out["shapes"]["x".join(map(str, shape))] = time_shape(shape, args.H, args.W, args.samples, args.warmup, rate)
    out["expectation_slice_plus_backward_below_torch_route_at_both_shapes"] = all(s["below_torch_route"] for s in out["shapes"].values())
    print(json.dumps(out))
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as fh:
            json.dump(out, fh, indent=1)


if __name__ == "__main__":
    main()
