"""Float64 reference for the per-Gaussian error scores of csrc/render_error.hip (test infrastructure, numpy).

walk(state, W, H, emap) is tests/contrib_ref.py's walk -- every pixel's tile list replayed with the oracle's decision rule in
float64 -- that folds w * e per Gaussian, w = alpha T (T in FRONT of the entry), e = emap[pixel] in float64:
-> Stats(err_sum f64 [P], hits i64 [P], final_T f64 [N], n_contrib i64 [N]). With e = 1 it performs contrib_ref.walk's operations
in contrib_ref.walk's order, so err_sum is that walk's weight_sum exactly.

brute_force(...) is the same rule without tiles: every visible Gaussian at every pixel in (depth, id) order.

fp32_stats(state, emap) is a SECOND evaluation: contrib_ref.fp32_stats' arithmetic (the kernel's rounding of the exponent, fp32
alpha, T and w), then ONE fp32 product with e, the products summed in float64 (what it differs by from the walk is the per-term
error, not a summation order).

standard_map(H, W) is the deterministic map the tests use, bounded away from zero: e = 0.25 + 0.75 hash(y, x) in fp32, so that
every term of a sum is non-negative and a relative bar on the sum means what it means for weight_sum.

pixel_trace(state, W, H, p) lists what the walk does at ONE pixel: the Gaussians it blends there, in list order, its final T and
how close (relative) any of its decisions came to the threshold it was compared with."""
import functools
from typing import NamedTuple

import numpy as np

from tests.alt_blend import _f, _fma
from tests.depth_ref import A_MAX, A_THR, T_THR, _alpha, _get


class Stats(NamedTuple):
    err_sum: np.ndarray
    hits: np.ndarray
    final_T: np.ndarray
    n_contrib: np.ndarray


def standard_map(H, W):
    y, x = np.meshgrid(np.arange(H, dtype=np.uint64), np.arange(W, dtype=np.uint64), indexing="ij")
    h = (((y * np.uint64(73856093)) ^ (x * np.uint64(19349663))) * np.uint64(2654435761)) & np.uint64(0xFFFFFFFF)
    u = ((h >> np.uint64(8)).astype(np.float32) / np.float32(1 << 24)).astype(np.float32)      # 24 bits: exact, in [0, 1)
    return (np.float32(0.25) + (np.float32(0.75) * u).astype(np.float32)).astype(np.float32)


def walk(state, W, H, emap):
    m = np.asarray(_get(state, "means2D"), np.float64)
    co = np.asarray(_get(state, "conic_opacity"), np.float64)
    pl = np.asarray(_get(state, "point_list")).astype(np.int64)
    rg = np.asarray(_get(state, "ranges")).astype(np.int64)
    e = np.asarray(emap, np.float64).reshape(-1)
    N, gx = W * H, (W + 15) // 16
    assert e.size == N
    py, px = np.divmod(np.arange(N), W)
    tile = (py // 16) * gx + px // 16
    first, length = rg[tile, 0], rg[tile, 1] - rg[tile, 0]
    xs, ys = px.astype(np.float64), py.astype(np.float64)
    T = np.ones(N)
    n_contrib = np.zeros(N, np.int64)
    err, hits = np.zeros(m.shape[0]), np.zeros(m.shape[0], np.int64)
    live = np.nonzero(length > 0)[0]                            # pixels still walking
    j = 0
    while live.size:
        gid = pl[first[live] + j]
        hit, alpha = _alpha(m, co, gid, xs[live], ys[live])
        test_T = T[live] * (1.0 - alpha)
        stop = hit & (test_T < T_THR)
        blend = hit & ~stop
        b = live[blend]
        np.add.at(err, gid[blend], alpha[blend] * T[b] * e[b])
        np.add.at(hits, gid[blend], 1)
        T[b] = test_T[blend]
        n_contrib[b] = j + 1
        j += 1
        live = live[~stop & (length[live] > j)]
    return Stats(err, hits, T, n_contrib)


def brute_force(state, W, H, visible, emap):
    """No tiles: every Gaussian of the boolean mask `visible` at every pixel, in (depth, id) order."""
    m = np.asarray(_get(state, "means2D"), np.float64)
    co = np.asarray(_get(state, "conic_opacity"), np.float64)
    depths = np.asarray(_get(state, "depths"), np.float32)
    e = np.asarray(emap, np.float64).reshape(-1)
    ids = np.nonzero(visible)[0]
    ids = ids[np.lexsort((ids, depths[ids].view(np.uint32)))]   # positive floats order like their bits (the sort's key)
    N = W * H
    py, px = np.divmod(np.arange(N), W)
    xs, ys = px.astype(np.float64), py.astype(np.float64)
    T, done = np.ones(N), np.zeros(N, bool)
    n_contrib = np.zeros(N, np.int64)
    err, hits = np.zeros(m.shape[0]), np.zeros(m.shape[0], np.int64)
    for j, g in enumerate(ids):
        hit, alpha = _alpha(m, co, np.full(N, g), xs, ys)
        hit &= ~done
        test_T = T * (1.0 - alpha)
        stop = hit & (test_T < T_THR)
        blend = hit & ~stop
        b = np.nonzero(blend)[0]
        np.add.at(err, np.full(b.size, g), alpha[b] * T[b] * e[b])
        hits[g] += b.size
        T = np.where(blend, test_T, T)
        n_contrib[b] = j + 1
        done |= stop
    return Stats(err, hits, T, n_contrib)


def fp32_stats(st, emap):
    """contrib_ref.fp32_stats' loop and arithmetic, folding fp32(w e) per Gaussian, w = fp32(alpha T), summed in float64."""
    W, H = st.W, st.H
    gx = (W + 15) // 16
    LOG2E = _f(1.4426950408889634)
    e32 = np.asarray(emap, _f).reshape(-1)
    err, hits = np.zeros(st.P), np.zeros(st.P, np.int64)
    final_T = np.ones(W * H)
    n_contrib = np.zeros(W * H, np.int64)
    for t in range(st.ranges.shape[0]):
        ty, tx = divmod(t, gx)
        ys, xs = np.meshgrid(np.arange(ty * 16, min(ty * 16 + 16, H)), np.arange(tx * 16, min(tx * 16 + 16, W)), indexing="ij")
        ys, xs = ys.ravel(), xs.ravel()
        pix = ys * W + xs
        ev = e32[pix]
        npx = ys.size
        T = np.ones(npx, _f)
        last = np.zeros(npx, np.int64)
        done = np.zeros(npx, bool)
        lst = st.point_list[st.ranges[t, 0]:st.ranges[t, 1]]
        for j, gid in enumerate(lst):
            if done.all():
                break
            mx, my = st.means2D[gid]
            a, b, c, op = st.conic_opacity[gid]
            ka, kb, kc = _f(a * _f(_f(-0.5) * LOG2E)), _f(b * _f(-LOG2E)), _f(c * _f(_f(-0.5) * LOG2E))
            dx, dy = (mx - xs.astype(_f)).astype(_f), (my - ys.astype(_f)).astype(_f)
            p2 = _fma(np.full(npx, kb, _f), (dx * dy).astype(_f), _fma(np.full(npx, kc, _f), (dy * dy).astype(_f), (ka * (dx * dx).astype(_f)).astype(_f)))
            G = np.exp2(np.minimum(p2, _f(60)).astype(np.float64)).astype(_f)
            alpha = np.minimum(_f(0.99), (op * G).astype(_f))
            hit = ~(p2 > 0) & ~(alpha < _f(1.0) / _f(255.0)) & ~done
            test_T = (T * (_f(1) - alpha)).astype(_f)
            stop = hit & (test_T < _f(0.0001))
            blend = hit & ~stop
            w = (alpha * T).astype(_f)[blend]
            if w.size:
                err[gid] += (w * ev[blend]).astype(_f).astype(np.float64).sum()
                hits[gid] += w.size
            T = np.where(blend, test_T, T)
            last = np.where(blend, j + 1, last)
            done |= stop
        final_T[pix] = T
        n_contrib[pix] = last
    return Stats(err, hits, final_T, n_contrib)


def compare(got_sum, got_hits, ref, label=""):
    """-> (rows whose hits differ, worst relative difference of err_sum over the rows whose hits agree); prints them."""
    same = np.asarray(got_hits).astype(np.int64) == ref.hits
    got = np.asarray(got_sum).astype(np.float64)
    rel = float((np.abs(got[same] - ref.err_sum[same]) / np.where(ref.err_sum[same] > 0, ref.err_sum[same], 1.0)).max()) if same.any() else 0.0
    out = int((~same).sum()), rel
    print(label, "Gaussians whose hits differ:", out[0], "of", same.size, "; largest relative difference of err_sum %.3g" % rel,
          "; blended pairs", int(ref.hits.sum()))
    return out


def pixel_trace(state, W, H, p):
    """-> (ids of the Gaussians the float64 walk blends at pixel p, in list order; final T; the smallest relative distance of any
    compared quantity from its threshold: power from 0 is not relative and is skipped unless |power| < 1e-9, alpha from 1/255,
    T (1 - alpha) from 1e-4)."""
    m = np.asarray(_get(state, "means2D"), np.float64)
    co = np.asarray(_get(state, "conic_opacity"), np.float64)
    pl = np.asarray(_get(state, "point_list")).astype(np.int64)
    rg = np.asarray(_get(state, "ranges")).astype(np.int64)
    py, px = divmod(int(p), W)
    tile = (py // 16) * ((W + 15) // 16) + px // 16
    T, ids, margin = 1.0, [], np.inf
    for g in pl[rg[tile, 0]:rg[tile, 1]]:
        dx, dy = m[g, 0] - px, m[g, 1] - py
        power = -0.5 * (co[g, 0] * dx * dx + co[g, 2] * dy * dy) - co[g, 1] * dx * dy
        if abs(power) < 1e-9:
            margin = 0.0
        if power > 0:
            continue
        alpha_raw = co[g, 3] * np.exp(power)
        margin = min(margin, abs(alpha_raw - A_THR) / A_THR)
        alpha = min(A_MAX, alpha_raw)
        if alpha < A_THR:
            continue
        test_T = T * (1.0 - alpha)
        margin = min(margin, abs(test_T - T_THR) / T_THR)
        if test_T < T_THR:
            break
        ids.append(int(g))
        T = test_T
    return np.array(ids, np.int64), T, margin


# ---------------------------------------------------------------------------------------------------------------- hidden scene
# What tests/test_render_error_gpu.py densifies by score on: a model, and the same model plus bright opaque Gaussians in front of
# ONE image region; the targets are rendered from the second ("hidden") one, so the image error of the first sits in that region.
HIDDEN_W, HIDDEN_H, HIDDEN_FOCAL = 90, 60, 80.0
REGION_U, REGION_V = (0.15, 0.9), (-0.85, 0.0)          # in the scene generator's normalised image coordinates (-1 .. 1)


def in_region(means3D):
    """bool [P]: does the centre project (identity camera) into the region?"""
    tfx, tfy = HIDDEN_W / (2.0 * HIDDEN_FOCAL), HIDDEN_H / (2.0 * HIDDEN_FOCAL)
    u = means3D[:, 0] / (means3D[:, 2] * tfx * 1.05)
    v = means3D[:, 1] / (means3D[:, 2] * tfy * 1.05)
    return (means3D[:, 2] > 0) & (u >= REGION_U[0]) & (u <= REGION_U[1]) & (v >= REGION_V[0]) & (v <= REGION_V[1])


def hidden_scene(P=3000, extra=1500):
    """-> (base, hidden): synth scenes (dicts of CPU tensors); hidden = base + `extra` Gaussians inside the region, nearer than
    everything else."""
    import torch
    from tests import synth
    W, H, focal = HIDDEN_W, HIDDEN_H, HIDDEN_FOCAL
    base = synth.scene(P, W=W, H=H, focal=focal, seed=23, scale_median=0.03, zmin=3.0, zmax=12.0)
    add = synth.scene(extra, W=W, H=H, focal=focal, seed=29, scale_median=0.03, zmin=2.0, zmax=2.8)
    g = torch.Generator().manual_seed(30)
    tfx, tfy = W / (2.0 * focal), H / (2.0 * focal)
    z = add["means3D"][:, 2]
    u = REGION_U[0] + (REGION_U[1] - REGION_U[0]) * (0.2 + 0.6 * torch.rand(extra, generator=g))
    v = REGION_V[0] + (REGION_V[1] - REGION_V[0]) * (0.2 + 0.6 * torch.rand(extra, generator=g))
    add["means3D"][:, 0], add["means3D"][:, 1] = u * z * tfx * 1.05, v * z * tfy * 1.05
    add["opacities"][:] = 0.9
    add["shs"][:, 0] = 3.0 * torch.sign(torch.randn(extra, 3, generator=g))
    hidden = {k: torch.cat((base[k], add[k])).contiguous() for k in base}
    return base, hidden


# ---------------------------------------------------------------------------------------------------------------- long run
# The scene tests/depth_ref.py lacks: a blended Gaussian whose run of slots exceeds 256 (two trips of stage B's whole-wave fold).
# One faint screen-filling Gaussian in front of 300 small ones on 272 x 272 pixels = 17 x 17 tiles: its run is 289 slots.
LONG_W = LONG_H = 272


@functools.lru_cache(maxsize=None)
def long_run_scene():
    """-> (inputs, cam, indexed); computed once per process, not to be modified."""
    import torch
    from oracle import oracle as orc
    from tests import synth
    W, H, focal = LONG_W, LONG_H, 200.0
    intr, ev = synth.camera(W, H, focal)
    sc = synth.scene(301, W, H, focal, seed=51, scale_median=0.05, zmin=3.0, zmax=9.0)
    sc["means3D"][0] = torch.tensor([0.0, 0.0, 2.5])           # in front of everything, over every tile
    sc["scales"][0] = 8.0
    sc["opacities"][0] = 0.05
    inp = dict(bg=torch.zeros(3), means3D=sc["means3D"], opacities=sc["opacities"], shs=sc["shs"], colors_precomp=None,
               scales=sc["scales"], rotations=sc["rotations"], cov3D_precomp=None, scale_factors=None, sh_indices=None,
               g_indices=None, degree=3, scale_modifier=1.0, prefiltered=False, clamp_color=True)
    return inp, orc.camera(intr.numpy(), ev.numpy()), False


@functools.lru_cache(maxsize=None)
def long_run_state():
    from tests import cases
    inp, cam, _ = long_run_scene()
    return cases.oracle_forward(inp, cam)
