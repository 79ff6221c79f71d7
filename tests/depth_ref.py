"""Float64 reference for the MEDIAN-depth map of csrc/render_depth.hip (test infrastructure, numpy), and the scenes its tests use.

walk(state, W, H) replays every pixel's tile list with the oracle's decision rule (forward.cu:330-360: power > 0 -> skip,
alpha = min(0.99, o exp(power)) < 1/255 -> skip, T (1 - alpha) < 1e-4 -> stop; the three thresholds are the fp32 constants) in
float64, from a RasterState-like dict or object (means2D, conic_opacity, depths, point_list, ranges), and returns per pixel the
float64 T AFTER each blended entry together with those entries' fp32 depths and 1-based list positions. The median of a pixel
is then the depth of the first entry whose T is below 0.5; the GPU test accepts any entry inside the fp32 error band around
that crossing (median_candidates).

brute_force(...) is the same rule without tiles: every visible Gaussian at every pixel, sorted by (depth, id). The two agree
exactly when every tile's list holds every visible Gaussian (tests/test_depth_ref_cpu.py builds such scenes and asserts it).

The walk is vectorised over ALL pixels of the image per list position (a few thousand numpy steps per scene), not over the
pixels of one tile per list entry (hundreds of thousands)."""
import functools

import numpy as np

A_MAX, A_THR, T_THR = float(np.float32(0.99)), float(np.float32(1.0) / np.float32(255.0)), float(np.float32(0.0001))
U = 2.0 ** -24                    # fp32 unit round-off


def _get(state, key):
    return state[key] if isinstance(state, dict) else getattr(state, key)


class Walk:
    """CSR over pixels (row-major): the blended entries of pixel p are [start[p], start[p + 1]) of T (float64, after the entry),
    z (float32 depth of the entry's Gaussian), pos (1-based position in the tile's list). n_contrib[p] = pos of the last one."""

    def __init__(self, start, T, z, pos):
        self.start, self.T, self.z, self.pos = start, T, z, pos
        n = np.zeros(start.size - 1, np.int64)
        has = start[1:] > start[:-1]
        n[has] = pos[start[1:][has] - 1]
        self.n_contrib = n

    def pixel(self, p):
        s = slice(self.start[p], self.start[p + 1])
        return self.T[s], self.z[s]


def _alpha(m, co, gid, xs, ys):
    dx, dy = m[gid, 0] - xs, m[gid, 1] - ys
    power = -0.5 * (co[gid, 0] * dx * dx + co[gid, 2] * dy * dy) - co[gid, 1] * dx * dy
    with np.errstate(over="ignore", invalid="ignore"):
        alpha = np.minimum(A_MAX, co[gid, 3] * np.exp(np.minimum(power, 0.0)))
    return (power <= 0) & (alpha >= A_THR), alpha


def _csr(N, pix, T, z, pos):
    pix = np.concatenate(pix) if pix else np.zeros(0, np.int64)
    order = np.argsort(pix, kind="stable")                     # list order is kept inside a pixel
    cat = lambda parts, dt: (np.concatenate(parts) if parts else np.zeros(0, dt))[order]      # noqa: E731
    start = np.zeros(N + 1, np.int64)
    np.cumsum(np.bincount(pix, minlength=N), out=start[1:])
    return Walk(start, cat(T, np.float64), cat(z, np.float32), cat(pos, np.int64))


def walk(state, W, H):
    m = np.asarray(_get(state, "means2D"), np.float64)
    co = np.asarray(_get(state, "conic_opacity"), np.float64)
    depths = np.asarray(_get(state, "depths"), np.float32)
    pl = np.asarray(_get(state, "point_list")).astype(np.int64)
    rg = np.asarray(_get(state, "ranges")).astype(np.int64)
    N, gx = W * H, (W + 15) // 16
    py, px = np.divmod(np.arange(N), W)
    tile = (py // 16) * gx + px // 16
    first, length = rg[tile, 0], rg[tile, 1] - rg[tile, 0]
    xs, ys = px.astype(np.float64), py.astype(np.float64)
    T = np.ones(N)
    live = np.nonzero(length > 0)[0]                            # pixels still walking
    out_pix, out_T, out_z, out_pos = [], [], [], []
    j = 0
    while live.size:
        gid = pl[first[live] + j]
        hit, alpha = _alpha(m, co, gid, xs[live], ys[live])
        test_T = T[live] * (1.0 - alpha)
        stop = hit & (test_T < T_THR)
        blend = hit & ~stop
        b = live[blend]
        T[b] = test_T[blend]
        out_pix.append(b); out_T.append(test_T[blend]); out_z.append(depths[gid[blend]]); out_pos.append(np.full(b.size, j + 1, np.int64))
        j += 1
        live = live[~stop & (length[live] > j)]
    return _csr(N, out_pix, out_T, out_z, out_pos)


def brute_force(state, W, H, visible):
    """No tiles: every Gaussian of the boolean mask `visible` at every pixel, in (depth, id) order. `pos` counts those."""
    m = np.asarray(_get(state, "means2D"), np.float64)
    co = np.asarray(_get(state, "conic_opacity"), np.float64)
    depths = np.asarray(_get(state, "depths"), np.float32)
    ids = np.nonzero(visible)[0]
    ids = ids[np.lexsort((ids, depths[ids].view(np.uint32)))]   # positive floats order like their bits (the sort's key)
    N = W * H
    py, px = np.divmod(np.arange(N), W)
    xs, ys = px.astype(np.float64), py.astype(np.float64)
    T, done = np.ones(N), np.zeros(N, bool)
    out_pix, out_T, out_z, out_pos = [], [], [], []
    for j, g in enumerate(ids):
        hit, alpha = _alpha(m, co, np.full(N, g), xs, ys)
        hit &= ~done
        test_T = T * (1.0 - alpha)
        stop = hit & (test_T < T_THR)
        blend = hit & ~stop
        T = np.where(blend, test_T, T)
        done |= stop
        b = np.nonzero(blend)[0]
        out_pix.append(b); out_T.append(test_T[b]); out_z.append(np.full(b.size, depths[g], np.float32)); out_pos.append(np.full(b.size, j + 1, np.int64))
    return _csr(N, out_pix, out_T, out_z, out_pos)


def median_candidates(T64, z, n):
    """The fp32 kernel's T differs from the float64 one by at most band = 4 (n + 1) u relative (two roundings per blended entry
    in T, alpha within 3 u; n = the pixel's n_contrib). -> (candidates, zero_ok): the median must be bit-equal to one of
    `candidates` (depths of the entries from the first with T64 < 0.5 (1 + band) to the first with T64 < 0.5 (1 - band),
    inclusive), or be 0 where zero_ok."""
    band = 4.0 * (n + 1) * U
    hi = np.nonzero(T64 < 0.5 * (1.0 + band))[0]
    lo = np.nonzero(T64 < 0.5 * (1.0 - band))[0]
    if lo.size:
        return z[hi[0]:lo[0] + 1], False
    if hi.size:
        return z[hi[0]:], True
    return z[:0], True


# ---------------------------------------------------------------------------------------------------------------- scenes
# What tests/test_render_depth_gpu.py renders, and tests/test_depth_ref_cpu.py checks the exemption cap on.
SCENES = ["indexed", "odd_size", "opaque_big", "needles_long", "huge_faint", "deep", "one_pixel"]
DEEP_W, DEEP_H = 70, 45           # 5 x 3 tiles, ragged on both edges


@functools.lru_cache(maxsize=None)
def scene(name):
    """-> (inputs, cam, indexed); computed once per process, not to be modified."""
    import torch
    from oracle import oracle as orc
    from tests import cases, synth
    if name in ("indexed", "odd_size", "opaque_big", "needles_long"):
        return cases.make_case(name)
    if name == "huge_faint":      # whole batches of dead entries in front of every list: compact index != list position
        from tests.test_compact_lists_gpu import _scene
        return _scene(name)
    plain = lambda sc: dict(bg=torch.zeros(3), means3D=sc["means3D"], opacities=sc["opacities"], shs=sc["shs"], colors_precomp=None,   # noqa: E731
                            scales=sc["scales"], rotations=sc["rotations"], cov3D_precomp=None, scale_factors=None, sh_indices=None,
                            g_indices=None, degree=3, scale_modifier=1.0, prefiltered=False, clamp_color=True)
    if name == "deep":
        # faint splats that each cover several tiles, stacked thousands deep: a pixel blends more than two staged batches of 256
        # compact entries before it stops, and T crosses 0.5 far down the list
        W, H, focal = DEEP_W, DEEP_H, 50.0
        intr, ev = synth.camera(W, H, focal)
        sc = synth.scene(3000, W, H, focal, seed=41, scale_median=0.35, zmin=3.0, zmax=9.0)
        g = torch.Generator().manual_seed(42)
        sc["opacities"] = (0.008 + 0.022 * torch.rand(sc["opacities"].shape, generator=g)).float()
        return plain(sc), orc.camera(intr.numpy(), ev.numpy()), False
    if name == "one_pixel":       # one Gaussian on a 1 x 1 image
        intr, ev = synth.camera(1, 1, 1.0)
        sc = synth.scene(1, 1, 1, 1.0, seed=5, scale_median=0.5)
        sc["means3D"][0] = torch.tensor([0.0, 0.0, 4.0])
        sc["opacities"][0] = 0.8
        cam = orc.camera(intr.numpy(), np.array([0, 0, 0, 1, 0, 0, 0], np.float32))
        return plain(sc), cam, False
    raise KeyError(name)


@functools.lru_cache(maxsize=None)
def oracle_state(name):
    """The oracle's forward of scene(name): computed once per process, shared by the tests, not to be modified."""
    from tests import cases
    inp, cam, _ = scene(name)
    return cases.oracle_forward(inp, cam)


def exemption_cap(pixels):
    return max(2, int(2e-5 * pixels))
