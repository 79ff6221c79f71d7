"""Float64 reference for the per-Gaussian blend statistics of csrc/render_contrib.hip (test infrastructure, numpy).

walk(state, W, H) is tests/depth_ref.py's walk -- every pixel's tile list replayed with the oracle's decision rule in float64 --
that also keeps each blended entry's Gaussian id and its weight w = alpha T (T in FRONT of the entry), and folds them per
Gaussian: -> Stats(weight_sum f64 [P], weight_max f64 [P], hits i64 [P], final_T f64 [N], n_contrib i64 [N]).

brute_force(...) is the same rule without tiles: every visible Gaussian at every pixel in (depth, id) order. The two agree
exactly when every tile's list holds every visible Gaussian (tests/test_contrib_ref_cpu.py asserts it on such scenes).

fp32_stats(state) is a SECOND evaluation: tests/alt_blend.py's arithmetic (the kernel's rounding of the exponent: pre-scaled
conic, three products, three fused multiply-adds, 2^x; fp32 alpha, T and w), accumulating the same three statistics (the sum
of the fp32 weights in float64, so that what it differs by from the walk is the per-weight error, not a summation order)."""
from typing import NamedTuple

import numpy as np

from tests import depth_ref
from tests.alt_blend import _f, _fma
from tests.depth_ref import T_THR, _alpha, _get


class Stats(NamedTuple):
    weight_sum: np.ndarray
    weight_max: np.ndarray
    hits: np.ndarray
    final_T: np.ndarray
    n_contrib: np.ndarray


class _Fold:
    def __init__(self, P):
        self.sum, self.max, self.hits = np.zeros(P), np.zeros(P), np.zeros(P, np.int64)

    def add(self, gid, w):
        np.add.at(self.sum, gid, w)
        np.maximum.at(self.max, gid, w)
        np.add.at(self.hits, gid, 1)


def walk(state, W, H):
    m = np.asarray(_get(state, "means2D"), np.float64)
    co = np.asarray(_get(state, "conic_opacity"), np.float64)
    pl = np.asarray(_get(state, "point_list")).astype(np.int64)
    rg = np.asarray(_get(state, "ranges")).astype(np.int64)
    N, gx = W * H, (W + 15) // 16
    py, px = np.divmod(np.arange(N), W)
    tile = (py // 16) * gx + px // 16
    first, length = rg[tile, 0], rg[tile, 1] - rg[tile, 0]
    xs, ys = px.astype(np.float64), py.astype(np.float64)
    T = np.ones(N)
    n_contrib = np.zeros(N, np.int64)
    fold = _Fold(m.shape[0])
    live = np.nonzero(length > 0)[0]                            # pixels still walking
    j = 0
    while live.size:
        gid = pl[first[live] + j]
        hit, alpha = _alpha(m, co, gid, xs[live], ys[live])
        test_T = T[live] * (1.0 - alpha)
        stop = hit & (test_T < T_THR)
        blend = hit & ~stop
        b = live[blend]
        fold.add(gid[blend], alpha[blend] * T[b])
        T[b] = test_T[blend]
        n_contrib[b] = j + 1
        j += 1
        live = live[~stop & (length[live] > j)]
    return Stats(fold.sum, fold.max, fold.hits, T, n_contrib)


def brute_force(state, W, H, visible):
    """No tiles: every Gaussian of the boolean mask `visible` at every pixel, in (depth, id) order."""
    m = np.asarray(_get(state, "means2D"), np.float64)
    co = np.asarray(_get(state, "conic_opacity"), np.float64)
    depths = np.asarray(_get(state, "depths"), np.float32)
    ids = np.nonzero(visible)[0]
    ids = ids[np.lexsort((ids, depths[ids].view(np.uint32)))]   # positive floats order like their bits (the sort's key)
    N = W * H
    py, px = np.divmod(np.arange(N), W)
    xs, ys = px.astype(np.float64), py.astype(np.float64)
    T, done = np.ones(N), np.zeros(N, bool)
    n_contrib = np.zeros(N, np.int64)
    fold = _Fold(m.shape[0])
    for j, g in enumerate(ids):
        hit, alpha = _alpha(m, co, np.full(N, g), xs, ys)
        hit &= ~done
        test_T = T * (1.0 - alpha)
        stop = hit & (test_T < T_THR)
        blend = hit & ~stop
        b = np.nonzero(blend)[0]
        fold.add(np.full(b.size, g), alpha[b] * T[b])
        T = np.where(blend, test_T, T)
        n_contrib[b] = j + 1
        done |= stop
    return Stats(fold.sum, fold.max, fold.hits, T, n_contrib)


def fp32_stats(st):
    """tests/alt_blend.py:forward's loop and arithmetic, folding w = fp32(alpha T) per Gaussian instead of the colours."""
    W, H = st.W, st.H
    gx = (W + 15) // 16
    LOG2E = _f(1.4426950408889634)
    fold = _Fold(st.P)
    final_T = np.ones(W * H)
    n_contrib = np.zeros(W * H, np.int64)
    for t in range(st.ranges.shape[0]):
        ty, tx = divmod(t, gx)
        ys, xs = np.meshgrid(np.arange(ty * 16, min(ty * 16 + 16, H)), np.arange(tx * 16, min(tx * 16 + 16, W)), indexing="ij")
        ys, xs = ys.ravel(), xs.ravel()
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
                fold.sum[gid] += w.astype(np.float64).sum()
                fold.max[gid] = max(fold.max[gid], float(w.max()))
                fold.hits[gid] += w.size
            T = np.where(blend, test_T, T)
            last = np.where(blend, j + 1, last)
            done |= stop
        pix = ys * W + xs
        final_T[pix] = T
        n_contrib[pix] = last
    return Stats(fold.sum, fold.max, fold.hits, final_T, n_contrib)


def exemption_cap(P):
    """Gaussians whose `hits` may differ between two correct evaluations (a threshold decision that flipped on some pixel)."""
    return max(2, int(2e-5 * P))


def compare(got_sum, got_max, got_hits, ref, label=""):
    """-> (exempt, worst relative difference of weight_sum, of weight_max) over the rows whose hits agree; prints them."""
    same = np.asarray(got_hits).astype(np.int64) == ref.hits
    rel = lambda a, b: float((np.abs(a[same].astype(np.float64) - b[same]) / np.where(b[same] > 0, b[same], 1.0)).max()) if same.any() else 0.0   # noqa: E731
    out = int((~same).sum()), rel(np.asarray(got_sum), ref.weight_sum), rel(np.asarray(got_max), ref.weight_max)
    print(label, "Gaussians whose hits differ:", out[0], "of", same.size, "; largest relative difference of weight_sum %.3g, of weight_max %.3g" % out[1:],
          "; blended pairs", int(ref.hits.sum()))
    return out


SCENES = depth_ref.SCENES
