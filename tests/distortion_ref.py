"""Float64 reference for the depth-distortion map and its gradient (csrc/render_distortion.hip, csrc/render_maps_backward.hip);
test infrastructure, built on tests/depth_ref.py's walk and tests/depth_grad_ref.py's walk_flipped / projection / chain.

Per pixel, over the entries k = 1..m the walk blends, with w_k = alpha_k T_k, T_{k+1} = T_k (1 - alpha_k), s_k = f(z_k):
    mode None ("raw")      f(z) = z
    mode (near, far)       f(z) = far / (far - near) * (1 - near / z)
    distortion = sum_i sum_j w_i w_j |s_i - s_j| = 2 sum_k w_k (s_k A_<k - S_<k),  A_<k = 1 - T_k,  S_<k = sum_{j<k} w_j s_j
    moment     = sum_k w_k s_k

  forward(...)          the maps by the prefix formula (segmented cumulative sums in float64)
  forward_brute(...)    the double sum with |.|, pixel by pixel: no ordering assumption
  closed_form(...)      depth_grad_ref.closed_form generalised: with gL = dL/d distortion, A_>k = T_{k+1} - T_{m+1},
                        S_>k = moment - S_<k - w_k s_k,
                            u_k = 2 gL (s_k (A_<k - A_>k) - S_<k + S_>k)          c_k = gD z_k + gA + u_k
                            dL/dalpha_k = T_k c_k - (sum_{j>k} w_j c_j) / (1 - alpha_k)
                            dL/dz_k = w_k (gD + 2 gL (A_<k - A_>k) f'(z_k))
                        folded per Gaussian as there; restated() chains the rows to the leaves as depth_grad_ref.restated does
  autograd_truth(...)   torch float64 autograd over the walk's (pixel, entry) pairs: alpha from projection() (the 0.99 clamp
                        straight through, as tests/dense_ref.py), T by a segmented cumulative product, the loss
                        sum(gD depth + gA alpha + gL distortion)
  fp32_restatement(...) numpy float32 of the recurrences the two kernels run, operation for operation: the PIVOTED ones (the forward
                        about the pixel's first blended s, the backward about moment / A); pivot=False restates the plain
                        backward recurrences instead, a figure to show what the pivot is for,
                        on the float64 walk's pairs with alpha rounded to fp32; the fold over pixels and the chain stay float64
                        (they are the depth backward's, not under test here)
  candidates(...)       as depth_grad_ref.candidates: the float64 gradients under the fp32 decisions and, for each ambiguous pair,
                        under both."""
import functools
import itertools
from types import SimpleNamespace

import numpy as np
import torch

from tests import depth_grad_ref as dgr, depth_ref

NDC = (0.2, 100.0)
MODES = {"raw": None, "ndc": NDC}
SALT = 3                               # of the hashed gL map (1 and 2 are depth_grad_ref.truth's gD and gA)


def f_map(z, mode):
    if mode is None:
        return z
    near, far = mode
    return far / (far - near) * (1.0 - near / z)


def df_map(z, mode):
    if mode is None:
        return z * 0.0 + 1.0
    near, far = mode
    return far * near / ((far - near) * z * z)


def _segments(wk):
    counts = np.diff(wk.start)
    return counts, np.repeat(np.arange(counts.size), counts)


def _seg_cumsum(v, start, counts):
    """inclusive cumulative sum inside every pixel's run, one list position of every pixel per step (a cumulative sum over all
    the pairs, cut afterwards, would round at the size of the image's total)"""
    out = np.array(v, np.float64)
    first = start[:-1]
    for k in range(1, int(counts.max()) if counts.size else 0):
        i = first[counts > k] + k
        out[i] += out[i - 1]
    return out


def _weights(wk):
    """-> (pixel of every pair, T before the pair, w = T before - T after)"""
    counts, pixel = _segments(wk)
    first = np.zeros(pixel.size, bool)
    first[wk.start[:-1][counts > 0]] = True
    Tb = np.where(first, 1.0, np.roll(wk.T, 1))
    return counts, pixel, Tb, Tb - wk.T


def forward(state, W, H, mode, shift=0.0, wk=None):
    """-> dict(distortion [H, W], moment [H, W], depth [H, W], n_contrib [H, W], smax): the prefix formula on depth_ref.walk's pairs.
    `shift` is added to every depth in float64 (the translation-invariance check of the raw mode)."""
    wk = depth_ref.walk(state, W, H) if wk is None else wk
    counts, pixel, Tb, w = _weights(wk)
    z = wk.z.astype(np.float64) + shift
    s = f_map(z, mode)
    ws = w * s
    N = W * H
    # the map does not change when every s of a pixel moves by a constant, but its float64 round-off does: the prefix sums are
    # formed on s - (the pixel's first s), which keeps the terms at the size of the ray's spread and not of s itself
    sc = s - np.repeat(s[wk.start[:-1][counts > 0]], counts[counts > 0]) if s.size else s
    wsc = w * sc
    S_lt = _seg_cumsum(wsc, wk.start, counts) - wsc
    dist = 2.0 * np.bincount(pixel, weights=w * (sc * (1.0 - Tb) - S_lt), minlength=N)
    pl = np.asarray(depth_ref._get(state, "point_list")).astype(np.int64)
    zs = np.asarray(depth_ref._get(state, "depths"), np.float64)[np.unique(pl)] + shift if pl.size else np.zeros(1)
    return dict(distortion=dist.reshape(H, W), moment=np.bincount(pixel, weights=ws, minlength=N).reshape(H, W),
                depth=np.bincount(pixel, weights=w * z, minlength=N).reshape(H, W), n_contrib=wk.n_contrib.reshape(H, W),
                smax=float(np.abs(f_map(zs, mode)).max()), walk=wk)


def forward_candidates(state, W, H, mode):
    """What the forward kernel is held to on an oracle forward `state`: forward() on the walk that takes every skip decision from
    the fp32 formula (depth_grad_ref.walk_flipped(fp32=)), and, for each of the at most 2 pairs whose fp32 alpha is within EXP_BAND
    of 1/255, under both decisions. -> [forward() dicts]; the first one also carries "ambiguous_pixels", the pixels of those pairs:
    only they may match another reference than the first."""
    d = {k: np.asarray(depth_ref._get(state, k)) for k in ("means2D", "conic_opacity", "depths", "point_list", "ranges")}
    f32 = (d["means2D"].astype(np.float32), d["conic_opacity"].astype(np.float32))
    report = {}
    out = [forward(d, W, H, mode, wk=dgr.walk_flipped(d, W, H, fp32=f32, report=report))]
    amb = sorted(set(report.get("ambiguous", [])))
    assert len(amb) <= 2, amb
    out[0]["ambiguous_pixels"] = sorted({int(p) for p, _ in amb})
    for k in range(1, len(amb) + 1):
        for sub in itertools.combinations(amb, k):
            out.append(forward(d, W, H, mode, wk=dgr.walk_flipped(d, W, H, flip=sub, fp32=f32)))
    return out


def forward_brute(state, W, H, mode, pixels=None, wk=None):
    """the double sum with the absolute value, for the pixels given (default: all) -> [len(pixels)]"""
    wk = depth_ref.walk(state, W, H) if wk is None else wk
    _, _, _, w = _weights(wk)
    pixels = np.arange(W * H) if pixels is None else np.asarray(pixels)
    out = np.zeros(pixels.size)
    for n, p in enumerate(pixels):
        sl = slice(wk.start[p], wk.start[p + 1])
        wp, sp = w[sl], f_map(wk.z[sl].astype(np.float64), mode)
        out[n] = float((wp[:, None] * wp[None, :] * np.abs(sp[:, None] - sp[None, :])).sum())
    return out


# ---------------------------------------------------------------------------------------------------------------- gradients
def _pairs(st, pix, conic, opac, z, flip=(), fp32=False, report=None):
    """the blended (pixel, entry) pairs of the walk on the float64 per-Gaussian values, as depth_grad_ref.closed_form sets them up"""
    W, H = st.W, st.H
    co = np.concatenate([conic, opac[:, None]], 1)
    state = dict(means2D=pix, conic_opacity=co, depths=z.astype(np.float32), point_list=st.point_list, ranges=st.ranges)
    if not flip and not fp32:
        wk = depth_ref.walk(state, W, H)
    else:
        f32 = (np.asarray(st.means2D, np.float32), np.asarray(st.conic_opacity, np.float32)) if fp32 else None
        wk = dgr.walk_flipped(state, W, H, flip, f32, report)
    counts, pixel, Tb, _ = _weights(wk)
    gx = (W + 15) // 16
    py, px = np.divmod(pixel, W)
    tile = (py // 16) * gx + px // 16
    gid = np.asarray(st.point_list).astype(np.int64)[np.asarray(st.ranges).astype(np.int64)[tile, 0] + wk.pos - 1]
    dx, dy = pix[gid, 0] - px, pix[gid, 1] - py
    power = -0.5 * (co[gid, 0] * dx * dx + co[gid, 2] * dy * dy) - co[gid, 1] * dx * dy
    G = np.exp(power)
    alpha = np.minimum(depth_ref.A_MAX, co[gid, 3] * G)
    assert np.allclose(wk.T / (1.0 - alpha), Tb, rtol=1e-12, atol=0)
    last = np.zeros(W * H, np.int64)
    has = counts > 0
    last[has] = wk.start[1:][has] - 1
    Tfin = np.where(has, wk.T[last] if wk.T.size else 1.0, 1.0)
    return SimpleNamespace(W=W, H=H, N=W * H, P=pix.shape[0], co=co, wk=wk, counts=counts, pixel=pixel, px=px, py=py, gid=gid,
                           dx=dx, dy=dy, G=G, alpha=alpha, Tb=Tb, Tfin=Tfin, z=z[gid], start=wk.start)


def _per_pair_f64(pr, gD, gA, gL, mode):
    """-> (dL/dalpha, dL/dz) of every pair, float64, from the equations"""
    a, Tb, z, pixel = pr.alpha, pr.Tb, pr.z, pr.pixel
    gD, gA, gL = (m.reshape(-1)[pixel] for m in (gD, gA, gL))
    w = a * Tb
    s = f_map(z, mode)
    ws = w * s
    incl = _seg_cumsum(ws, pr.start, pr.counts)
    M = np.bincount(pixel, weights=ws, minlength=pr.N)[pixel]
    S_lt, S_gt = incl - ws, M - incl
    dA = (1.0 - Tb) - (Tb * (1.0 - a) - pr.Tfin[pixel])
    u = 2.0 * gL * (s * dA - S_lt + S_gt)
    c = gD * z + gA + u
    wc = w * c
    suffix = np.bincount(pixel, weights=wc, minlength=pr.N)[pixel] - _seg_cumsum(wc, pr.start, pr.counts)
    return Tb * c - suffix / (1.0 - a), w * (gD + 2.0 * gL * dA * df_map(z, mode))


def _fma(a, b, c):
    """fp32 fused multiply-add: the product of two fp32 values is exact in float64; one float64 rounding in front of the fp32 one"""
    return (a.astype(np.float64) * b.astype(np.float64) + c.astype(np.float64)).astype(np.float32)


def _s_fp32(z, mode):
    """(s, f', and s - p as fn(pair indices, p)) as common.hpp's DistortionMap forms them: s = fmaf(-c1, 1 / z, c0), and about a pivot
    fmaf(-c1, 1 / z, c0 - p), one rounding at the size of the difference (raw: z and z - p)"""
    f = np.float32
    if mode is None:
        return z, np.ones_like(z), (lambda i, p: z[i] + (-p)), z, f(0.0)
    near, far = mode
    c0d = float(f(far)) / (float(f(far)) - float(f(near)))
    c0, c1 = f(c0d), f(c0d * float(f(near)))
    rz = f(1.0) / z
    about = lambda i, p: _fma(np.full(i.size, -c1, f), rz[i], c0 - p)      # noqa: E731
    return _fma(np.full_like(z, -c1), rz, np.full_like(z, c0)), (c1 * rz) * rz, about, -c1 * rz, c0


def _per_pair_f32(pr, gD, gA, gL, mode, maps=None, pivot=True):
    """the kernels' recurrences in numpy float32, one list position of every pixel per step. -> (dL/dalpha, dL/dz) float64 arrays
    of fp32 values; `maps`, a dict, receives the forward kernel's "distortion" and "moment" [H, W]."""
    f = np.float32
    a_all, z_all = pr.alpha.astype(f), pr.z.astype(f)
    s_all, ds_all, s_about, srel_all, c0 = _s_fp32(z_all, mode)
    N, counts, start = pr.N, pr.counts, pr.start[:-1]
    one = f(1.0)
    # render_distortion_kernel, front to back: the sums run on s about the pixel's first blended entry (without the mapping's
    # constant c0), and the moment is put together at the end
    Tr, S, dist, p1 = np.ones(N, f), np.zeros(N, f), np.zeros(N, f), np.zeros(N, f)
    for k in range(int(counts.max()) if counts.size else 0):
        act = np.nonzero(counts > k)[0]
        i = start[act] + k
        a = a_all[i]
        if k == 0:
            p1[act] = srel_all[i]                                # T == 1: nothing blended in front
        s = srel_all[i] - p1[act]
        w = a * Tr[act]
        dist[act] = _fma(w, _fma(s, one - Tr[act], -S[act]), dist[act])
        S[act] = _fma(s, w, S[act])
        Tr[act] = Tr[act] * (one - a)
    Tfin = Tr.copy()
    M = _fma(np.full(N, c0, f), one - Tfin, _fma(p1, one - Tfin, S))
    if maps is not None:
        maps["distortion"], maps["moment"] = (f(2.0) * dist).reshape(pr.H, pr.W), M.reshape(pr.H, pr.W)
    # render_maps_backward_kernel<DIST = true>, back to front; M is the forward kernel's moment, Tfin its final T
    gD, gA = gD.reshape(-1).astype(f), gA.reshape(-1).astype(f)
    gL2 = f(2.0) * gL.reshape(-1).astype(f)
    Sd, Ss = np.zeros(N, f), np.zeros(N, f)
    dLda, dz = np.zeros(a_all.size, f), np.zeros(a_all.size, f)
    if pivot:                                                   # s -> s - moment / A, moment -> moment - pivot A (about 0)
        A = one - Tfin
        with np.errstate(divide="ignore", invalid="ignore"):
            piv = np.where(A > 0, M / A, f(0.0)).astype(f)
        M = _fma(-piv, A, M)
    else:
        piv = np.zeros(N, f)
    for k in range(int(counts.max()) if counts.size else 0):
        act = np.nonzero(counts > k)[0]
        i = start[act] + counts[act] - 1 - k
        a, s, z = a_all[i], (s_about(i, piv[act]) if pivot else s_all[i]), z_all[i]
        rinv = one / (one - a)
        Tk = Tr[act] * rinv
        dA = (one - Tk) - (Tr[act] - Tfin[act])
        Tr[act] = Tk
        wgt = a * Tk
        ws = wgt * s
        Slt = (M[act] - Ss[act]) - ws
        u = gL2[act] * _fma(s, dA, Ss[act] - Slt)
        cd = (z * gD[act] + gA[act]) + u
        dLda[i] = _fma(Tk, cd, -(rinv * Sd[act]))
        Sd[act] = _fma(wgt, cd, Sd[act])
        Ss[act] = Ss[act] + ws
        dz[i] = wgt * _fma(gL2[act] * dA, ds_all[i], gD[act])
    return dLda.astype(np.float64), dz.astype(np.float64)


def _fold(pr, dL_dalpha, dz):
    """per pair -> per Gaussian: depth_grad_ref.closed_form's fold"""
    co, gid, dx, dy, G, P = pr.co, pr.gid, pr.dx, pr.dy, pr.G, pr.P
    gG = co[gid, 3] * dL_dalpha * G                               # straight through the 0.99 clamp
    out = dict(opacity=np.zeros(P), conic=np.zeros((P, 3)), mean2D=np.zeros((P, 2)), z=np.zeros(P))
    np.add.at(out["opacity"], gid, G * dL_dalpha)
    np.add.at(out["conic"][:, 0], gid, gG * (-0.5 * dx * dx))
    np.add.at(out["conic"][:, 1], gid, gG * (-dx * dy))
    np.add.at(out["conic"][:, 2], gid, gG * (-0.5 * dy * dy))
    np.add.at(out["mean2D"][:, 0], gid, gG * (-co[gid, 0] * dx - co[gid, 1] * dy))
    np.add.at(out["mean2D"][:, 1], gid, gG * (-co[gid, 2] * dy - co[gid, 1] * dx))
    np.add.at(out["z"], gid, dz)
    out["pairs"] = int(gid.size)
    return out


def closed_form(st, pix, conic, opac, z, gD, gA, gL, mode, flip=(), fp32=False, report=None, per_pair=_per_pair_f64):
    pr = _pairs(st, pix, conic, opac, z, flip, fp32, report)
    return _fold(pr, *per_pair(pr, gD, gA, gL, mode))


def restated(st, inp, gD, gA, gL, mode, flip=(), fp32=False, report=None, per_pair=_per_pair_f64):
    """closed_form + depth_grad_ref's chain -> dict of numpy float64 gradients per leaf (LEAF_ORDER names), plus "z" and "pairs"."""
    lv = dgr._leaves(inp)
    pix, conic, z = dgr.projection(st, lv)
    opac = lv["opacities"].reshape(-1)
    cf = closed_form(st, pix.detach().numpy(), conic.detach().numpy(), opac.detach().numpy(), z.detach().numpy(), gD, gA, gL, mode,
                     flip, fp32, report, per_pair)
    t = lambda a: torch.as_tensor(a, dtype=torch.float64)           # noqa: E731
    s = (t(cf["conic"]) * conic).sum() + (t(cf["mean2D"]) * pix).sum() + (t(cf["z"]) * z).sum() + (t(cf["opacity"]) * opac).sum()
    s.backward()
    g = dgr._grads(lv)
    g["z"], g["pairs"] = cf["z"], cf["pairs"]
    return g


def fp32_restatement(st, inp, gD, gA, gL, mode, flip=(), fp32=False, pivot=True):
    """-> (leaf gradients as restated(), dict(distortion, moment) of the forward recurrences), the per-pair part in numpy float32.
    pivot=True is what the backward kernel runs; False, the plain recurrences, is kept to show what the pivot is for."""
    maps = {}
    g = restated(st, inp, gD, gA, gL, mode, flip, fp32, per_pair=functools.partial(_per_pair_f32, maps=maps, pivot=pivot))
    return g, maps


def autograd_truth(st, inp, gD, gA, gL, mode, flip=(), fp32=False, chunk=2048):
    """float64 autograd over the walk's pairs -> dict of numpy float64 gradients per leaf, plus "z" [P]"""
    lv = dgr._leaves(inp)
    pix, conic, z_proj = dgr.projection(st, lv)
    opac = lv["opacities"].reshape(-1)
    pr = _pairs(st, pix.detach().numpy(), conic.detach().numpy(), opac.detach().numpy(), z_proj.detach().numpy(), flip, fp32)
    dd = torch.float64
    # the depth the maps read, as a node of its own (projection()'s tz also feeds the conic): its gradient is dL/dz alone
    view = torch.tensor(st.inputs["viewmatrix"], dtype=dd).reshape(4, 4)
    z = (torch.cat([lv["means3D"], torch.ones(lv["means3D"].shape[0], 1, dtype=dd)], 1) @ view)[:, 2]
    z.retain_grad()
    maps = [torch.as_tensor(m.reshape(-1), dtype=dd) for m in (gD, gA, gL)]
    pixels = np.nonzero(pr.counts > 0)[0]
    for c0 in range(0, pixels.size, chunk):
        pp = pixels[c0:c0 + chunk]
        cnt = pr.counts[pp]
        m = int(cnt.max())
        col = np.arange(m)[None, :]
        mask = col < cnt[:, None]
        idx = np.where(mask, pr.start[pp][:, None] + col, 0)
        gid = torch.as_tensor(pr.gid[idx])
        msk = torch.as_tensor(mask)
        px, py = (torch.as_tensor(v[idx], dtype=dd) for v in (pr.px, pr.py))
        dx, dy = pix[gid, 0] - px, pix[gid, 1] - py
        power = -0.5 * (conic[gid, 0] * dx * dx + conic[gid, 2] * dy * dy) - conic[gid, 1] * dx * dy
        raw = opac[gid] * torch.exp(power)
        alpha = raw + (torch.clamp_max(raw, depth_ref.A_MAX) - raw).detach()    # the clamp passes the gradient straight through
        alpha = torch.where(msk, alpha, torch.zeros_like(alpha))
        T_after = torch.cumprod(1.0 - alpha, 1)                                    # the segmented cumulative product
        Tb = torch.cat([torch.ones(len(pp), 1, dtype=dd), T_after[:, :-1]], 1)
        w = alpha * Tb
        zz = z[gid]
        s = f_map(zz, mode)
        ws = w * s
        S_lt = torch.cumsum(ws, 1) - ws
        dist = 2.0 * (w * (s * (1.0 - Tb) - S_lt)).sum(1)
        tp = torch.as_tensor(pp)
        loss = (maps[0][tp] * (w * zz).sum(1) + maps[1][tp] * w.sum(1) + maps[2][tp] * dist).sum()
        loss.backward(retain_graph=True)
    g = dgr._grads(lv)
    g["z"] = (torch.zeros_like(z) if z.grad is None else z.grad).numpy().copy()
    return g


def gl_map(W, H):
    return dgr.hashed_map(W, H, SALT, signed=True)


@functools.lru_cache(maxsize=None)
def candidates(name, mode_name, with_depth_maps=False):
    """The float64 gradients the kernel is held to on depth_grad_ref.black_state(name) under the signed hashed gL map (and, with
    `with_depth_maps`, depth_grad_ref.truth's gD and gA next to it; zeros otherwise): once per process, not to be modified.
    -> (replayed pairs, ambiguous pairs, [gradients]), as depth_grad_ref.candidates."""
    st, inp, _, _ = dgr.black_state(name)
    mode = MODES[mode_name]
    gL = gl_map(st.W, st.H)
    zero = np.zeros((st.H, st.W))
    gD, gA = (dgr.hashed_map(st.W, st.H, 1), dgr.hashed_map(st.W, st.H, 2)) if with_depth_maps else (zero, zero)
    report = {}
    first = restated(st, inp, gD, gA, gL, mode, fp32=True, report=report)
    replayed, amb = sorted(set(report.get("replayed", []))), sorted(set(report.get("ambiguous", [])))
    if not replayed and not amb:
        return replayed, amb, [autograd_truth(st, inp, gD, gA, gL, mode)]
    assert len(amb) <= 2, amb
    out = [first]
    for k in range(1, len(amb) + 1):
        for sub in itertools.combinations(amb, k):
            out.append(restated(st, inp, gD, gA, gL, mode, flip=sub, fp32=True))
    return replayed, amb, out
