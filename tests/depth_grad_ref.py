"""Float64 reference for the gradients through the depth and alpha maps (csrc/render_maps_backward.hip); test infrastructure.

Two independent float64 computations of the same gradients, on the discrete structure of one oracle forward (which Gaussians
are in which tile, in which order), as tests/dense_ref.py borrows it:

  closed_form(...)   numpy, from the equations. Per pixel, over the entries k = 1..m that tests/depth_ref.py's walk() blends, with
                     w_k = alpha_k T_k, c_k = gD z_k + gA:
                         dL/dalpha_k = T_k c_k - (sum_{j>k} w_j c_j) / (1 - alpha_k)         dL/dz_g = sum over pixels of w_k gD
                     then the product's chain for a colour channel (the 0.99 clamp passes the gradient straight through):
                         dL/dopacity = G dL/dalpha,  dL/dG = o dL/dalpha,  G = exp(power),
                         power = -0.5 (a dx^2 + c dy^2) - b dx dy,  dx = mean_x - pixel_x,
                     folded per Gaussian into dL/dopacity [P], dL/dconic [P, 3], dL/dmean2D in pixels [P, 2] and dL/dz [P].
  chain(...)         torch: those four rows times the Jacobians of projection() (this file's restatement of the EWA projection:
                     2D mean in pixels, conic, view-space depth as functions of the float64 leaves) -> the gradient of every
                     leaf, the z -> means3D row of the view matrix included.
  autograd_truth(...) float64 autograd of dense_ref.dense_render with colors_precomp = (z(means3D), 1, 0) built differentiably,
                     a black background and the image gradient (gD, gA, 0).

walk() decides on the float64 values projection() gives, as dense_render decides on its own float64 values, so both see the
same blends.

Replayed decisions. The gradients are those of the entries THE FORWARD blended: the 1/255 skip is the forward's decision, replayed
and not re-decided. A float64 reference decides again, and where a pair's alpha lies within the fp32 formula's error of 1/255
the two differ: then the reference differentiates another set of entries than the forward blended. On `odd_size` one pair has
alpha64 / (1/255) - 1 = -3.4e-6 while the fp32 formula gives +1.3e-5: blended in fp32, skipped in float64, and with it 1.9e-3
of dL_dmeans3D's largest element (the CPU oracle's backward, the reference's own fp32 formula, is that far from the float64
autograd there as well). walk_flipped(fp32=) therefore takes the skip decision of every visited pair from the fp32 formula on the
oracle's fp32 per-Gaussian values (forward.cu:330-354), and reports the pairs it `replayed` (fp32 and float64 disagree) and the
`ambiguous` ones: fp32 alpha within EXP_BAND (relative) of 1/255, where two fp32 evaluations of the formula (expf, or exp2 of a
pre-scaled exponent) may themselves disagree; EXP_BAND = 4e-6 is (|power| + 3) x 2^-23 at |power| = ln(255) = 5.54, a few ulp of
the exponent's terms and of exp itself. candidates() gives the float64 gradients under the fp32 decisions and, for each
ambiguous pair, under both (as tests/depth_ref.py's median_candidates accepts any entry inside the fp32 band around T = 0.5)."""
import functools

import numpy as np
import torch

from tests import dense_ref, depth_ref

LEAF_ORDER = ("means3D", "means2D", "opacities", "scales", "rotations", "scale_factors", "cov3D_precomp")


def hashed_map(W, H, salt, signed=False):
    """[H, W] float64 in [0.25, 1) (or, signed, the same magnitudes with hashed signs): a multiplicative hash of the pixel index"""
    p = np.arange(W * H, dtype=np.uint64)
    h = ((p + np.uint64(salt) * np.uint64(7919) + np.uint64(1)) * np.uint64(2654435761)) & np.uint64(0xFFFFFFFF)
    v = 0.25 + 0.75 * (h.astype(np.float64) / 2.0 ** 32)
    if signed:
        s = ((h >> np.uint64(7)) & np.uint64(1)).astype(np.float64) * 2.0 - 1.0
        v = v * s
    return v.reshape(H, W).astype(np.float32).astype(np.float64)          # exactly representable in fp32: the GPU sees the same maps


def projection(st, leaves):
    """-> (pix [P, 2], conic [P, 3], z [P]) as float64 torch functions of the leaves; dense_ref.dense_render's expressions"""
    i = st.inputs
    dd = torch.float64
    view = torch.tensor(i["viewmatrix"], dtype=dd).reshape(4, 4)
    proj = torch.tensor(i["projmatrix"], dtype=dd).reshape(4, 4)
    W, H = st.W, st.H
    tfx, tfy = float(i["tan_fovx"]), float(i["tan_fovy"])
    fx, fy = W / (2.0 * tfx), H / (2.0 * tfy)
    mean = leaves["means3D"]
    P = mean.shape[0]
    ones = torch.ones(P, 1, dtype=dd)
    hom = torch.cat([mean, ones], 1) @ proj
    p_w = 1.0 / (hom[:, 3] + 0.0000001)
    ndc = hom[:, :2] * p_w[:, None]
    t = (torch.cat([mean, ones], 1) @ view)[:, :3]
    if "cov3D_precomp" in leaves:
        c6 = leaves["cov3D_precomp"]
    else:
        sc, rt = leaves["scales"], leaves["rotations"]
        mod = float(i["scale_modifier"])
        if i["g_indices"] is not None:
            gi = torch.as_tensor(i["g_indices"])
            s = sc[gi] * (leaves["scale_factors"].reshape(-1, 1) * mod)
            Rm = dense_ref._rot(rt[gi])
        else:
            s = sc * mod
            Rm = dense_ref._rot(rt)
        Lm = Rm * s[:, None, :]
        Sg = Lm @ Lm.transpose(1, 2)
        c6 = torch.stack([Sg[:, 0, 0], Sg[:, 0, 1], Sg[:, 0, 2], Sg[:, 1, 1], Sg[:, 1, 2], Sg[:, 2, 2]], -1)
    Sigma = torch.stack([c6[:, 0], c6[:, 1], c6[:, 2], c6[:, 1], c6[:, 3], c6[:, 4], c6[:, 2], c6[:, 4], c6[:, 5]], -1).reshape(-1, 3, 3)
    limx, limy = 1.3 * tfx, 1.3 * tfy
    txtz, tytz = t[:, 0] / t[:, 2], t[:, 1] / t[:, 2]
    cx = (txtz < -limx) | (txtz > limx)
    cy = (tytz < -limy) | (tytz > limy)
    tx = torch.where(cx, (txtz.clamp(-limx, limx) * t[:, 2]).detach(), t[:, 0])
    ty = torch.where(cy, (tytz.clamp(-limy, limy) * t[:, 2]).detach(), t[:, 1])
    tz = t[:, 2]
    zero = torch.zeros_like(tz)
    J = torch.stack([fx / tz, zero, -(fx * tx) / (tz * tz), zero, fy / tz, -(fy * ty) / (tz * tz)], -1).reshape(-1, 2, 3)
    A = J @ view[:3, :3].T
    cov = A @ Sigma @ A.transpose(1, 2)
    a, b, c = cov[:, 0, 0] + 0.3, cov[:, 0, 1], cov[:, 1, 1] + 0.3
    det = a * c - b * b
    conic = torch.stack([c / det, -b / det, a / det], -1)
    m2d = leaves["means2D"]
    pixx = ((ndc[:, 0] + 1.0) * W - 1.0) * 0.5 + 0.5 * W * m2d[:, 0]
    pixy = ((ndc[:, 1] + 1.0) * H - 1.0) * 0.5 + 0.5 * H * m2d[:, 1]
    return torch.stack([pixx, pixy], -1), conic, tz


EXP_BAND = 4e-6


def _hit_fp32(m32, co32, gid, px, py):
    """the forward's skip decision in the reference's fp32 formula (forward.cu:330-354) -> (hit, alpha) in float32"""
    f = np.float32
    dx, dy = m32[gid, 0] - px.astype(f), m32[gid, 1] - py.astype(f)
    power = f(-0.5) * (co32[gid, 0] * dx * dx + co32[gid, 2] * dy * dy) - co32[gid, 1] * dx * dy
    with np.errstate(over="ignore", invalid="ignore"):
        alpha = np.minimum(f(0.99), co32[gid, 3] * np.exp(np.minimum(power, f(0)), dtype=f))
    return (power <= 0) & (alpha >= f(1.0) / f(255.0)), alpha


def walk_flipped(state, W, H, flip=(), fp32=None, report=None):
    """depth_ref.walk with the hit decision of the pairs in `flip` -- (pixel, 1-based list position) -- inverted. Without flips
    and `fp32` it IS depth_ref.walk (asserted by tests/test_depth_grad_ref_cpu.py). fp32 = (means2D, conic_opacity) float32 of
    the oracle's forward: the skip decisions are the fp32 formula's on them (T and the stop stay float64), and `report`, a dict,
    receives "replayed", the pairs where that changed the decision, and "ambiguous", those with fp32 alpha within EXP_BAND of 1/255."""
    m = np.asarray(state["means2D"], np.float64)
    co = np.asarray(state["conic_opacity"], np.float64)
    depths = np.asarray(state["depths"], np.float32)
    pl = np.asarray(state["point_list"]).astype(np.int64)
    rg = np.asarray(state["ranges"]).astype(np.int64)
    N, gx = W * H, (W + 15) // 16
    py, px = np.divmod(np.arange(N), W)
    tile = (py // 16) * gx + px // 16
    first, length = rg[tile, 0], rg[tile, 1] - rg[tile, 0]
    xs, ys = px.astype(np.float64), py.astype(np.float64)
    T = np.ones(N)
    live = np.nonzero(length > 0)[0]
    out_pix, out_T, out_z, out_pos = [], [], [], []
    by_pos = {}
    for p, pos in flip:
        by_pos.setdefault(int(pos), []).append(int(p))
    j = 0
    while live.size:
        gid = pl[first[live] + j]
        hit, alpha = depth_ref._alpha(m, co, gid, xs[live], ys[live])
        if fp32 is not None:
            hit32, alpha32 = _hit_fp32(fp32[0], fp32[1], gid, px[live], py[live])
            if report is not None:
                near = np.abs(alpha32.astype(np.float64) / depth_ref.A_THR - 1.0) < EXP_BAND
                report.setdefault("ambiguous", []).extend((int(p), j + 1) for p in live[near])
                report.setdefault("replayed", []).extend((int(p), j + 1) for p in live[hit32 != hit])
            hit = hit32
        if j + 1 in by_pos:
            hit = hit ^ np.isin(live, by_pos[j + 1])
        test_T = T[live] * (1.0 - alpha)
        stop = hit & (test_T < depth_ref.T_THR)
        blend = hit & ~stop
        b = live[blend]
        T[b] = test_T[blend]
        out_pix.append(b); out_T.append(test_T[blend]); out_z.append(depths[gid[blend]]); out_pos.append(np.full(b.size, j + 1, np.int64))
        j += 1
        live = live[~stop & (length[live] > j)]
    return depth_ref._csr(N, out_pix, out_T, out_z, out_pos)


def closed_form(st, pix, conic, opac, z, gD, gA, flip=(), fp32=False, report=None):
    """numpy float64. pix [P, 2], conic [P, 3], opac [P], z [P]: the per-Gaussian values; gD, gA [H, W].
    -> dict(opacity [P], conic [P, 3], mean2D [P, 2] (pixel units), z [P])"""
    W, H = st.W, st.H
    P = pix.shape[0]
    co = np.concatenate([conic, opac[:, None]], 1)
    state = dict(means2D=pix, conic_opacity=co, depths=z.astype(np.float32), point_list=st.point_list, ranges=st.ranges)
    if not flip and not fp32:
        wk = depth_ref.walk(state, W, H)
    else:
        f32 = (np.asarray(st.means2D, np.float32), np.asarray(st.conic_opacity, np.float32)) if fp32 else None
        wk = walk_flipped(state, W, H, flip, f32, report)
    N = W * H
    counts = np.diff(wk.start)
    pixel = np.repeat(np.arange(N), counts)                       # pixel of every blended (pixel, entry) pair, list order inside
    gx = (W + 15) // 16
    py, px = np.divmod(pixel, W)
    tile = (py // 16) * gx + px // 16
    gid = np.asarray(st.point_list).astype(np.int64)[np.asarray(st.ranges).astype(np.int64)[tile, 0] + wk.pos - 1]
    dx, dy = pix[gid, 0] - px, pix[gid, 1] - py
    power = -0.5 * (co[gid, 0] * dx * dx + co[gid, 2] * dy * dy) - co[gid, 1] * dx * dy
    G = np.exp(power)
    alpha = np.minimum(depth_ref.A_MAX, co[gid, 3] * G)
    T_before = wk.T / (1.0 - alpha)
    # T_before must be the running product: check it against the previous entry's T_after (1 for a pixel's first entry)
    first = np.zeros(pixel.size, bool)
    first[wk.start[:-1][counts > 0]] = True
    prev = np.where(first, 1.0, np.roll(wk.T, 1))
    assert np.allclose(T_before, prev, rtol=1e-12, atol=0)
    T_before = prev
    w = alpha * T_before
    c = gD.reshape(-1)[pixel] * z[gid] + gA.reshape(-1)[pixel]
    wc = w * c
    # suffix_k = sum_{j > k} w_j c_j inside the pixel: the pixel's total minus the inclusive prefix, both in float64
    csum = np.cumsum(wc)
    base = np.repeat(np.concatenate([[0.0], csum])[wk.start[:-1]], counts)
    incl = csum - base
    total = np.bincount(pixel, weights=wc, minlength=N)[pixel]
    suffix = total - incl
    dL_dalpha = T_before * c - suffix / (1.0 - alpha)
    dL_dG = co[gid, 3] * dL_dalpha                                # straight through the 0.99 clamp
    gG = dL_dG * G
    out = dict(opacity=np.zeros(P), conic=np.zeros((P, 3)), mean2D=np.zeros((P, 2)), z=np.zeros(P))
    np.add.at(out["opacity"], gid, G * dL_dalpha)
    np.add.at(out["conic"][:, 0], gid, gG * (-0.5 * dx * dx))
    np.add.at(out["conic"][:, 1], gid, gG * (-dx * dy))
    np.add.at(out["conic"][:, 2], gid, gG * (-0.5 * dy * dy))
    np.add.at(out["mean2D"][:, 0], gid, gG * (-co[gid, 0] * dx - co[gid, 1] * dy))
    np.add.at(out["mean2D"][:, 1], gid, gG * (-co[gid, 2] * dy - co[gid, 1] * dx))
    np.add.at(out["z"], gid, w * gD.reshape(-1)[pixel])
    out["pairs"] = int(pixel.size)
    return out


def _grads(lv):
    return {k: (torch.zeros_like(v) if v.grad is None else v.grad).numpy().copy() for k, v in lv.items() if k in LEAF_ORDER}


def _leaves(inp):
    lv = dense_ref.leaves_of(inp)
    lv.pop("shs", None)
    lv.pop("colors_precomp", None)
    return lv


def restated(st, inp, gD, gA, flip=(), fp32=False, report=None):
    """closed_form + chain -> dict of numpy float64 gradients per leaf (LEAF_ORDER names), plus "z" [P] and "pairs"."""
    lv = _leaves(inp)
    pix, conic, z = projection(st, lv)
    opac = lv["opacities"].reshape(-1)
    cf = closed_form(st, pix.detach().numpy(), conic.detach().numpy(), opac.detach().numpy(), z.detach().numpy(), gD, gA, flip,
                     fp32, report)
    t = lambda a: torch.as_tensor(a, dtype=torch.float64)           # noqa: E731
    # the four rows times the Jacobians of projection(): one backward of a linear surrogate. The z -> means3D row is the
    # third column of the (transposed) view matrix, through z = projection()'s tz
    s = (t(cf["conic"]) * conic).sum() + (t(cf["mean2D"]) * pix).sum() + (t(cf["z"]) * z).sum() + (t(cf["opacity"]) * opac).sum()
    s.backward()
    g = _grads(lv)
    g["z"], g["pairs"] = cf["z"], cf["pairs"]
    view = np.asarray(st.inputs["viewmatrix"], np.float64).reshape(4, 4)
    g["z_row"] = cf["z"][:, None] * view[:3, 2][None, :]          # what the fold kernel adds to dL_dmeans3D
    return g


def autograd_truth(st, inp, gD, gA):
    """float64 autograd of dense_render on the colour-coded scene -> dict of numpy float64 gradients per leaf, plus "z" [P]"""
    lv = _leaves(inp)
    view = torch.tensor(st.inputs["viewmatrix"], dtype=torch.float64).reshape(4, 4)
    P = lv["means3D"].shape[0]
    z = (torch.cat([lv["means3D"], torch.ones(P, 1, dtype=torch.float64)], 1) @ view)[:, 2]
    col = torch.stack([z, torch.ones_like(z), torch.zeros_like(z)], -1)
    col.retain_grad()
    img = dense_ref.dense_render(st, dict(lv, colors_precomp=col))
    dL = torch.stack([torch.as_tensor(gD), torch.as_tensor(gA), torch.zeros(st.H, st.W, dtype=torch.float64)])
    (img * dL).sum().backward()
    g = _grads(lv)
    g["z"] = col.grad[:, 0].numpy().copy()
    return g


@functools.lru_cache(maxsize=None)
def black_state(name):
    """The oracle forward of depth_ref.scene(name) over a black background (the lists do not depend on it; dense_render reads the
    background from the state): computed once per process, not to be modified. -> (st, inp, cam, indexed)"""
    from tests import cases
    inp, cam, indexed = depth_ref.scene(name) if name in depth_ref.SCENES else cases.make_case(name)
    inp = dict(inp, bg=torch.zeros(3))
    return cases.oracle_forward(inp, cam), inp, cam, indexed


@functools.lru_cache(maxsize=None)
def truth(name, signed=False):
    """autograd_truth of black_state(name) under the hashed maps (salts 1 and 2): once per process, shared, not to be modified.
    -> (gD, gA, gradients)"""
    st, inp, _, _ = black_state(name)
    gD, gA = hashed_map(st.W, st.H, 1, signed), hashed_map(st.W, st.H, 2, signed)
    return gD, gA, autograd_truth(st, inp, gD, gA)


@functools.lru_cache(maxsize=None)
def candidates(name):
    """The float64 gradients the kernel is held to on black_state(name) under truth(name)'s maps: once per process, not to be
    modified. -> (replayed pairs, ambiguous pairs, [gradients]). Where the fp32 and the float64 decisions agree on every pair
    and none is ambiguous: [truth(name)'s autograd gradients]. Otherwise restated() under the fp32 decisions, and for k
    ambiguous pairs (k <= 2 asserted) under each of their 2^k decisions."""
    import itertools
    st, inp, _, _ = black_state(name)
    gD, gA, want = truth(name)
    report = {}
    first = restated(st, inp, gD, gA, fp32=True, report=report)
    replayed, amb = sorted(set(report.get("replayed", []))), sorted(set(report.get("ambiguous", [])))
    if not replayed and not amb:
        return replayed, amb, [want]
    assert len(amb) <= 2, amb
    out = [first]
    for k in range(1, len(amb) + 1):
        for sub in itertools.combinations(amb, k):
            out.append(restated(st, inp, gD, gA, flip=sub, fp32=True))
    return replayed, amb, out


def rel_inf(a, b):
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    return float(np.abs(a - b).max() / max(np.abs(b).max(), 1e-300)) if a.size else 0.0
