"""Float64 references for the normal maps (csrc/normals.hip, csrc/render_normal.hip, csrc/render_maps_backward.hip); test
infrastructure, numpy / torch, built on tests/depth_ref.py, tests/depth_grad_ref.py and tests/distortion_ref.py.

All normals are in VIEW space (x right, y down, z forward). The definitions, restated:

  per-Gaussian normal   q, s = the Gaussian's rotation / scale rows, or with g_indices the codebook rows it selects.
                        m = argmin_j s[j] on the RAW row (no modifier, no scale factor), the lowest j on a tie;
                        c = column m of the rotation matrix of q (q as stored, not normalised); v = R_view c / |c|, or 0 where
                        |c| == 0; sigma = -1 where v . p > 0 for the view-space mean p, else +1; n = sigma v.
                        m and sigma are piecewise constant: the only gradient is dn/dq, the 1 / |c| included.
                        A Gaussian is SIGN-AMBIGUOUS where |v . p| / |p| < AMBIGUOUS_COS in float64: there fp32 may round the
                        other way, and a reference adopts the sign it is given (`sigma=`).
  normal map            N = sum_k w_k n_k over the pairs the forward blended (tests/depth_ref.py's walk), not normalised, no
                        background.
  depth_to_normal       P(x, y) = z(x, y) ((x + 0.5 - W / 2) / fx, (y + 0.5 - H / 2) / fy, 1), fx = W / (2 tan_fovx); interior pixels
                        normalize(cross(P(x, y + 1) - P(x, y - 1), P(x + 1, y) - P(x - 1, y))), normalize(c) = c / max(|c|, 1e-12);
                        the one-pixel border 0.
  gradients             c_k of tests/depth_grad_ref.py / tests/distortion_ref.py gains gN . n_k; dL/dn_g = sum over pixels of w_k gN.
                        restated() is the float64 closed form on the walk's pairs (under replayed fp32 decisions if asked, as
                        depth_grad_ref.candidates), autograd_truth() the float64 autograd of dense_ref.dense_render with the normals
                        as colours plus the other maps' references; tests/test_normal_ref_cpu.py ties the two.
The `_f32` functions restate the kernels' arithmetic in numpy float32, operation for operation."""
import functools
import itertools

import numpy as np
import torch

from tests import dense_ref, depth_grad_ref as dgr, depth_ref, distortion_ref as dr

AMBIGUOUS_COS = 1e-5
SALT = 4                                # of the hashed gN maps (4, 5, 6); 1, 2, 3 are gD, gA, gL


# ---------------------------------------------------------------------------------------------------------------- per Gaussian
def _rows(inp):
    """-> (q [P, 4], s [P, 3] raw rows, g_indices or None) as numpy of the stored dtype"""
    gi = inp.get("g_indices")
    sc, rt = np.asarray(inp["scales"]), np.asarray(inp["rotations"])
    if gi is not None:
        gi = np.asarray(gi).astype(np.int64)
        return rt[gi], sc[gi], gi
    return rt, sc, None


def smallest_axis(s):
    """argmin on the raw fp32 row, the lowest index on a tie (np.argmin returns the first minimum)"""
    return np.argmin(np.asarray(s), axis=1).astype(np.int64)


def _rot_np(q, dt):
    r, x, y, z = (q[:, k].astype(dt) for k in range(4))
    one, two = dt(1), dt(2)
    R = np.empty((q.shape[0], 3, 3), dt)
    R[:, 0, 0] = one - two * (y * y + z * z); R[:, 0, 1] = two * (x * y - r * z); R[:, 0, 2] = two * (x * z + r * y)
    R[:, 1, 0] = two * (x * y + r * z); R[:, 1, 1] = one - two * (x * x + z * z); R[:, 1, 2] = two * (y * z - r * x)
    R[:, 2, 0] = two * (x * z - r * y); R[:, 2, 1] = two * (y * z + r * x); R[:, 2, 2] = one - two * (x * x + y * y)
    return R


def gaussian_normals(inp, viewmatrix, dt=np.float64, sigma=None):
    """-> dict(n [P, 3], m [P], sigma [P], cos [P] = v . p / |p|, v [P, 3]) in `dt`: float64 is the reference, float32 restates
    gaussian_normals_kernel operation for operation. `sigma`: signs to adopt (a [P] array; nan / 0 entries keep the computed one)."""
    q, s, _ = _rows(inp)
    m = smallest_axis(s)
    view = np.asarray(viewmatrix, dt).reshape(-1)
    R = _rot_np(q, dt)
    c = R[np.arange(q.shape[0]), :, m]
    with np.errstate(divide="ignore", invalid="ignore"):
        ln = np.sqrt((c[:, 0] * c[:, 0] + c[:, 1] * c[:, 1]) + c[:, 2] * c[:, 2])
        inv = np.where(ln > 0, dt(1) / ln, dt(0)).astype(dt)
    ch = c * inv[:, None]
    v = np.stack([(view[i] * ch[:, 0] + view[4 + i] * ch[:, 1]) + view[8 + i] * ch[:, 2] for i in range(3)], 1)
    mean = np.asarray(inp["means3D"]).astype(dt)
    p = np.stack([((view[i] * mean[:, 0] + view[4 + i] * mean[:, 1]) + view[8 + i] * mean[:, 2]) + view[12 + i] for i in range(3)], 1)
    dot = (v[:, 0] * p[:, 0] + v[:, 1] * p[:, 1]) + v[:, 2] * p[:, 2]
    sg = np.where(dot > 0, dt(-1), dt(1)).astype(dt)
    if sigma is not None:
        given = np.asarray(sigma, np.float64)
        sg = np.where(np.abs(given) == 1.0, given, sg).astype(dt)
    with np.errstate(divide="ignore", invalid="ignore"):
        cos = dot.astype(np.float64) / np.sqrt((p.astype(np.float64) ** 2).sum(1))
    return dict(n=sg[:, None] * v, m=m, sigma=sg, cos=cos, v=v)


def adopt_ambiguous_signs(ref, gpu_w):
    """the signs a reference takes from the GPU's buffer column w = sigma (m + 1): only where the Gaussian is sign-ambiguous.
    -> (sigma [P] to pass as `sigma=`, the ambiguous ids)"""
    amb = np.nonzero(np.abs(ref["cos"]) < AMBIGUOUS_COS)[0]
    sg = np.zeros(ref["sigma"].shape[0])
    sg[amb] = np.sign(np.asarray(gpu_w, np.float64)[amb])
    return sg, amb


def normals_torch(inp, rotations, viewmatrix, m, sigma):
    """n [P, 3] as a float64 torch function of the `rotations` leaf (a codebook under inp's g_indices), m and sigma held constant"""
    dd = torch.float64
    gi = inp.get("g_indices")
    q = rotations[torch.as_tensor(np.asarray(gi).astype(np.int64))] if gi is not None else rotations
    r, x, y, z = q[:, 0], q[:, 1], q[:, 2], q[:, 3]
    cols = [torch.stack([1 - 2 * (y * y + z * z), 2 * (x * y + r * z), 2 * (x * z - r * y)], 1),
            torch.stack([2 * (x * y - r * z), 1 - 2 * (x * x + z * z), 2 * (y * z + r * x)], 1),
            torch.stack([2 * (x * z + r * y), 2 * (y * z - r * x), 1 - 2 * (x * x + y * y)], 1)]
    mt = torch.as_tensor(m)
    c = torch.where((mt == 0)[:, None], cols[0], torch.where((mt == 1)[:, None], cols[1], cols[2]))
    ln = c.norm(dim=1, keepdim=True)
    ch = torch.where(ln > 0, c / torch.where(ln > 0, ln, torch.ones_like(ln)), torch.zeros_like(c))
    view = torch.as_tensor(np.asarray(viewmatrix, np.float64).reshape(4, 4), dtype=dd)
    return torch.as_tensor(np.asarray(sigma, np.float64), dtype=dd)[:, None] * (ch @ view[:3, :3])


def normal_chain(q, m, sigma, viewmatrix, g, dt=np.float64):
    """dL/dq [P, 4] from g = dL/dn [P, 3]: gsgrad.hpp's normal_grad_to_quat, operation for operation in `dt`"""
    view = np.asarray(viewmatrix, dt).reshape(-1)
    q, g, sigma = q.astype(dt), g.astype(dt), np.asarray(sigma).astype(dt)
    R = _rot_np(q, dt)
    c = R[np.arange(q.shape[0]), :, m]
    with np.errstate(divide="ignore", invalid="ignore"):
        ln = np.sqrt((c[:, 0] * c[:, 0] + c[:, 1] * c[:, 1]) + c[:, 2] * c[:, 2])
        inv = np.where(ln > 0, dt(1) / ln, dt(0)).astype(dt)
    ch = c * inv[:, None]
    gh = np.stack([sigma * ((view[4 * k] * g[:, 0] + view[4 * k + 1] * g[:, 1]) + view[4 * k + 2] * g[:, 2]) for k in range(3)], 1)
    d = (ch[:, 0] * gh[:, 0] + ch[:, 1] * gh[:, 1]) + ch[:, 2] * gh[:, 2]
    gc = (gh - ch * d[:, None]) * inv[:, None]
    r, x, y, z = (q[:, k] for k in range(4))
    g0, g1, g2 = gc[:, 0], gc[:, 1], gc[:, 2]
    two, four = dt(2), dt(4)
    by_m = [np.stack([two * z * g1 - two * y * g2, two * y * g1 + two * z * g2, -four * y * g0 + two * x * g1 - two * r * g2,
                      -four * z * g0 + two * r * g1 + two * x * g2], 1),
            np.stack([-two * z * g0 + two * x * g2, two * y * g0 - four * x * g1 + two * r * g2, two * x * g0 + two * z * g2,
                      -two * r * g0 - four * z * g1 + two * y * g2], 1),
            np.stack([two * y * g0 - two * x * g1, two * z * g0 - two * r * g1 - four * x * g2, two * r * g0 + two * z * g1 - four * y * g2,
                      two * x * g0 + two * y * g1], 1)]
    return np.where((m == 0)[:, None], by_m[0], np.where((m == 1)[:, None], by_m[1], by_m[2]))


# ---------------------------------------------------------------------------------------------------------------- the map
def _state_dict(state):
    return {k: np.asarray(depth_ref._get(state, k)) for k in ("means2D", "conic_opacity", "depths", "point_list", "ranges")}


def _pair_ids(state, W, wk):
    counts, pixel, Tb, w = dr._weights(wk)
    gx = (W + 15) // 16
    py, px = np.divmod(pixel, W)
    tile = (py // 16) * gx + px // 16
    gid = np.asarray(state["point_list"]).astype(np.int64)[np.asarray(state["ranges"]).astype(np.int64)[tile, 0] + wk.pos - 1]
    return pixel, gid, w


def normal_map(state, W, H, n, wk=None):
    """-> dict(normal [3, H, W] float64, n_contrib [H, W], walk): the float64 sum over the walk's blended pairs"""
    d = _state_dict(state)
    wk = depth_ref.walk(d, W, H) if wk is None else wk
    pixel, gid, w = _pair_ids(d, W, wk)
    N = np.stack([np.bincount(pixel, weights=w * n[gid, c], minlength=W * H) for c in range(3)]).reshape(3, H, W)
    return dict(normal=N, n_contrib=wk.n_contrib.reshape(H, W), walk=wk)


def normal_map_candidates(state, W, H, n):
    """What render_normal_kernel is held to on an oracle forward: normal_map() on the walk that takes every skip decision from the
    fp32 formula, and for each of the at most 2 pairs whose fp32 alpha is within EXP_BAND of 1/255 under both decisions, as
    distortion_ref.forward_candidates. The first also carries "ambiguous_pixels"."""
    d = _state_dict(state)
    f32 = (d["means2D"].astype(np.float32), d["conic_opacity"].astype(np.float32))
    report = {}
    out = [normal_map(d, W, H, n, wk=dgr.walk_flipped(d, W, H, fp32=f32, report=report))]
    amb = sorted(set(report.get("ambiguous", [])))
    assert len(amb) <= 2, amb
    out[0]["ambiguous_pixels"] = sorted({int(p) for p, _ in amb})
    for k in range(1, len(amb) + 1):
        for sub in itertools.combinations(amb, k):
            out.append(normal_map(d, W, H, n, wk=dgr.walk_flipped(d, W, H, flip=sub, fp32=f32)))
    return out


def normal_map_brute(state, W, H, n, stride=1):
    """per pixel, a plain loop over the tile's list with the oracle's rule -> [3, H, W]; with `stride`, every stride-th pixel of
    the row-major order only (the others stay NaN)"""
    d = _state_dict(state)
    m, co = d["means2D"].astype(np.float64), d["conic_opacity"].astype(np.float64)
    pl, rg = d["point_list"].astype(np.int64), d["ranges"].astype(np.int64)
    gx = (W + 15) // 16
    out = np.full((3, H, W), np.nan)
    for pix in range(0, W * H, stride):
        py, px = divmod(pix, W)
        lo, hi = rg[(py // 16) * gx + px // 16]
        T, acc = 1.0, np.zeros(3)
        for g in pl[lo:hi]:
            dx, dy = m[g, 0] - px, m[g, 1] - py
            power = -0.5 * (co[g, 0] * dx * dx + co[g, 2] * dy * dy) - co[g, 1] * dx * dy
            if power > 0:
                continue
            alpha = min(depth_ref.A_MAX, co[g, 3] * np.exp(power))
            if alpha < depth_ref.A_THR:
                continue
            if T * (1.0 - alpha) < depth_ref.T_THR:
                break
            acc += alpha * T * n[g]
            T *= 1.0 - alpha
        out[:, py, px] = acc
    return out


# ---------------------------------------------------------------------------------------------------------------- the stencil
def _rays(W, H, tan_fovx, tan_fovy, dt=np.float64):
    fx, fy = W / (2.0 * tan_fovx), H / (2.0 * tan_fovy)
    return ((np.arange(W) + 0.5 - W / 2.0) / fx).astype(dt), ((np.arange(H) + 0.5 - H / 2.0) / fy).astype(dt)


def depth_to_normal(z, tan_fovx, tan_fovy, parts=False):
    """float64 numpy. z [H, W] -> [3, H, W]"""
    z = np.asarray(z, np.float64)
    H, W = z.shape
    out = np.zeros((3, H, W))
    if W < 3 or H < 3:
        return (out, None) if parts else out
    xs, ys = _rays(W, H, tan_fovx, tan_fovy)
    P = np.stack([z * xs[None, :], z * ys[:, None], z], -1)
    a = P[2:, 1:-1] - P[:-2, 1:-1]
    b = P[1:-1, 2:] - P[1:-1, :-2]
    c = np.cross(a, b)
    ln = np.maximum(np.sqrt((c * c).sum(-1)), 1e-12)
    out[:, 1:-1, 1:-1] = np.moveaxis(c / ln[..., None], -1, 0)
    return (out, (a, b, c, ln, xs, ys)) if parts else out


def depth_to_normal_torch(z, tan_fovx, tan_fovy):
    """the same in float64 torch, for autograd"""
    H, W = z.shape
    if W < 3 or H < 3:
        return torch.zeros(3, H, W, dtype=z.dtype) + 0.0 * z.sum()
    xs, ys = (torch.as_tensor(v) for v in _rays(W, H, tan_fovx, tan_fovy))
    P = torch.stack([z * xs[None, :], z * ys[:, None], z], -1)
    a = P[2:, 1:-1] - P[:-2, 1:-1]
    b = P[1:-1, 2:] - P[1:-1, :-2]
    c = torch.linalg.cross(a, b)
    n = c / c.norm(dim=-1, keepdim=True).clamp_min(1e-12)
    return torch.nn.functional.pad(n.permute(2, 0, 1), (1, 1, 1, 1))


def depth_to_normal_backward(z, g, tan_fovx, tan_fovy):
    """float64 numpy, from the equations: g [3, H, W] = dL/dnormal -> dL/dz [H, W]"""
    z, g = np.asarray(z, np.float64), np.asarray(g, np.float64)
    H, W = z.shape
    _, parts = depth_to_normal(z, tan_fovx, tan_fovy, parts=True)
    if parts is None:
        return np.zeros((H, W))
    a, b, c, ln, xs, ys = parts
    gi = np.moveaxis(g[:, 1:-1, 1:-1], 0, -1)
    raw = np.sqrt((c * c).sum(-1))
    n = c / ln[..., None]
    gc = np.where((raw > 1e-12)[..., None], (gi - n * (n * gi).sum(-1, keepdims=True)) / ln[..., None], gi / 1e-12)
    ga, gb = np.cross(b, gc), np.cross(gc, a)
    gP = np.zeros((H, W, 3))
    gP[2:, 1:-1] += ga; gP[:-2, 1:-1] -= ga
    gP[1:-1, 2:] += gb; gP[1:-1, :-2] -= gb
    return gP[..., 0] * xs[None, :] + gP[..., 1] * ys[:, None] + gP[..., 2]


def _stencil_f32(z, tan_fovx, tan_fovy):
    """a, b, c, |c| of every interior pixel as depth_to_normal_kernel forms them, numpy float32"""
    f = np.float32
    z = np.asarray(z, f)
    H, W = z.shape
    fx, fy = f(W) / (f(2.0) * f(tan_fovx)), f(H) / (f(2.0) * f(tan_fovy))
    rfx, rfy = f(1.0) / fx, f(1.0) / fy
    hx = (np.arange(W, dtype=f) + f(0.5) - f(0.5) * f(W))[None, 1:-1]
    hy = (np.arange(H, dtype=f) + f(0.5) - f(0.5) * f(H))[1:-1, None]
    zu, zd, zl, zr = z[:-2, 1:-1], z[2:, 1:-1], z[1:-1, :-2], z[1:-1, 2:]
    a2 = zd - zu
    a = [(hx * rfx) * a2, ((hy + f(1)) * rfy) * zd - ((hy - f(1)) * rfy) * zu, a2]
    b2 = zr - zl
    b = [((hx + f(1)) * rfx) * zr - ((hx - f(1)) * rfx) * zl, (hy * rfy) * b2, b2]
    return a, b, hx * rfx, hy * rfy, (rfx, rfy)


def _cross_f32(a, b):
    return [a[1] * b[2] - a[2] * b[1], a[2] * b[0] - a[0] * b[2], a[0] * b[1] - a[1] * b[0]]


def depth_to_normal_f32(z, tan_fovx, tan_fovy):
    f = np.float32
    z = np.asarray(z, f)
    H, W = z.shape
    out = np.zeros((3, H, W), f)
    if W < 3 or H < 3:
        return out
    a, b, _, _, _ = _stencil_f32(z, tan_fovx, tan_fovy)
    c = _cross_f32(a, b)
    ln = np.maximum(np.sqrt((c[0] * c[0] + c[1] * c[1]) + c[2] * c[2]), f(1e-12))
    for k in range(3):
        out[k, 1:-1, 1:-1] = c[k] / ln
    return out


def depth_to_normal_backward_f32(z, g, tan_fovx, tan_fovy):
    """depth_to_normal_backward_kernel's arithmetic per stencil; the four signed contributions of a pixel are added in the kernel's
    order (above, below, left, right)"""
    f = np.float32
    z, g = np.asarray(z, f), np.asarray(g, f)
    H, W = z.shape
    if W < 3 or H < 3:
        return np.zeros((H, W), f)
    a, b, _, _, (rfx, rfy) = _stencil_f32(z, tan_fovx, tan_fovy)
    c = _cross_f32(a, b)
    ln = np.sqrt((c[0] * c[0] + c[1] * c[1]) + c[2] * c[2])
    gi = [g[k, 1:-1, 1:-1] for k in range(3)]
    with np.errstate(divide="ignore", invalid="ignore"):
        n = [c[k] / ln for k in range(3)]
        d = (n[0] * gi[0] + n[1] * gi[1]) + n[2] * gi[2]
        gc = [np.where(ln > f(1e-12), (gi[k] - n[k] * d) / ln, gi[k] / f(1e-12)).astype(f) for k in range(3)]
    ga, gb = _cross_f32(b, gc), _cross_f32(gc, a)
    gP = np.zeros((3, H, W), f)
    for k in range(3):
        gP[k, 2:, 1:-1] += ga[k]
    for k in range(3):
        gP[k, :-2, 1:-1] -= ga[k]
    for k in range(3):
        gP[k, 1:-1, 2:] += gb[k]
    for k in range(3):
        gP[k, 1:-1, :-2] -= gb[k]
    rx = ((np.arange(W, dtype=f) + f(0.5) - f(0.5) * f(W)) * rfx)[None, :]
    ry = ((np.arange(H, dtype=f) + f(0.5) - f(0.5) * f(H)) * rfy)[:, None]
    return (rx * gP[0] + ry * gP[1]) + gP[2]


def plane_depth(W, H, tan_fovx, tan_fovy, a, d):
    """z [H, W] float64 of the plane a . X = d seen through the pixel centres: z = d / (a . ray)"""
    xs, ys = _rays(W, H, tan_fovx, tan_fovy)
    return d / (a[0] * xs[None, :] + a[1] * ys[:, None] + a[2])


def smooth_surface(W, H, seed=0, zmin=2.0, zmax=9.0):
    """a smooth random surface with z in [zmin, zmax]: a few low-frequency waves; float64 values exactly representable in fp32"""
    rng = np.random.default_rng(seed)
    y, x = np.mgrid[0:H, 0:W]
    s = np.zeros((H, W))
    for _ in range(4):
        fx, fy, ph = rng.uniform(0.5, 2.5) / W, rng.uniform(0.5, 2.5) / H, rng.uniform(0, 2 * np.pi)
        s += rng.uniform(0.3, 1.0) * np.sin(2 * np.pi * (fx * x + fy * y) + ph)
    s = (s - s.min()) / (s.max() - s.min())
    return (zmin + (zmax - zmin) * s).astype(np.float32).astype(np.float64)


def normal_consistency(depth, alpha, normal, tan_fovx, tan_fovy):
    """float64 torch restatement of c3dgs_amd.normals.normal_consistency"""
    z = depth / alpha.clamp_min(1e-6)
    surface = depth_to_normal_torch(z, tan_fovx, tan_fovy) * alpha.detach()
    return (1.0 - (normal * surface).sum(0)).mean()


# ---------------------------------------------------------------------------------------------------------------- gradients
def gn_map(W, H):
    return np.stack([dgr.hashed_map(W, H, SALT + c, signed=True) for c in range(3)])


def _normal_pairs(pr, gN, n):
    """-> (dL/dalpha of every pair through the normal map, dL/dn [P, 3])"""
    g = gN.reshape(3, -1)[:, pr.pixel].T
    cn = (g * n[pr.gid]).sum(1)
    w = pr.alpha * pr.Tb
    wc = w * cn
    suffix = np.bincount(pr.pixel, weights=wc, minlength=pr.N)[pr.pixel] - dr._seg_cumsum(wc, pr.start, pr.counts)
    dn = np.zeros((pr.P, 3))
    np.add.at(dn, pr.gid, w[:, None] * g)
    return pr.Tb * cn - suffix / (1.0 - pr.alpha), dn


def restated(st, inp, gN, gD=None, gA=None, gL=None, mode=None, flip=(), fp32=False, report=None, sigma=None):
    """The float64 closed form on the walk's pairs + the chains -> dict of numpy float64 gradients per leaf (depth_grad_ref's
    LEAF_ORDER names), plus "n" [P, 3] = dL/dn, "z" and "pairs". Maps that are None count as zeros."""
    lv = dgr._leaves(inp)
    pix, conic, z = dgr.projection(st, lv)
    opac = lv["opacities"].reshape(-1)
    pr = dr._pairs(st, pix.detach().numpy(), conic.detach().numpy(), opac.detach().numpy(), z.detach().numpy(), flip, fp32, report)
    zero = np.zeros((st.H, st.W))
    dLda, dz = dr._per_pair_f64(pr, zero if gD is None else gD, zero if gA is None else gA, zero if gL is None else gL, mode)
    ng = gaussian_normals(inp, st.inputs["viewmatrix"], sigma=sigma)
    dn_alpha, dn = _normal_pairs(pr, gN, ng["n"])
    cf = dr._fold(pr, dLda + dn_alpha, dz)
    t = lambda a: torch.as_tensor(a, dtype=torch.float64)           # noqa: E731
    nt = normals_torch(inp, lv["rotations"], st.inputs["viewmatrix"], ng["m"], ng["sigma"])
    s = (t(cf["conic"]) * conic).sum() + (t(cf["mean2D"]) * pix).sum() + (t(cf["z"]) * z).sum() + (t(cf["opacity"]) * opac).sum() + \
        (t(dn) * nt).sum()
    s.backward()
    g = dgr._grads(lv)
    g["z"], g["pairs"], g["n"] = cf["z"], cf["pairs"], dn
    return g


def autograd_truth(st, inp, gN, gD=None, gA=None, sigma=None):
    """float64 autograd of dense_ref.dense_render with the normals (built differentiably from the rotations) as colours, a black
    background and the image gradient gN; plus, with gD / gA, depth_grad_ref.autograd_truth's gradients. Decides every pair in
    float64: for scenes where no decision is replayed."""
    lv = dgr._leaves(inp)
    ng = gaussian_normals(inp, st.inputs["viewmatrix"], sigma=sigma)
    col = normals_torch(inp, lv["rotations"], st.inputs["viewmatrix"], ng["m"], ng["sigma"])
    img = dense_ref.dense_render(st, dict(lv, colors_precomp=col))
    (img * torch.as_tensor(gN)).sum().backward()
    g = dgr._grads(lv)
    if gD is not None or gA is not None:
        zero = np.zeros((st.H, st.W))
        other = dgr.autograd_truth(st, inp, zero if gD is None else gD, zero if gA is None else gA)
        g = {k: g[k] + other[k] for k in g}
    return g


def candidates(name, combo, mode_name="raw", sigma=None):
    """The float64 gradients the backward is held to on depth_grad_ref.black_state(name). combo: "gN", "gD+gA+gN" or
    "gD+gA+gL+gN"; the maps are the hashed ones of the three reference files. -> (replayed, ambiguous, [gradients]) as
    depth_grad_ref.candidates: restated() under the fp32 decisions, and for each ambiguous pair under both."""
    st, inp, _, _ = dgr.black_state(name)
    W, H = st.W, st.H
    gN = gn_map(W, H)
    gD, gA = (dgr.hashed_map(W, H, 1), dgr.hashed_map(W, H, 2)) if "gD" in combo else (None, None)
    gL = dr.gl_map(W, H) if "gL" in combo else None
    mode = dr.MODES[mode_name]
    report = {}
    first = restated(st, inp, gN, gD, gA, gL, mode, fp32=True, report=report, sigma=sigma)
    replayed, amb = sorted(set(report.get("replayed", []))), sorted(set(report.get("ambiguous", [])))
    assert len(amb) <= 2, amb
    out = [first]
    for k in range(1, len(amb) + 1):
        for sub in itertools.combinations(amb, k):
            out.append(restated(st, inp, gN, gD, gA, gL, mode, flip=sub, fp32=True, sigma=sigma))
    return replayed, amb, out


@functools.lru_cache(maxsize=None)
def scene_normals(name):
    """gaussian_normals (float64) of depth_ref.scene(name) under its camera: once per process, not to be modified"""
    inp, cam, _ = depth_ref.scene(name)
    return gaussian_normals(inp, cam["viewmatrix"])


# ---------------------------------------------------------------------------------------------------------------- bars
U = 2.0 ** -24


def stencil_inputs():
    """The maps the stencil tests run on: the two tilted planes at 70 x 45 (focal 50) and 16 x 16 (focal 125), and a smooth random
    surface with z in [2, 9] at 70 x 45. -> [(label, z as fp32-representable float64 [H, W], tan_fovx, tan_fovy)]"""
    out = []
    for W, H, focal in ((70, 45, 50.0), (16, 16, 125.0)):
        tfx, tfy = W / (2.0 * focal), H / (2.0 * focal)
        for k, a in enumerate(TILTED):
            z = plane_depth(W, H, tfx, tfy, a, 4.0).astype(np.float32).astype(np.float64)
            out.append((f"plane{k} {W}x{H} f{focal:g}", z, tfx, tfy))
    out.append(("surface 70x45 f50", smooth_surface(70, 45, seed=7), 70 / 100.0, 45 / 100.0))
    return out


def _unit(a):
    a = np.asarray(a, np.float64)
    return a / np.sqrt((a * a).sum())


TILTED = (_unit((0.3, -0.2, 1.0)), _unit((-0.5, 0.4, 1.0)))


@functools.lru_cache(maxsize=None)
def stencil_bars():
    """-> dict(forward=(worst, k), backward=(worst, bar)): the fp32 restatement's worst error on stencil_inputs() against float64 on
    the same fp32 input. Forward: in units of 2^-24 max(fx, fy) (the error grows like 2^-24 max(fx, fy) zmax / dz); k = 4 x that
    worst is the GPU bar's constant. Backward: rel-inf under gn_map's gradient; the GPU bar is 4 x the worst."""
    wf = wb = 0.0
    for label, z, tfx, tfy in stencil_inputs():
        H, W = z.shape
        unit = U * max(W / (2.0 * tfx), H / (2.0 * tfy))
        wf = max(wf, float(np.abs(depth_to_normal_f32(z, tfx, tfy).astype(np.float64) - depth_to_normal(z, tfx, tfy)).max()) / unit)
        g = gn_map(W, H)
        wb = max(wb, dgr.rel_inf(depth_to_normal_backward_f32(z, g, tfx, tfy), depth_to_normal_backward(z, g, tfx, tfy)))
    return dict(forward=(wf, 4.0 * wf), backward=(wb, 4.0 * wb))


@functools.lru_cache(maxsize=None)
def gaussian_normals_bar():
    """-> (the fp32 restatement's worst component error over depth_ref.SCENES, sign-ambiguous Gaussians aside; the GPU bar):
    16 x 2^-24 per component, or 4 x the restatement's worst where that is more"""
    worst = 0.0
    for name in depth_ref.SCENES:
        inp, cam, _ = depth_ref.scene(name)
        ref = gaussian_normals(inp, cam["viewmatrix"])
        f32 = gaussian_normals(inp, cam["viewmatrix"], np.float32)
        ok = np.abs(ref["cos"]) >= AMBIGUOUS_COS
        worst = max(worst, float(np.abs(f32["n"].astype(np.float64) - ref["n"])[ok].max()))
    return worst, (16 * U if worst <= 16 * U else 4 * worst)
