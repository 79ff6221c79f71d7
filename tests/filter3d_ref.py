"""Restatements of the 3D smoothing filter (TEST INFRASTRUCTURE; csrc/filter3d.hip, include/c3dgs_hip.h "3D smoothing filter").

filter_np(xyz, table, dtype): the filter in NumPy, in the kernel's operation order -- in float32 every operation is the kernel's
single IEEE operation, so the result is the kernel's bit for bit; in float64 (from the same fp32 inputs and the same fp32
constants) it is what the float32 one is measured against. Also returns `near`: the rows with a camera test within
1e-4 x max(|bound|, 1) of its bound (evaluated in the function's dtype), where the two precisions may decide differently.

apply(...): Sigma', o' in torch, dtype-generic and differentiable: float64 is the reference of the kernels, float32 (the same
expressions in cov3d_from_scale_rot's order, tests/aa_ref.py: cov3d) a second fp32 evaluation whose distance from float64 is the
yardstick of the GPU bars. apply_backward(...): the backward's formulas written out (no autograd), the kernel's chain."""
import math

import numpy as np
import torch

from tests import aa_ref

NEAR = np.float32(0.2)
LO, HI = np.float32(-0.15), np.float32(1.15)
SQRT_02 = np.float32(math.sqrt(0.2))


def ring_scene(P, C, seed=0, W=64, H=48, focal=60.0, radius=4.0, extent=3.0):
    """P points uniform in +-extent, C cameras on a ring of `radius` in the xz plane looking at the origin; camera k has focal
    `focal` (1 + 0.1 k) and, for odd k, a 48 x 64 portrait image -> (xyz f32 [P, 3], table f32 [C, 16])"""
    rng = np.random.default_rng(seed)
    xyz = rng.uniform(-extent, extent, (P, 3)).astype(np.float32)
    table = np.zeros((C, 16), np.float32)
    for k in range(C):
        a = 2 * math.pi * k / C
        pos = np.array([radius * math.sin(a), 0.3 * math.sin(3 * a), radius * math.cos(a)])
        fwd = -pos / np.linalg.norm(pos)
        right = np.cross([0.0, 1.0, 0.0], fwd)
        right /= np.linalg.norm(right)
        up = np.cross(fwd, right)
        R = np.stack([right, up, fwd])                        # world -> camera rotation
        table[k, :12] = np.concatenate([R, (-R @ pos)[:, None]], 1).reshape(-1)
        w, h = (H, W) if k % 2 else (W, H)
        table[k, 12] = table[k, 13] = focal * (1 + 0.1 * k)
        table[k, 14], table[k, 15] = w, h
    return xyz, table


def filter_np(xyz, table, dtype=np.float32):
    """-> (filter_3D [P], seen bool [P], near bool [P]) in `dtype`"""
    f = dtype
    p = np.asarray(xyz, np.float32).astype(f)
    t = np.asarray(table, np.float32).astype(f)
    px, py, pz = p[:, 0], p[:, 1], p[:, 2]
    P = p.shape[0]
    dist = np.full(P, np.inf, f)
    near = np.zeros(P, bool)
    focal = f(-np.inf)
    half, lo, hi, z0 = f(0.5), f(LO), f(HI), f(NEAR)
    with np.errstate(divide="ignore", invalid="ignore", over="ignore"):
        for m in t:
            x = m[0] * px + m[1] * py + m[2] * pz + m[3]
            y = m[4] * px + m[5] * py + m[6] * pz + m[7]
            z = m[8] * px + m[9] * py + m[10] * pz + m[11]
            fx, fy, W, H = m[12], m[13], m[14], m[15]
            u = x / z * fx + W * half
            v = y / z * fy + H * half
            valid = (z > z0) & (u >= lo * W) & (u <= hi * W) & (v >= lo * H) & (v <= hi * H)
            dist = np.where(valid, np.minimum(dist, z), dist)
            focal = max(focal, fx)
            for val, bound in ((z, z0), (u, lo * W), (u, hi * W), (v, lo * H), (v, hi * H)):
                near |= np.abs(val - bound) <= f(1e-4) * max(abs(float(bound)), 1.0)
    seen = dist < np.inf
    far = dist[seen].max() if seen.any() else f(0)
    out = (np.where(seen, dist, far) / focal * f(SQRT_02)).astype(f)
    return out, seen, near


def upstream_loop(xyz, table):
    """upstream's compute_3D_filter restated in torch ops on xyz's device: a Python loop over the cameras -> filter_3D [P]"""
    P = xyz.shape[0]
    distance = torch.full((P,), 100000.0, device=xyz.device)
    valid_points = torch.zeros(P, dtype=torch.bool, device=xyz.device)
    focal_length = 0.0
    for m in table.cpu().tolist():
        R = torch.tensor([m[0:3], m[4:7], m[8:11]], device=xyz.device)
        T = torch.tensor([m[3], m[7], m[11]], device=xyz.device)
        xyz_cam = xyz @ R.T + T[None, :]
        valid_depth = xyz_cam[:, 2] > 0.2
        x, y, z = xyz_cam[:, 0], xyz_cam[:, 1], xyz_cam[:, 2]
        z = torch.clamp(z, min=0.001)
        x = x / z * m[12] + m[14] / 2.0
        y = y / z * m[13] + m[15] / 2.0
        in_screen = torch.logical_and(torch.logical_and(x >= -0.15 * m[14], x <= m[14] * 1.15),
                                      torch.logical_and(y >= -0.15 * m[15], y <= 1.15 * m[15]))
        valid = torch.logical_and(valid_depth, in_screen)
        distance[valid] = torch.min(distance[valid], z[valid])
        valid_points = torch.logical_or(valid_points, valid)
        focal_length = max(focal_length, m[12])
    distance[~valid_points] = distance[valid_points].max()
    return distance / focal_length * (0.2 ** 0.5)


def hashed_filter(P, scale, salt=3):
    """a filter for the apply tests: around `scale`, every 7th row 0 and every 11th row 100 x scale (f >> s)"""
    f = (0.25 + aa_ref.hashed(P, salt, signed=False)) * scale
    f[::7] = 0.0
    f[5::11] = 100.0 * scale
    return torch.as_tensor(f, dtype=torch.float32)


def _rows(scales, rotations, scale_factors, g_indices):
    """per-row scales (without the factor), rotations and factor"""
    if g_indices is not None:
        gi = torch.as_tensor(g_indices).to(scales.device).long()
        return scales[gi], rotations[gi], scale_factors.reshape(-1)
    return scales, rotations, torch.ones_like(scales[:, 0])


def coef_of(scales, rotations, f, scale_factors=None, g_indices=None):
    sc, _, sf = _rows(scales, rotations, scale_factors, g_indices)
    s2, f2 = (sf[:, None] * sc) ** 2, (f * f)[:, None]
    r = torch.where(f2 == 0, torch.ones_like(s2), s2 / (s2 + f2))
    return torch.sqrt(r[:, 0] * r[:, 1] * r[:, 2])


def apply(opacities, scales, rotations, f, scale_modifier=1.0, scale_factors=None, g_indices=None, cov3d=None):
    """-> (cov3D' [n, 6], o' [n]) in the dtype of `scales`; `f` [n] a constant of the same dtype. `cov3d` [n, 6]: a caller's
    covariance in place of the one scales and rotations build (the scales then serve the opacity factor alone)"""
    lv = dict(scales=scales, rotations=rotations)
    if g_indices is not None:
        lv["scale_factors"] = scale_factors
    sm = float(np.float32(scale_modifier))                     # the kernel's argument is a float
    c6 = [cov3d[:, k] for k in range(6)] if cov3d is not None else aa_ref.cov3d(lv, dict(scale_modifier=sm, g_indices=g_indices))
    mf = sm * f
    add = torch.where(f == 0, torch.zeros_like(f), mf * mf)
    cov = torch.stack([c6[0] + add, c6[1], c6[2], c6[3] + add, c6[4], c6[5] + add], 1)
    return cov, opacities.reshape(-1) * coef_of(scales, rotations, f, scale_factors, g_indices)


def apply_backward(opacities, scales, rotations, f, d_cov, gp, scale_modifier=1.0, scale_factors=None, g_indices=None):
    """The backward's formulas written out: -> dict(opacities [n], scales, rotations (row- or codebook-sized), scale_factors
    [n] | None). d_cov [n, 6] the gradient of cov3D' (off-diagonal elements counted once: G has half of each on either side),
    gp [n] the gradient of o'."""
    sc, rt, sf = _rows(scales, rotations, scale_factors, g_indices)
    sm = float(np.float32(scale_modifier))
    mod = sf * sm
    s = mod[:, None] * sc
    r, x, y, z = rt[:, 0], rt[:, 1], rt[:, 2], rt[:, 3]
    Rm = torch.stack([1 - 2 * (y * y + z * z), 2 * (x * y - r * z), 2 * (x * z + r * y),
                      2 * (x * y + r * z), 1 - 2 * (x * x + z * z), 2 * (y * z - r * x),
                      2 * (x * z - r * y), 2 * (y * z + r * x), 1 - 2 * (x * x + y * y)], 1).reshape(-1, 3, 3)
    G = torch.stack([d_cov[:, 0], 0.5 * d_cov[:, 1], 0.5 * d_cov[:, 2], 0.5 * d_cov[:, 1], d_cov[:, 3], 0.5 * d_cov[:, 4],
                     0.5 * d_cov[:, 2], 0.5 * d_cov[:, 4], d_cov[:, 5]], 1).reshape(-1, 3, 3)
    L = Rm * s[:, None, :]
    col = 2.0 * (G @ L)                                     # dL/dL
    d_s = (Rm * col).sum(1)                                 # with respect to the scaled scale
    Q = col * s[:, None, :]                                 # dL/dRm
    dq = torch.stack([
        2 * z * (Q[:, 1, 0] - Q[:, 0, 1]) + 2 * y * (Q[:, 0, 2] - Q[:, 2, 0]) + 2 * x * (Q[:, 2, 1] - Q[:, 1, 2]),
        2 * y * (Q[:, 0, 1] + Q[:, 1, 0]) + 2 * z * (Q[:, 0, 2] + Q[:, 2, 0]) + 2 * r * (Q[:, 2, 1] - Q[:, 1, 2]) - 4 * x * (Q[:, 2, 2] + Q[:, 1, 1]),
        2 * x * (Q[:, 0, 1] + Q[:, 1, 0]) + 2 * r * (Q[:, 0, 2] - Q[:, 2, 0]) + 2 * z * (Q[:, 2, 1] + Q[:, 1, 2]) - 4 * y * (Q[:, 2, 2] + Q[:, 0, 0]),
        2 * r * (Q[:, 1, 0] - Q[:, 0, 1]) + 2 * x * (Q[:, 0, 2] + Q[:, 2, 0]) + 2 * y * (Q[:, 2, 1] + Q[:, 1, 2]) - 4 * z * (Q[:, 1, 1] + Q[:, 0, 0])], 1)
    coef = coef_of(scales, rotations, f, scale_factors, g_indices)
    sk, f2 = sf[:, None] * sc, (f * f)[:, None]
    og = (opacities.reshape(-1) * gp * coef)[:, None]
    live = (sk != 0) & (f2 != 0)
    d_c = torch.where(live, og * f2 / (torch.where(live, sk, torch.ones_like(sk)) * (sk * sk + f2)), torch.zeros_like(sk))
    drow = d_s * mod[:, None] + d_c * sf[:, None]
    out = dict(opacities=coef * gp, scale_factors=None)
    if g_indices is not None:
        gi = torch.as_tensor(g_indices).to(scales.device).long()
        out["scales"] = torch.zeros_like(scales).index_add_(0, gi, drow)
        out["rotations"] = torch.zeros_like(rotations).index_add_(0, gi, dq)
        out["scale_factors"] = sm * (d_s * sc).sum(1) + (d_c * sc).sum(1)
    else:
        out["scales"], out["rotations"] = drow, dq
    return out


def autograd_backward(opacities, scales, rotations, f, d_cov, gp, scale_modifier=1.0, scale_factors=None, g_indices=None,
                      dtype=torch.float64):
    """the same gradients by autograd of apply() in `dtype` -> dict as apply_backward (float64 numpy-free torch tensors)"""
    lv = {k: (None if v is None else v.detach().to(dtype).clone().requires_grad_())
          for k, v in dict(opacities=opacities, scales=scales, rotations=rotations, scale_factors=scale_factors).items()}
    cov, o = apply(lv["opacities"], lv["scales"], lv["rotations"], f.to(dtype), scale_modifier, lv["scale_factors"], g_indices)
    ((cov * d_cov.to(dtype)).sum() + (o * gp.to(dtype)).sum()).backward()
    return {k: (None if v is None else (torch.zeros_like(v) if v.grad is None else v.grad).reshape(
        -1 if k in ("opacities", "scale_factors") else v.shape).double()) for k, v in lv.items()}


def relinf(a, b):
    """max |a - b| over max |b| (b the reference)"""
    a, b = torch.as_tensor(a).double().reshape(-1), torch.as_tensor(b).double().reshape(-1)
    return float((a - b).abs().max() / max(float(b.abs().max()), 1e-30)) if b.numel() else 0.0


def apply_inputs(name):
    """the inputs of the antialiasing preset `name` (tests/aa_ref.py: aa_case) that apply() reads, with a hashed filter sized by
    the preset's median scale -> dict(opacities, scales, rotations, scale_factors | None, g_indices | None, scale_modifier, f)"""
    inp = aa_ref.aa_case(name)["inp"]
    gi = inp.get("g_indices")
    sf = inp.get("scale_factors") if gi is not None else None
    sc = inp["scales"] if gi is None else inp["scales"][gi] * sf.reshape(-1, 1)
    n = inp["opacities"].shape[0]
    return dict(opacities=inp["opacities"].reshape(-1).float(), scales=inp["scales"].float(), rotations=inp["rotations"].float(),
                scale_factors=None if sf is None else sf.reshape(-1).float(), g_indices=gi,
                scale_modifier=float(inp["scale_modifier"]), f=hashed_filter(n, float(sc.median())))


def f32_deviation(name):
    """reference against reference on preset `name`: the float32 restatement's rel-inf distance from float64, for cov3D', o' and,
    under hashed cotangents, every gradient -> dict"""
    a = apply_inputs(name)
    n = a["opacities"].shape[0]
    d_cov = torch.as_tensor(aa_ref.hashed(6 * n, 11)).reshape(n, 6)
    gp = torch.as_tensor(aa_ref.hashed(n, 13))
    out = {}
    res = {}
    for dt in (torch.float64, torch.float32):
        c = lambda t: None if t is None else t.to(dt)       # noqa: E731
        with torch.no_grad():
            cov, o = apply(c(a["opacities"]), c(a["scales"]), c(a["rotations"]), c(a["f"]), a["scale_modifier"], c(a["scale_factors"]),
                           a["g_indices"])
        g = autograd_backward(a["opacities"], a["scales"], a["rotations"], a["f"], d_cov, gp, a["scale_modifier"], a["scale_factors"],
                              a["g_indices"], dtype=dt)
        res[dt] = dict(cov3D=cov.double(), opacity=o.double(), **{"d_" + k: v for k, v in g.items() if v is not None})
    for k in res[torch.float64]:
        out[k] = relinf(res[torch.float32][k], res[torch.float64][k])
    return out
