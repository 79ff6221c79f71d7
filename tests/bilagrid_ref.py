"""Reference of the bilateral-grid slice and its total variation (include/c3dgs_hip.h, "bilateral grid"), test infrastructure:

    slice_direct / slice_backward_direct     the contract's formula and its closed-form backward, numpy float64
    slice_grid_sample                        the same through torch.nn.functional.grid_sample with autograd, in any dtype: float64
                                             pins the direct formula, float32 sizes the bars of the GPU tests
    tv / tv_backward_direct                  the total variation and its gradient
plus the hashed inputs of the tests. An image is conditioned so that, in float64, every pixel's z keeps 1e-3 from every integer
and every luma 1e-3 / max(L - 1, 1) from 0 and 1: the gradient through the guidance is piecewise constant and flips there."""
import numpy as np
import torch

LUMA = np.array([0.299, 0.587, 0.114])
SHAPES = [(1, 1, 1), (2, 2, 2), (8, 16, 16), (3, 2, 5), (1, 4, 3), (4, 1, 1)]        # (L, Hg, Wg)
SIZES = [(1, 1), (3, 5), (17, 33), (64, 64), (70, 130)]                            # (H, W)
CASES = [(s, hw) for s in SHAPES for hw in SIZES] + [((8, 16, 16), (5, 3))]      # 5x3: most vertices see no pixel
# the per-pixel kernels stage the part of the grid a 256-pixel row segment reaches in LDS: a row of three segments, the last one
# ragged, that reach 8 of the 16 columns each; and a grid whose staged part exceeds the LDS budget (the through-the-caches path)
CASES += [((8, 16, 16), (3, 700)), ((40, 2, 16), (5, 7))]


def hashed(shape, seed):
    """Deterministic values in [0, 1): a splitmix64 of the element index, float64."""
    n = int(np.prod(shape))
    with np.errstate(over="ignore"):
        x = np.arange(n, dtype=np.uint64) + np.uint64(seed) * np.uint64(0x9E3779B97F4A7C15)
        x = (x ^ (x >> np.uint64(30))) * np.uint64(0xBF58476D1CE4E5B9)
        x = (x ^ (x >> np.uint64(27))) * np.uint64(0x94D049BB133111EB)
        x = x ^ (x >> np.uint64(31))
    return ((x >> np.uint64(11)).astype(np.float64) / float(1 << 53)).reshape(shape)


def offenders(rgb, L):
    """Pixels of a float32 image whose guidance sits too close to a kink, judged in float64."""
    luma = np.tensordot(LUMA, rgb.astype(np.float64), 1)
    z = np.clip(luma, 0.0, 1.0) * (L - 1)
    edge = 1e-3 / max(L - 1, 1)
    bad = (np.abs(luma) < edge) | (np.abs(luma - 1.0) < edge)
    if L > 1:
        inside = (luma > 0.0) & (luma < 1.0)
        bad |= inside & (np.abs(z - np.round(z)) < 1e-3)
    return bad


def make_image(H, W, L, seed):
    """float32 [3, H, W] hashed into [-0.2, 1.2] (lumas are clamped at both ends), offenders nudged until none remains."""
    rgb = (hashed((3, H, W), seed) * 1.4 - 0.2).astype(np.float32)
    for _ in range(64):
        bad = offenders(rgb, L)
        if not bad.any():
            return rgb
        rgb[:, bad] += np.float32(0.0037)
    raise AssertionError("make_image: offenders remain")


def make_grid(L, Hg, Wg, seed, noise=0.2):
    """float32 [12, L, Hg, Wg]: the identity affine plus hashed noise."""
    eye = np.eye(3, 4).reshape(12, 1, 1, 1)
    return (eye + noise * (hashed((12, L, Hg, Wg), seed) - 0.5)).astype(np.float32)


def _axis(n, ng):
    if ng == 1:
        return np.zeros(n, dtype=np.int64), np.zeros(n, dtype=np.int64), np.zeros(n)
    g = (np.arange(n) + 0.5) / n * (ng - 1)
    i0 = np.minimum(np.floor(g), ng - 2).astype(np.int64)
    return i0, i0 + 1, g - i0


def _coords(G, rgb):
    _, L, Hg, Wg = G.shape
    _, H, W = rgb.shape
    i0, i1, fx = _axis(W, Wg)
    j0, j1, fy = _axis(H, Hg)
    luma = np.tensordot(LUMA, rgb, 1)
    if L == 1:
        k0 = k1 = np.zeros((H, W), dtype=np.int64)
        fz = np.zeros((H, W))
    else:
        z = np.clip(luma, 0.0, 1.0) * (L - 1)
        k0 = np.minimum(np.floor(z), L - 2).astype(np.int64)
        k1, fz = k0 + 1, z - k0
    inside = (luma > 0.0) & (luma < 1.0) & (L > 1)
    corners = []                   # (k [H,W], j [H,1], i [1,W], weight [H,W], xy weight [H,W], sign of d/dz)
    for k, wz, sz in ((k0, 1.0 - fz, -1.0), (k1, fz, 1.0)):
        for j, wy in ((j0, 1.0 - fy), (j1, fy)):
            for i, wx in ((i0, 1.0 - fx), (i1, fx)):
                wxy = wy[:, None] * wx[None, :]
                corners.append((k, j[:, None], i[None, :], wz * wxy, wxy, sz))
    return corners, inside


def slice_direct(G, rgb):
    """float64 out [3, H, W] of the contract's formula."""
    G, rgb = G.astype(np.float64), rgb.astype(np.float64)
    corners, _ = _coords(G, rgb)
    A = sum(w * G[:, k, j, i] for k, j, i, w, _, _ in corners).reshape(3, 4, *rgb.shape[1:])
    return (A[:, :3] * rgb[None]).sum(1) + A[:, 3]


def slice_backward_direct(G, rgb, dout):
    """-> (dL_dG, dL_drgb, magnitude): float64, closed form; magnitude[e] = the sum of |contribution| into dL_dG[e]."""
    G, rgb, dout = G.astype(np.float64), rgb.astype(np.float64), dout.astype(np.float64)
    L = G.shape[1]
    corners, inside = _coords(G, rgb)
    H, W = rgb.shape[1:]
    c1 = np.concatenate([rgb, np.ones((1, H, W))])                                  # (r, g, b, 1)
    outer = (dout[:, None] * c1[None]).reshape(12, H, W)
    dG, mag = np.zeros_like(G), np.zeros_like(G)
    A, dA = np.zeros((12, H, W)), np.zeros((12, H, W))
    rows = np.arange(12)[:, None, None]
    for k, j, i, w, wxy, sz in corners:
        kk, jj, ii = np.broadcast_arrays(k, j, i)
        np.add.at(dG, (rows, kk[None], jj[None], ii[None]), w * outer)
        np.add.at(mag, (rows, kk[None], jj[None], ii[None]), np.abs(w * outer))
        A += w * G[:, k, j, i]
        dA += sz * wxy * G[:, k, j, i]
    A, dA = A.reshape(3, 4, H, W), dA.reshape(3, 4, H, W)
    drgb = (A[:, :3] * dout[:, None]).sum(0)
    dz = (dout * ((dA[:, :3] * rgb[None]).sum(1) + dA[:, 3])).sum(0) * inside
    drgb = drgb + dz[None] * (L - 1) * LUMA[:, None, None]
    return dG, drgb, mag


def slice_grid_sample(G, rgb, dout=None, dtype=torch.float64):
    """The grid_sample form in `dtype` -> out, or with dout (out, dL_dG, dL_drgb) by autograd; numpy arrays of that dtype."""
    g = torch.tensor(np.asarray(G), dtype=dtype, requires_grad=dout is not None)
    c = torch.tensor(np.asarray(rgb), dtype=dtype, requires_grad=dout is not None)
    _, H, W = c.shape
    xs = ((torch.arange(W, dtype=dtype) + 0.5) / W)[None, :].expand(H, W)
    ys = ((torch.arange(H, dtype=dtype) + 0.5) / H)[:, None].expand(H, W)
    luma = torch.tensor([0.299, 0.587, 0.114], dtype=dtype) @ c.reshape(3, -1)
    u = torch.stack([2 * xs - 1, 2 * ys - 1, 2 * luma.reshape(H, W) - 1], -1)[None, None]
    A = torch.nn.functional.grid_sample(g[None], u, mode="bilinear", padding_mode="border", align_corners=True)[0, :, 0]
    A = A.reshape(3, 4, H, W)
    out = (A[:, :3] * c[None]).sum(1) + A[:, 3]
    if dout is None:
        return out.detach().numpy()
    out.backward(torch.tensor(np.asarray(dout), dtype=dtype))
    return out.detach().numpy(), g.grad.numpy(), c.grad.numpy()


def tv_torch(X):
    """The contract's total variation of a torch tensor [C, 12, L, Hg, Wg] (differentiable)."""
    total = (X * 0).sum()                    # a shape of one vertex still has a (zero) gradient
    for axis in (2, 3, 4):
        if X.shape[axis] >= 2:
            d = X.narrow(axis, 1, X.shape[axis] - 1) - X.narrow(axis, 0, X.shape[axis] - 1)
            total = total + d.square().sum() / d[0].numel()
    return total / X.shape[0]


def tv(X, dtype=torch.float64):
    return float(tv_torch(torch.tensor(np.asarray(X), dtype=dtype)))


def tv_backward_autograd(X, dtype=torch.float64):
    x = torch.tensor(np.asarray(X), dtype=dtype, requires_grad=True)
    tv_torch(x).backward()
    return x.grad.numpy()


def tv_backward_direct(X):
    """-> (d tv / dX, magnitude): float64, each element from its up to six neighbours; magnitude = the sum of |term|."""
    X = np.asarray(X, dtype=np.float64)
    C = X.shape[0]
    grad, mag = np.zeros_like(X), np.zeros_like(X)
    for axis in (2, 3, 4):
        n = X.shape[axis]
        if n < 2:
            continue
        d = np.diff(X, axis=axis)
        s = 2.0 / (C * d[0].size)
        lo = [slice(None)] * 5
        hi = [slice(None)] * 5
        lo[axis], hi[axis] = slice(0, n - 1), slice(1, n)
        grad[tuple(hi)] += s * d
        grad[tuple(lo)] -= s * d
        mag[tuple(hi)] += s * np.abs(d)
        mag[tuple(lo)] += s * np.abs(d)
    return grad, mag


def jitter_exposure(cams, S, seed=0):
    """The demonstration's exposure differences: every camera's original_image becomes a_k * image + b_k with per-camera,
    per-channel a in [1 - S, 1 + S] and b in [-S / 4, S / 4] from a seeded generator. -> [(a, b)] per camera (CPU tensors)."""
    gen = torch.Generator().manual_seed(seed)
    drawn = []
    for cam in cams:
        a = 1.0 + S * (2.0 * torch.rand(3, generator=gen) - 1.0)
        b = (S / 4.0) * (2.0 * torch.rand(3, generator=gen) - 1.0)
        img = cam.original_image
        cam.original_image = (img * a.to(img.device)[:, None, None] + b.to(img.device)[:, None, None]).contiguous()
        drawn.append((a, b))
    return drawn
