"""Numpy restatement of the contract of c3dgs_image_from_u8 (include/c3dgs_hip.h, csrc/image_io.hip): decoded 8-bit texels
[Hs][Ws][C] -> planar [3][Hd][Wd] in [0, 1]. Test infrastructure; it is our own statement of OpenCV's documented INTER_LINEAR,
not a recording of cv2.resize.

    image_from_u8(src, Hd, Wd, flip=0, bg=None, dtype=np.float32)

dtype=float32: every operation of the contract in its stated order, each rounded to fp32 on its own (numpy never fuses a
multiply and an add); the kernel must match it bit for bit. dtype=float64: the same taps and weights (the weights are fp32
values in both forms) evaluated in fp64; the fp32 form lies within BOUND of it.
"""
import numpy as np

# values and weights are in [0, 1]; a level is two products and one sum: 3u from the horizontal pass, carried through a convex
# combination, plus 3u from the vertical pass = 6u, u = 2^-24; 8u leaves the margin of one more level
BOUND = 8 * 2.0 ** -24

# (Hs, Ws) -> (Hd, Wd): the smallest shapes that reach every path of the kernel
SHAPES = (((1, 1), (1, 1)), ((1, 1), (5, 7)), ((1, 9), (1, 4)), ((9, 1), (20, 1)), ((7, 5), (7, 5)), ((23, 37), (9, 16)),
          ((23, 37), (31, 53)), ((143, 611), (70, 300)), ((143, 611), (71, 301)), ((64, 64), (16, 16)))


def taps(dst, src):
    """-> (s0 int64[dst], s1 int64[dst], f float32[dst]) of one axis."""
    scale = 1.0 / (float(dst) / float(src))                              # python floats are fp64
    f = ((np.arange(dst, dtype=np.float64) + 0.5) * scale - 0.5).astype(np.float32)
    fl = np.floor(f)
    s = fl.astype(np.int64)
    f = f - fl
    low, high = s < 0, s >= src - 1
    s = np.where(low, 0, np.where(high, src - 1, s))
    f = np.where(low | high, np.float32(0), f).astype(np.float32)
    return s, np.minimum(s + 1, src - 1), f


def texels(src, bg=None, dtype=np.float32):
    """[Hs][Ws][C] uint8 -> [Hs][Ws][3]: u / 255, alpha, background."""
    src = np.asarray(src)
    if src.dtype != np.uint8 or src.ndim != 3 or src.shape[2] not in (3, 4):
        raise ValueError("src must be uint8 [H][W][3|4]")
    if bg is not None and src.shape[2] == 3:
        raise ValueError("a background needs an alpha channel")
    v = src[:, :, :3].astype(dtype) / dtype(255.0)
    if src.shape[2] == 4:
        a = src[:, :, 3:4].astype(dtype) / dtype(255.0)
        v = v * a
        if bg is not None:
            v = v + np.asarray(bg, dtype=np.float32).astype(dtype) * (dtype(1.0) - a)
    return v


def image_from_u8(src, Hd, Wd, flip=0, bg=None, dtype=np.float32):
    v = texels(src, bg, dtype)
    if flip:
        v = v[::-1, ::-1]
    Hs, Ws = v.shape[:2]
    y0, y1, fy = taps(Hd, Hs)
    x0, x1, fx = taps(Wd, Ws)
    fx, fy = fx.astype(dtype)[None, :, None], fy.astype(dtype)[:, None, None]
    one = dtype(1.0)
    h0 = v[y0][:, x0] * (one - fx) + v[y0][:, x1] * fx
    h1 = v[y1][:, x0] * (one - fx) + v[y1][:, x1] * fx
    o = h0 * (one - fy) + h1 * fy
    assert o.dtype == dtype
    return np.ascontiguousarray(np.clip(o, dtype(0), dtype(1)).transpose(2, 0, 1))


def unit_by_fma(u):
    """The kernel's division-free fl(u / 255) in exact rational arithmetic: q = fl(u r), e = u - 255 q (exact in fp32),
    fl(q + e r), r = fl(1 / 255). -> fractions.Fraction"""
    from fractions import Fraction as F

    def rn(x):                                                           # round to nearest even fp32, exactly
        if x == 0:
            return F(0)
        e = 0
        while F(2) ** e > abs(x):
            e -= 1
        while F(2) ** (e + 1) <= abs(x):
            e += 1
        q = abs(x) / F(2) ** (e - 23)
        n, rem = divmod(q.numerator, q.denominator)
        rem = F(rem, q.denominator)
        if rem > F(1, 2) or (rem == F(1, 2) and n % 2):
            n += 1
        return (1 if x > 0 else -1) * n * F(2) ** (e - 23)

    r = rn(F(1, 255))
    q = rn(u * r)
    e = F(u) - q * 255
    assert rn(e) == e
    return rn(q + e * r), rn(F(u, 255))
