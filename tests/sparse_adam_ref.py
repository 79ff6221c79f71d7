"""Reference restatement of sparse Adam (csrc/sparse_adam.hip) -- TEST INFRASTRUCTURE. numpy.

select: the rows a mask lists, ascending (np.flatnonzero): bool / uint8 non-zero, int32 > 0.
step:   the listed rows go through tests/adam_ref.py (step32 for bits, moments64 / param64 / excess64 for the float64 bars);
        every other row is copied, bit for bit. tests/test_sparse_adam_ref_cpu.py pins it to torch.optim.Adam in float64 run on
        the gathered rows."""
import numpy as np

from tests import adam_ref as R


def listed(mask):
    """-> bool [P]: the rows `mask` lists."""
    mask = np.asarray(mask)
    if mask.dtype == np.int32:
        return mask > 0
    if mask.dtype in (np.bool_, np.uint8):
        return mask != 0
    raise TypeError(f"mask dtype {mask.dtype}")


def select(mask):
    """-> (rows int64 [count], count)"""
    rows = np.flatnonzero(listed(mask))
    return rows, int(rows.size)


def step32(p, g, m, v, mask, s):
    """p, g, m, v: float32 [P, ...]. -> (p', m', v'): adam_ref.step32 on the listed rows, the other rows' bits as they were.
    The gradient of an unlisted row is never read (a NaN there is invisible)."""
    rows, _ = select(mask)
    out = [np.array(a, np.float32, copy=True) for a in (p, m, v)]
    if rows.size:
        p2, m2, v2 = R.step32(p[rows], g[rows], m[rows], v[rows], s)
        out[0][rows], out[1][rows], out[2][rows] = p2, m2, v2
    return tuple(out)


def step64(p, g, m, v, mask, s):
    """Float64, from the exact formula chained (moments64 then param64 on ITS moments), for pinning to torch in float64:
    -> (p', m', v') float64, unlisted rows copied."""
    rows, _ = select(mask)
    out = [np.array(a, np.float64, copy=True) for a in (p, m, v)]
    if rows.size:
        m2, v2 = R.moments64(g[rows], m[rows], v[rows], s)
        p2, _ = R.param64(p[rows], m2, v2, s)
        out[0][rows], out[1][rows], out[2][rows] = p2, m2, v2
    return tuple(out)


def excess64(p, g, m, v, p_new, m_new, v_new, mask, s):
    """adam_ref.excess64 over the listed rows -> (em, ev, ep), (0, 0, 0) when nothing is listed."""
    rows, n = select(mask)
    if n == 0:
        return 0.0, 0.0, 0.0
    return R.excess64(p[rows], g[rows], m[rows], v[rows], p_new[rows], m_new[rows], v_new[rows], s)
