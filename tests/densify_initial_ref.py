"""numpy restatement of GaussianModel.densify_initial as c3dgs_amd computes it (include/c3dgs_hip.h, csrc/ray_fill.hip,
DESIGN.md "Initial densification"), and of the neighbour table it starts from (c3dgs_amd.knn.knn3).

    knn3_brute       the three smallest (d2, index) pairs over j != i, lexicographic; d2 as tests/knn_ref.py forms it
    average_step     dist_thr_coeff * (prod(max - min) / n) ** (1/3): the product in fp32, the rest in Python doubles
    plan             the closed form: per slot nb, r2 = second-largest rel (with multiplicity), point i gets
                     c = max(0, floor(min(rel[i], r2)) - 1) rows at levels 1..c; rows ordered by slot, level, source index
    positions        x[i] * (1 - a) + a * x[j], a = float32(level) / rel, every operation rounded to fp32 on its own
    level_loop       the reference's double loop (scene/gaussian_model.py:1369-1387) transcribed literally, on a neighbour
                     table whose column 0 is the point itself
"""
import numpy as np

FLT_MAX = np.float32(np.finfo(np.float32).max)
INT32_MAX = 2 ** 31 - 1


def knn3_brute(xyz, chunk=256):
    """(idx int32[P,3], d2 float32[P,3]); missing slots (P <= 3) hold -1 and FLT_MAX."""
    x = np.ascontiguousarray(xyz, dtype=np.float32)
    P = x.shape[0]
    idx = np.full((P, 3), -1, np.int32)
    d2 = np.full((P, 3), FLT_MAX, np.float32)
    k = min(3, P - 1)
    for a in range(0, P, chunk):
        q = x[a:a + chunk]
        with np.errstate(over="ignore", invalid="ignore"):
            dx = x[None, :, 0] - q[:, None, 0]
            d = dx * dx
            dy = x[None, :, 1] - q[:, None, 1]
            d = d + dy * dy
            dz = x[None, :, 2] - q[:, None, 2]
            d = d + dz * dz
        rows = np.arange(q.shape[0])
        d[rows, a + rows] = np.inf                                    # j != i by index
        if k > 0:
            order = np.argsort(d, axis=1, kind="stable")[:, :k]       # stable: equal distances in ascending index
            idx[a:a + chunk, :k] = order
            d2[a:a + chunk, :k] = np.take_along_axis(d, order, axis=1)
    return idx, d2


def average_step(xyz, dist_thr_coeff):
    x = np.asarray(xyz, np.float32)
    e = x.max(axis=0) - x.min(axis=0)
    with np.errstate(over="ignore"):
        prod = np.float32(np.float32(e[0] * e[1]) * e[2])
    return dist_thr_coeff * (float(prod) / x.shape[0]) ** (1.0 / 3)


def relative_distance(d2, step):
    with np.errstate(over="ignore"):
        return np.sqrt(np.asarray(d2, np.float32)) / np.float32(step)


def counts(d2, step):
    """int64[P,3]: rows every point receives per slot, saturated at INT32_MAX like the kernel's."""
    rel = relative_distance(d2, step)
    P = rel.shape[0]
    c = np.zeros((P, 3), np.int64)
    for nb in range(3):
        r = rel[:, nb]
        r2 = np.sort(r)[-2] if P >= 2 else np.float32(-1)
        m = np.minimum(r, r2).astype(np.float64)
        c[:, nb] = np.where(m >= 2.0, np.minimum(np.floor(np.minimum(m, 2.0 ** 31)) - 1, INT32_MAX), 0).astype(np.int64)
    return c


def plan(d2, step):
    """(src int32[n], slot uint8[n], level int32[n], (n0, n1, n2)) of the new rows."""
    c = counts(d2, step)
    src, slot, level, totals = [], [], [], []
    for nb in range(3):
        n = 0
        for L in range(1, int(c[:, nb].max(initial=0)) + 1):
            rows = np.nonzero(c[:, nb] >= L)[0]
            src.append(rows)
            slot.append(np.full(rows.size, nb))
            level.append(np.full(rows.size, L))
            n += rows.size
        totals.append(n)
    cat = lambda parts, dt: np.concatenate(parts).astype(dt) if parts else np.zeros(0, dt)     # noqa: E731
    return cat(src, np.int32), cat(slot, np.uint8), cat(level, np.int32), tuple(totals)


def positions(xyz, idx, d2, step, src, slot, level):
    x = np.asarray(xyz, np.float32)
    rel = relative_distance(d2, step)[src, slot]
    a = (level.astype(np.float32) / rel).astype(np.float32)
    one_minus = (np.float32(1.0) - a).astype(np.float32)
    j = np.asarray(idx)[src, slot]
    return (x[src] * one_minus[:, None] + a[:, None] * x[j]).astype(np.float32)


def level_loop(xyz, indices, step):
    """The reference's loop on `indices` int[P,4] (column 0 the point itself). -> (src, slot, level, new positions) in the
    order its densify_and_clone calls append them."""
    data = np.asarray(xyz, np.float32)
    n = data.shape[0]
    idx = np.arange(n)
    src, slot_out, level, pos = [], [], [], []
    for nb in range(1, 4):
        delta_pt = data[indices[:, nb]] - data
        relative = np.sqrt((delta_pt ** 2.0).sum(axis=1)) / np.float32(step)
        assert relative.dtype == np.float32
        for dist in range(1, int(relative.max())):
            slot = relative >= dist + 1
            if slot.sum() > 1:
                alpha = (dist / relative[slot]).astype(np.float32)
                selected = indices[slot, nb]
                rows = idx[slot]
                coords = [data[rows, i] * (np.float32(1.0) - alpha) + alpha * data[selected, i] for i in range(3)]
                src.append(rows)
                slot_out.append(np.full(rows.size, nb - 1))
                level.append(np.full(rows.size, dist))
                pos.append(np.stack(coords, axis=1).astype(np.float32))
    if not src:
        return np.zeros(0, np.int32), np.zeros(0, np.uint8), np.zeros(0, np.int32), np.zeros((0, 3), np.float32)
    return (np.concatenate(src).astype(np.int32), np.concatenate(slot_out).astype(np.uint8),
            np.concatenate(level).astype(np.int32), np.concatenate(pos))
