"""numpy restatement of the 3-NN contract of c3dgs_amd.knn.distCUDA2 (include/c3dgs_hip.h, csrc/knn.hip):

    d(i,j) = dx*dx + dy*dy + dz*dz in fp32, left to right, dx = x[j] - x[i];   j != i by index
    out[i] = ((d0 + d1) + d2) / 3 over the three smallest d(i,j); for P <= 3 the missing slots are FLT_MAX

Brute force over all pairs, in row chunks so that P = 30000 stays within a few hundred MB."""
import numpy as np

FLT_MAX = np.float32(np.finfo(np.float32).max)


def combine(d3):
    """[n,3] ascending fp32 triples -> ((d0 + d1) + d2) / 3 in fp32."""
    d3 = np.asarray(d3, np.float32)
    with np.errstate(over="ignore"):
        return ((d3[:, 0] + d3[:, 1]) + d3[:, 2]) / np.float32(3.0)


def smallest3(xyz, rows=None, chunk=256):
    """Ascending three smallest d(i,j) over j != i for each i in `rows` (default: all), FLT_MAX-padded."""
    x = np.ascontiguousarray(xyz, dtype=np.float32)
    P = x.shape[0]
    rows = np.arange(P) if rows is None else np.asarray(rows)
    out = np.empty((rows.size, 3), np.float32)
    k = min(3, P - 1)
    for a in range(0, rows.size, chunk):
        r = rows[a:a + chunk]
        q = x[r]
        with np.errstate(over="ignore", invalid="ignore"):
            dx = x[None, :, 0] - q[:, None, 0]
            d = dx * dx
            dy = x[None, :, 1] - q[:, None, 1]
            d = d + dy * dy
            dz = x[None, :, 2] - q[:, None, 2]
            d = d + dz * dz
        del dx, dy, dz
        d[np.arange(r.size), r] = np.inf                  # j != i by index
        best = np.full((r.size, 3), FLT_MAX, np.float32)
        if k > 0:
            best[:, :k] = np.sort(np.partition(d, k - 1, axis=1)[:, :k], axis=1)
        out[a:a + chunk] = best
    return out


def mean_dist2(xyz, chunk=256):
    return combine(smallest3(xyz, chunk=chunk))


def mean_dist2_loop(xyz):
    """The contract as a plain Python loop (checks the vectorised version for small P)."""
    x = np.asarray(xyz, np.float32)
    P = x.shape[0]
    out = np.empty(P, np.float32)
    for i in range(P):
        ds = []
        for j in range(P):
            if j == i:
                continue
            dx, dy, dz = x[j, 0] - x[i, 0], x[j, 1] - x[i, 1], x[j, 2] - x[i, 2]
            ds.append(np.float32(np.float32(dx * dx + dy * dy) + dz * dz))
        ds = sorted(ds)[:3] + [FLT_MAX] * max(0, 3 - len(ds))
        out[i] = combine(np.array([ds], np.float32))[0]
    return out
