"""Restatements of the mesh extraction (TEST INFRASTRUCTURE; csrc/mesh.hip, include/c3dgs_hip.h "mesh extraction").

integrate(...): the TSDF fusion in NumPy float32, every operation the kernel's single IEEE operation in the kernel's order, so the
planes are the kernel's bit for bit. extract(...): welded marching tetrahedra (six Kuhn tetrahedra per cell) with the kernel's
vertex order, interpolation and combinatorial winding; the vertices and colours are the kernel's bit for bit, the faces the
kernel's as a set. brute_force(...): the same surface without welding and without the winding rule, one Python loop per
tetrahedron, wound by geometry -- what extract() itself is checked against. Mesh properties (edges, Euler characteristic, signed
volume) and the analytic scenes of the tests are here too."""
import itertools
import math

import numpy as np

F = np.float32
SLOT_DIR = ((1, 0, 0), (0, 1, 0), (0, 0, 1), (1, 1, 0), (1, 0, 1), (0, 1, 1), (1, 1, 1))        # (dx, dy, dz) of the 7 owned edges
AXES = ((1, 0, 0), (0, 1, 0), (0, 0, 1))


def kuhn_paths():
    """the six tetrahedra as paths of four corners (dx, dy, dz), by permutation of the axes in lexicographic order, and the sign of
    det[q1 - q0, q2 - q0, q3 - q0]"""
    out = []
    for perm in itertools.permutations(range(3)):
        q = [np.zeros(3, int)]
        for a in perm:
            q.append(q[-1] + np.array(AXES[a]))
        det = round(float(np.linalg.det(np.array([q[1] - q[0], q[2] - q[0], q[3] - q[0]], float))))
        out.append(([tuple(int(v) for v in c) for c in q], det))
    return out


def axis_points(origin, h, dims):
    """-> (px [Nx], py [Ny], pz [Nz]) float32: origin + float(index) * h"""
    return tuple(F(origin[a]) + np.arange(dims[a]).astype(F) * F(h) for a in range(3))


def integrate(tsdf, weight, color_planes, origin, h, depth, table, sdf_trunc, depth_min=0.2, depth_max=np.inf, color=None):
    """One call of the kernel on copies of the planes ([Nz, Ny, Nx] float32; color_planes [3, Nz, Ny, Nx] or None) -> the new
    (tsdf, weight, color_planes). depth [K, H, W], color [K, 3, H, W] or None, table [K, 16]."""
    tsdf, weight = tsdf.astype(F).copy(), weight.astype(F).copy()
    cp = None if color_planes is None else color_planes.astype(F).copy()
    Nz, Ny, Nx = tsdf.shape
    ax, ay, az = axis_points(origin, h, (Nx, Ny, Nz))
    pz, py, px = np.meshgrid(az, ay, ax, indexing="ij")
    trunc, dmin, dmax, half, one = F(sdf_trunc), F(depth_min), F(depth_max), F(0.5), F(1.0)
    depth = np.asarray(depth, F)
    K, H, W = depth.shape
    with np.errstate(all="ignore"):
        for c in range(K):
            m = np.asarray(table[c], F)
            x = m[0] * px + m[1] * py + m[2] * pz + m[3]
            y = m[4] * px + m[5] * py + m[6] * pz + m[7]
            z = m[8] * px + m[9] * py + m[10] * pz + m[11]
            ok = ~(z < dmin)
            u = m[12] * x / z + half * m[14]
            v = m[13] * y / z + half * m[15]
            ok &= (u >= 0) & (u < m[14]) & (v >= 0) & (v < m[15])
            ui = np.where(ok, u, 0).astype(np.int64)
            vi = np.where(ok, v, 0).astype(np.int64)
            ok &= (ui < W) & (vi < H)
            ui, vi = np.minimum(ui, W - 1), np.minimum(vi, H - 1)
            d = depth[c][vi, ui]
            ok &= (d > 0) & ~(d > dmax)
            sdf = d - z
            ok &= ~(sdf < -trunc)
            s = np.minimum(one, sdf / trunc)
            w1 = weight + one
            tsdf = np.where(ok, (tsdf * weight + s) / w1, tsdf)
            if cp is not None:
                for q in range(3):
                    cp[q] = np.where(ok, (cp[q] * weight + np.asarray(color[c][q], F)[vi, ui]) / w1, cp[q])
            weight = np.where(ok, w1, weight)
    return tsdf.astype(F), weight.astype(F), cp


def _shift(a, d, fill=False):
    """a[k + dz, j + dy, i + dx] for d = (dx, dy, dz) with offsets in {-1, 0, 1}, `fill` outside"""
    Nz, Ny, Nx = a.shape
    p = np.full((Nz + 2, Ny + 2, Nx + 2), fill, a.dtype)
    p[1:-1, 1:-1, 1:-1] = a
    return p[1 + d[2]:1 + d[2] + Nz, 1 + d[1]:1 + d[1] + Ny, 1 + d[0]:1 + d[0] + Nx]


def _classify(tsdf, weight):
    """-> (inside, cell_valid indexed by the cell's low corner [Nz, Ny, Nx], edge [7, Nz, Ny, Nx] bool)"""
    inside = tsdf < 0
    wpos = weight > 0
    cell = np.ones(tsdf.shape, bool)
    for q in itertools.product((0, 1), repeat=3):
        cell &= _shift(wpos, q)
    edge = np.zeros((7,) + tsdf.shape, bool)
    for s, d in enumerate(SLOT_DIR):
        around = np.zeros(tsdf.shape, bool)
        for c in itertools.product(*[((0,) if d[a] else (-1, 0)) for a in range(3)]):
            around |= _shift(cell, c)
        edge[s] = (inside ^ _shift(inside, d)) & around
    return inside, cell, edge


def extract(tsdf, weight, origin, h, color_planes=None):
    """-> (vertices [V, 3] f32, colors [V, 3] f32 | None, faces [F, 3] int32) in the kernel's vertex order"""
    tsdf, weight = np.asarray(tsdf, F), np.asarray(weight, F)
    Nz, Ny, Nx = tsdf.shape
    inside, cell, edge = _classify(tsdf, weight)
    per_point = edge.sum(0).reshape(-1)
    base = np.concatenate([[0], np.cumsum(per_point)]).astype(np.int64)
    V = int(base[-1])
    vid = np.full((7, Nz, Ny, Nx), -1, np.int64)
    below = np.zeros(tsdf.shape, np.int64)
    for s in range(7):
        vid[s] = np.where(edge[s], base[:-1].reshape(tsdf.shape) + below, -1)
        below = below + edge[s]
    ax, ay, az = axis_points(origin, h, (Nx, Ny, Nz))
    vertices = np.zeros((V, 3), F)
    colors = None if color_planes is None else np.zeros((V, 3), F)
    with np.errstate(all="ignore"):
        for s, d in enumerate(SLOT_DIR):
            k, j, i = np.nonzero(edge[s])
            at = vid[s][k, j, i]
            va, vb = tsdf[k, j, i], tsdf[k + d[2], j + d[1], i + d[0]]
            t = va / (va - vb)
            for q, (axis, idx) in enumerate(((ax, i), (ay, j), (az, k))):
                pa, pb = axis[idx], axis[idx + d[q]]
                vertices[at, q] = pa + t * (pb - pa)
            if colors is not None:
                for q in range(3):
                    ca, cb = color_planes[q][k, j, i], color_planes[q][k + d[2], j + d[1], i + d[0]]
                    colors[at, q] = ca + t * (cb - ca)
    faces = []
    slot_of = {d: s for s, d in enumerate(SLOT_DIR)}
    for path, det in kuhn_paths():
        ins = [_shift(inside, c) for c in path]
        code = sum(ins[q].astype(int) << q for q in range(4))
        for m in range(1, 15):
            k, j, i = np.nonzero(cell & (code == m))
            if not k.size:
                continue
            n = bin(m).count("1")
            first = (~m & 15) if n == 3 else m
            L = [q for q in range(4) if (first >> q) & 1] + [q for q in range(4) if not (first >> q) & 1]
            inv = sum(L[a] > L[b] for a in range(4) for b in range(a + 1, 4))
            positive = ((-1) ** inv) * det > 0
            keep = (not positive) if n == 3 else positive

            def vertex(p, q):
                lo, hi = path[min(p, q)], path[max(p, q)]
                s = slot_of[tuple(hi[a] - lo[a] for a in range(3))]
                got = vid[s][k + lo[2], j + lo[1], i + lo[0]]
                assert (got >= 0).all()
                return got

            if n == 2:
                ac, ad, bd, bc = vertex(L[0], L[2]), vertex(L[0], L[3]), vertex(L[1], L[3]), vertex(L[1], L[2])
                tris = [(ac, ad, bd), (ac, bd, bc)]
            else:
                tris = [(vertex(L[0], L[1]), vertex(L[0], L[2]), vertex(L[0], L[3]))]
            for a, b, c in tris:
                faces.append(np.stack([a, b, c] if keep else [a, c, b], 1))
    faces = np.concatenate(faces).astype(np.int32) if faces else np.zeros((0, 3), np.int32)
    return vertices, colors, faces


def brute_force(tsdf, weight, origin, h):
    """Unwelded marching tetrahedra, one tetrahedron at a time: -> list of triangles, each three (edge key, position float64) with
    edge key = (linear index of a, linear index of b), a < b, wound BY GEOMETRY so that the normal points along the gradient of the
    linear interpolant over the tetrahedron (from negative to positive). Degenerate triangles (zero area in float64) come with
    `None` as their winding mark: -> [(keys (3), positions [3, 3], wound bool)]"""
    tsdf, weight = np.asarray(tsdf, F), np.asarray(weight, F)
    Nz, Ny, Nx = tsdf.shape
    ax, ay, az = axis_points(origin, h, (Nx, Ny, Nz))
    lin = lambda c: (c[2] * Ny + c[1]) * Nx + c[0]                      # noqa: E731
    out = []
    for k, j, i in itertools.product(range(Nz - 1), range(Ny - 1), range(Nx - 1)):
        if not all(weight[k + q[2], j + q[1], i + q[0]] > 0 for q in itertools.product((0, 1), repeat=3)):
            continue
        for path, _ in kuhn_paths():
            corners = [(i + c[0], j + c[1], k + c[2]) for c in path]
            val = [tsdf[c[2], c[1], c[0]] for c in corners]
            pos = [np.array([ax[c[0]], ay[c[1]], az[c[2]]], np.float64) for c in corners]
            ins = [v < 0 for v in val]
            n = sum(ins)
            if n in (0, 4):
                continue

            def cut(p, q):
                a, b = (p, q) if lin(corners[p]) < lin(corners[q]) else (q, p)
                with np.errstate(all="ignore"):
                    t = val[a] / (val[a] - val[b])
                    x = np.array([F(pos[a][c]) + t * (F(pos[b][c]) - F(pos[a][c])) for c in range(3)], F)
                return (lin(corners[a]), lin(corners[b])), x.astype(np.float64)

            I = [q for q in range(4) if ins[q]]
            O = [q for q in range(4) if not ins[q]]
            if n == 1:
                polys = [[cut(I[0], o) for o in O]]
            elif n == 3:
                polys = [[cut(O[0], q) for q in I]]
            else:
                quad = [cut(I[0], O[0]), cut(I[0], O[1]), cut(I[1], O[1]), cut(I[1], O[0])]
                polys = [[quad[0], quad[1], quad[2]], [quad[0], quad[2], quad[3]]]
            # gradient of the linear interpolant: solve [p1 - p0; p2 - p0; p3 - p0] g = [v1 - v0; ...]
            A = np.array([pos[q] - pos[0] for q in (1, 2, 3)])
            g = np.linalg.solve(A, np.array([float(val[q]) - float(val[0]) for q in (1, 2, 3)]))
            for tri in polys:
                P = np.array([t[1] for t in tri])
                nrm = np.cross(P[1] - P[0], P[2] - P[0])
                if np.linalg.norm(nrm) < 1e-14:
                    out.append(([t[0] for t in tri], P, None))
                    continue
                if nrm @ g < 0:
                    tri = [tri[0], tri[2], tri[1]]
                    P = P[[0, 2, 1]]
                out.append(([t[0] for t in tri], P, True))
    return out


def edge_keys(tsdf, weight):
    """the (a, b) linear-index key of every vertex of extract(), in its order"""
    tsdf = np.asarray(tsdf, F)
    Nz, Ny, Nx = tsdf.shape
    _, _, edge = _classify(tsdf, np.asarray(weight, F))
    keys = []
    for s, d in enumerate(SLOT_DIR):
        k, j, i = np.nonzero(edge[s])
        a = (k * Ny + j) * Nx + i
        keys.append(np.stack([a, a + (d[2] * Ny + d[1]) * Nx + d[0], np.full_like(a, s)], 1))
    keys = np.concatenate(keys)
    return keys[np.lexsort((keys[:, 2], keys[:, 0]))][:, :2]


# ---- mesh properties
def canonical_faces(faces):
    """each face rotated to its smallest index first, the rows sorted"""
    f = np.asarray(faces, np.int64).reshape(-1, 3)
    if not f.size:
        return f
    r = np.argmin(f, 1)
    f = np.stack([f[np.arange(len(f)), (r + q) % 3] for q in range(3)], 1)
    return f[np.lexsort((f[:, 2], f[:, 1], f[:, 0]))]


def closed_oriented(faces):
    """every directed edge occurs once and its opposite occurs once"""
    f = np.asarray(faces, np.int64)
    e = np.concatenate([f[:, [0, 1]], f[:, [1, 2]], f[:, [2, 0]]])
    if (e[:, 0] == e[:, 1]).any():
        return False
    fwd = set(map(tuple, e))
    return len(fwd) == len(e) and all((b, a) in fwd for a, b in fwd)


def euler(n_vertices, faces):
    f = np.asarray(faces, np.int64)
    e = np.sort(np.concatenate([f[:, [0, 1]], f[:, [1, 2]], f[:, [2, 0]]]), 1)
    return n_vertices - len(np.unique(e, axis=0)) + len(f)


def signed_volume(vertices, faces):
    v = np.asarray(vertices, np.float64)[np.asarray(faces, np.int64)]
    return float(np.einsum("ij,ij->i", v[:, 0], np.cross(v[:, 1], v[:, 2])).sum() / 6.0)


def triangle_areas(vertices, faces):
    v = np.asarray(vertices, np.float64)[np.asarray(faces, np.int64)]
    return 0.5 * np.linalg.norm(np.cross(v[:, 1] - v[:, 0], v[:, 2] - v[:, 0]), axis=1)


# ---- scenes
def sphere_lattice(n, radius=0.3, centre=(0.5, 0.5, 0.5)):
    """the sphere SDF on an n^3 lattice over the unit box -> (tsdf, weight, origin, h)"""
    h = F(1.0 / (n - 1))
    ax, ay, az = axis_points((0, 0, 0), h, (n, n, n))
    z, y, x = np.meshgrid(az.astype(np.float64), ay.astype(np.float64), ax.astype(np.float64), indexing="ij")
    sdf = np.sqrt((x - centre[0]) ** 2 + (y - centre[1]) ** 2 + (z - centre[2]) ** 2) - radius
    return sdf.astype(F), np.ones((n, n, n), F), (0.0, 0.0, 0.0), float(h)


def random_lattice(dims=(7, 6, 5), seed=5, zero_weight=0.2):
    """values in [-1, 1] with exact 0.0 and -0.0 entries and `zero_weight` of the points without weight, random colours
    -> (tsdf, weight, color_planes, origin, h)"""
    rng = np.random.default_rng(seed)
    Nx, Ny, Nz = dims
    t = rng.uniform(-1, 1, (Nz, Ny, Nx)).astype(F)
    flat = t.reshape(-1)
    pick = rng.permutation(flat.size)
    flat[pick[:flat.size // 12]] = F(0.0)
    flat[pick[flat.size // 12:flat.size // 6]] = F(-0.0)
    w = (rng.uniform(0, 1, t.shape) >= zero_weight).astype(F) * rng.integers(1, 5, t.shape).astype(F)
    c = rng.uniform(0, 1, (3,) + t.shape).astype(F)
    return t, w, c, (-0.3, 0.1, 0.25), 0.07


def look_at_row(pos, target, focal, W, H, up=(0.0, 1.0, 0.0)):
    """one camera-table row (world -> camera rows, fx, fy, W, H): at `pos`, looking at `target`"""
    pos, target = np.asarray(pos, np.float64), np.asarray(target, np.float64)
    fwd = (target - pos) / np.linalg.norm(target - pos)
    upv = np.asarray(up, np.float64)
    if abs(fwd @ upv) > 0.99:
        upv = np.array([0.0, 0.0, 1.0])
    right = np.cross(upv, fwd)
    right /= np.linalg.norm(right)
    down = np.cross(fwd, right)
    R = np.stack([right, down, fwd])
    row = np.zeros(16, F)
    row[:12] = np.concatenate([R, (-R @ pos)[:, None]], 1).reshape(-1)
    row[12] = row[13] = focal
    row[14], row[15] = W, H
    return row


def sphere_depth(row, W, H, centre=(0.5, 0.5, 0.5), radius=0.3):
    """ray-sphere view-space depth at the pixel centres of camera `row` (0 off the sphere) and a smooth colour -> ([H, W], [3, H, W])"""
    m = row.astype(np.float64)
    R, t = m[:12].reshape(3, 4)[:, :3], m[:12].reshape(3, 4)[:, 3]
    c = R @ np.asarray(centre, np.float64) + t                    # the centre in view space
    v, u = np.meshgrid(np.arange(H) + 0.5, np.arange(W) + 0.5, indexing="ij")
    d = np.stack([(u - 0.5 * m[14]) / m[12], (v - 0.5 * m[15]) / m[13], np.ones_like(u)], -1)     # z = 1 rays
    a = (d * d).sum(-1)
    b = d @ c
    disc = b * b - a * (c @ c - radius * radius)
    s = (b - np.sqrt(np.maximum(disc, 0))) / a
    depth = np.where((disc > 0) & (s > 0), s, 0.0).astype(F)
    col = np.stack([0.5 + 0.5 * np.sin(0.1 * u + q) * np.cos(0.07 * v - q) for q in range(3)]).astype(F)
    return depth, col


def six_cameras(W=64, H=48, focal=60.0, dist=1.6, centre=(0.5, 0.5, 0.5)):
    """six cameras looking at `centre` from the six axis directions -> table [6, 16]"""
    c = np.asarray(centre, np.float64)
    rows = [look_at_row(c + dist * np.array(d, np.float64), c, focal, W, H)
            for d in ((1, 0, 0), (-1, 0, 0), (0, 1, 0), (0, -1, 0), (0, 0, 1), (0, 0, -1))]
    return np.stack(rows)


def perturbed(table, K, seed=9, amount=0.03):
    """K rows: copies of the table's rows in turn, each with its translation moved by up to `amount`"""
    rng = np.random.default_rng(seed)
    out = np.stack([table[q % len(table)] for q in range(K)]).copy()
    out[:, [3, 7, 11]] += rng.uniform(-amount, amount, (K, 3)).astype(F)
    return out


def radial_error_bound(h, radius):
    """linear interpolation of the sphere SDF over an edge of length at most sqrt(3) h"""
    return 3 * h * h / (8 * (radius - math.sqrt(3) * h)) + 1e-5
