"""3-nearest-neighbour scale initialiser: the reference's `simple_knn._C.distCUDA2` (scene/gaussian_model.py:39,459).

    distCUDA2(points[P,3]) -> float32[P]   mean squared distance of every point to its 3 nearest other points
    knn3(points[P,3]) -> (int32[P,3], float32[P,3])   their indices and squared distances (GaussianModel.densify_initial)
    NearestIndex(points[P,3]).query(queries[Q,3]) -> (int32[Q], float32[Q])   nearest point of ANOTHER set (metrics.geometry_metrics)
    nearest(queries, points)                          the same in one call

GaussianModel.load_ply uses it for a point cloud without scale_* properties (COLMAP / DUSt3R output): the initial scale
of a point is log(sqrt(max(distCUDA2, 1e-7))) on every axis. The search is exact (csrc/knn.hip; DESIGN.md "3-NN"):
the result equals a brute force over all pairs bit for bit. No CPU path.
"""
import torch

from . import _lib


def _checked(points, what):
    if not isinstance(points, torch.Tensor) or not points.is_cuda:
        raise RuntimeError(f"c3dgs_amd: {what} needs a GPU tensor (there is no CPU path)")
    if points.dim() != 2 or points.size(1) != 3:
        raise RuntimeError(f"{what}: points must have dimensions (num_points, 3), got {tuple(points.shape)}")
    x = points.detach().to(torch.float32).contiguous()
    if x.size(0) and not bool(torch.isfinite(x).all()):       # one host read; the search runs once per loaded scene
        raise RuntimeError(f"{what}: points must be finite")
    return x


def distCUDA2(points):
    """((d0 + d1) + d2) / 3 of the three smallest fp32 squared distances to the other points (FLT_MAX fills the
    missing slots when there are fewer than 3 other points). `points` is a finite [P,3] GPU tensor."""
    x = _checked(points, "distCUDA2")
    P = int(x.size(0))
    out = torch.empty(P, dtype=torch.float32, device=x.device)
    if P == 0:
        return out
    L = _lib.lib()
    ws = torch.empty(int(L.c3dgs_knn_workspace_bytes(P)), dtype=torch.uint8, device=x.device)
    with torch.cuda.device(x.device):
        rc = L.c3dgs_knn_mean_dist2(P, x.data_ptr(), out.data_ptr(), ws.data_ptr(),
                                    _lib.stream(x.device))
    _lib.check(rc)
    return out


def knn3(points):
    """(idx int32[P,3], d2 float32[P,3]): the three smallest (fp32 squared distance, index) pairs over the other points, in
    ascending lexicographic order, so equal distances go to the lowest index. A point with three or more coincident other
    points reports any three of them in ascending index order. Missing slots (P <= 3): idx -1, d2 FLT_MAX. The distances
    are the ones distCUDA2 averages. `points` is a finite [P,3] GPU tensor."""
    x = _checked(points, "knn3")
    P = int(x.size(0))
    idx = torch.empty((P, 3), dtype=torch.int32, device=x.device)
    d2 = torch.empty((P, 3), dtype=torch.float32, device=x.device)
    if P == 0:
        return idx, d2
    L = _lib.lib()
    ws = torch.empty(int(L.c3dgs_knn_workspace_bytes(P)), dtype=torch.uint8, device=x.device)
    with torch.cuda.device(x.device):
        rc = L.c3dgs_knn_neighbours(P, x.data_ptr(), idx.data_ptr(), d2.data_ptr(), ws.data_ptr(),
                                    _lib.stream(x.device))
    _lib.check(rc)
    return idx, d2


# Which order the queries are walked in (csrc/nn_query.hip; the results are the same either way), as measured by
# tools/time_geometry.py on an MI355X (profiles/geometry_time.json). Queries in no particular order: Morton order
# wins (1M x 1M: 1.77 ms against 2.74 ms; 4M x 4M: 4.87 against 11.30). The face-ordered samples of mesh.sample_surface are
# coherent already, and the sort only costs: the caller's order wins (1.56 ms against 1.67 ms; 4.34 against 4.65).
SORT_QUERIES = True                      # query(sort=None)
SORT_FACE_ORDERED_QUERIES = False        # what metrics.mesh_metrics passes for its samples


class NearestIndex:
    """The exact nearest-neighbour index of a finite [P,3] GPU point set: built once (the Morton sort and box tree of the 3-NN
    search), then read by any number of `query` calls.

        idx, d2 = NearestIndex(points).query(queries)      int32 [Q], float32 [Q]

    (d2[i], idx[i]) is the lexicographically smallest (fp32 squared distance dx*dx + dy*dy + dz*dz, index) pair over the points:
    among equal distances the lowest index wins, at distance 0 too. The bits of a brute force. P == 0, or a query with a
    non-finite coordinate: idx -1, d2 FLT_MAX."""

    def __init__(self, points):
        x = _checked(points, "NearestIndex")
        self.points, self.device, self.P = x, x.device, int(x.size(0))
        L = _lib.lib()
        self.index = torch.empty(int(L.c3dgs_nn_index_bytes(self.P)) if self.P else 0, dtype=torch.uint8, device=x.device)
        if self.P:
            with torch.cuda.device(x.device):
                rc = L.c3dgs_nn_build(self.P, x.data_ptr(), self.index.data_ptr(), _lib.stream(x.device))
            _lib.check(rc)

    def query(self, queries, sort=None, leaves=False):
        """`sort`: walk the queries in Morton order (True: the faster for queries in no particular order), in the given order
        (False: the faster for queries that are spatially coherent already, and it needs no workspace), or SORT_QUERIES (None); the
        result does not depend on it. `leaves=True` also returns the int32 [Q] number of leaves scanned per query (a measurement)."""
        if not isinstance(queries, torch.Tensor) or not queries.is_cuda or queries.device != self.device:
            raise RuntimeError(f"NearestIndex.query: queries must be a GPU tensor on the index's device {self.device}")
        if queries.dim() != 2 or queries.size(1) != 3:
            raise RuntimeError(f"NearestIndex.query: queries must have dimensions (num_queries, 3), got {tuple(queries.shape)}")
        q = queries.detach().to(torch.float32).contiguous()
        Q = int(q.size(0))
        idx = torch.empty(Q, dtype=torch.int32, device=q.device)
        d2 = torch.empty(Q, dtype=torch.float32, device=q.device)
        count = torch.empty(Q, dtype=torch.int32, device=q.device) if leaves else None
        if Q:
            L = _lib.lib()
            sort = bool(SORT_QUERIES if sort is None else sort) and self.P > 0
            ws = torch.empty(int(L.c3dgs_nn_query_workspace_bytes(Q)), dtype=torch.uint8, device=q.device) if sort else None
            with torch.cuda.device(q.device):
                rc = L.c3dgs_nn_query(self.P, _lib.ptr(self.index) if self.P else None, Q, q.data_ptr(),
                                      int(sort), idx.data_ptr(), d2.data_ptr(), _lib.ptr(count), _lib.ptr(ws),
                                      _lib.stream(q.device))
            _lib.check(rc)
        return (idx, d2, count) if leaves else (idx, d2)


def nearest(queries, points, sort=None):
    """NearestIndex(points).query(queries): the one-shot form."""
    return NearestIndex(points).query(queries, sort=sort)
