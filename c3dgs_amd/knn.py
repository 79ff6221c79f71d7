"""3-nearest-neighbour scale initialiser: the reference's `simple_knn._C.distCUDA2` (scene/gaussian_model.py:39,459).

    distCUDA2(points[P,3]) -> float32[P]   mean squared distance of every point to its 3 nearest other points
    knn3(points[P,3]) -> (int32[P,3], float32[P,3])   their indices and squared distances (GaussianModel.densify_initial)

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
