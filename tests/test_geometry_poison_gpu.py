"""-m gpu: the scratch contracts of the geometry evaluation (DESIGN.md "Scratch contracts"): the index, the query workspace, the
sampler's workspace and the reduction's partials are handed out poisoned (0x00, 0xFF, 0x7F) between guard bands. Every output is
bit-equal across the three bytes and equal to the restatement, and no guard band is touched."""
import numpy as np
import pytest
import torch

from tests import geometry_ref as G
from tests import poison
from tests import test_geometry_metrics_gpu as tm
from tests import test_mesh_sample_gpu as ts
from tests import test_nearest_gpu as tn

pytestmark = pytest.mark.gpu


def _gpu(a, dtype=torch.float32):
    return torch.as_tensor(np.ascontiguousarray(a), dtype=dtype, device="cuda")


def test_nearest_under_poison(hip):
    from c3dgs_amd import knn
    rng = np.random.default_rng(0)
    x, q = rng.standard_normal((3000, 3)).astype(np.float32), rng.standard_normal((1100, 3)).astype(np.float32)
    q[17] = np.nan
    ri, rd = G.nearest(q, x)
    xs, qs = _gpu(x), _gpu(q)

    def run():
        index = knn.NearestIndex(xs)
        out = {}
        for sort in (False, True):
            idx, d2, leaves = index.query(qs, sort=sort, leaves=True)
            out.update({f"idx{sort}": idx, f"d2{sort}": d2, f"leaves{sort}": leaves})
        return out

    def check(o):
        for sort in (False, True):
            assert (o[f"idx{sort}"] == ri).all() and (o[f"d2{sort}"].view(np.uint32) == rd.view(np.uint32)).all()
        assert (o["leavesTrue"] == o["leavesFalse"]).all()           # the walk of a query does not depend on its neighbours

    poison.assert_independent(run, exact=("idxFalse", "d2False", "leavesFalse", "idxTrue", "d2True", "leavesTrue"), check=check)
    poison.under_every_byte(lambda: tn.test_small_trees_and_ragged_grids(hip, 33, 63))
    poison.under_every_byte(lambda: tn.test_no_reference_points(hip))


def test_mesh_sample_under_poison(hip):
    from c3dgs_amd import mesh
    rng = np.random.default_rng(1)
    v = rng.standard_normal((80, 3)).astype(np.float32)
    f = rng.integers(0, 80, (1000, 3)).astype(np.int32)
    rp, rf, _ = G.sample_surface(v, f, 5.0, 9)
    vs, fs = _gpu(v), _gpu(f, torch.int32)

    def run():
        points, face = mesh.sample_surface(vs, fs, 5.0, 9)
        return {"points": points, "face": face}

    def check(o):
        assert o["points"].shape == rp.shape and (o["points"].view(np.uint32) == rp.view(np.uint32)).all() and (o["face"] == rf).all()

    poison.assert_independent(run, exact=("points", "face"), check=check)
    poison.under_every_byte(lambda: ts.test_one_large_face_among_tiny_ones(hip))
    poison.under_every_byte(lambda: ts.test_bad_meshes_raise(hip))       # a refused count leaves nothing behind for the next


def test_reduction_and_metrics_under_poison(hip):
    from c3dgs_amd import metrics
    rng = np.random.default_rng(2)
    a = _gpu(rng.standard_normal((4000, 3)))
    b = _gpu(rng.standard_normal((3000, 3)))

    def run():
        m = metrics.geometry_metrics(a, b, thresholds=(0.05, 0.2), max_dist=1.0, bounds=((-1, -1, -1), (1, 1, 1)))
        return {k: np.float64(m[k]) for k in ("accuracy", "completeness", "chamfer", "n_accuracy", "n_completeness")} | \
            {f"{k}{t}": np.float64(m[k][t]) for k in ("precision", "recall", "fscore") for t in (0.05, 0.2)}

    names = ("accuracy", "completeness", "chamfer", "n_accuracy", "n_completeness") + \
        tuple(f"{k}{t}" for k in ("precision", "recall", "fscore") for t in (0.05, 0.2))
    poison.assert_independent(run, exact=names)
    poison.under_every_byte(lambda: tm.test_counts_and_sums(hip, 300_001))
    poison.under_every_byte(lambda: tm.test_sphere_against_sphere_end_to_end(hip))
