"""-m gpu: the 3-NN scale initialiser (csrc/knn.hip, c3dgs_amd.knn.distCUDA2) is exact -- the same bits as the brute
force of tests/knn_ref.py -- on clouds built to stress the search and its pruning, fast on degenerate clouds, and
reachable under the reference's module name."""
import time

import numpy as np
import pytest
import torch

from tests import knn_ref, synth

pytestmark = pytest.mark.gpu


def _cloud(kind, P, seed=0):
    g = np.random.default_rng(seed)
    if kind == "gaussian":                                     # anisotropic
        x = g.normal(size=(P, 3)) * [3.0, 0.7, 0.05]
    elif kind == "uniform":
        x = g.uniform(-1, 1, size=(P, 3))
    elif kind == "planar":
        x = g.uniform(-1, 1, size=(P, 3))
        x[:, 2] = 0.25
    elif kind == "collinear":
        x = np.outer(g.uniform(-5, 5, size=P), [0.3, -0.5, 0.8])
    elif kind == "lattice":                                    # integer grid: massive distance ties
        side = int(np.ceil(P ** (1 / 3))) + 1
        x = np.stack(np.unravel_index(g.permutation(side ** 3)[:P], (side, side, side)), 1).astype(np.float64)
    elif kind == "duplicates":                                 # 10 % copies of other points
        x = g.normal(size=(P, 3))
        k = P // 10
        x[g.choice(P, k, replace=False)] = x[g.choice(P, k)]
    elif kind == "outliers":
        x = g.normal(size=(P, 3))
        x[g.choice(P, max(1, P // 200), replace=False)] *= 1e6
    elif kind == "offset":                                     # fine spacing far from the origin: rounding matters
        x = 1e4 + 1e-3 * g.normal(size=(P, 3))
    elif kind == "mixed":
        x = g.normal(size=(P, 3)) * g.choice([-1.0, 1.0], size=(P, 3)) * np.exp(g.normal(size=(P, 3)))
    else:
        raise ValueError(kind)
    return np.ascontiguousarray(x, dtype=np.float32)


def _bits(t):
    return t.detach().cpu().numpy().view(np.uint32)


def _check(hip, x):
    got = hip.knn.distCUDA2(torch.from_numpy(x).cuda())
    ref = knn_ref.mean_dist2(x)
    np.testing.assert_array_equal(_bits(got), ref.view(np.uint32))


KINDS = ["gaussian", "uniform", "planar", "collinear", "lattice", "duplicates", "outliers", "offset", "mixed"]


@pytest.mark.parametrize("kind", KINDS)
def test_exact_4097(hip, kind):
    _check(hip, _cloud(kind, 4097, seed=KINDS.index(kind)))


@pytest.mark.parametrize("kind", ["gaussian", "lattice"])
@pytest.mark.parametrize("P", [1, 2, 3, 4, 5, 63, 64, 65, 1000])
def test_exact_small(hip, kind, P):
    _check(hip, _cloud(kind, P, seed=P))


@pytest.mark.parametrize("kind", ["gaussian", "lattice", "duplicates"])
def test_exact_30000(hip, kind):
    _check(hip, _cloud(kind, 30000, seed=11))


def _torch_smallest3(xg, rows, chunk=24):
    """Brute force on the device with explicit elementwise fp32 ops (no cdist, no fused multiply-add)."""
    out = []
    for a in range(0, rows.numel(), chunk):
        r = rows[a:a + chunk]
        q = xg[r]
        dx = xg[None, :, 0] - q[:, None, 0]
        d = dx * dx
        del dx
        dy = xg[None, :, 1] - q[:, None, 1]
        d = d + dy * dy
        del dy
        dz = xg[None, :, 2] - q[:, None, 2]
        d = d + dz * dz
        del dz
        d[torch.arange(r.numel(), device=xg.device), r] = float("inf")
        out.append(torch.topk(d, 3, dim=1, largest=False, sorted=True).values)
    return torch.cat(out).cpu().numpy()


@pytest.mark.parametrize("P", [1_000_000, 3_000_000])
def test_exact_large_synth_sampled(hip, P):
    g = np.random.default_rng(P)
    x = synth.scene(P)["means3D"].numpy().copy()
    dups = g.choice(P, 2048, replace=False)
    src = g.choice(P, 2048)
    x[dups] = x[src]
    outl = g.choice(P, 64, replace=False)
    x[outl] *= 1e5
    rows = np.unique(np.concatenate([g.choice(P, 4096, replace=False), dups, src, outl]))
    xg = torch.from_numpy(x).cuda()
    got = _bits(hip.knn.distCUDA2(xg))[rows]
    d3 = _torch_smallest3(xg, torch.from_numpy(rows).cuda())
    np.testing.assert_array_equal(got, knn_ref.combine(d3).view(np.uint32))


def test_repeatable_and_permutation_invariant(hip):
    x = torch.from_numpy(_cloud("duplicates", 200_000, seed=5)).cuda()
    a = hip.knn.distCUDA2(x)
    b = hip.knn.distCUDA2(x)
    assert torch.equal(a.view(torch.int32), b.view(torch.int32))
    perm = torch.randperm(x.shape[0], generator=torch.Generator().manual_seed(1)).cuda()
    c = torch.empty_like(a)
    c[perm] = hip.knn.distCUDA2(x[perm])
    assert torch.equal(a.view(torch.int32), c.view(torch.int32))


def test_identical_cloud_is_fast(hip):
    x = torch.full((1_000_000, 3), 0.375, device="cuda")
    hip.knn.distCUDA2(x[:1000])
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    out = hip.knn.distCUDA2(x)
    torch.cuda.synchronize()
    dt = time.perf_counter() - t0
    assert torch.count_nonzero(out).item() == 0
    assert dt < 5.0, dt


def test_errors(hip):
    with pytest.raises(RuntimeError, match="GPU"):
        hip.knn.distCUDA2(torch.zeros(10, 3))
    for shape in [(10,), (10, 2), (10, 4), (2, 3, 3)]:
        with pytest.raises(RuntimeError, match="dimensions"):
            hip.knn.distCUDA2(torch.zeros(shape, device="cuda"))
    bad = torch.zeros(10, 3, device="cuda")
    bad[4, 1] = float("nan")
    with pytest.raises(RuntimeError, match="finite"):
        hip.knn.distCUDA2(bad)
    bad[4, 1] = float("inf")
    with pytest.raises(RuntimeError, match="finite"):
        hip.knn.distCUDA2(bad)
    assert hip.knn.distCUDA2(torch.zeros(0, 3, device="cuda")).shape == (0,)


def test_reference_module_name(hip):
    hip.install_as_reference_modules()
    from simple_knn._C import distCUDA2
    x = torch.from_numpy(_cloud("gaussian", 5000, seed=3)).cuda()
    assert torch.equal(distCUDA2(x).view(torch.int32), hip.knn.distCUDA2(x).view(torch.int32))
    import weighted_distance._C  # noqa: F401 -- the earlier registrations stay in place
    import diff_gaussian_rasterization_no_camera  # noqa: F401
