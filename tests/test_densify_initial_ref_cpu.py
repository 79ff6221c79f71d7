"""CPU: the numpy restatement of densify_initial (tests/densify_initial_ref.py) equals the reference's own output bit for bit
on every case of tests/golden/densify_initial.npz (row order, source rows, new positions, the step), and equals a literal
transcription of the reference's level loop on random clouds. What the GPU tests compare the kernels with is therefore the
reference's method, not a reading of it."""
import os

import numpy as np
import pytest

from tests import densify_initial_ref as ref

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "densify_initial.npz")


@pytest.fixture(scope="module")
def golden():
    return np.load(GOLDEN)


def case_names():
    return [str(c) for c in np.load(GOLDEN)["cases"]]


@pytest.mark.parametrize("name", case_names())
def test_closed_form_equals_the_reference(golden, name):
    g = {k.split("/", 1)[1]: golden[k] for k in golden.files if k.startswith(name + "/")}
    x = g["xyz"]
    step = ref.average_step(x, float(g["dist_thr_coeff"][0]))
    assert step == float(g["step"][0])
    idx, d2 = ref.knn3_brute(x)
    src, slot, level, totals = ref.plan(d2, step)
    assert np.array_equal(src, g["src"]) and np.array_equal(slot, g["slot"]) and np.array_equal(level, g["level"])
    assert list(totals) == list(g["totals"])
    pos = ref.positions(x, idx, d2, step, src, slot, level)
    assert pos.dtype == np.float32 and np.array_equal(pos.view(np.uint32), g["new_xyz"].view(np.uint32))
    n = int(g["P"][0]) + len(src)
    assert tuple(g["xyz_gradient_accum_shape"]) == (n, 1) and tuple(g["denom_shape"]) == (n, 1)
    assert tuple(g["max_radii2D_shape"]) == (n,)


def test_golden_covers_what_it_is_for(golden):
    names = case_names()
    get = lambda n, k: golden[f"{n}/{k}"]                                               # noqa: E731
    assert {float(get(n, "dist_thr_coeff")[0]) for n in names} >= {0.3, 1.0}
    assert any(get(n, "quantization")[0] and get(n, "use_factor_scaling")[0] and len(get(n, "src")) for n in names)
    assert any(not get(n, "quantization")[0] and not get(n, "use_factor_scaling")[0] and len(get(n, "src")) for n in names)
    assert any(len(get(n, "src")) == 0 for n in names)
    assert any(get(n, "levels_removed")[0] > 0 and len(get(n, "src")) for n in names)
    assert all(200 <= int(get(n, "P")[0]) <= 300 for n in names)
    assert len(golden["versions"]) == 3


def _cloud(seed, P, outliers):
    rng = np.random.default_rng(seed)
    x = rng.uniform(-1, 1, (P, 3)).astype(np.float32)
    x[: P // 2] *= np.float32(0.25)                       # a dense core, so that the halo's gaps span several steps
    for k in range(outliers):
        x[P - 1 - k] = rng.uniform(-1, 1, 3) * 0.3 + np.array([3.0 + 4 * k, -2.0 * k, 1.0 + k])
    return x


@pytest.mark.parametrize("seed,P,outliers,coeff", [(1, 64, 0, 0.25), (2, 150, 1, 0.5), (3, 300, 3, 0.3), (4, 120, 2, 1.0),
                                                   (5, 200, 0, 0.3), (6, 90, 1, 0.25)])
def test_closed_form_equals_the_level_loop(seed, P, outliers, coeff):
    x = _cloud(seed, P, outliers)
    step = ref.average_step(x, coeff)
    idx, d2 = ref.knn3_brute(x)
    table = np.concatenate([np.arange(P)[:, None], idx], axis=1)
    want = ref.level_loop(x, table, step)
    src, slot, level, totals = ref.plan(d2, step)
    assert len(want[0]) > 0
    assert np.array_equal(src, want[0]) and np.array_equal(slot, want[1]) and np.array_equal(level, want[2])
    assert sum(totals) == len(src) and [int((slot == k).sum()) for k in range(3)] == list(totals)
    pos = ref.positions(x, idx, d2, step, src, slot, level)
    assert np.array_equal(pos.view(np.uint32), want[3].view(np.uint32))


def test_quirk_drops_the_levels_only_one_point_reaches():
    x = _cloud(7, 100, 1)
    step = ref.average_step(x, 0.3)
    _, d2 = ref.knn3_brute(x)
    rel = ref.relative_distance(d2, step)
    c = ref.counts(d2, step)
    far = 99
    for nb in range(3):
        second = np.sort(rel[:, nb])[-2]
        assert rel[far, nb] == rel[:, nb].max() and np.floor(rel[far, nb]) > np.floor(second)
        assert c[far, nb] == max(0, int(np.floor(second)) - 1)


def test_knn3_brute_ties_go_to_the_lowest_index():
    g = np.stack(np.meshgrid(*[np.arange(4.0)] * 3, indexing="ij"), -1).reshape(-1, 3).astype(np.float32)
    idx, d2 = ref.knn3_brute(g)
    i = 21                                                  # (1,1,1): six neighbours at distance 1
    assert list(d2[i]) == [1.0, 1.0, 1.0] and list(idx[i]) == [5, 17, 20]
    idx, d2 = ref.knn3_brute(g[:3])
    assert idx[0, 2] == -1 and d2[0, 2] == ref.FLT_MAX
