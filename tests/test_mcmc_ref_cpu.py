"""CPU: the mathematics of tests/mcmc_ref.py, the host restatement tests/test_mcmc_gpu.py holds csrc/mcmc.hip to. These tests
run no code of the package: they pass with or without the feature and only pin the reference itself."""
import math

import numpy as np
import pytest

from tests import mcmc_ref as ref

OPACITIES = (0.006, 0.3, 0.9, 0.99, 1 - 1e-6)
NS = (1, 2, 3, 5, 20, 51)


@pytest.mark.parametrize("o", OPACITIES)
@pytest.mark.parametrize("N", NS)
def test_n_copies_of_the_new_opacity_composite_to_the_old_one(o, N):
    on, _ = ref.relocation(o, N, min_opacity=0.0)
    assert abs((1 - (1 - on) ** N) - o) <= 1e-12


@pytest.mark.parametrize("o", OPACITIES)
def test_a_single_copy_keeps_its_scale(o):
    on, c = ref.relocation(o, 1, min_opacity=0.0)
    assert abs(on - o) <= 1e-15 and abs(c - 1) <= 1e-15


@pytest.mark.parametrize("o", OPACITIES)
def test_the_scale_factor_decreases_with_the_number_of_copies(o):
    cs = [ref.relocation(o, N, min_opacity=0.0)[1] for N in range(1, ref.MAX_N + 1)]
    assert all(a > b for a, b in zip(cs, cs[1:])), cs
    assert all(0 < c <= 1 for c in cs)


def test_the_new_opacity_is_clamped():
    on, _ = ref.relocation(0.006, 51, min_opacity=0.005)
    assert on == float(np.float32(0.005))
    assert ref.relocation(1 - 1e-12, 1)[0] == 1.0 - ref.FLT_EPSILON


def test_the_vector_form_agrees_with_the_scalar_form():
    for o in OPACITIES:
        raw = np.float32(math.log(o / (1 - o)))
        o32 = float(ref.sigmoid(raw))
        for N in NS[1:]:
            on, c = ref.relocation(o32, N)
            rows, on_v, c_v = ref.values(np.array([raw]), np.array([N - 1]))
            assert rows.tolist() == [0]
            assert abs(on_v[0] - on) <= 1e-9 * on and abs(c_v[0] - c) <= 1e-9 * c      # log(1 - o) two ways near o = 1


def _weights():
    rng = np.random.default_rng(5)
    raw = rng.normal(0, 2, 300).astype(np.float32)
    dead = rng.random(300) < 0.3
    dead[:3] = True
    dead[-4:] = True
    return ref.weights(raw, dead)[0], dead


def test_a_row_without_weight_is_never_chosen():
    q, dead = _weights()
    draws = np.random.default_rng(6).random(20000)
    sources, counts, T = ref.sample(q, draws)
    assert T == int(q.sum()) and counts.sum() == 20000
    assert not dead[sources].any() and (counts[dead] == 0).all()
    assert (q[sources] > 0).all()


def test_the_extreme_draws_choose_the_first_and_the_last_eligible_row():
    q, dead = _weights()
    alive = np.nonzero(q > 0)[0]
    sources, _, _ = ref.sample(q, np.array([0.0, np.nextafter(1.0, 0.0)]))
    assert sources.tolist() == [alive[0], alive[-1]] and alive[0] >= 3 and alive[-1] <= 295      # dead rows at both ends


def test_nothing_is_sampled_without_weight():
    sources, counts, T = ref.sample(np.zeros(7, dtype=np.int64), np.array([0.0, 0.5]))
    assert T == 0 and sources.tolist() == [-1, -1] and not counts.any()


def test_the_prefix_is_held_in_python_integers():
    q = np.full(5000, ref.weights(np.full(5000, math.log(0.99 / 0.01), dtype=np.float32))[0][0])
    C = ref.prefix(q)
    assert isinstance(C[-1], int) and C[-1] > 2 ** 32 and C[-1] == 5000 * int(q[0])


def test_stratified_draws_reproduce_the_weights():
    q, _ = _weights()
    n = 1 << 16
    _, counts, T = ref.sample(q, (np.arange(n) + 0.5) / n)
    assert np.abs(counts - q / T * n).max() <= 1


def test_the_noise_is_the_covariance_applied_to_the_draw():
    rng = np.random.default_rng(7)
    P = 9
    rot, sc, xi = rng.normal(size=(P, 4)).astype(np.float32), rng.normal(-2, 0.5, (P, 3)).astype(np.float32), rng.normal(size=(P, 3)).astype(np.float32)
    raw_op = np.full(P, math.log(0.001 / 0.999), dtype=np.float32)
    d = ref.noise(None, rot, sc, None, raw_op, xi, 5e5, 1e-4)
    qn = rot.astype(np.float64) / np.linalg.norm(rot.astype(np.float64), axis=1, keepdims=True)
    for p in range(P):
        r, x, y, z = qn[p]
        R = np.array([[1 - 2 * (y * y + z * z), 2 * (x * y - r * z), 2 * (x * z + r * y)],
                      [2 * (x * y + r * z), 1 - 2 * (x * x + z * z), 2 * (y * z - r * x)],
                      [2 * (x * z - r * y), 2 * (y * z + r * x), 1 - 2 * (x * x + y * y)]])
        S = R @ np.diag(np.exp(sc[p].astype(np.float64)) ** 2) @ R.T
        g = 1 / (1 + math.exp(-100 * ((1 - float(ref.sigmoid(raw_op[p]))) - 0.995)))
        assert np.allclose(d[p], S @ xi[p].astype(np.float64) * g * 5e5 * 1e-4, rtol=1e-12, atol=0)
    assert 0.5 < g < 0.7                                         # o = 0.001 sits on the open side of the gate
    gate = lambda o: 1 / (1 + math.exp(-100 * ((1 - o) - 0.995)))       # noqa: E731
    assert gate(0.9) < 1e-38 and gate(0.05) < 0.02 and gate(0.005) == 0.5


def test_apply_moves_rows_and_corrects_source_and_destination_alike():
    rng = np.random.default_rng(8)
    params = {"xyz": rng.normal(size=(4, 3)).astype(np.float32), "opacity": np.float32([[-6.0], [0.5], [1.5], [2.0]]),
              "scale": rng.normal(-3, 0.3, (4, 1)).astype(np.float32)}
    moments = {k: (np.ones_like(v), np.ones_like(v)) for k, v in params.items()}
    counts = np.array([0, 0, 1, 0])
    new, mom = ref.apply(params, moments, [0], [2], counts, True, "scale")
    on, c = ref.relocation(float(ref.sigmoid(np.float32(1.5))), 2)
    assert np.array_equal(new["xyz"][0], params["xyz"][2]) and np.array_equal(new["xyz"][1:], params["xyz"][1:])
    assert new["opacity"][0] == new["opacity"][2] and abs(new["opacity"][2, 0] - math.log(on / (1 - on))) <= 1e-12
    assert new["scale"][0] == new["scale"][2] and abs(new["scale"][2, 0] - (float(params["scale"][2, 0]) + math.log(c))) <= 1e-12
    assert np.array_equal(new["opacity"][[1, 3]], params["opacity"][[1, 3]]) and np.array_equal(new["scale"][[1, 3]], params["scale"][[1, 3]])
    for k in mom:
        for a in mom[k]:
            assert not a[[0, 2]].any() and a[[1, 3]].all()
    grown, _ = ref.apply(params, moments, [3], [2], counts, False, "scale")
    assert np.array_equal(grown["xyz"], params["xyz"]) and grown["opacity"][3] == grown["opacity"][2] == new["opacity"][2]
