"""CPU: the float64 reference of tests/error_ref.py (per-Gaussian sum of alpha T x a per-pixel map) is right, and the bar
tests/test_render_error_gpu.py holds the kernel to is one an fp32 evaluation with the kernel's arithmetic meets.

  * with e = 1 the walk is tests/contrib_ref.py's: err_sum equals its weight_sum exactly, and so do hits, final T, n_contrib.
  * walk() against brute_force() -- no tiles -- on the full-cover scenes of tests/test_depth_ref_cpu.py, with the standard map:
    same float64 operations in the same order, identical results. Conservation: sum err_sum = sum e (1 - T).
  * walk() against fp32_stats() on every scene of the GPU test (those of tests/depth_ref.py and `long_run`), standard map: at
    most max(2, 2e-5 P) Gaussians differ in hits, every other row agrees to 1e-4 relative (measured: 0 Gaussians, 1.19e-5 at
    most, on `needles_long`).
  * the standard map is fp32, deterministic, within [0.25, 1) and not constant."""
import numpy as np
import pytest

from tests import cases, contrib_ref, depth_ref, error_ref
from tests.test_depth_ref_cpu import _full_cover_scene


def test_standard_map():
    e = error_ref.standard_map(45, 70)
    assert e.dtype == np.float32 and e.shape == (45, 70)
    assert e.min() >= 0.25 and e.max() < 1.0 and np.unique(e).size > 3000
    np.testing.assert_array_equal(e, error_ref.standard_map(45, 70))
    np.testing.assert_array_equal(e[:20, :30], error_ref.standard_map(20, 30))      # a function of (y, x) alone
    assert abs(float(e.mean()) - 0.625) < 0.02


@pytest.mark.parametrize("name", ["odd_size", "one_pixel"])
def test_a_map_of_ones_gives_the_contrib_walk(orc, name):
    st = depth_ref.oracle_state(name)
    c = contrib_ref.walk(st, st.W, st.H)
    w = error_ref.walk(st, st.W, st.H, np.ones((st.H, st.W)))
    np.testing.assert_array_equal(w.err_sum, c.weight_sum)
    np.testing.assert_array_equal(w.hits, c.hits)
    np.testing.assert_array_equal(w.final_T, c.final_T)
    np.testing.assert_array_equal(w.n_contrib, c.n_contrib)
    assert w.hits.sum() > 0


@pytest.mark.parametrize("P,W,H,seed,opacity", [(50, 32, 32, 3, (0.02, 0.4)), (37, 31, 19, 4, (0.3, 1.0)), (50, 17, 32, 6, (0.005, 0.05)),
                                                 (1, 1, 1, 8, (0.9, 0.9))])
def test_walk_matches_tile_free_brute_force(orc, P, W, H, seed, opacity):
    inp, cam = _full_cover_scene(P, W, H, seed, opacity)
    st = cases.oracle_forward(inp, cam)
    vis = st.radii > 0
    assert (st.tiles_touched[vis] == st.T).all(), "a splat misses a tile: the brute force would walk more than the lists hold"
    e = error_ref.standard_map(H, W)
    w = error_ref.walk(st, W, H, e)
    b = error_ref.brute_force(st, W, H, vis, e)
    np.testing.assert_array_equal(w.hits, b.hits)
    np.testing.assert_array_equal(w.final_T, b.final_T)
    np.testing.assert_array_equal(w.err_sum, b.err_sum)
    np.testing.assert_array_equal(w.n_contrib, st.n_contrib.astype(np.int64))
    assert (w.hits[~vis] == 0).all() and (w.err_sum[~vis] == 0).all() and w.hits.sum() > 0
    np.testing.assert_allclose(w.err_sum.sum(), (e.astype(np.float64).ravel() * (1.0 - w.final_T)).sum(), rtol=1e-12)
    # the map matters: the scores are not the weights
    if P > 1:
        assert not np.array_equal(w.err_sum, contrib_ref.walk(st, W, H).weight_sum)


@pytest.mark.parametrize("name", depth_ref.SCENES + ["long_run"])
def test_fp32_evaluation_meets_the_gpu_bar(orc, name):
    st = error_ref.long_run_state() if name == "long_run" else depth_ref.oracle_state(name)
    if name == "long_run":                                      # what the scene is there for
        assert st.tiles_touched[0] == 17 * 17 > 256
    e = error_ref.standard_map(st.H, st.W)
    ref = error_ref.walk(st, st.W, st.H, e)
    np.testing.assert_array_equal(ref.n_contrib, st.n_contrib.astype(np.int64))
    emu = error_ref.fp32_stats(st, e)
    differ, rel = error_ref.compare(emu.err_sum, emu.hits, ref, name)
    assert differ <= contrib_ref.exemption_cap(st.P)
    assert rel <= 1e-4
    assert ref.hits.sum() > 0 and (ref.hits[st.radii == 0] == 0).all() and (ref.err_sum[ref.hits == 0] == 0).all()
