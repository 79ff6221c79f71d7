"""CPU: the float64 reference of tests/contrib_ref.py (per-Gaussian sum / max of alpha T and blended-pair count) is right, and the
exemption tests/test_render_contrib_gpu.py grants is not needed by the reference side.

  * walk() against brute_force() -- no tiles, every visible Gaussian at every pixel in (depth, id) order -- on the full-cover
    scenes of tests/test_depth_ref_cpu.py (every tile's list holds every visible Gaussian, asserted): same float64 operations
    in the same order per pixel, and both fold a Gaussian's weights in pixel order (every live pixel of a step has the same
    Gaussian), so sum, max and hits are identical. The walk's n_contrib is the oracle's and its final T the oracle's.
  * walk() against fp32_stats() -- tests/alt_blend.py's arithmetic, the kernel's rounding of the exponent -- on every scene of
    the GPU test (tests/depth_ref.py's and tests/error_ref.py's `long_run`): the Gaussians whose hits differ are within max(2, 2e-5 P), every other row agrees to 1e-4 relative in
    weight_sum and weight_max, the bar the GPU test holds the kernel to (measured: 0 Gaussians, 1.15e-5 and 4.3e-6 at most)."""
import numpy as np
import pytest

from tests import cases, contrib_ref, depth_ref, error_ref
from tests.test_depth_ref_cpu import _full_cover_scene


@pytest.mark.parametrize("P,W,H,seed,opacity", [(50, 32, 32, 3, (0.02, 0.4)), (37, 31, 19, 4, (0.3, 1.0)), (50, 17, 32, 6, (0.005, 0.05)),
                                                 (1, 1, 1, 8, (0.9, 0.9))])
def test_walk_matches_tile_free_brute_force(orc, P, W, H, seed, opacity):
    inp, cam = _full_cover_scene(P, W, H, seed, opacity)
    st = cases.oracle_forward(inp, cam)
    vis = st.radii > 0
    assert (st.tiles_touched[vis] == st.T).all(), "a splat misses a tile: the brute force would walk more than the lists hold"
    w = contrib_ref.walk(st, W, H)
    b = contrib_ref.brute_force(st, W, H, vis)
    np.testing.assert_array_equal(w.hits, b.hits)
    np.testing.assert_array_equal(w.weight_max, b.weight_max)
    np.testing.assert_array_equal(w.final_T, b.final_T)
    np.testing.assert_array_equal(w.weight_sum, b.weight_sum)
    np.testing.assert_array_equal(w.n_contrib, st.n_contrib.astype(np.int64))
    np.testing.assert_allclose(w.final_T, st.final_T, rtol=1e-4, atol=1e-5)
    # culled rows are exact zeros; something is blended; what is blended is conserved: sum_g weight_sum = sum_pix (1 - T)
    assert (w.hits[~vis] == 0).all() and (w.weight_sum[~vis] == 0).all() and (w.weight_max[~vis] == 0).all()
    assert w.hits.sum() > 0
    assert (w.weight_max <= w.weight_sum).all() and w.weight_max.max() <= 0.99
    np.testing.assert_allclose(w.weight_sum.sum(), (1.0 - w.final_T).sum(), rtol=1e-12)
    # the depth reference walks the same entries
    d = depth_ref.walk(st, W, H)
    assert d.T.size == w.hits.sum()


@pytest.mark.parametrize("name", list(contrib_ref.SCENES) + ["long_run"])
def test_fp32_evaluation_meets_the_gpu_bar(orc, name):
    """`long_run` (tests/error_ref.py: a Gaussian over 17 x 17 tiles) measured on the CPU: 0 of 301 Gaussians exempt, weight_sum
    2.4e-7, weight_max 2.6e-7, 117,064 blended pairs."""
    st = error_ref.long_run_state() if name == "long_run" else depth_ref.oracle_state(name)
    ref = contrib_ref.walk(st, st.W, st.H)
    np.testing.assert_array_equal(ref.n_contrib, st.n_contrib.astype(np.int64))
    emu = contrib_ref.fp32_stats(st)
    exempt, rel_sum, rel_max = contrib_ref.compare(emu.weight_sum, emu.weight_max, emu.hits, ref, name)
    assert exempt <= contrib_ref.exemption_cap(st.P)
    assert rel_sum <= 1e-4 and rel_max <= 1e-4
    assert ref.hits.sum() > 0 and (ref.hits[st.radii == 0] == 0).all()
