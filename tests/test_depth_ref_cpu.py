"""CPU: the float64 median reference of tests/depth_ref.py is right, and the exemption the GPU test grants is not needed by
the reference side.

  * walk() against brute_force() -- no tiles, every visible Gaussian at every pixel in (depth, id) order -- on scenes of at
    most 50 Gaussians and 32 x 32 pixels whose splats are large enough that every tile's list holds every visible Gaussian
    (asserted: otherwise the two walk different sets). Same float64 operations in the same order: the T sequences, depths and
    positions must be identical, and so must the oracle's own n_contrib.
  * tests/test_render_depth_gpu.py skips the pixels where the HIP forward and the oracle disagree on n_contrib and caps their
    number at max(2, 2e-5 x pixels). tests/alt_blend.py (the kernel's rounding of the exponent, emulated) stands in for the HIP
    forward here: on every scene of the GPU test the disagreeing pixels are within that cap.
  * median_candidates() on hand-made T sequences: the band's two ends, the zero cases."""
import numpy as np
import pytest
import torch

from tests import alt_blend, cases, depth_ref, synth


def _full_cover_scene(P, W, H, seed, opacity):
    from oracle import oracle as orc
    focal = 30.0
    intr, ev = synth.camera(W, H, focal, extrinsic_vector=(0.05, -0.03, 0.02, 0.99, 0.1, -0.05, 0.2))
    sc = synth.scene(P, W, H, focal, seed=seed, scale_median=8.0, zmin=2.0, zmax=9.0, behind_fraction=0.2 if P > 1 else 0.0)
    g = torch.Generator().manual_seed(seed + 1)
    sc["opacities"] = (opacity[0] + (opacity[1] - opacity[0]) * torch.rand(P, 1, generator=g)).float()
    if P > 1:
        sc["means3D"][1, 2] = sc["means3D"][0, 2]              # a depth tie: id order decides
    inp = dict(bg=torch.zeros(3), means3D=sc["means3D"], opacities=sc["opacities"], shs=sc["shs"], colors_precomp=None,
               scales=sc["scales"], rotations=sc["rotations"], cov3D_precomp=None, scale_factors=None, sh_indices=None,
               g_indices=None, degree=3, scale_modifier=1.0, prefiltered=False, clamp_color=True)
    return inp, orc.camera(intr.numpy(), ev.numpy())


@pytest.mark.parametrize("P,W,H,seed,opacity", [(50, 32, 32, 3, (0.02, 0.4)), (37, 31, 19, 4, (0.3, 1.0)), (50, 17, 32, 6, (0.005, 0.05)),
                                                 (1, 1, 1, 8, (0.9, 0.9))])
def test_walk_matches_tile_free_brute_force(orc, P, W, H, seed, opacity):
    inp, cam = _full_cover_scene(P, W, H, seed, opacity)
    st = cases.oracle_forward(inp, cam)
    vis = st.radii > 0
    assert vis.sum() >= max(1, P // 2)
    assert (st.tiles_touched[vis] == st.T).all(), "a splat misses a tile: the brute force would walk more than the lists hold"
    w = depth_ref.walk(st, W, H)
    b = depth_ref.brute_force(st, W, H, vis)
    np.testing.assert_array_equal(w.start, b.start)
    np.testing.assert_array_equal(w.T, b.T)
    np.testing.assert_array_equal(w.z.view(np.uint32), b.z.view(np.uint32))
    np.testing.assert_array_equal(w.pos, b.pos)
    np.testing.assert_array_equal(w.n_contrib, st.n_contrib.astype(np.int64))
    if P > 1:
        assert (np.diff(w.start) >= 2).any()                   # something is blended over something
        # the same walk from a plain dict (what the GPU test may hand in)
        d = dict(means2D=st.means2D, conic_opacity=st.conic_opacity, depths=st.depths, point_list=st.point_list, ranges=st.ranges)
        np.testing.assert_array_equal(depth_ref.walk(d, W, H).T, w.T)
    # T after the last blended entry is the oracle's final_T (fp32), at the bar tests/test_raster_gpu.py holds final_T to
    last = np.ones(W * H)
    has = w.start[1:] > w.start[:-1]
    last[has] = w.T[w.start[1:][has] - 1]
    np.testing.assert_allclose(last, st.final_T, rtol=1e-4, atol=1e-5)


@pytest.mark.parametrize("name", depth_ref.SCENES)
def test_exemption_cap_is_met_by_the_reference_side(orc, name):
    st = depth_ref.oracle_state(name)
    emu = alt_blend.forward(st)
    differ = int((emu["n_contrib"] != st.n_contrib).sum())
    print(name, "pixels where the emulated kernel rounding and the oracle disagree on n_contrib:", differ)
    assert differ <= depth_ref.exemption_cap(st.N)
    # and the walk is the oracle's: same last contributor on every pixel
    np.testing.assert_array_equal(depth_ref.walk(st, st.W, st.H).n_contrib, st.n_contrib.astype(np.int64))


def test_median_candidates():
    z = np.arange(1, 6, dtype=np.float32)
    f = depth_ref.median_candidates
    c, zero = f(np.array([0.9, 0.7, 0.4, 0.2, 0.1]), z, 5)
    assert list(c) == [3.0] and not zero
    c, zero = f(np.array([0.9, 0.8, 0.7, 0.6, 0.55]), z, 5)
    assert c.size == 0 and zero
    c, zero = f(np.zeros(0), z[:0], 0)
    assert c.size == 0 and zero
    band = 4 * 6 * depth_ref.U
    c, zero = f(np.array([0.9, 0.5 * (1 + 0.5 * band), 0.5 * (1 - 0.5 * band), 0.3, 0.1]), z, 5)   # two entries inside the band
    assert list(c) == [2.0, 3.0, 4.0] and not zero
    c, zero = f(np.array([0.9, 0.8, 0.5 * (1 + 0.5 * band)]), z[:3], 5)                             # ends inside the band
    assert list(c) == [3.0] and zero
