"""CPU: the closed form of the gradients through the depth and alpha maps (tests/depth_grad_ref.py: per entry, folded per
Gaussian, chained to the leaves with the z -> means3D row) against float64 autograd of tests/dense_ref.py's dense_render on the
colour-coded scene (colours (z(means3D), 1, 0), black background, image gradient (gD, gA, 0)).

Float64 against float64: the bar is 1e-8 rel-inf (max abs difference over the reference's max abs) per tensor, loose on
purpose; round-off times the 1 / (1 - alpha) <= 100 conditioning is orders of magnitude below it.
Measured (rel-inf, worst tensor): tiny 1.9e-14, indexed 1.2e-12, odd_size 1.3e-12, one_pixel 0; signed maps on tiny 5.8e-15."""
import numpy as np
import pytest

from tests import depth_grad_ref as dgr

BAR = 1e-8


def _compare(name, signed=False):
    st, inp, _, _ = dgr.black_state(name)
    gD, gA, want = dgr.truth(name, signed)
    got = dgr.restated(st, inp, gD, gA)
    assert got["pairs"] > 0
    worst = 0.0
    for k in dgr.LEAF_ORDER + ("z",):
        if k not in want:
            continue
        assert np.isfinite(got[k]).all() and np.isfinite(want[k]).all(), k
        if name == "one_pixel" and np.abs(want[k]).max() == 0:    # the mean sits on the pixel centre: dx = dy = 0 exactly
            assert np.abs(got[k]).max() == 0, k
            continue
        assert np.abs(want[k]).max() > 0, k                       # the tensor is exercised at all
        e = dgr.rel_inf(got[k], want[k])
        print(name, "signed" if signed else "positive", k, "rel-inf", e)
        worst = max(worst, e)
        assert e <= BAR, (k, e)
    print(name, "worst", worst)
    return got, want


@pytest.mark.parametrize("name", ["tiny", "indexed", "odd_size", "one_pixel"])
def test_closed_form_matches_float64_autograd(name):
    got, want = _compare(name)
    # the z -> means3D row is part of dL_dmeans3D: without it the tensor misses the bar (the term is not negligible)
    without = got["means3D"] - got["z_row"]
    assert dgr.rel_inf(without, want["means3D"]) > BAR


def test_walk_without_flips_is_depth_ref_walk_and_a_replayed_decision_moves_the_gradient():
    """walk_flipped() is depth_ref.walk() when nothing is flipped. On odd_size one visited pair is skipped in float64
    (alpha64 / thr - 1 = -3.4e-6) and blended by the fp32 formula: under the forward's decision dL_dmeans3D is 1.9e-3 away
    from the float64 reference's own, more than any bar a test of the kernel uses; inverting that decision by hand gives the
    reference's own gradients back."""
    from tests import depth_ref
    st, inp, _, _ = dgr.black_state("odd_size")
    gD, gA, want = dgr.truth("odd_size")
    lv = dgr._leaves(inp)
    pix, conic, z = dgr.projection(st, lv)
    co = np.concatenate([conic.detach().numpy(), lv["opacities"].detach().numpy().reshape(-1, 1)], 1)
    state = dict(means2D=pix.detach().numpy(), conic_opacity=co, depths=z.detach().numpy().astype(np.float32),
                 point_list=st.point_list, ranges=st.ranges)
    a, b = depth_ref.walk(state, st.W, st.H), dgr.walk_flipped(state, st.W, st.H)
    for k in ("start", "T", "z", "pos"):
        assert np.array_equal(getattr(a, k), getattr(b, k)), k
    replayed, amb, cands = dgr.candidates("odd_size")
    print("odd_size: pairs (pixel, list position) replayed:", replayed, "ambiguous:", amb)
    assert replayed == [(89 * 203 + 25, replayed[0][1])] and len(cands) == 2 ** len(amb)
    moved = dgr.rel_inf(cands[0]["means3D"], want["means3D"])
    print("odd_size: dL_dmeans3D under the forward's decision, rel-inf to the float64 reference's own:", moved)
    assert 1e-3 < moved < 3e-3
    back = dgr.restated(st, inp, gD, gA, flip=tuple(replayed), fp32=True)
    for k in dgr.LEAF_ORDER:
        if k in want:
            assert dgr.rel_inf(back[k], want[k]) <= BAR, k
    r, amb, cands = dgr.candidates("tiny")
    assert r == [] and amb == [] and cands[0] is dgr.truth("tiny")[2]


def test_signed_maps():
    _compare("tiny", signed=True)


def test_hashed_maps():
    a, b = dgr.hashed_map(75, 50, 1), dgr.hashed_map(75, 50, 2)
    assert a.shape == (50, 75) and a.min() >= 0.25 and a.max() < 1.0 and not np.array_equal(a, b)
    assert np.array_equal(a, a.astype(np.float32).astype(np.float64))
    s = dgr.hashed_map(75, 50, 1, signed=True)
    assert (s < 0).any() and (s > 0).any() and np.array_equal(np.abs(s), a)
