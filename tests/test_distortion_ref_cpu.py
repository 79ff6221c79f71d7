"""CPU: the float64 reference of the depth-distortion map and its gradient (tests/distortion_ref.py) against itself, and the fp32
restatement of the kernels' recurrences against it -- the check that the GPU bars of tests/test_distortion_gpu.py are reachable in
fp32 before any GPU run.

  prefix = brute force     the prefix formula (which assumes ascending s inside a pixel) against the double sum with |.|, 1e-12
                           of the map's largest value; on `deep` (hundreds of entries per pixel) the double sum on every 16th pixel
  closed form = autograd   closed_form + chain against float64 autograd over the walk's pairs, rel-inf 1e-9 per leaf, with gL alone
                           and with gD, gA, gL together
  translation invariance   raw mode: every depth + 3.25 leaves the map unchanged to 1e-10
  fp32 restatement         numpy float32 of the recurrences the kernels run (PIVOTED: the forward about the pixel's first s, the
                           backward about moment / A) against float64 on the same pairs: forward maps within half of the GPU
                           test's bar smax 2e-5 + 1e-4 |ref|, every leaf gradient within half of rel-inf 1e-4. The plain recurrences
                           are printed next to them and miss that bar in the ndc mode, which is why the kernels do not run them.
  one_pixel                a single Gaussian: distortion exactly 0, every gradient exactly 0 (float64; fp32 leaves 5e-9)

Measured (fp32 restatement, worst leaf rel-inf, gL alone / three maps; forward: largest error over its bar):
see FP32_MEASURED."""
import functools

import numpy as np
import pytest

from tests import depth_grad_ref as dgr, distortion_ref as dr

SCENES = ["tiny", "indexed", "odd_size", "cov_precomp", "colors_precomp", "deep", "one_pixel"]
MODE_NAMES = ["raw", "ndc"]
FP32_MEASURED = ("worst leaf rel-inf, gL alone (plain recurrences in brackets): raw tiny 1.2e-5 (6.5e-6), indexed 1.5e-6 (1.2e-6), odd_size "
                 "2.1e-6 (7.3e-7), cov_precomp 1.6e-6 (9.4e-7), colors_precomp 2.0e-6 (9.7e-7), deep 1.1e-5 (1.2e-5); ndc tiny 1.3e-5 (1.8e-4), "
                 "indexed 1.9e-6 (2.0e-5), odd_size 2.8e-6 (3.4e-5), cov_precomp 2.1e-6 (2.6e-5), colors_precomp 4.5e-6 (2.8e-5), deep 1.1e-5 "
                 "(4.4e-4); three maps: at most 3.4e-7; forward maps: at most 0.034 of their bar (deep, ndc)")


@functools.lru_cache(maxsize=None)
def _case(name):
    st, inp, cam, indexed = dgr.black_state(name)
    return st, inp, st.W, st.H


@functools.lru_cache(maxsize=None)
def _forward(name, mode_name):
    st, _, W, H = _case(name)
    return dr.forward(st, W, H, dr.MODES[mode_name])


@pytest.mark.parametrize("mode_name", MODE_NAMES)
@pytest.mark.parametrize("name", SCENES)
def test_prefix_formula_equals_the_brute_force_double_sum(name, mode_name):
    st, _, W, H = _case(name)
    fw = _forward(name, mode_name)
    pixels = np.arange(0, W * H, 16 if name == "deep" else 1)
    brute = dr.forward_brute(st, W, H, dr.MODES[mode_name], pixels, wk=fw["walk"])
    got = fw["distortion"].reshape(-1)[pixels]
    scale = max(float(np.abs(brute).max()), 1e-300)
    e = float(np.abs(got - brute).max()) / scale
    print(name, mode_name, "prefix against brute force: largest difference over the largest value", e, "largest value", scale)
    assert e <= 1e-12
    assert (brute >= 0).all()
    if name == "one_pixel":
        assert not fw["distortion"].any() and fw["moment"].max() > 0
    else:
        assert brute.max() > 0 and (np.diff(fw["walk"].start) > 1).any()


@pytest.mark.parametrize("name", SCENES)
def test_translation_invariance_raw(name):
    st, _, W, H = _case(name)
    a = _forward(name, "raw")
    b = dr.forward(st, W, H, None, shift=3.25, wk=a["walk"])
    scale = max(float(np.abs(a["distortion"]).max()), 1e-300)
    e = float(np.abs(a["distortion"] - b["distortion"]).max()) / scale
    print(name, "raw: shift by 3.25, largest difference over the largest value", e)
    assert e <= 1e-10
    if name != "one_pixel":
        assert np.abs(a["moment"] - b["moment"]).max() > 1.0 * np.abs(a["moment"]).max() * 0.1     # the moment does move


def _maps(st, three):
    zero = np.zeros((st.H, st.W))
    gL = dr.gl_map(st.W, st.H)
    return (dgr.hashed_map(st.W, st.H, 1), dgr.hashed_map(st.W, st.H, 2), gL) if three else (zero, zero, gL)


def _compare(got, want, bar, label, zero_ok=False, zero_tol=0.0):
    worst = 0.0
    for k in dgr.LEAF_ORDER + ("z",):
        if k not in want:
            continue
        assert np.isfinite(got[k]).all() and np.isfinite(want[k]).all(), k
        if np.abs(want[k]).max() == 0:
            assert zero_ok, k
            assert np.abs(got[k]).max() <= zero_tol, (k, float(np.abs(got[k]).max()))
            continue
        e = dgr.rel_inf(got[k], want[k])
        print(label, k, "rel-inf %.3e" % e, "reference max %.3e" % float(np.abs(want[k]).max()))
        worst = max(worst, e)
        assert e <= bar, (label, k, e)
    return worst


@pytest.mark.parametrize("three", [False, True], ids=["gL", "gD+gA+gL"])
@pytest.mark.parametrize("mode_name", MODE_NAMES)
@pytest.mark.parametrize("name", SCENES)
def test_closed_form_matches_float64_autograd(name, mode_name, three):
    st, inp, W, H = _case(name)
    mode = dr.MODES[mode_name]
    gD, gA, gL = _maps(st, three)
    got = dr.restated(st, inp, gD, gA, gL, mode)
    want = dr.autograd_truth(st, inp, gD, gA, gL, mode)
    assert got["pairs"] > 0
    # one_pixel: a single entry has no partner (and sits on the pixel centre): with gL alone every gradient is an exact zero
    worst = _compare(got, want, 1e-9, f"closed form {name} {mode_name}:", zero_ok=(name == "one_pixel"))
    print(f"closed form {name} {mode_name} {'three maps' if three else 'gL alone'}: worst rel-inf {worst:.3e}")
    if name == "one_pixel" and not three:
        for k in dgr.LEAF_ORDER + ("z",):
            if k in got:
                assert not np.asarray(got[k]).any() and not np.asarray(want[k]).any(), k


@pytest.mark.parametrize("three", [False, True], ids=["gL", "gD+gA+gL"])
@pytest.mark.parametrize("mode_name", MODE_NAMES)
@pytest.mark.parametrize("name", SCENES)
def test_fp32_restatement_meets_half_the_gpu_bars(name, mode_name, three):
    st, inp, W, H = _case(name)
    mode = dr.MODES[mode_name]
    gD, gA, gL = _maps(st, three)
    want = dr.restated(st, inp, gD, gA, gL, mode)
    got, maps = dr.fp32_restatement(st, inp, gD, gA, gL, mode)
    # the forward maps against the float64 prefix formula on the same per-Gaussian float64 values (restated()'s walk)
    ref = _restated_forward(name, mode_name)
    smax = ref["smax"]
    for k in ("distortion", "moment"):
        err = np.abs(maps[k].astype(np.float64) - ref[k])
        over = float((err / (smax * 2e-5 + 1e-4 * np.abs(ref[k]))).max())
        print(f"fp32 restatement {name} {mode_name}: {k} largest error {float(err.max()):.3e}, largest error over its GPU bar {over:.3e}, "
              f"smax {smax:.4f}")
        assert over <= 0.5, (k, over)
    # one_pixel under gL alone: the float64 gradients are exact zeros; fp32 leaves the round-off of the pivot, a few ulp of s
    # (at most 4 here) times w |gL| <= 1: held to 1e-6, where a term that should not be there is of the size of s, i.e. 1
    worst = _compare(got, want, 0.5e-4, f"fp32 restatement {name} {mode_name}:", zero_ok=(name == "one_pixel"), zero_tol=1e-6)
    # what the pivot is for: the plain recurrences on the same pairs (a figure, no bar: they are not what the kernel runs)
    plain, _ = dr.fp32_restatement(st, inp, gD, gA, gL, mode, pivot=False)
    worst_plain = max([dgr.rel_inf(plain[k], want[k]) for k in dgr.LEAF_ORDER if k in want and np.abs(want[k]).max() > 0] or [0.0])
    print(f"fp32 restatement {name} {mode_name} {'three maps' if three else 'gL alone'}: worst leaf rel-inf {worst:.3e} "
          f"(plain recurrences, no pivot: {worst_plain:.3e})")


@functools.lru_cache(maxsize=None)
def _restated_forward(name, mode_name):
    """forward() on the float64 per-Gaussian values of projection(): the pairs restated() and fp32_restatement() walk"""
    st, inp, W, H = _case(name)
    lv = dgr._leaves(inp)
    pix, conic, z = dgr.projection(st, lv)
    co = np.concatenate([conic.detach().numpy(), lv["opacities"].detach().numpy().reshape(-1, 1)], 1)
    state = dict(means2D=pix.detach().numpy(), conic_opacity=co, depths=z.detach().numpy().astype(np.float32),
                 point_list=st.point_list, ranges=st.ranges)
    return dr.forward(state, W, H, dr.MODES[mode_name])


def test_modes_and_maps():
    z = np.array([0.5, 1.0, 7.0])
    near, far = dr.NDC
    assert np.allclose(dr.f_map(z, dr.NDC), far / (far - near) * (1 - near / z)) and (np.diff(dr.f_map(z, dr.NDC)) > 0).all()
    h = 1e-6
    assert np.allclose(dr.df_map(z, dr.NDC), (dr.f_map(z + h, dr.NDC) - dr.f_map(z - h, dr.NDC)) / (2 * h), rtol=1e-6)
    assert np.array_equal(dr.f_map(z, None), z) and np.array_equal(dr.df_map(z, None), np.ones(3))
    g = dr.gl_map(75, 50)
    assert (g < 0).any() and (g > 0).any() and not np.array_equal(np.abs(g), dgr.hashed_map(75, 50, 1))
