"""CPU: the edge-Gaussian cases of tests/cases.py (opaque, needle, disc, un-normalised, near-camera) before a kernel is involved.
  * every case is what it claims to be (cases.edge_guard, asserted inside cases.edge_reference);
  * the oracle against the float64 truth of tests/dense_ref.py: within test_oracle_dense.py's TOL where the reference's fp32
    formula is well conditioned (opaque_big, discs, unnorm_quat); on needles and near-camera floaters its deviation d_ref is
    printed per tensor and must stay <= 5e-3 -- a CONDITION on the case (beyond it the case says nothing and a milder one must
    be chosen), not a tolerance on any code;
  * two fp32 evaluations of the blend (the oracle's and tests/alt_blend.py's, rounded as render.hip rounds) take the same
    decisions within the flip cap of the GPU bars, every flip proven: the inputs are feasible for those bars;
  * the clamp semantics are told apart: autograd through a hard min(0.99, o G) is far from the oracle, straight-through agrees.
"""
import numpy as np
import pytest

from tests import alt_blend, cases, dense_ref, fullsize
from tests.test_oracle_dense import TOL

D_REF_MAX = 5e-3


@pytest.mark.parametrize("name", cases.EDGE_GAUSSIAN_CASES)
def test_edge_case_oracle_vs_float64(orc, name):
    e = cases.edge_reference(name)
    st = e["st"]
    print(name, "guard", e["guard"], "d_ref", {k: f"{v:.2e}" for k, v in e["d_ref"].items()})
    assert st.num_rendered > 0
    assert set(e["d_ref"]) >= {"dL_dmeans3D", "dL_dmeans2D", "dL_dopacity", "dL_dsh", "dL_dscales", "dL_drotations", "dL_dcolors",
                               "dL_dcov3D"} | ({"dL_dscale_factors"} if e["indexed"] else set())
    for k, t in e["truth"].items():
        assert np.isfinite(t).all() and np.isfinite(e["ref"][k]).all(), k
        assert np.abs(t).max() > 0, k
    # the oracle and float64 took the same blend decisions (the criterion of fullsize.flipped_pixels), so d_ref is rounding alone
    dimg = np.abs(e["img64"] - st.out_color)
    assert (dimg <= 2e-5 + 1e-4 * np.abs(e["img64"])).all(), dimg.max()
    worst = max(e["d_ref"].values())
    assert worst <= D_REF_MAX, f"{name} is too ill-conditioned to say anything: {e['d_ref']}"
    if name in cases.EDGE_WITHIN_TOL:
        assert dimg.max() < 5e-6
        assert worst < TOL, e["d_ref"]


@pytest.mark.parametrize("name", cases.EDGE_GAUSSIAN_CASES)
def test_edge_case_is_feasible_for_the_gpu_bars(orc, name):
    st = cases.edge_reference(name)["st"]
    u = alt_blend.forward(st)
    flipped = fullsize.flipped_pixels(u, st)
    n = int(flipped.sum())
    print(name, n, "flips")
    assert n <= max(2, int(2e-5 * st.W * st.H))
    proof = fullsize.prove_flips(u, st, flipped)
    assert proof["outside_band"] == 0 and proof["oracle_outside_band"] == 0, proof
    ok = ~flipped
    assert np.abs(u["out_color"] - st.out_color)[:, ok].max() <= 2e-5 + 1e-4 * np.abs(st.out_color).max()


def test_the_clamp_passes_its_gradient_straight_through(orc):
    """backward.cu:499-554 differentiates o G as if unclamped. On opaque_big (4 % of the blends clamped) autograd through a
    hard min() must be FAR from the oracle -- otherwise this suite could not tell the two semantics apart -- and the
    straight-through form within TOL."""
    e = cases.edge_reference("opaque_big")
    hard = dense_ref.truth(e["st"], e["inp"], e["dL"], hard_clamp=True)[1]
    rel = lambda a, b: float(np.abs(a - b).max() / np.abs(b).max())
    d_hard = rel(e["ref"]["dL_dopacity"], hard["dL_dopacity"])
    print("dL_dopacity: oracle vs hard clamp", d_hard, "vs straight-through", e["d_ref"]["dL_dopacity"])
    assert d_hard > 100 * TOL
    assert e["d_ref"]["dL_dopacity"] < TOL and e["d_ref"]["dL_dmeans3D"] < TOL
    assert np.array_equal(hard["dL_dsh"] != 0, e["truth"]["dL_dsh"] != 0)       # the same pairs blend either way
