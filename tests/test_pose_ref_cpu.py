"""CPU: the derivation behind csrc/pose_grad.hip. tests/pose_ref.py's float64 restatement of the kernels' arithmetic (24 sums,
then dL/dt = R^-T S_g and dL/dR = R^-T [M1 + M2 + S_d c^T] through the quaternion matrix), fed the ORACLE backward's
dL_dmeans3D, dL_dcov3D and dL_dcolors, against torch.autograd of a float64 dense render that has the pose as a leaf.
Bar: the project's gradient bar, rel-inf <= 1e-4 over the seven components. Measured (max |diff| / max |truth|):
tiny 1.5e-6, indexed 1.6e-6, indexed_scale_mod 1.5e-6, cov_precomp 1.1e-6, colors_precomp 9.5e-6, frustum_edge 1.3e-6,
clamp_hits 1.3e-6, deg1 7.7e-7, nonunit_quat 2.0e-7 (the oracle's own fp32 gradients are what is left)."""
import numpy as np
import pytest

from tests import pose_ref

CASES = ["tiny", "indexed", "indexed_scale_mod", "cov_precomp", "colors_precomp", "frustum_edge", "clamp_hits", "deg1",
         "nonunit_quat"]
BAR = 1e-4


def rel_inf(a, b):
    return float(np.abs(a - b).max() / max(np.abs(b).max(), 1e-30))


@pytest.mark.parametrize("name", CASES)
def test_sums_and_epilogue_give_the_autograd_pose_gradient(name):
    r = pose_ref.reference(name)
    st = r["st"]
    assert int((st.radii > 0).sum()) >= 10 and st.num_rendered > 0                  # something is seen from this pose
    # the float64 render is the oracle's image (a pixel may differ where fp32 and float64 fall on two sides of a blend threshold)
    assert np.abs(r["img64"] - st.out_color).mean() < 1e-5
    assert np.abs(r["truth"]).min() > 0
    err = rel_inf(r["grad"], r["truth"])
    print(f"{name}: rel-inf {err:.3e}  truth {r['truth']}  got {r['grad']}")
    assert err <= BAR, (name, err)


def test_the_direction_term_and_the_covariance_term_matter():
    """Dropping gdir's rerouting or M2 misses the bar by orders of magnitude: the test above can tell the formula from its parts."""
    r = pose_ref.reference("tiny")
    inp, st, ref = r["inp"], r["st"], r["ref"]
    sig = pose_ref.sigma_of(inp)
    no_dir, _ = pose_ref.pose_grad_ref(r["pose"], inp["means3D"].numpy(), sig, st.radii, ref["dL_dmeans3D"], ref["dL_dcov3D"],
                                       np.zeros_like(r["gdir"]))
    no_cov, _ = pose_ref.pose_grad_ref(r["pose"], inp["means3D"].numpy(), sig, st.radii, ref["dL_dmeans3D"],
                                       np.zeros_like(ref["dL_dcov3D"]), r["gdir"])
    assert rel_inf(no_dir, r["truth"]) > 10 * BAR
    assert rel_inf(no_cov, r["truth"]) > 10 * BAR


def test_nonunit_pose_is_far_from_a_rotation():
    R, inv, _, _ = pose_ref.pose_camera(pose_ref.NONUNIT_POSE)
    assert np.abs(R @ R.T - np.eye(3)).max() > 0.2          # 1e-7 for a unit quaternion
    assert np.abs(inv - R.T).max() > 0.1


def test_contributions_sum_to_the_gradient():
    r = pose_ref.reference("tiny")
    np.testing.assert_allclose(r["contrib"].sum(0), r["grad"], rtol=1e-12, atol=0)
    assert (r["contrib"][r["st"].radii <= 0] == 0).all()
