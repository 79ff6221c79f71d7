"""-m gpu: the HIP rasterizer on what a TRAINED scene holds and synth-v1 does not (tests/cases.py: EDGE_GAUSSIAN_CASES) --
large splats whose opacity saturated at 1 (and raw opacities above it), needles, flat discs (thickness down to exactly 0),
quaternions whose norm drifted, floaters centimetres from the camera on either side of the z <= 0.01 cull.

Forward, every case: test_raster_gpu._check_forward unchanged -- radii, rectangles, depths, means2D, conic, colours and keys
bit-exact, the image bars with the existing flip cap.

Backward:
  * opaque_big, discs, unnorm_quat -- the oracle is within 2e-5 of float64 there (tests/test_edge_gaussians_cpu.py), so the
    kernels are held to the oracle at the 1e-4 of test_backward_parity (fullsize.check_grads);
  * needles, needles_long, indexed_needles, near_camera -- on needles the reference's OWN fp32 formula leaves 1e-4 (det = a c - b^2
    of cov2D cancels; its deviation d_ref from float64 reaches 2e-3), so a fixed bar would fail a correct kernel or hide a wrong
    one. The kernels are compared with the float64 truth T (tests/dense_ref.py), per tensor:
        ||kernel - T||_inf <= max(1e-4 ||T||_inf, 4 ||oracle - T||_inf),      both sides measured at run time.
    The factor 4 is test_loss_content_classes_...'s, for the same reason: two fp32 orders of one cancelling expression may err
    in opposite directions (x 2), and the kernel rounds elsewhere than the reference's order -- FMA, exp2 of a pre-scaled conic,
    rcp (x 2). Flipped pixels keep the treatment of check_grads: each proven, 5 x the bar for tensors that share a tile with one.
Anisotropy of 40 and more (radii of thousands of pixels) is out of scope: there two legitimate fp32 evaluations of the
reference's formula differ by 0.2 in the image, and hundreds of blend decisions flip.

Observed on an MI355X, rel-inf against T: kernel deviation / d_ref = ratio (the first measurements of the kernels in this
regime; no pixel flipped in any case; where 4 d_ref < 1e-4 the 1e-4 floor is the bar):
                      needles                     needles_long                indexed_needles             near_camera
    dL_dmeans2D       1.12e-05 / 7.06e-06 = 1.59  1.36e-05 / 7.38e-06 = 1.84  2.23e-05 / 1.95e-05 = 1.14  1.50e-06 / 1.40e-06 = 1.07
    dL_dcolors        1.57e-05 / 1.48e-05 = 1.06  1.17e-05 / 1.76e-05 = 0.67  4.17e-06 / 4.30e-06 = 0.97  4.82e-07 / 4.78e-07 = 1.01
    dL_dopacity       9.47e-06 / 1.06e-05 = 0.90  1.00e-05 / 3.45e-05 = 0.29  2.30e-06 / 2.22e-06 = 1.04  3.88e-07 / 5.50e-07 = 0.71
    dL_dmeans3D       6.54e-05 / 2.40e-05 = 2.72  1.01e-04 / 3.28e-05 = 3.08  1.71e-05 / 1.46e-04 = 0.12  1.29e-06 / 1.29e-06 = 1.00
    dL_dcov3D         4.37e-05 / 3.38e-05 = 1.30  3.50e-05 / 1.60e-05 = 2.18  1.84e-05 / 2.73e-05 = 0.67  2.23e-06 / 3.60e-06 = 0.62
    dL_dsh            1.44e-05 / 1.36e-05 = 1.06  1.13e-05 / 1.70e-05 = 0.67  3.87e-06 / 4.05e-06 = 0.96  4.63e-07 / 4.70e-07 = 0.99
    dL_dscales        5.47e-04 / 1.70e-04 = 3.23  6.93e-04 / 2.40e-04 = 2.88  1.84e-04 / 1.13e-03 = 0.16  3.21e-06 / 2.77e-06 = 1.16
    dL_dscale_factors -                           -                           1.42e-04 / 1.18e-03 = 0.12  -
    dL_drotations     1.27e-03 / 1.05e-03 = 1.20  1.32e-03 / 4.96e-04 = 2.67  2.03e-04 / 1.09e-03 = 0.19  1.50e-06 / 1.19e-06 = 1.26
The kernels are never further from the truth than 3.3 x the reference's own formula, and on indexed_needles' geometry tensors
5-8 x closer than it. The largest ratios are on the needle cases' dL_dscales / dL_dmeans3D, which pass through the conic
gradient's 1/det^2 terms (backward_preprocess.hip). Nothing is outside 4 x, every forward quantity is bit-exact, and no kernel
had to change. near_camera's norms are carried by the floaters themselves (their float64 gradients are ~15 x the other rows').

The non-indexed backward on opaque_big and needles_long is bitwise reproducible.
"""
import numpy as np
import pytest

from tests import cases, fullsize, gpu_util, synth
from tests.test_raster_gpu import GRAD_TOL, _check_forward

pytestmark = pytest.mark.gpu

AGAINST_FLOAT64 = [c for c in cases.EDGE_GAUSSIAN_CASES if c not in cases.EDGE_WITHIN_TOL]
FACTOR = 4.0


@pytest.mark.parametrize("name", cases.EDGE_GAUSSIAN_CASES)
def test_edge_forward_parity(hip, orc, name):
    inp, cam, indexed = cases.make_case(name)
    st = cases.oracle_forward(inp, cam)
    cases.edge_guard(name, st)
    _check_forward(gpu_util.unpack(gpu_util.hip_forward(inp, cam, indexed)), st)


@pytest.mark.parametrize("name", cases.EDGE_WITHIN_TOL)
def test_edge_backward_parity_with_the_oracle(hip, orc, name):
    inp, cam, indexed = cases.make_case(name)
    st = cases.oracle_forward(inp, cam)
    cases.edge_guard(name, st)
    dL = synth.grad_image(cam["W"], cam["H"]).numpy()
    ref = orc.rasterize_backward(st, dL)
    fw = gpu_util.hip_forward(inp, cam, indexed)
    got = gpu_util.hip_backward(fw, dL)
    for k in ("dL_dmeans3D", "dL_dopacity", "dL_dscales", "dL_drotations", "dL_dsh"):
        assert np.abs(got[k]).max() > 0, k
    fullsize.check_grads(st, gpu_util.unpack(fw), got, ref, GRAD_TOL, name)


@pytest.mark.parametrize("name", AGAINST_FLOAT64)
def test_edge_backward_within_four_times_the_references_own_error(hip, orc, name):
    e = cases.edge_reference(name)
    st, truth = e["st"], e["truth"]
    fw = gpu_util.hip_forward(e["inp"], e["cam"], e["indexed"])
    got = gpu_util.hip_backward(fw, e["dL"])
    tols = fullsize.truth_tols(e["d_ref"], GRAD_TOL, FACTOR)
    assert set(got) <= set(tols)
    for k, v in got.items():
        dev = gpu_util.rel_inf(v, truth[k])
        d = e["d_ref"][k]
        print(f"{name:16s} {k:18s} kernel {dev:.2e}  d_ref {d:.2e}  kernel/d_ref {dev / max(d, 1e-30):6.2f}  bar {tols[k]:.2e}")
    n_flip = fullsize.check_grads(st, gpu_util.unpack(fw), got, e["ref"], GRAD_TOL, name, target=truth, tols=tols)
    print(name, n_flip, "flipped pixels")


@pytest.mark.parametrize("name", ["opaque_big", "needles_long"])
def test_edge_backward_is_deterministic(hip, name):
    """No global float atomics on the non-indexed path: two runs are bitwise identical, also with clamped and needle blends."""
    inp, cam, indexed = cases.make_case(name)
    assert not indexed
    dL = synth.grad_image(cam["W"], cam["H"]).numpy()
    fw = gpu_util.hip_forward(inp, cam, indexed)
    g1 = gpu_util.hip_backward(fw, dL)
    g2 = gpu_util.hip_backward(fw, dL)
    assert np.abs(g1["dL_dmeans3D"]).max() > 0
    for k in g1:
        np.testing.assert_array_equal(g1[k].view(np.uint32), g2[k].view(np.uint32), err_msg=k)
