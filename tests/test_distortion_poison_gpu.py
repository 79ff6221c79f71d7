"""-m gpu: the distortion map and the three-map backward under tests/poison.py's three fill bytes (0x00, 0xFF, 0x7F): no result may
depend on what scratch and outputs hold on entry, and no guard band may change. Driven the way tests/test_scratch_poison_gpu.py
drives render_depth and the depth / alpha backward: the outputs are bit-equal across the three runs (the codebook gradients of
the indexed backward, float atomics, are held to their bar on every run instead), and the 0xFF run is checked against the float64
reference with the family's own check, so that being equal to a wrong baseline is not enough."""
import numpy as np
import pytest

from tests import depth_grad_ref as dgr, depth_ref, distortion_ref as dr, gpu_util, poison
from tests.test_distortion_gpu import TRUTH_NAMES, _backward, _best, _render, _worst, check_forward
from tests.test_scratch_poison_gpu import SCATTERED, _forward_outputs

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("mode_name", ["raw", "ndc"])
@pytest.mark.parametrize("name", ["odd_size", "indexed"])
def test_render_distortion(hip, orc, name, mode_name):
    inp, cam, indexed = depth_ref.scene(name)
    st = depth_ref.oracle_state(name)
    fwd_names = ("radii", "depths", "n_contrib", "final_T")

    def run():
        fw = gpu_util.hip_forward(inp, cam, indexed)
        d, m = _render(fw, dr.MODES[mode_name])
        u = _forward_outputs(fw)
        return dict(distortion=d, moment=m, **{k: u[k] for k in fwd_names})

    poison.assert_independent(run, exact=("distortion", "moment") + fwd_names, check_bytes=(0xFF,),
                              check=lambda o: check_forward(name, mode_name, o, st, o["distortion"].astype(np.float64),
                                                            o["moment"].astype(np.float64)))


@pytest.mark.parametrize("image_gradient", ["none", "zeros"])
@pytest.mark.parametrize("name,mode_name", [("odd_size", "raw"), ("indexed", "ndc")])
def test_three_map_backward(hip, name, mode_name, image_gradient):
    """gD, gA and gL together; without an image gradient (no colour blend launch: the replay is the first to write the partial sums
    and their flags) and with one of zeros (the colour blend has flagged the slots before it)"""
    st, inp, cam, indexed = dgr.black_state(name)
    W, H = cam["W"], cam["H"]
    mode = dr.MODES[mode_name]
    gD, gA, gL = dgr.hashed_map(W, H, 1), dgr.hashed_map(W, H, 2), dr.gl_map(W, H)
    _, _, cands = dr.candidates(name, mode_name, True)
    dL = None if image_gradient == "none" else np.zeros((3, H, W), np.float32)

    def run():
        fw = gpu_util.hip_forward(inp, cam, indexed)
        _, moment = _render(fw, mode)
        return _backward(fw, dL, gD, gA, gL, moment, mode)

    def check(o):
        ref = _best(o, cands, TRUTH_NAMES, f"poisoned {name} {mode_name} {image_gradient}")
        _worst(o, ref, tuple(ref), 1e-4, f"poisoned {name} {mode_name} {image_gradient}:")

    probe = run()
    barred = {k: None for k in probe if indexed and k in SCATTERED}
    base = poison.assert_independent(run, exact=tuple(k for k in probe if k not in barred), barred=barred, check=check)
    assert np.abs(base["dL_dopacity"]).max() > 0 and not base["dL_dcolors"].any() and not base["dL_dsh"].any()
