"""-m gpu: the normal family under tests/poison.py's three fill bytes (0x00, 0xFF, 0x7F): no result may depend on what scratch and
outputs hold on entry, and no guard band may change. Driven the way tests/test_distortion_poison_gpu.py drives the distortion
family: the outputs are bit-equal across the three runs (the codebook gradients of the indexed backward, float atomics, are held
to their bar on every run instead), and the 0xFF run is checked against the float64 reference with the family's own check, so that
being equal to a wrong baseline is not enough."""
import numpy as np
import pytest
import torch

from tests import depth_grad_ref as dgr, depth_ref, distortion_ref as dr, gpu_util, normal_ref as nr, poison
from tests.test_normal_gpu import TRUTH_NAMES, _backward, _best, _normals, _render, _worst, check_forward, check_gaussian_normals
from tests.test_scratch_poison_gpu import SCATTERED, _forward_outputs

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("name", ["odd_size", "indexed"])
def test_gaussian_normals_and_render_normal(hip, orc, name):
    inp, cam, indexed = depth_ref.scene(name)
    st = depth_ref.oracle_state(name)
    fwd_names = ("radii", "depths", "n_contrib", "final_T")

    def run():
        fw = gpu_util.hip_forward(inp, cam, indexed)
        nb = _normals(fw)
        u = _forward_outputs(fw)
        return dict(normals=nb, normal=_render(fw, nb), **{k: u[k] for k in fwd_names})

    def check(o):
        ref = check_gaussian_normals(f"poisoned {name}", inp, cam["viewmatrix"], o["normals"])
        check_forward(f"poisoned {name}", o, st, o["normal"].astype(np.float64), ref["n"])

    poison.assert_independent(run, exact=("normals", "normal") + fwd_names, check_bytes=(0xFF,), check=check)


@pytest.mark.parametrize("image_gradient", ["none", "zeros"])
@pytest.mark.parametrize("name,mode_name", [("odd_size", "raw"), ("indexed", "ndc")])
def test_four_map_backward(hip, name, mode_name, image_gradient):
    """gD, gA, gL and gN together; without an image gradient (no colour blend launch: the replay is the first to write the partial
    sums and their flags) and with one of zeros (the colour blend has flagged the slots before it)"""
    from c3dgs_amd import rasterizer
    st, inp, cam, indexed = dgr.black_state(name)
    W, H = cam["W"], cam["H"]
    mode = dr.MODES[mode_name]
    gD, gA, gL, gN = dgr.hashed_map(W, H, 1), dgr.hashed_map(W, H, 2), dr.gl_map(W, H), nr.gn_map(W, H)
    _, _, cands = nr.candidates(name, "gD+gA+gL+gN", mode_name)
    dL = None if image_gradient == "none" else np.zeros((3, H, W), np.float32)

    def run():
        fw = gpu_util.hip_forward(inp, cam, indexed)
        nb = _normals(fw)
        moment = rasterizer._C.render_distortion(st.P, W, H, fw["num_rendered"], fw["geom"], fw["binning"], fw["img"], mode)[1]
        return _backward(fw, dL, gN, nb, gD, gA, gL, moment, mode)

    def check(o):
        ref = _best(o, cands, TRUTH_NAMES, f"poisoned {name} {mode_name} {image_gradient}")
        _worst(o, ref, tuple(ref), 1e-4, f"poisoned {name} {mode_name} {image_gradient}:")

    probe = run()
    barred = {k: None for k in probe if indexed and k in SCATTERED}
    base = poison.assert_independent(run, exact=tuple(k for k in probe if k not in barred), barred=barred, check=check)
    assert np.abs(base["dL_drotations"]).max() > 0 and not base["dL_dcolors"].any() and not base["dL_dsh"].any()


def test_depth_to_normal_pair(hip):
    from c3dgs_amd import normals
    label, z64, tfx, tfy = nr.stencil_inputs()[0]
    H, W = z64.shape
    intr = torch.zeros(3, 3)
    intr[0, 0], intr[1, 1], intr[0, 2], intr[1, 2] = 2 * np.arctan(tfx), 2 * np.arctan(tfy), W, H
    g = torch.from_numpy(nr.gn_map(W, H).astype(np.float32)).cuda()

    def run():
        z = torch.from_numpy(z64.astype(np.float32)).cuda().requires_grad_()
        n = normals.depth_to_normal(z, intr)
        (n * g).sum().backward()
        return dict(normal=n.detach(), dz=z.grad)

    def check(o):
        from c3dgs_amd.rasterizer import _intrinsic_scalars
        k = nr.stencil_bars()["forward"][1]
        t = _intrinsic_scalars(intr)[0][:2]                     # the tangents the library receives
        e = np.abs(o["normal"].astype(np.float64) - nr.depth_to_normal(z64, *t)).max() / (nr.U * max(W / (2 * t[0]), H / (2 * t[1])))
        assert e <= k, e

    poison.assert_independent(run, exact=("normal", "dz"), check_bytes=(0xFF,), check=check)
