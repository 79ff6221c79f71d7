"""-m gpu: the covariance -> scale / rotation chain of csrc/gsgrad.hpp and its restatement in the hot kernel are one chain.

filter3d_apply_backward_kernel calls cov3d_grad_to_scale_rot() in fp32; backward_preprocess_kernel keeps the same operations
written out in the same order (called, it measured slower: profiles/gsgrad/README.md). Both files are built without
contraction, so on the same dL/dSigma, scales and rotations they give the same values, and an edit to one side alone fails
here: the rasterizer's
dL_drotations as they are, its dL_dscales (with respect to the scaled scale, the reference's semantics) times the float32
scale_modifier the filter kernel multiplies by. Values, not bit patterns: the filter kernel adds its `+ 0` opacity term, which
turns a -0 into +0."""
import ctypes as C

import numpy as np
import pytest
import torch

from tests import cases, gpu_util, synth

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("scale_modifier", [1.0, 1.7])
def test_filter_and_rasterizer_share_the_covariance_chain(hip, scale_modifier):
    from c3dgs_amd import _lib, filter3d
    inp, cam, indexed = cases.make_case("tiny")
    assert not indexed and inp["cov3D_precomp"] is None
    inp = dict(inp, scale_modifier=scale_modifier)
    fw = gpu_util.hip_forward(inp, cam, indexed)                                  # the pybind-order entries: nothing skipped
    got = gpu_util.hip_backward(fw, synth.grad_image(cam["W"], cam["H"]).numpy())
    d_cov = torch.as_tensor(got["dL_dcov3D"]).cuda().contiguous()
    n_rows = int((d_cov != 0).any(1).sum())
    assert n_rows >= 10, n_rows

    scales, rotations = inp["scales"].cuda().contiguous(), inp["rotations"].cuda().contiguous()
    opac = inp["opacities"].cuda().contiguous()
    r, t, _ = filter3d._rows(opacities=opac, scales=scales, rotations=rotations, filter_3D=torch.zeros_like(opac).reshape(-1),
                             scale_modifier=scale_modifier, scale_factors=None, g_indices=None, visible=None, rank=None)
    d_scales, d_rot = torch.zeros_like(scales), torch.zeros_like(rotations)
    gr = _lib.Filter3DGrads(dL_dcov3D=d_cov.data_ptr(), dL_dopacity_out=None, dL_dscales=d_scales.data_ptr(),
                            dL_drotations=d_rot.data_ptr())
    _lib.check(_lib.lib().c3dgs_filter3d_apply_backward(C.byref(r), C.byref(gr), None))
    torch.cuda.synchronize()

    want_rot = torch.as_tensor(got["dL_drotations"])
    want_scales = torch.as_tensor(got["dL_dscales"]) * torch.tensor(np.float32(scale_modifier))
    assert want_scales.dtype == torch.float32 and int((want_rot != 0).any(1).sum()) >= 10
    bad_r, bad_s = (d_rot.cpu() != want_rot), (d_scales.cpu() != want_scales)
    for name, bad, a, b in (("dL_drotations", bad_r, d_rot.cpu(), want_rot), ("dL_dscales", bad_s, d_scales.cpu(), want_scales)):
        if bad.any():
            i = bad.nonzero()[0].tolist()
            print(f"{name}: {int(bad.sum())} elements differ, first {i}: filter {a[tuple(i)].item()!r} rasterizer {b[tuple(i)].item()!r}")
    assert torch.equal(d_rot.cpu(), want_rot)
    assert torch.equal(d_scales.cpu(), want_scales)
