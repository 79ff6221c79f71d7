"""-m gpu: the forward whose small launches behind preprocess are merged (csrc/radix_sort.hip os_hist_scan_kernel: the id-order scan
with its host store of num_rendered in workgroup 0, the depth sort's histograms in the others) against the CPU oracle, through
the rasterizers that take the camera as a 7-element POSE on the device -- the indexed one with the camera gradient and the
non-indexed one. Two sizes: 40 x 24 pixels with 300 Gaussians (one depth-sort tile, 3 x 2 tiles) and 64 x 64 with 5000 (many
256-Gaussian workgroups under the scan). num_rendered, radii, the depth order, the sorted point list, the ranges: equal; the
image: the bars of tests/test_raster_gpu.py. A second call follows an in-place `.data` write to the pose and must render the new
pose: the camera is rebuilt on the device from the pose's live values on every call."""
import numpy as np
import pytest
import torch

from tests import cases, gpu_util, synth
from tests.test_raster_gpu import _check_forward

pytestmark = pytest.mark.gpu

SIZES = {"40x24_p300": dict(W=40, H=24, P=300, focal=30.0, scale_median=0.2, zmin=2.0, zmax=6.0),
         "64x64_p5000": dict(W=64, H=64, P=5000, focal=50.0, scale_median=0.05, zmin=2.0, zmax=9.0)}
POSES = [(0.05, -0.03, 0.02, 0.99, 0.1, -0.05, 0.2), (-0.04, 0.06, 0.01, 0.98, -0.25, 0.15, 0.6)]


class _Ctx:
    """what _autograd_forward needs of an autograd context; keeps the forward's buffers for unpacking"""
    def save_for_backward(self, *tensors):
        self.saved = tensors

    def set_materialize_grads(self, flag):
        pass

    def mark_non_differentiable(self, *tensors):
        pass


def _render(hip, indexed, inp, intr, pose, W, H):
    """the forward of GaussianRasterizerIndexed(optimize_camera=True) / GaussianRasterizer for the pose tensor `pose` -> unpacked"""
    from c3dgs_amd import rasterizer as rz
    dev = pose.device
    d = lambda k: gpu_util.to_dev(inp.get(k), dev)
    rs = hip.GaussianRasterizationSettings(intrinsic=intr, extrinsic_vector=pose, bg=d("bg"), scale_modifier=1.0, sh_degree=3,
                                           prefiltered=False, debug=False, clamp_color=True)
    ctx = _Ctx()
    E = torch.Tensor([])
    color, radii = rz._autograd_forward(ctx, indexed, d("means3D"), d("shs"), d("sh_indices") if indexed else None,
                                        d("g_indices") if indexed else None, E, d("opacities"), d("scales"),
                                        d("scale_factors") if indexed else None, d("rotations"), E, rs, pose)
    torch.cuda.synchronize()
    geom, binning, img = ctx.saved[9], ctx.saved[10], ctx.saved[11]
    return gpu_util.unpack(dict(num_rendered=ctx.num_rendered, color=color, radii=radii, geom=geom, binning=binning, img=img, W=W, H=H))


@pytest.mark.parametrize("indexed", [True, False], ids=["indexed_camera", "non_indexed"])
@pytest.mark.parametrize("size", list(SIZES))
def test_forward_with_merged_launches_matches_oracle_and_follows_the_pose(hip, orc, size, indexed):
    s = SIZES[size]
    W, H = s["W"], s["H"]
    intr, ev0 = synth.camera(W, H, s["focal"], extrinsic_vector=POSES[0])
    sc = synth.scene(s["P"], W, H, s["focal"], seed=21, sh_degree=3, scale_median=s["scale_median"], zmin=s["zmin"], zmax=s["zmax"])
    inp = dict(bg=torch.tensor([0.2, 0.4, 0.1]), means3D=sc["means3D"], opacities=sc["opacities"], shs=sc["shs"], colors_precomp=None,
               scales=sc["scales"], rotations=sc["rotations"], cov3D_precomp=None, scale_factors=None, sh_indices=None,
               g_indices=None, degree=3, scale_modifier=1.0, prefiltered=False, clamp_color=True)
    if indexed:
        ix = synth.index_scene(sc, shs_extra=64, gs_extra=64)
        inp.update(shs=ix["shs"], scales=ix["scales"], rotations=ix["rotations"], scale_factors=ix["scale_factors"],
                   sh_indices=ix["sh_indices"], g_indices=ix["g_indices"])
    pose = ev0.clone().cuda()
    images = []
    for k, ev in enumerate(POSES):
        if k:
            pose.data.copy_(torch.tensor(ev, dtype=torch.float32))           # in place: same tensor, same storage
        st = cases.oracle_forward(inp, orc.camera(intr.numpy(), np.asarray(ev, dtype=np.float32)))
        assert st.num_rendered > 0 and int((st.radii > 0).sum()) >= s["P"] // 4, (st.num_rendered, int((st.radii > 0).sum()))
        got = _render(hip, indexed, inp, intr, pose, W, H)
        _check_forward(got, st)
        images.append(got["out_color"])
    assert np.abs(images[0] - images[1]).max() > 1e-2, "the two poses must give different images"
