"""c3dgs_amd -- MI355X (gfx950) rasterizer + VQ hot path of Compressed 3D Gaussian Splatting.

Drop-in for the reference's two native extensions and the Python directly around them:

    c3dgs_amd.rasterizer  <->  diff_gaussian_rasterization_no_camera (quaternion `extrinsic_vector` API)
    c3dgs_amd.rasterizer_matrix <-> diff_gaussian_rasterization / diff_gaussian_rasterization_camera (4x4 `extrinsic` API)
    c3dgs_amd.vq          <->  weighted_distance._C.weightedDistance + compression/vq.py
    c3dgs_amd.loss        <->  utils/loss_utils.py (l1_loss, ssim) + the fused QAT loss of finetune.py:48
    c3dgs_amd.metrics     <->  utils/image_utils.py:psnr + 4-D ssim + compress.py:render_and_eval (no gradient)
    c3dgs_amd.sensitivity <->  compress.py:calc_importance_experimental (camera-sharded)
    c3dgs_amd.encode      <->  GaussianModel._sort_morton / mortonEncode
    c3dgs_amd.knn         <->  simple_knn._C.distCUDA2 (initial scales of a point cloud in load_ply)
    c3dgs_amd.ply         <->  the plyfile reads / writes of GaussianModel.load_ply / save_ply
    c3dgs_amd.model       <->  GaussianModel getters + FakeQuantize modules + render() glue + adaptive density control
                               (scene/gaussian_model.py)
    c3dgs_amd.pipeline    <->  train.py / finetune.py / compress.py drivers
    c3dgs_amd.optim       <->  the torch.optim.Adam step of the QAT loop (finetune.py:65-66), one fused launch; beyond the
                               reference, SparseGaussianAdam: the same step over the Gaussians a view saw only

Beyond the reference, the rasterizer also returns depth / accumulated-opacity / median-depth maps, per-Gaussian blend statistics and
error scores and the exact pose gradient; with GaussianRasterizationSettings(depth_grad=True) the depth and alpha maps carry
gradient (csrc/render_maps_backward.hip), which GaussianModel.render(depth_grad=True) and pipeline.train(lambda_depth=,
lambda_alpha=) use for depth and silhouette losses; GaussianRasterizationSettings(antialiasing=True) / PipelineParams(antialiasing=True)
compensate every opacity for the rasterizer's 0.3 px^2 low-pass (csrc/aa_opacity.hip), upstream 3DGS's `antialiasing`.
pipeline.train(strategy="mcmc", cap_max=N) trains towards a hard budget of Gaussians ("3DGS as Markov Chain Monte Carlo":
GaussianModel.relocate_gs / add_new_gs / add_position_noise on csrc/mcmc.hip; thin entries in c3dgs_amd.mcmc).
c3dgs_amd.bilagrid (BilateralGrid, ExposureModel on csrc/bilagrid.hip) is a per-image colour model, gsplat's bilateral grid and
upstream 3DGS's `exposure`, which pipeline.train(bilagrid=...) trains and pipeline.finetune(bilagrid=...) applies frozen.
GaussianModel.compute_3D_filter(cameras) / pipeline.train(filter_3d=True) give every Gaussian Mip-Splatting's 3D smoothing filter,
a minimum world-space size from the training cameras' sampling rates that render() applies (c3dgs_amd.filter3d on csrc/filter3d.hip).

The numeric work runs in c3dgs_amd/libc3dgs_hip.so (include/c3dgs_hip.h); build it with
`python -m c3dgs_amd.build`.  There is no CPU fallback.
"""
import sys
import types

from . import bilagrid, encode, filter3d, knn, loss, mcmc, metrics, model, optim, ply, rasterizer, rasterizer_matrix, sensitivity, vq  # noqa: F401
from .rasterizer import (GaussianRasterizationSettings, GaussianRasterizer, GaussianRasterizerIndexed,  # noqa: F401
                         getProjectionMatrix, mat_to_quat, quat_to_mat, rasterize_gaussians,
                         rasterize_gaussians_indexed, rasterize_gaussians_indexed_camera,
                         rasterize_gaussians_camera_exact, rasterize_gaussians_indexed_camera_exact)
from .vq import (CompressionSettings, VectorQuantize, compress_color, compress_covariance, compress_gaussians,  # noqa: F401
                 join_features, vq_features, weightedDistance)

from .loss import l1_loss, l1_ssim_loss, ssim  # noqa: F401,E402
from .encode import morton_codes, morton_order  # noqa: F401,E402
from .knn import distCUDA2  # noqa: F401,E402

__version__ = "0.1.0"


def install_as_reference_modules():
    """Register this package under the module names the reference imports
    (scene/gaussian_model.py:39,43-44, compression/vq.py:12), so the reference's Python runs unmodified."""
    sys.modules["diff_gaussian_rasterization_no_camera"] = rasterizer
    for name in ("diff_gaussian_rasterization", "diff_gaussian_rasterization_camera"):   # the matrix-`extrinsic` siblings
        sys.modules[name] = rasterizer_matrix
    wd = types.ModuleType("weighted_distance")
    wdc = types.ModuleType("weighted_distance._C")
    wdc.weightedDistance = lambda coefs, codebook: weightedDistance(coefs, codebook)
    wd._C = wdc
    sys.modules["weighted_distance"] = wd
    sys.modules["weighted_distance._C"] = wdc
    sk = types.ModuleType("simple_knn")
    skc = types.ModuleType("simple_knn._C")
    skc.distCUDA2 = distCUDA2
    sk._C = skc
    sys.modules["simple_knn"] = sk
    sys.modules["simple_knn._C"] = skc
