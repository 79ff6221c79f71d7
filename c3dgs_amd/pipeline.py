"""The drivers either side of the hot path: the QAT fine-tuning loop and the compression run.

    train(...)               <- train.py:15-173          (optimise a scene from a point cloud, with adaptive density control)
    finetune(...)            <- finetune.py:10-66        (hot loop C of SURVEY.md section 3)
    run_vq(...)              <- compress.py:202-303      (sensitivity -> prune + VQ -> fine-tune -> npz [-> evaluation])
    OptimizationParams / CompressionParams / ModelParams <- arguments/__init__.py:43-136 (defaults only, no argparse)

c3dgs_amd.scene.Scene builds a scene from a COLMAP / Blender / Dust3r dataset; the drivers take anything with
`getTrainCameras()` -> sequence of cameras carrying `intrinsic`, `extrinsic_vector` and `original_image` (a plain list
of such cameras is accepted too), and `loaded_iter` (default 0). Everything numeric runs in the package's HIP kernels:
GaussianModel.render (fused getters + rasterizer), the fused L1+SSIM loss, the fused Adam.
"""
import gc
import json
import os
import time
from random import randint
from typing import Optional

import torch

from . import bilagrid as _bilagrid
from . import loss as _loss
from . import metrics as _metrics
from . import normals as _normals
from . import optim as _optim
from . import sensitivity as _sensitivity
from .vq import CompressionSettings, compress_gaussians


class OptimizationParams:
    """arguments/__init__.py:116-136."""

    def __init__(self, **overrides):
        self.iterations = 30_000
        self.position_lr_init = 0.00016
        self.position_lr_final = 0.0000016
        self.position_lr_delay_mult = 0.01
        self.position_lr_max_steps = 30_000
        self.feature_lr = 0.0025
        self.opacity_lr = 0.05
        self.scaling_lr = 0.005
        self.rotation_lr = 0.001
        self.percent_dense = 0.01
        self.lambda_dssim = 0.2
        self.densification_interval = 100
        self.opacity_reset_interval = 3000
        self.densify_from_iter = 500
        self.densify_until_iter = 15_000
        self.densify_grad_threshold = 0.0002
        self.random_background = False
        self.not_quantization_aware = False
        self.optimizer_type = "default"      # "sparse_adam": GaussianModel.training_setup builds optim.SparseGaussianAdam (not in the reference)
        _apply(self, overrides)


class ModelParams:
    """arguments/__init__.py:43-73: where a scene is read from and written to (c3dgs_amd.scene.Scene reads these)."""

    def __init__(self, **overrides):
        self.sh_degree = 3
        self.source_path = ""
        self.model_path = ""
        self.images = "images"
        self.resolution = -1
        self.white_background = False
        self.data_device = "cuda"
        self.eval = False
        _apply(self, overrides)

    def extract(self, args=None):
        """The reference's extract() without its argparse half: the source path made absolute."""
        self.source_path = os.path.abspath(self.source_path)
        return self


class CompressionParams:
    """arguments/__init__.py:85-113."""

    def __init__(self, **overrides):
        self.load_iteration = -1
        self.finetune_iterations = 5000
        self.color_codebook_size = 2 ** 12
        self.color_importance_include = 0.6 * 1e-6
        self.color_importance_prune = 0.0
        self.color_cluster_iterations = 100
        self.color_decay = 0.8
        self.color_batch_size = 2 ** 18
        self.color_weights_per_param = False
        self.color_compress_non_dir = True
        self.not_compress_color = False
        self.gaussian_codebook_size = 2 ** 12
        self.gaussian_importance_include = 0.3 * 1e-5
        self.gaussian_cluster_iterations = 800
        self.gaussian_decay = 0.8
        self.gaussian_batch_size = 2 ** 20
        self.not_compress_gaussians = False
        self.not_sort_morton = False
        self.prune_threshold = 0.
        self.output_vq = "./eval_vq"
        self.start_checkpoint = ""
        _apply(self, overrides)


def _apply(obj, overrides):
    for k, v in overrides.items():
        if not hasattr(obj, k):
            raise TypeError(f"{type(obj).__name__} has no parameter {k!r}")
        setattr(obj, k, v)


def _train_cameras(scene):
    return list(scene.getTrainCameras()) if hasattr(scene, "getTrainCameras") else list(scene)


def finetune(scene, dataset, opt, comp, pipe, debug_from=-1, log=None, *, prune_interval=0, prune_min_opacity=0.005,
             prune_min_views=0, bilagrid=None, lambda_dist=0.0, dist_near_far=None, dist_from_iter=0, lambda_normal=0.0,
             normal_from_iter=0):
    """finetune.py:10-66. One camera per iteration, drawn without replacement from a stack that is refilled when empty
    (`pop(randint(0, len - 1))` on Python's `random`, like the reference); render -> (1 - l) L1 + l (1 - SSIM) ->
    backward -> learning-rate update -> Adam step (not after the last iteration).

    The reference reads `loss.item()` every iteration for its progress bar, which drains the GPU queue each time; here
    the losses stay on the device and the same exponential moving average (0.4 / 0.6) is evaluated every 10 iterations.
    Returns that average after the last iteration. `dataset` needs `white_background` only; `log(iteration, ema)` is
    called where the reference updates its progress bar.

    `prune_interval` = N > 0 (not in the reference; 0 changes nothing): after the optimizer step of every N-th iteration the
    Gaussians with sigmoid(_opacity) < `prune_min_opacity` are removed, on the raw parameter (get_opacity would move the opacity
    observer), with prune_points_indexed on an indexed model (unreferenced codebook rows go with them) and prune_points
    otherwise; `log(iteration, ema)` is called once more after each prune.
    `prune_min_views` = V > 0 (0 changes nothing): when `prune_interval` fires, the Gaussians that
    GaussianModel.contribution_stats over the training cameras sees blended in fewer than V views go as well
    (prune_by_contribution): what no training view blends costs sort, list and codebook space in every view. The statistics
    pass renders every training camera once but leaves the QAT observers as it found them (contribution_stats restores them).
    `bilagrid` (not in the reference; None changes nothing): a trained bilagrid.BilateralGrid whose row k belongs to camera k of
    the training list. The loss then sees bilagrid.slice(render, k), so the fine-tuning does not fight the exposure differences
    the grids had absorbed. The grids are frozen: no optimizer, requires_grad is switched off for the call and restored.
    `lambda_dist`, `dist_near_far`, `dist_from_iter`: train()'s depth-distortion term (see there; 0, the default, changes
    nothing), from the `dist_from_iter`-th iteration of this call on.
    `lambda_normal`, `normal_from_iter`: train()'s normal-consistency term (see there; 0, the default, changes nothing), from the
    `normal_from_iter`-th iteration of this call on. Both terms together still cost one blend replay per backward."""
    gaussians = scene.gaussians if hasattr(scene, "gaussians") else dataset.gaussians
    if lambda_normal < 0:
        raise ValueError("finetune: lambda_normal must be >= 0")
    dist = (_distortion_option("finetune", lambda_dist, dist_near_far), float(lambda_dist), int(dist_from_iter),
            float(lambda_normal), int(normal_from_iter))
    if bilagrid is not None:
        camera_index = _camera_indices(_train_cameras(scene), bilagrid)
        grids_required_grad = bilagrid.grids.requires_grad
        bilagrid.grids.requires_grad_(False)
        try:
            return _finetune(scene, dataset, opt, comp, pipe, debug_from, log, prune_interval, prune_min_opacity, prune_min_views,
                             gaussians, bilagrid, camera_index, dist)
        finally:
            bilagrid.grids.requires_grad_(grids_required_grad)
    return _finetune(scene, dataset, opt, comp, pipe, debug_from, log, prune_interval, prune_min_opacity, prune_min_views, gaussians,
                     None, None, dist)


def _distortion_option(who, lambda_dist, dist_near_far):
    """-> what render(distortion=) takes for the depth-distortion term of train() / finetune(): False when the weight is 0"""
    if lambda_dist < 0:
        raise ValueError(f"{who}: lambda_dist must be >= 0")
    if lambda_dist == 0:
        return False
    from .rasterizer import _distortion_setting
    return _distortion_setting(True if dist_near_far is None else dist_near_far)


def _camera_indices(cameras, bilagrid):
    """{id(camera): its index in the training list}, the row of `bilagrid` it owns"""
    if bilagrid.num_cameras != len(cameras):
        raise ValueError(f"bilagrid: {bilagrid.num_cameras} grids for {len(cameras)} training cameras")
    return {id(cam): k for k, cam in enumerate(cameras)}


def _finetune(scene, dataset, opt, comp, pipe, debug_from, log, prune_interval, prune_min_opacity, prune_min_views, gaussians,
              bilagrid, camera_index, dist=(False, 0.0, 0, 0.0, 0)):
    distortion, lambda_dist, dist_from_iter, lambda_normal, normal_from_iter = dist
    first_iter = int(getattr(scene, "loaded_iter", 0) or 0)
    max_iter = first_iter + comp.finetune_iterations
    bg_color = [1, 1, 1] if getattr(dataset, "white_background", False) else [0, 0, 0]
    background = torch.tensor(bg_color, dtype=torch.float32, device=gaussians.device)

    gaussians.training_setup(opt)
    gaussians.update_learning_rate(first_iter)

    viewpoint_stack = None
    ema_loss_for_log = 0.0
    pending = []
    first_iter += 1
    for iteration in range(first_iter, max_iter + 1):
        if not viewpoint_stack:
            viewpoint_stack = _train_cameras(scene).copy()
        viewpoint_cam = viewpoint_stack.pop(randint(0, len(viewpoint_stack) - 1))
        if (iteration - 1) == debug_from:
            pipe.debug = True
        with_dist = distortion is not False and iteration - first_iter >= dist_from_iter
        with_normal = lambda_normal > 0 and iteration - first_iter >= normal_from_iter
        render_pkg = gaussians.render(viewpoint_cam, pipe, background, **({"distortion": distortion} if with_dist else {}),
                                      **({"normal": True} if with_normal else {}))
        image = render_pkg["render"]
        if bilagrid is not None:
            image = bilagrid.slice(image, camera_index[id(viewpoint_cam)])
        gt_image = viewpoint_cam.original_image.to(image.device)
        loss = _loss.l1_ssim_loss(image, gt_image, opt.lambda_dssim)
        if with_dist:
            loss = loss + lambda_dist * render_pkg["distortion"].mean()
        if with_normal:
            loss = loss + lambda_normal * _normals.normal_consistency(render_pkg["depth"], render_pkg["alpha"], render_pkg["normal"],
                                                                      viewpoint_cam.intrinsic)
        loss.backward()
        gaussians.update_learning_rate(iteration)
        pending.append(loss.detach())
        if iteration % 10 == 0 or iteration == max_iter:
            for v in torch.stack(pending).tolist():                 # one host read per 10 iterations
                ema_loss_for_log = 0.4 * v + 0.6 * ema_loss_for_log
            pending = []
            if log is not None:
                log(iteration, ema_loss_for_log)
        if iteration < max_iter:
            gaussians.optimizer.step()
            gaussians.optimizer.zero_grad(set_to_none=True)
            if prune_interval > 0 and (iteration - first_iter + 1) % prune_interval == 0:
                with torch.no_grad():
                    mask = (torch.sigmoid(gaussians._opacity.detach()) < prune_min_opacity).squeeze(-1)
                    if gaussians.is_color_indexed or gaussians.is_gaussian_indexed:
                        gaussians.prune_points_indexed(mask)
                    else:
                        gaussians.prune_points(mask)
                if prune_min_views > 0:
                    stats = gaussians.contribution_stats(_train_cameras(scene), pipe, background)
                    gaussians.prune_by_contribution(stats, min_views=prune_min_views)
                if gaussians.filter_3D is not None:                  # the survivors carry their values; a pruned scene is re-measured
                    gaussians.compute_3D_filter(_train_cameras(scene))
                if log is not None:
                    log(iteration, ema_loss_for_log)
    return ema_loss_for_log


def train(scene, dataset, opt, pipe, log=None, extent=None, camera_stride=10, degree_up_iter=1000, *, densify_by="grad",
          error_threshold=None, optimizer_type=None, optimizer_visibility="radii", lambda_depth=0.0, lambda_alpha=0.0,
          strategy="default", cap_max=None, noise_lr=5e5, opacity_reg=0.01, scale_reg=0.01, min_opacity=0.005,
          bilagrid=None, bilagrid_lr=2e-3, bilagrid_tv=10.0, filter_3d=False, filter_3d_interval=100, lambda_dist=0.0,
          dist_near_far=None, dist_from_iter=0, lambda_normal=0.0, normal_from_iter=0):
    """train.py:15-173 without its disabled compression-statistics branch: optimise a non-indexed model (usually
    GaussianModel.load_ply of a point cloud) with adaptive density control.

    The schedule is the reference's, counted in epochs: epoch_count = iterations // len(cameras) and every `*_iter` /
    `*_interval` of `opt` is converted with calc_epoch(i) = max(1, i * epoch_count // iterations); one epoch visits
    cameras[::camera_stride] in order (the reference's stride is 10 while its epoch count is over all cameras), SH degree up
    every calc_epoch(degree_up_iter) epochs. Per view: learning-rate update, render of the precomputed covariance exactly as
    train.py:62-67 (the covariance is a detached leaf: in this loop scale and rotation move through densification only, as
    in the reference), fused L1 + SSIM loss, Adam step, densification statistics while epoch < densify_until_epoch. After an
    epoch: densify_and_prune (screen-size threshold 20 once past the opacity-reset interval) and reset_opacity on the
    reference's conditions (train.py:160-173).

    `scene`: as for finetune(), plus `cameras_extent` (or pass `extent`). The model's `spatial_lr_scale` is the caller's to set
    (the reference's scene loader sets it to the camera extent). `log(epoch, info)` is called after every epoch with
    {"iteration", "ema_loss", "N", "densified": None | (rows before, (kept, clones, S, parents with children)), "reset_opacity"}.
    Returns the number of iterations run.

    `densify_by` = "grad" is the loop above. "error" (not in the reference) densifies by image error instead of the view-space
    gradient: every view renders with error_target=gt_image, GaussianModel.add_error_stats keeps each Gaussian's largest score
    E = sum over its blended pixels of alpha T x mean |render - gt| over the epoch's views in place of the gradient
    accumulation, and the epoch's densification is densify_and_prune(error_threshold, ..., scores=error_max).
    add_densification_stats still runs with `radii`, so max_radii2D and the screen-size prune work as before. `error_threshold`
    is required in that mode and has no default: its scale grows with the resolution, and nobody has tuned it.

    `optimizer_type` goes to GaussianModel.training_setup (None: opt.optimizer_type; "default" is the loop above).
    "sparse_adam" (not in the reference; upstream 3DGS's accelerated optimizer) steps only the Gaussians the view saw and
    leaves the parameters and moments of all others as they are. `optimizer_visibility` names what "saw" means and is used
    with that optimizer only: "radii" (upstream's rule) lists the rows with radii > 0; "blended" lists the rows at least one
    pixel blended, the `contrib_hits` of a render with return_contrib=True, which costs the contribution pass
    (csrc/render_contrib.hip) in every view; None steps every row (the dense step through the sparse optimizer).

    `lambda_depth`, `lambda_alpha` (not in the reference) add losses on the depth and alpha maps of render(depth_grad=True)
    (csrc/render_maps_backward.hip) for the views whose camera object carries a target, attached by the caller as [H, W] fp32:
    `alpha_target` (a mask or silhouette) adds lambda_alpha x mean |alpha - alpha_target|; `depth_target` (0 = no measurement)
    adds lambda_depth x the mean over the measured pixels of |depth - alpha x depth_target|, a residual in weight space (depth is
    sum alpha T z, not normalised), so nothing is divided. Both at 0 (the default), and views without the attributes, run the
    loop above with its launches.

    `lambda_dist` (not in the reference: the depth-distortion loss of Mip-NeRF 360 as 2DGS and gsplat use it;
    csrc/render_distortion.hip, csrc/render_maps_backward.hip) = 0 is the loop above, launch for launch. A positive value
    adds lambda_dist x render(distortion=...)["distortion"].mean() from iteration `dist_from_iter` on (counted like `iteration`
    of `info`, from 0): per pixel sum_i sum_j w_i w_j |s_i - s_j| over the blended entries, which pulls the mass along a ray
    together and needs no measured depth. `dist_near_far` = None takes s = the view-space depth; a pair (near, far) takes 2DGS's
    mapping far / (far - near) (1 - near / z). There is no default weight because nobody has tuned one here: 2DGS's own values
    (100 to 1000, from iteration 3000) are for ITS mapping and its normalised depth, which is the reason `dist_near_far` is
    offered; in raw mode the loss scales with the square of the scene's depth unit. A negative value raises ValueError.

    `lambda_normal` (not in the reference: 2DGS's normal-consistency loss; csrc/normals.hip, csrc/render_normal.hip,
    csrc/render_maps_backward.hip) = 0 is the loop above, launch for launch. A positive value adds
    lambda_normal x normals.normal_consistency(depth, alpha, normal, intrinsic) of render(normal=True) from iteration
    `normal_from_iter` on: the mean over the pixels of 1 - N . Ns, with N the blended map of the Gaussians' shortest axes and Ns the
    normal of the rendered depth map, weighted by alpha. A normal needs axes, so from that iteration on the render takes the
    model's scales and rotations and not the loop's frozen covariance: they receive gradients (from the image as well), which is
    what the term is for. With `lambda_dist` the two terms share one blend replay in the backward. 2DGS uses 0.05 from iteration
    7000; nobody has tuned a value here. With `filter_3d` the filtered covariance is blended and the normals come from the
    unfiltered axes. A negative value raises ValueError.

    `strategy` = "default" is the loop above, launch for launch. "mcmc" (not in the reference: "3D Gaussian Splatting as Markov
    Chain Monte Carlo", gsplat's MCMCStrategy; csrc/mcmc.hip) trains towards a hard budget of `cap_max` Gaussians (required):
      - it renders WITHOUT the precomputed covariance, so scale and rotation are learnable, which the method presumes (moving
        a Gaussian rescales it); the reference's loop, and the default strategy here, freeze them between densifications;
      - the loss gains opacity_reg x mean sigmoid(_opacity) + scale_reg x mean get_scaling;
      - GaussianModel.add_position_noise(noise_lr) follows every optimizer step;
      - after an epoch, on the default loop's densification schedule (the same densify_from / until / interval conversion), it
        calls relocate_gs(min_opacity=min_opacity) and then add_new_gs(cap_max): dead Gaussians move onto live ones, the scene
        grows by 5 % up to the cap. The schedule INCLUDES epoch densify_from_epoch itself (epoch >= densify_from_epoch, where the
        default loop asks >): that epoch already ends past densify_from_iter, and a refinement reads the opacities as they are,
        it has no gradient statistics to gather over an interval first. tests/train_scene.py's schedule(400) thus refines at
        epochs 5, 10, ... 35, seven times. No densify_and_prune, no reset_opacity, no add_densification_stats.
    `info` keeps "densified": None and "reset_opacity": False and gains "mcmc": None | (relocated, added). Both optimizer types
    work. densify_by="error" with it raises ValueError, as does an unknown strategy.

    `bilagrid` (not in the reference: gsplat's bilateral grid; shape (1, 1, 1) is upstream 3DGS's per-image `exposure`;
    csrc/bilagrid.hip) = None is the loop above, launch for launch. A shape (L, Hg, Wg) builds a bilagrid.BilateralGrid with one
    identity grid per training camera and hands it out as info["bilagrid"] on the first log call; a BilateralGrid is trained in
    place. Row k belongs to camera k of the training list (all of them, whatever `camera_stride` visits). The loss then sees
    bilagrid.slice(render, k) in place of the render, plus `bilagrid_tv` x bilagrid.tv_loss() when the shape has more than one
    vertex and bilagrid_tv > 0. The grids get an optim.Adam of their own at `bilagrid_lr`, stepped and zeroed next to the model's:
    they stay out of the model's optimizer, so densification and MCMC never see their moments. The defaults (2e-3, 10.0) are
    gsplat's, quoted from memory; nobody has tuned them here. densify_by="error" with a grid raises ValueError: the error map
    inside render() would compare the uncorrected image. Every epoch's `info` also carries "epoch_loss", the mean of the epoch's
    losses (the values the moving average is fed).

    `filter_3d` (not in the reference: the 3D smoothing filter of Mip-Splatting; csrc/filter3d.hip) = False is the loop above,
    launch for launch. True trains with GaussianModel.compute_3D_filter over ALL training cameras (whatever `camera_stride`
    visits): computed before the first iteration, again in front of every iteration that is a positive multiple of
    `filter_3d_interval`, and after every step that changed rows (densify_and_prune by gradient or by error, MCMC relocation or
    growth). The camera table is built once per call (the one place that reads the poses on the host); the recomputes are
    stream-ordered. The loop itself is unchanged: the default strategy still hands render() its frozen covariance, which the
    filtered render takes as cov3d + f^2 I. The model keeps the filter when train() returns."""
    if filter_3d and int(filter_3d_interval) < 1:
        raise ValueError("train: filter_3d_interval must be a positive number of iterations")
    if bilagrid is not None and densify_by == "error":
        raise ValueError("train: densify_by='error' compares the uncorrected render inside render(); it cannot be combined with bilagrid")
    if strategy not in ("default", "mcmc"):
        raise ValueError(f"train: strategy must be 'default' or 'mcmc', not {strategy!r}")
    mcmc = strategy == "mcmc"
    if mcmc and densify_by != "grad":
        raise ValueError("train: strategy='mcmc' has its own density control; densify_by must stay 'grad'")
    if mcmc and cap_max is None:
        raise ValueError("train: strategy='mcmc' needs cap_max, the budget of Gaussians (there is no default)")
    if lambda_depth < 0 or lambda_alpha < 0:
        raise ValueError("train: lambda_depth and lambda_alpha must be >= 0")
    distortion = _distortion_option("train", lambda_dist, dist_near_far)
    if lambda_normal < 0:
        raise ValueError("train: lambda_normal must be >= 0")
    if optimizer_visibility not in ("radii", "blended", None):
        raise ValueError(f"train: optimizer_visibility must be 'radii', 'blended' or None, not {optimizer_visibility!r}")
    if densify_by not in ("grad", "error"):
        raise ValueError(f"train: densify_by must be 'grad' or 'error', not {densify_by!r}")
    by_error = densify_by == "error"
    if by_error and error_threshold is None:
        raise ValueError("train: densify_by='error' needs an error_threshold (there is no default)")
    gaussians = scene.gaussians if hasattr(scene, "gaussians") else dataset.gaussians
    if mcmc:
        gaussians._dense_only("train(strategy='mcmc')")
    cameras = _train_cameras(scene)
    if extent is None and not mcmc:
        extent = scene.cameras_extent
    grid_optimizer = None
    if bilagrid is not None:
        if not isinstance(bilagrid, _bilagrid.BilateralGrid):
            bilagrid = _bilagrid.BilateralGrid(len(cameras), bilagrid, device=gaussians.device).set_cameras(cameras)
        camera_index = _camera_indices(cameras, bilagrid)
        grid_optimizer = _optim.Adam([bilagrid.grids], lr=bilagrid_lr, eps=1e-15)
        grid_tv = float(bilagrid_tv) if bilagrid_tv and max(bilagrid.shape) > 1 else 0.0
    gaussians.training_setup(opt, optimizer_type=optimizer_type)
    gaussians.update_learning_rate(0)
    sparse = isinstance(gaussians.optimizer, _optim.SparseGaussianAdam) and optimizer_visibility is not None
    extra_base = {"return_contrib": True} if sparse and optimizer_visibility == "blended" else {}
    dev = gaussians.device
    bg = torch.rand(3, device=dev) if opt.random_background else torch.tensor([0, 0, 0], dtype=torch.float32, device=dev)
    ema_loss_for_log = 0.0
    epoch_count = opt.iterations // len(cameras)
    calc_epoch = lambda i: max(1, i * epoch_count // opt.iterations)        # noqa: E731
    densify_until_epoch = calc_epoch(opt.densify_until_iter)
    densify_from_epoch = calc_epoch(opt.densify_from_iter)
    densification_interval = calc_epoch(opt.densification_interval)
    opacity_reset_interval = calc_epoch(opt.opacity_reset_interval)
    degree_up = calc_epoch(degree_up_iter)

    iteration = 0
    if filter_3d:
        from . import filter3d as _filter3d
        camera_table = _filter3d.camera_table(cameras, gaussians.device)
        gaussians.compute_3D_filter(cameras, camera_table)
    for epoch in range(epoch_count):
        pending = []
        for viewpoint_cam in cameras[::camera_stride]:
            gaussians.update_learning_rate(iteration)
            if filter_3d and iteration > 0 and iteration % int(filter_3d_interval) == 0:
                gaussians.compute_3D_filter(cameras, camera_table)
            if not mcmc:
                cov3d_scaled = gaussians.get_covariance().detach()
                scaling_factor = gaussians.get_scaling_factor
                coeff = scaling_factor.detach().square() if torch.is_tensor(scaling_factor) else 1.0
                cov3d = (cov3d_scaled / coeff).requires_grad_(True)
            # every row goes to the rasterizer (it culls them itself): radii and the screen-space gradient are then indexed
            # by Gaussian, which is what the reference scatters them back to (train.py:103-105)
            alpha_target = getattr(viewpoint_cam, "alpha_target", None) if lambda_alpha > 0 else None
            depth_target = getattr(viewpoint_cam, "depth_target", None) if lambda_depth > 0 else None
            extra = dict(extra_base, depth_grad=True) if (alpha_target is not None or depth_target is not None) else extra_base
            with_dist = distortion is not False and iteration >= dist_from_iter
            if with_dist:
                extra = dict(extra, distortion=distortion)
            with_normal = lambda_normal > 0 and iteration >= normal_from_iter
            if with_normal:
                extra = dict(extra, normal=True)
            # a normal needs axes: with the term the rasterizer builds the covariance from the scales and rotations itself
            frozen = {} if (mcmc or with_normal) else {"cov3d": cov3d * coeff}
            if by_error:
                gt_image = viewpoint_cam.original_image.to(dev)
                render_pkg = gaussians.render(viewpoint_cam, pipe, bg, clamp_color=False, gather_visible=False,
                                              error_target=gt_image, **frozen, **extra)
            else:
                render_pkg = gaussians.render(viewpoint_cam, pipe, bg, clamp_color=False, gather_visible=False, **frozen, **extra)
            image, viewspace_point_tensor, radii = render_pkg["render"], render_pkg["viewspace_points"], render_pkg["radii"]
            if not by_error:
                gt_image = viewpoint_cam.original_image.to(image.device)
            if bilagrid is not None:
                image = bilagrid.slice(image, camera_index[id(viewpoint_cam)])
            loss = _loss.l1_ssim_loss(image, gt_image, opt.lambda_dssim)
            if grid_optimizer is not None and grid_tv > 0:
                loss = loss + grid_tv * bilagrid.tv_loss()
            if alpha_target is not None:
                loss = loss + lambda_alpha * (render_pkg["alpha"] - alpha_target.to(dev)).abs().mean()
            if depth_target is not None:
                target = depth_target.to(dev)
                measured = target > 0
                residual = ((render_pkg["depth"] - render_pkg["alpha"] * target).abs() * measured).sum()
                loss = loss + lambda_depth * residual / measured.sum().clamp(min=1)
            if with_dist:
                loss = loss + lambda_dist * render_pkg["distortion"].mean()
            if with_normal:
                loss = loss + lambda_normal * _normals.normal_consistency(render_pkg["depth"], render_pkg["alpha"],
                                                                          render_pkg["normal"], viewpoint_cam.intrinsic)
            if mcmc:
                loss = loss + opacity_reg * torch.sigmoid(gaussians._opacity).mean() + scale_reg * gaussians.get_scaling.mean()
            loss.backward()
            pending.append(loss.detach())
            if sparse:
                gaussians.optimizer.step(render_pkg["contrib_hits"] if extra_base else radii)
            else:
                gaussians.optimizer.step()
            gaussians.optimizer.zero_grad(set_to_none=True)
            if grid_optimizer is not None:
                grid_optimizer.step()
                grid_optimizer.zero_grad(set_to_none=True)
            if mcmc:
                gaussians.add_position_noise(noise_lr)
            elif epoch < densify_until_epoch:
                with torch.no_grad():
                    gaussians.add_densification_stats(viewspace_point_tensor, render_pkg["visibility_filter"], radii)
                    if by_error:
                        gaussians.add_error_stats(render_pkg["error_sum"])
            iteration += 1
        epoch_losses = torch.stack(pending).tolist()               # one host read per epoch
        for v in epoch_losses:
            ema_loss_for_log = 0.4 * v + 0.6 * ema_loss_for_log
        info = {"iteration": iteration, "ema_loss": ema_loss_for_log, "densified": None, "reset_opacity": False,
                "epoch_loss": sum(epoch_losses) / len(epoch_losses)}
        if bilagrid is not None and epoch == 0:
            info["bilagrid"] = bilagrid
        if mcmc:
            info["mcmc"] = None
            if densify_from_epoch <= epoch < densify_until_epoch and epoch % densification_interval == 0:
                relocated = gaussians.relocate_gs(min_opacity=min_opacity)
                info["mcmc"] = (relocated, gaussians.add_new_gs(cap_max, min_opacity=min_opacity))
        with torch.no_grad():
            if epoch < densify_until_epoch and not mcmc:
                if epoch > densify_from_epoch and epoch % densification_interval == 0:
                    size_threshold = 20 if epoch > opacity_reset_interval else None
                    rows = gaussians._xyz.shape[0]
                    if by_error:
                        plan = gaussians.densify_and_prune(float(error_threshold), 0.005, extent, size_threshold,
                                                           scores=gaussians._error_accumulators()[0])
                    else:
                        plan = gaussians.densify_and_prune(opt.densify_grad_threshold, 0.005, extent, size_threshold)
                    info["densified"] = (rows, plan[3])
                if epoch > 0 and epoch % opacity_reset_interval == 0:
                    gaussians.reset_opacity()
                    info["reset_opacity"] = True
        if filter_3d and gaussians._filter_3D_stale:                 # rows were created: their filter values are measured now
            gaussians.compute_3D_filter(cameras, camera_table)
        if epoch % degree_up == 0:
            gaussians.oneupSHdegree()
        info["N"] = gaussians._xyz.shape[0]
        if log is not None:
            log(epoch, info)
    return iteration


def refine_poses(scene_or_cameras, gaussians, pipe, background, iterations, lr=1e-3, lambda_dssim=0.2, cameras=None, log=None,
                 pose_grad="exact"):
    """train_camera.py:56-112 without its plotting: optimise camera poses against a FROZEN model. One torch.optim.Adam over the
    chosen cameras' `extrinsic_vector` (one parameter group per camera, as the reference builds them); `iterations` passes over
    them, per camera and pass: render -> fused (1 - l) L1 + l (1 - SSIM) against `cam.original_image` -> backward -> step.

    `scene_or_cameras`: a scene with getTrainCameras() or a list of cameras; `cameras`: indices into it (None: all). Each
    chosen camera's `extrinsic_vector` becomes a leaf on the model's device that requires grad (the same tensor when it already
    lives there, so the caller sees the refined pose in place); nothing else about the cameras changes. The model's
    parameters have `requires_grad` switched off for the run and put back on exit, its optimizer is not touched, and as in
    GaussianModel.contribution_stats the QAT observer / quantiser state is saved in front and put back behind.
    `pose_grad`: "exact" (the default), the gradient of the render itself (csrc/pose_grad.hip); "reference", the reference's
    formula, which exists on the indexed rasterizer only.
    The losses stay on the device: one host read per 10 passes, where `log(pass, [loss per camera])` is called.
    -> [(first loss, last loss) per chosen camera]."""
    cams = _train_cameras(scene_or_cameras)
    if cameras is not None:
        cams = [cams[i] for i in cameras]
    if not cams:
        return []
    if gaussians.filter_3D is not None or gaussians._filter_3D_stale:
        raise ValueError("refine_poses: the render with a 3D filter has no pose gradient; clear_3D_filter() first")
    dev = gaussians.device
    params = gaussians.parameters()
    was = [t.requires_grad for t in params]
    fq_saved = gaussians._fq_state.clone()
    groups = []
    for i, cam in enumerate(cams):
        cam.extrinsic_vector = cam.extrinsic_vector.detach().to(dev, torch.float32).requires_grad_(True)
        groups.append({"params": [cam.extrinsic_vector], "lr": lr, "name": f"extr{i}"})
    optimizer = torch.optim.Adam(groups)
    history, pending = [], []
    try:
        for t in params:
            t.requires_grad_(False)
        for it in range(1, int(iterations) + 1):
            row = []
            for cam in cams:
                image = gaussians.render(cam, pipe, background, pose_grad=pose_grad)["render"]
                loss = _loss.l1_ssim_loss(image, cam.original_image.to(dev), lambda_dssim)
                loss.backward()
                optimizer.step()
                optimizer.zero_grad(set_to_none=True)
                row.append(loss.detach())
            pending.append(torch.stack(row))
            if it % 10 == 0 or it == iterations:
                vals = torch.stack(pending).tolist()                # one host read per 10 passes
                history.extend(vals)
                pending = []
                if log is not None:
                    log(it, vals[-1])
    finally:
        for t, r in zip(params, was):
            t.requires_grad_(r)
        with torch.no_grad():
            gaussians._fq_state.copy_(fq_saved)
    return [(history[0][k], history[-1][k]) for k in range(len(cams))] if history else [(float("nan"),) * 2 for _ in cams]


def run_vq(gaussians, scene, optim_params, pipeline_params, comp_params, dataset=None, group=None, silent=True,
           out_file: Optional[str] = None, eval_cameras=None, eval_name="test", background=None):
    """compress.py:202-303 on an already constructed model and camera set: sensitivity (use_gt) -> prune + colour /
    covariance VQ -> QAT fine-tuning -> Morton-sorted npz. Returns (timings dict, npz path).
    `group`: process group for the camera-sharded sensitivity pass and the sharded Lloyd steps (None = one GPU).
    With `eval_cameras` (views carrying `original_image`), the evaluation pass follows the npz as in compress.py:293-303:
    metrics.render_and_eval (SSIM / PSNR; LPIPS is not bundled and reported as None) against `background` (default: that
    of `dataset`, black without one), PNGs under output_vq/<eval_name>/ours_<iteration>/, and output_vq/results.json =
    {"ours_<iteration>": {SSIM, PSNR, LPIPS, size}} with size the npz size in MB."""
    timings = {}
    dev = gaussians.device

    def clock():
        if dev.type == "cuda":
            torch.cuda.synchronize(dev)
        return time.time()

    cameras = _train_cameras(scene)
    t0 = clock()
    color_importance, gaussian_sensitivity = _sensitivity.calc_importance_experimental(
        gaussians, cameras, pipeline_params, use_gt=True, group=group)
    timings["sensitivity_calculation"] = clock() - t0

    with torch.no_grad():
        t0 = clock()
        color_importance_n = color_importance.amax(-1)
        gaussian_importance_n = gaussian_sensitivity.amax(-1)
        del color_importance, gaussian_sensitivity
        color_settings = CompressionSettings(
            codebook_size=comp_params.color_codebook_size, importance_prune=comp_params.color_importance_prune,
            importance_include=None, importance_include_relative=0.9, steps=int(comp_params.color_cluster_iterations),
            decay=comp_params.color_decay, batch_size=comp_params.color_batch_size)
        gaussian_settings = CompressionSettings(
            codebook_size=comp_params.gaussian_codebook_size, importance_prune=None, importance_include=None,
            importance_include_relative=0.75, steps=int(comp_params.gaussian_cluster_iterations),
            decay=comp_params.gaussian_decay, batch_size=comp_params.gaussian_batch_size)
        compress_gaussians(gaussians, color_importance_n, gaussian_importance_n,
                           color_settings if not comp_params.not_compress_color else None,
                           gaussian_settings if not comp_params.not_compress_gaussians else None,
                           comp_params.color_compress_non_dir, prune_threshold=comp_params.prune_threshold,
                           silent=silent, group=group)
        timings["clustering"] = clock() - t0
    gc.collect()

    os.makedirs(comp_params.output_vq, exist_ok=True)
    with open(os.path.join(comp_params.output_vq, "cfg_args_comp"), "w") as f:
        f.write(str(vars(comp_params)))

    iteration = int(getattr(scene, "loaded_iter", 0) or 0) + comp_params.finetune_iterations
    if comp_params.finetune_iterations > 0:
        t0 = clock()
        holder = _SceneView(gaussians, cameras, getattr(scene, "loaded_iter", 0))
        finetune(holder, dataset if dataset is not None else _Dataset(), optim_params, comp_params, pipeline_params,
                 debug_from=-1)
        timings["finetune"] = clock() - t0

    if out_file is None:
        out_file = os.path.join(comp_params.output_vq, f"point_cloud/iteration_{iteration}/point_cloud.npz")
    os.makedirs(os.path.dirname(out_file) or ".", exist_ok=True)
    t0 = clock()
    gaussians.save_npz(out_file, sort_morton=not comp_params.not_sort_morton)
    timings["encode"] = clock() - t0
    timings["total"] = sum(timings.values())
    with open(os.path.join(comp_params.output_vq, "times.json"), "w") as f:
        json.dump(timings, f)

    if eval_cameras is not None:
        if background is None:
            white = getattr(dataset, "white_background", False) if dataset is not None else False
            background = torch.tensor([1, 1, 1] if white else [0, 0, 0], dtype=torch.float32, device=dev)
        metrics = _metrics.render_and_eval(gaussians, eval_cameras, pipeline_params, background,
                                           out_dir=os.path.join(comp_params.output_vq, eval_name, f"ours_{iteration}"))
        metrics["size"] = os.path.getsize(out_file) / 1024 ** 2
        with open(os.path.join(comp_params.output_vq, "results.json"), "w") as f:
            json.dump({f"ours_{iteration}": metrics}, f, indent=4)
    return timings, out_file


class _Dataset:
    white_background = False


class _SceneView:
    def __init__(self, gaussians, cameras, loaded_iter):
        self.gaussians, self._cameras, self.loaded_iter = gaussians, cameras, int(loaded_iter or 0)

    def getTrainCameras(self):
        return self._cameras
