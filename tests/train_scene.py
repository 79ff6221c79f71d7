"""A small synthetic "optimise a scene from a point cloud" problem, shared by tests/test_densify_gpu.py and
tools/run_train.py: a synth-v1 teacher scene rendered from a few nearby views as ground truth, and a student that starts
from every `keep_every`-th teacher position written as a point-cloud PLY and read back with GaussianModel.load_ply (the exact
3-nearest-neighbour scale initialiser is on the path)."""
import os

import numpy as np
import torch

from tests import synth

EXTENT = 5.0          # plays the part of the reference's scene.cameras_extent


class Cam:
    def __init__(self, intrinsic, ev, device):
        self.intrinsic, self.extrinsic_vector = intrinsic.to(device), ev.to(device)
        self.original_image = None


def teacher_model(P, W, H, focal, device, seed=31):
    from c3dgs_amd.model import GaussianModel
    sc = synth.scene(P, W=W, H=H, focal=focal, seed=seed, scale_median=0.06, zmin=3.0, zmax=8.0)
    op = sc["opacities"].clamp(0.3, 1 - 1e-6)
    norm = sc["scales"].norm(dim=1, keepdim=True)
    m = GaussianModel(3, quantization=False, device=device)
    m.set_tensors(xyz=sc["means3D"], features_dc=sc["shs"][:, :1], features_rest=sc["shs"][:, 1:], scaling=sc["scales"] / norm,
                  rotation=sc["rotations"], opacity=torch.log(op / (1 - op)), scaling_factor=torch.log(norm))
    return m, sc


def make(tmp_dir, device="cuda", P_teacher=4000, keep_every=8, views=8, W=160, H=112, focal=150.0, quantization=True):
    """-> (student GaussianModel, cameras with original_image, EXTENT)."""
    from c3dgs_amd import ply
    from c3dgs_amd.model import GaussianModel, PipelineParams
    teacher, sc = teacher_model(P_teacher, W, H, focal, device)
    cams = []
    bg = torch.zeros(3, device=device)
    for k in range(views):
        a = 2 * np.pi * k / views
        ev = (0.015 * np.sin(a), 0.015 * np.cos(a), 0.0, 1.0, 0.25 * np.cos(a), 0.25 * np.sin(a), 0.0)
        intr, e = synth.camera(W, H, focal, extrinsic_vector=ev)
        cam = Cam(intr, e, device)
        with torch.no_grad():
            cam.original_image = teacher.render(cam, PipelineParams(), bg)["render"].clamp(0, 1).clone()
        cams.append(cam)
    xyz = sc["means3D"][::keep_every].numpy()
    rgb = np.clip((0.5 + 0.28209479177387814 * sc["shs"][::keep_every, 0].numpy()) * 255.0, 0, 255).round()
    path = os.path.join(str(tmp_dir), "points3D.ply")
    ply.write_ply(path, {"x": xyz[:, 0], "y": xyz[:, 1], "z": xyz[:, 2], "red": rgb[:, 0], "green": rgb[:, 1], "blue": rgb[:, 2]})
    student = GaussianModel(3, quantization=quantization, device=device).load_ply(path)
    student.spatial_lr_scale = EXTENT
    return student, cams, EXTENT


def schedule(iterations=400, densify=True):
    """OptimizationParams with the reference's intervals scaled down to `iterations`: with 8 views and camera_stride=1, 50
    epochs; densification every 5 epochs from epoch 10 to 35 (six times), opacity reset at epochs 15 and 30."""
    from c3dgs_amd.pipeline import OptimizationParams
    return OptimizationParams(iterations=iterations, position_lr_max_steps=iterations, densify_from_iter=iterations // 10,
                              densification_interval=iterations // 10, opacity_reset_interval=3 * iterations // 10,
                              densify_until_iter=(8 * iterations // 10) if densify else 0)


def mean_psnr(model, cams):
    from c3dgs_amd import metrics
    from c3dgs_amd.model import PipelineParams
    bg = torch.zeros(3, device=model.device)
    vals = []
    with torch.no_grad():
        for cam in cams:
            img = model.render(cam, PipelineParams(), bg)["render"].clamp(0, 1)
            vals.append(float(metrics.psnr(img[None], cam.original_image[None]).mean()))
    return sum(vals) / len(vals)
