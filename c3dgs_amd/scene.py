"""Scenes from datasets on disk: COLMAP, Blender (NeRF synthetic) and Dust3r readers, cameras, ground-truth images.

    Scene(args, gaussians, ...)          <- scene/__init__.py:24-117
    read*Info / read*Cameras, getNerfppNorm, storePly / fetchPly, sceneLoadTypeCallbacks   <- scene/dataset_readers.py:27-353
    Camera                               <- scene/cameras.py:28-92
    loadCam, cameraList_from_camInfos, camera_to_JSON                                      <- utils/camera_utils.py:17-68
    searchForMaxIteration                <- utils/system_utils.py:26

The readers are host code (numpy); names, return shapes and the order of the floating-point operations follow the reference,
so CameraInfo, the normalisation and cameras.json agree with it to the last bit (tests/golden/scene.npz). PLY files go through
ply.py. What differs, on purpose:

  * Camera.original_image. The reference decodes, converts, premultiplies, flips, resizes and clamps on the host, on every
    access when save_memory is set. Here the file is decoded once, its bytes go to the device as one uint8 tensor and ONE
    HIP kernel (csrc/image_io.hip) produces the planar fp32 image at the camera's resolution. save_memory=True keeps the
    bytes (1 B per channel at source size) and rebuilds the float image per access with no host work; save_memory=False
    keeps the float image and drops the bytes.
  * flip. The reference flips both axes of EVERY image, under the comment "for DUST3R ONLY". Here `flip` defaults to False and
    Scene passes True for Dust3r scenes only.
  * background. None premultiplies onto black, as the reference does; Scene(..., composite_background=True) hands each
    camera the dataset's background colour, so that a white-background Blender set is trained against what is rendered.
  * errors. An unsupported camera model, an unrecognised directory and a malformed file raise ValueError; a binary COLMAP
    model that exists but cannot be read is an error, not a reason to try the text files.
"""
import glob
import json
import math
import os
import random
import shutil
from pathlib import Path
from typing import NamedTuple, Optional

import numpy as np
import torch

from . import colmap, image_io, ply
from .rasterizer import mat_to_quat

INTRINSIC_DEVICE = "cuda"        # Camera.intrinsic lives on the device (cameras.py:39)


class BasicPointCloud(NamedTuple):
    points: np.ndarray
    colors: np.ndarray
    normals: np.ndarray


class CameraInfo(NamedTuple):
    uid: int
    extrinsic: np.ndarray        # float64 [4,4] world-to-camera
    intrinsic: np.ndarray        # float64 [3,3]: [0,0] = fov x, [1,1] = fov y (radians), [0,2] / [1,2] = principal point
    image_path: str
    image_name: str
    width: int
    height: int


class SceneInfo(NamedTuple):
    point_cloud: Optional[BasicPointCloud]
    train_cameras: list
    test_cameras: list
    nerf_normalization: dict
    ply_path: str


def fov2focal(fov, pixels):
    return pixels / (2 * math.tan(fov / 2))


def focal2fov(focal, pixels):
    return 2 * math.atan(pixels / (2 * focal))


def getWorld2View2(Rt, translate=np.array([.0, .0, .0]), scale=1.0):
    """The world-to-view matrix with the camera centre moved by `translate` and scaled, as float32 (which is why the radius of
    getNerfppNorm is a float32)."""
    C2W = np.linalg.inv(Rt)
    C2W[:3, 3] = (C2W[:3, 3] + translate) * scale
    return np.float32(np.linalg.inv(C2W))


def getNerfppNorm(cam_info):
    centers = [np.linalg.inv(getWorld2View2(cam.extrinsic))[:3, 3:4] for cam in cam_info]
    centers = np.hstack(centers)
    center = np.mean(centers, axis=1, keepdims=True)
    diagonal = np.max(np.linalg.norm(centers - center, axis=0, keepdims=True))
    return {"translate": -center.flatten(), "radius": diagonal * 1.1}


def readColmapCameras(cam_extrinsics, cam_intrinsics, images_folder):
    cam_infos = []
    for extr in cam_extrinsics.values():
        intr = cam_intrinsics[extr.camera_id]
        height, width = intr.height, intr.width
        Rt = np.eye(4)
        Rt[:3, :3] = colmap.qvec2rotmat(extr.qvec)
        Rt[:3, 3] = np.array(extr.tvec)
        if intr.model == "SIMPLE_PINHOLE":
            fov_y, fov_x = focal2fov(intr.params[0], height), focal2fov(intr.params[0], width)
        elif intr.model == "PINHOLE":
            fov_y, fov_x = focal2fov(intr.params[1], height), focal2fov(intr.params[0], width)
        else:
            raise ValueError(f"COLMAP camera model {intr.model!r} is not handled: only undistorted datasets (PINHOLE or "
                             "SIMPLE_PINHOLE cameras) are supported")
        image_path = os.path.join(images_folder, os.path.basename(extr.name))
        image_name = os.path.basename(image_path).split(".")[0]
        intrinsic = np.asarray([[fov_x, 0, width / 2], [0, fov_y, height / 2], [0, 0, 1]])
        cam_infos.append(CameraInfo(uid=intr.id, extrinsic=Rt, intrinsic=intrinsic, image_path=image_path, image_name=image_name,
                                    width=width, height=height))
    return cam_infos


def fetchPly(path):
    v = ply.read_ply(path)
    positions = np.vstack([v["x"], v["y"], v["z"]]).T
    if "red" in v:
        colors = np.vstack([v["red"], v["green"], v["blue"]]).T / 255.0
    else:
        colors = np.vstack([v["f_dc_0"], v["f_dc_1"], v["f_dc_2"]]).T
    normals = np.vstack([v["nx"], v["ny"], v["nz"]]).T if "nx" in v else np.zeros_like(positions)
    return BasicPointCloud(points=positions, colors=colors, normals=normals)


def storePly(path, xyz, rgb):
    """x y z nx ny nz as float, red green blue as uchar, binary little-endian: the file plyfile writes for the reference."""
    xyz, rgb = np.asarray(xyz), np.asarray(rgb)
    names = [("x", "<f4"), ("y", "<f4"), ("z", "<f4"), ("nx", "<f4"), ("ny", "<f4"), ("nz", "<f4"), ("red", "u1"), ("green", "u1"),
             ("blue", "u1")]
    rec = np.zeros(xyz.shape[0], dtype=np.dtype(names))
    for k, c in enumerate("xyz"):
        rec[c] = xyz[:, k]
    for k, c in enumerate(("red", "green", "blue")):
        rec[c] = rgb[:, k]
    props = "".join(f"property {'float' if t == '<f4' else 'uchar'} {n}\n" for n, t in names)
    with open(path, "wb") as f:
        f.write(f"ply\nformat binary_little_endian 1.0\nelement vertex {len(rec)}\n{props}end_header\n".encode("ascii"))
        rec.tofile(f)


def _fetch_or_none(ply_path):
    try:
        return fetchPly(ply_path)
    except (OSError, ValueError, KeyError) as e:
        print(f"Error fetching point cloud. {e}")
        return None


def readColmapSceneInfo(path, images, eval, llffhold=8):
    sparse = os.path.join(path, "sparse/0")
    if os.path.exists(os.path.join(sparse, "images.bin")) and os.path.exists(os.path.join(sparse, "cameras.bin")):
        cam_extrinsics = colmap.read_extrinsics_binary(os.path.join(sparse, "images.bin"))
        cam_intrinsics = colmap.read_intrinsics_binary(os.path.join(sparse, "cameras.bin"))
    else:
        cam_extrinsics = colmap.read_extrinsics_text(os.path.join(sparse, "images.txt"))
        cam_intrinsics = colmap.read_intrinsics_text(os.path.join(sparse, "cameras.txt"))
    reading_dir = "images" if images is None else images
    cam_infos = sorted(readColmapCameras(cam_extrinsics, cam_intrinsics, os.path.join(path, reading_dir)),
                       key=lambda c: c.image_name)
    if eval:
        train_cam_infos = [c for idx, c in enumerate(cam_infos) if idx % llffhold != 0]
        test_cam_infos = [c for idx, c in enumerate(cam_infos) if idx % llffhold == 0]
    else:
        train_cam_infos, test_cam_infos = cam_infos, []
    nerf_normalization = getNerfppNorm(train_cam_infos)

    ply_path = os.path.join(sparse, "points3D.ply")
    if not os.path.exists(ply_path):
        print("Converting point3d.bin to .ply, will happen only the first time you open the scene.")
        bin_path = os.path.join(sparse, "points3D.bin")
        if os.path.exists(bin_path):
            xyz, rgb, _ = colmap.read_points3D_binary(bin_path)
        else:
            xyz, rgb, _ = colmap.read_points3D_text(os.path.join(sparse, "points3D.txt"))
        storePly(ply_path, xyz, rgb)
    return SceneInfo(point_cloud=_fetch_or_none(ply_path), train_cameras=train_cam_infos, test_cameras=test_cam_infos,
                     nerf_normalization=nerf_normalization, ply_path=ply_path)


def _image_size(path):
    from PIL import Image
    with Image.open(path) as im:
        return im.size


def readCamerasFromTransforms(path, transformsfile, white_background, extension=".png"):
    """transforms_*.json of the NeRF synthetic sets. fov / focal / size / principal point come from the file's head; whatever is
    missing is derived at the first frame and then PERSISTS for the frames after it (w, h from the first image; cx, cy from
    them), as in the reference. A missing camera_angle_x without fl_x leaves fov x = w / 2, also as there."""
    cam_infos = []
    with open(os.path.join(path, transformsfile)) as f:
        contents = json.load(f)
    fovx, fovy = contents.get("camera_angle_x"), None
    fl_x, fl_y = contents.get("fl_x"), contents.get("fl_y")
    w, h, cx, cy = contents.get("w"), contents.get("h"), contents.get("cx"), contents.get("cy")
    for idx, frame in enumerate(contents["frames"]):
        image_path = os.path.join(path, os.path.splitext(frame["file_path"])[0] + extension)
        c2w = np.array(frame["transform_matrix"])
        c2w[:3, 1:3] *= -1                       # OpenGL / Blender axes (y up, z back) -> COLMAP (y down, z forward)
        w2c = np.linalg.inv(c2w)
        if w is None:
            w, h = _image_size(image_path)
        if fl_x is not None:
            fovx = focal2fov(fl_x, w)
        if fl_y is not None:
            fovy = focal2fov(fl_y, h)
        if fovx is None:
            fovx = w / 2
        if fovy is None:
            fovy = focal2fov(fov2focal(fovx, w), h)
        if cx is None:
            cx = w / 2
        if cy is None:
            cy = h / 2
        intrinsic = np.asarray([[fovx, 0, cx], [0, fovy, cy], [0, 0, 1]])
        cam_infos.append(CameraInfo(uid=idx, extrinsic=w2c, intrinsic=intrinsic, image_path=image_path,
                                    image_name=Path(image_path).stem, width=w, height=h))
    return cam_infos


def readCamerasFromTransformsDust3r(path, transformsfile, white_background, extension=".png"):
    cam_infos = []
    with open(os.path.join(path, transformsfile)) as f:
        contents = json.load(f)
    for idx, frame in enumerate(contents["frames"]):
        extrinsic = np.linalg.inv(np.array(frame["transform_matrix"]))
        intrinsic = np.array(frame["intrinsic_matrix"])
        image_path = os.path.join(path, frame["file_path"])
        w, h = _image_size(image_path)
        intrinsic[0][0] = focal2fov(intrinsic[0][0], w)
        intrinsic[1][1] = focal2fov(intrinsic[1][1], h)
        cam_infos.append(CameraInfo(uid=idx, extrinsic=extrinsic, intrinsic=intrinsic, image_path=image_path,
                                    image_name=Path(image_path).stem, width=w, height=h))
    return cam_infos


def readDustrInfo(path, white_background, eval):
    return SceneInfo(point_cloud=None, train_cameras=readCamerasFromTransformsDust3r(path, "transforms_dust3r.json", white_background),
                     test_cameras=[], nerf_normalization={"translate": [0.0, 0.0, 0.0], "radius": 1.0},
                     ply_path=os.path.join(path, "scene.ply"))


def readNerfSyntheticInfo(path, white_background, eval, extension=".png"):
    train_cam_infos = readCamerasFromTransforms(path, "transforms_train.json", white_background, extension)
    test_cam_infos = []
    if os.path.exists(os.path.join(path, "transforms_test.json")):
        test_cam_infos = readCamerasFromTransforms(path, "transforms_test.json", white_background, extension)
        if not eval:
            train_cam_infos.extend(test_cam_infos)
            test_cam_infos = []
    nerf_normalization = getNerfppNorm(train_cam_infos)
    ply_path = os.path.join(path, "points3d.ply")
    if not os.path.exists(ply_path):
        # no COLMAP data in these sets: start from random points inside the bounds of the synthetic Blender scenes
        num_pts = 100_000
        print(f"Generating random point cloud ({num_pts})...")
        xyz = np.random.random((num_pts, 3)) * 2.6 - 1.3
        shs = np.random.random((num_pts, 3)) / 255.0
        storePly(ply_path, xyz, (shs * 0.28209479177387814 + 0.5) * 255)
    return SceneInfo(point_cloud=_fetch_or_none(ply_path), train_cameras=train_cam_infos, test_cameras=test_cam_infos,
                     nerf_normalization=nerf_normalization, ply_path=ply_path)


sceneLoadTypeCallbacks = {"Colmap": readColmapSceneInfo, "Blender": readNerfSyntheticInfo, "Dust3r": readDustrInfo}


def searchForMaxIteration(folder):
    return max(int(name.split("_")[-1]) for name in os.listdir(folder))


class Camera:
    """cameras.py:28-92. `extrinsic_vector` (qx, qy, qz, qw, tx, ty, tz) is a CPU fp32 tensor; `intrinsic` is on the device with
    [0,2] = w and [1,2] = h of the image the camera is trained at. `original_image` is float32 [3, h, w] on `data_device`."""

    def __init__(self, colmap_id, extrinsic, intrinsic, h, w, image_name, image_path, uid, trans=np.array([0.0, 0.0, 0.0]),
                 scale=1.0, data_device="cuda", save_memory=False, flip=False, background=None):
        self.uid = uid
        self.colmap_id = colmap_id
        m = torch.tensor(np.asarray(extrinsic), dtype=torch.float32)
        self.extrinsic_vector = torch.stack([v.clone() for v in mat_to_quat(m)])
        self.intrinsic = torch.tensor(np.asarray(intrinsic), dtype=torch.float32).to(INTRINSIC_DEVICE)
        self.intrinsic[0, 2] = w
        self.intrinsic[1, 2] = h
        self.image_width, self.image_height = int(w), int(h)
        self.image_name = image_name
        self.image_path = image_path
        self.data_device = torch.device(data_device)
        self.save_memory = save_memory
        self.flip = bool(flip)
        self.background = None if background is None else [float(v) for v in background]
        self._image = None       # float32 [3, h, w]: kept only without save_memory
        self._bytes = None       # uint8 [Hs][Ws][C] on the GPU: kept only with save_memory

    @property
    def original_image(self):
        if self._image is not None:
            return self._image
        src = self._bytes
        if src is None:
            src = torch.from_numpy(image_io.decode_u8(self.image_path)).to("cuda")
        background = self.background if src.shape[2] == 4 else None
        image = image_io.image_from_u8(src, self.image_height, self.image_width, self.flip, background).to(self.data_device)
        if self.save_memory:
            self._bytes = src
        else:
            self._image = image
        return image


def loadCam(args, id, cam_info, resolution_scale, save_memory=False, flip=False, background=None):
    """The reference's resolution rule: `resolution` in {1, 2, 4, 8} divides and rounds; -1 keeps the size up to 1600 pixels of
    width and scales wider images down to 1600; any other value is the wanted width. The last two truncate."""
    orig_w, orig_h = cam_info.width, cam_info.height
    if args.resolution in [1, 2, 4, 8]:
        resolution = round(orig_w / (resolution_scale * args.resolution)), round(orig_h / (resolution_scale * args.resolution))
    else:
        if args.resolution == -1:
            global_down = orig_w / 1600 if orig_w > 1600 else 1
        else:
            global_down = orig_w / args.resolution
        scale = float(global_down) * float(resolution_scale)
        resolution = (int(orig_w / scale), int(orig_h / scale))
    return Camera(colmap_id=cam_info.uid, extrinsic=cam_info.extrinsic, intrinsic=cam_info.intrinsic, h=resolution[1], w=resolution[0],
                  image_name=cam_info.image_name, image_path=cam_info.image_path, uid=id, data_device=args.data_device,
                  save_memory=save_memory, flip=flip, background=background)


def cameraList_from_camInfos(cam_infos, resolution_scale, save_memory, args, flip=False, background=None):
    return [loadCam(args, id, c, resolution_scale, save_memory=save_memory, flip=flip, background=background)
            for id, c in enumerate(cam_infos)]


def camera_to_JSON(id, camera):
    """One entry of cameras.json from a CameraInfo."""
    C2W = np.linalg.inv(camera.extrinsic)
    return {"id": id, "img_name": camera.image_name, "width": camera.width, "height": camera.height,
            "position": C2W[:3, 3].tolist(), "rotation": [row.tolist() for row in C2W[:3, :3]],
            "intrinsic": [row.tolist() for row in camera.intrinsic]}


class Scene:
    """scene/__init__.py:24-117. `args` carries source_path, model_path, images, eval, white_background, resolution and
    data_device (pipeline.ModelParams(...).extract())."""

    def __init__(self, args, gaussians, load_iteration=None, shuffle=True, resolution_scales=[1.0], override_quantization=False,
                 save_memory=False, composite_background=False):
        self.model_path = args.model_path
        self.loaded_iter = None
        self.gaussians = gaussians
        sub_path = os.path.join(self.model_path, "point_cloud")
        if load_iteration:
            if load_iteration == -1 and os.path.exists(sub_path):
                self.loaded_iter = searchForMaxIteration(sub_path)
            else:
                self.loaded_iter = load_iteration
            print(f"Loading trained model at iteration {self.loaded_iter}")

        if os.path.exists(os.path.join(args.source_path, "sparse")):
            self.kind = "Colmap"
            scene_info = sceneLoadTypeCallbacks["Colmap"](args.source_path, args.images, args.eval)
        elif os.path.exists(os.path.join(args.source_path, "transforms_train.json")):
            self.kind = "Blender"
            scene_info = sceneLoadTypeCallbacks["Blender"](args.source_path, args.white_background, args.eval)
        elif os.path.exists(os.path.join(args.source_path, "transforms_dust3r.json")):
            self.kind = "Dust3r"
            scene_info = sceneLoadTypeCallbacks["Dust3r"](args.source_path, args.white_background, args.eval)
        else:
            raise ValueError(f"{args.source_path}: could not recognise the scene type (no sparse/, transforms_train.json or "
                             "transforms_dust3r.json)")

        if not self.loaded_iter:
            os.makedirs(self.model_path, exist_ok=True)
            shutil.copyfile(scene_info.ply_path, os.path.join(self.model_path, "input.ply"))
            camlist = list(scene_info.test_cameras) + list(scene_info.train_cameras)
            with open(os.path.join(self.model_path, "cameras.json"), "w") as f:
                json.dump([camera_to_JSON(id, cam) for id, cam in enumerate(camlist)], f)

        if shuffle:
            random.shuffle(scene_info.train_cameras)      # the same order at every resolution scale
            random.shuffle(scene_info.test_cameras)

        self.cameras_extent = scene_info.nerf_normalization["radius"]
        flip = self.kind == "Dust3r"
        background = ([1.0, 1.0, 1.0] if args.white_background else [0.0, 0.0, 0.0]) if composite_background else None
        self.train_cameras, self.test_cameras = {}, {}
        for resolution_scale in resolution_scales:
            self.train_cameras[resolution_scale] = cameraList_from_camInfos(
                scene_info.train_cameras, resolution_scale, save_memory=save_memory, args=args, flip=flip, background=background)
            self.test_cameras[resolution_scale] = cameraList_from_camInfos(
                scene_info.test_cameras, resolution_scale, save_memory=save_memory, args=args, flip=flip, background=background)

        if self.loaded_iter and os.path.exists(sub_path):
            found = sorted(glob.glob(os.path.join(sub_path, "iteration_" + str(self.loaded_iter), "point_cloud.*")))
            if not found:
                raise ValueError(f"{sub_path}: no point_cloud.* saved for iteration {self.loaded_iter}")
            self.gaussians.load(found[0], override_quantization=override_quantization)
        else:
            self.gaussians.load_ply(scene_info.ply_path)
            self.gaussians.spatial_lr_scale = scene_info.nerf_normalization["radius"]

    def save(self, iteration):
        self.gaussians.save_ply(os.path.join(self.model_path, f"point_cloud/iteration_{iteration}", "point_cloud.ply"))

    def getTrainCameras(self, scale=1.0):
        return self.train_cameras[scale]

    def getTestCameras(self, scale=1.0):
        return self.test_cameras[scale]

    def getSomeCameras(self, scale=1.0):
        ret = self.getTestCameras(scale)
        if len(ret) > 0:
            return ret, "test"
        return self.getTrainCameras(scale), "train"

    def __len__(self, scale=1.0):
        return len(self.train_cameras[scale]) + len(self.test_cameras[scale])
