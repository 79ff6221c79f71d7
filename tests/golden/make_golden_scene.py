#!/usr/bin/env python3
"""Writes the scene fixtures under tests/golden/scene/ and tests/golden/scene.npz = what the REFERENCE's readers and Camera
return for them. Run once, where a checkout of the reference is at hand:

    python tests/golden/make_golden_scene.py /path/to/reference

The reference runs on the CPU with four stand-ins: `plyfile` whose PlyData.read raises (the path readColmapSceneInfo itself
catches: point_cloud = None), an empty `cv2` (scene/cameras.py imports it; original_image is never touched), `.cuda()` as the
identity, and PIL's Image.fromarray taking the int8 array of the Blender reader as the same bytes (only its size is used). Its
`scene` package is entered without its __init__ (which pulls in the CUDA rasterizer). Nothing of the reference is stored but
the data its programs returned.

Fixtures (files the reference's programs read, a few KB each):
    scene/colmap/          sparse/0/{cameras,images,points3D}.{bin,txt}, sparse/0/points3D.ply, images/*.png (8x6)
                           10 images on two cameras (PINHOLE 8x6, SIMPLE_PINHOLE 16x12), names sorted differently from file order
    scene/blender_angle/   camera_angle_x only; train + test; 8x6 RGB PNGs
    scene/blender_focal/   fl_x, fl_y, w, h given (no camera_angle_x)
    scene/blender_rgba/    camera_angle_x, RGBA PNGs
The reference's text reader for cameras refuses every model but PINHOLE, so the text/binary agreement of the intrinsics is
asserted on a temporary file that holds the PINHOLE camera only; extrinsics and points are asserted on the fixture itself.
"""
import json
import os
import sys
import tempfile
import types

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
OUT = os.path.join(HERE, "scene")

from tests import scene_fixture as sf  # noqa: E402


def write_fixtures():
    sf.colmap_dataset(os.path.join(OUT, "colmap"), seed=0)
    from c3dgs_amd import colmap, scene
    xyz, rgb, _ = colmap.read_points3D_binary(os.path.join(OUT, "colmap", "sparse", "0", "points3D.bin"))
    scene.storePly(os.path.join(OUT, "colmap", "sparse", "0", "points3D.ply"), xyz, rgb)
    rng = np.random.default_rng(5)
    heads = {"blender_angle": {"camera_angle_x": 0.6911112070083618},
             "blender_focal": {"fl_x": 11.5, "fl_y": 10.75, "w": 8, "h": 6},
             "blender_rgba": {"camera_angle_x": 0.8}}
    for name, head in heads.items():
        d = os.path.join(OUT, name)
        poses = sf.ring(5, radius=3.0, seed=len(name))
        for split, sel in (("train", poses[:3]), ("test", poses[3:])):
            frames = sf.blender_frames(sel, split)
            sf.write_blender(d, split, frames, head)
            for k, fr in enumerate(frames):
                sf.write_png(os.path.join(d, fr["file_path"] + ".png"), sf.pattern(6, 8, 100 + k, alpha=name == "blender_rgba"))
        scene.storePly(os.path.join(d, "points3d.ply"), rng.uniform(-1, 1, (25, 3)), rng.integers(0, 256, (25, 3)))


def enter_reference(ref):
    import torch
    sys.path.insert(0, ref)
    plyfile = types.ModuleType("plyfile")

    class PlyData:
        @staticmethod
        def read(path):
            raise RuntimeError("plyfile is not installed")

    plyfile.PlyData, plyfile.PlyElement = PlyData, object
    sys.modules["plyfile"] = plyfile
    sys.modules["cv2"] = types.ModuleType("cv2")
    pkg = types.ModuleType("scene")
    pkg.__path__ = [os.path.join(ref, "scene")]
    sys.modules["scene"] = pkg
    torch.Tensor.cuda = lambda self, *a, **k: self
    # the Blender reader builds a PIL image from an int8 array to take its SIZE; a current PIL refuses int8, so hand it the same bytes
    from PIL import Image
    fromarray = Image.fromarray
    Image.fromarray = lambda a, mode=None: fromarray(a.view(np.uint8) if a.dtype == np.int8 else a, mode)


def infos(tag, cams, root, d):
    d[tag + "_uid"] = np.array([c.uid for c in cams], dtype=np.int64)
    d[tag + "_extrinsic"] = np.array([c.extrinsic for c in cams], dtype=np.float64).reshape(-1, 4, 4)
    d[tag + "_intrinsic"] = np.array([c.intrinsic for c in cams], dtype=np.float64).reshape(-1, 3, 3)
    d[tag + "_name"] = np.array([c.image_name for c in cams], dtype=str)
    d[tag + "_path"] = np.array([os.path.relpath(c.image_path, root).replace(os.sep, "/") for c in cams], dtype=str)
    d[tag + "_size"] = np.array([(c.width, c.height) for c in cams], dtype=np.int64).reshape(-1, 2)


def main(ref):
    write_fixtures()
    enter_reference(os.path.abspath(ref))
    from scene import colmap_loader as cl, dataset_readers as dr
    from utils import camera_utils as cu
    d = {}
    root = os.path.join(OUT, "colmap")
    sparse = os.path.join(root, "sparse", "0")

    # ---- the reference's binary and text readers agree on the fixture
    eb, et = cl.read_extrinsics_binary(os.path.join(sparse, "images.bin")), cl.read_extrinsics_text(os.path.join(sparse, "images.txt"))
    assert list(eb) == list(et)
    for k in eb:
        assert all(np.array_equal(getattr(eb[k], f), getattr(et[k], f)) for f in ("qvec", "tvec"))
        assert (eb[k].camera_id, eb[k].name) == (et[k].camera_id, et[k].name)
        assert np.array_equal(eb[k].xys.reshape(-1, 2), et[k].xys.reshape(-1, 2))
        assert np.array_equal(eb[k].point3D_ids, et[k].point3D_ids)
    pb, pt = cl.read_points3D_binary(os.path.join(sparse, "points3D.bin")), cl.read_points3D_text(os.path.join(sparse, "points3D.txt"))
    assert all(np.array_equal(a, b) for a, b in zip(pb, pt))
    cb = cl.read_intrinsics_binary(os.path.join(sparse, "cameras.bin"))
    with tempfile.TemporaryDirectory() as tmp:
        lines = [ln for ln in open(os.path.join(sparse, "cameras.txt")) if ln.startswith("#") or " PINHOLE " in ln]
        open(os.path.join(tmp, "cameras.txt"), "w").writelines(lines)
        ct = cl.read_intrinsics_text(os.path.join(tmp, "cameras.txt"))
    assert list(ct) == [1] and ct[1].model == cb[1].model and (ct[1].width, ct[1].height) == (cb[1].width, cb[1].height)
    assert np.array_equal(ct[1].params, cb[1].params)

    d["img_id"] = np.array(list(eb), dtype=np.int64)
    d["img_qvec"] = np.array([eb[k].qvec for k in eb], dtype=np.float64)
    d["img_tvec"] = np.array([eb[k].tvec for k in eb], dtype=np.float64)
    d["img_camera_id"] = np.array([eb[k].camera_id for k in eb], dtype=np.int64)
    d["img_name"] = np.array([eb[k].name for k in eb], dtype=str)
    d["img_nobs"] = np.array([len(eb[k].point3D_ids) for k in eb], dtype=np.int64)
    d["img_xys"] = np.concatenate([eb[k].xys.reshape(-1, 2) for k in eb]).astype(np.float64)
    d["img_point3D_ids"] = np.concatenate([np.asarray(eb[k].point3D_ids, dtype=np.int64) for k in eb])
    d["cam_id"] = np.array(list(cb), dtype=np.int64)
    d["cam_model"] = np.array([cb[k].model for k in cb], dtype=str)
    d["cam_size"] = np.array([(cb[k].width, cb[k].height) for k in cb], dtype=np.int64)
    d["cam_nparams"] = np.array([len(cb[k].params) for k in cb], dtype=np.int64)
    d["cam_params"] = np.concatenate([cb[k].params for k in cb]).astype(np.float64)
    d["pts_xyz"], d["pts_rgb"], d["pts_error"] = pb

    # ---- readColmapSceneInfo: no hold-out, llffhold 8 and 3
    for tag, ev, hold in (("colmap_all", False, 8), ("colmap_h8", True, 8), ("colmap_h3", True, 3)):
        info = dr.readColmapSceneInfo(root, None, ev, llffhold=hold)
        assert info.point_cloud is None
        infos(tag + "_train", info.train_cameras, root, d)
        infos(tag + "_test", info.test_cameras, root, d)
        d[tag + "_translate"] = info.nerf_normalization["translate"]
        d[tag + "_radius"] = np.asarray(info.nerf_normalization["radius"])
        if tag == "colmap_h8":
            d["cameras_json"] = np.array(json.dumps([cu.camera_to_JSON(i, c) for i, c in
                                                     enumerate(list(info.test_cameras) + list(info.train_cameras))]))
            args = types.SimpleNamespace(resolution=-1, data_device="cpu")
            cams = cu.cameraList_from_camInfos(info.train_cameras, 1.0, save_memory=False, args=args)
            d["camera_extrinsic_vector"] = np.stack([c.extrinsic_vector.numpy() for c in cams])
            d["camera_intrinsic"] = np.stack([c.intrinsic.numpy() for c in cams])
            d["camera_uid"] = np.array([c.uid for c in cams], dtype=np.int64)
            d["camera_colmap_id"] = np.array([c.colmap_id for c in cams], dtype=np.int64)
            # ---- loadCam's resolution rule, on an 8x6, a 16x12 (both in the fixture) and a 3200x2133 CameraInfo
            wide = info.train_cameras[0]._replace(width=3200, height=2133)
            rows = []
            for ci in (info.train_cameras[0], info.train_cameras[1], wide):
                for res in (1, 2, 4, 8, -1, 400):
                    for rs in (1.0, 2.0):
                        cam = cu.loadCam(types.SimpleNamespace(resolution=res, data_device="cpu"), 0, ci, rs)
                        rows.append((ci.width, ci.height, res, rs, int(cam.intrinsic[0, 2]), int(cam.intrinsic[1, 2])))
            d["loadcam"] = np.array(rows, dtype=np.float64)

    # ---- Blender
    for name in ("blender_angle", "blender_focal", "blender_rgba"):
        broot = os.path.join(OUT, name)
        for tag, ev in ((name + "_eval", True), (name + "_all", False)):
            info = dr.readNerfSyntheticInfo(broot, False, ev)
            infos(tag + "_train", info.train_cameras, broot, d)
            infos(tag + "_test", info.test_cameras, broot, d)
            d[tag + "_translate"] = info.nerf_normalization["translate"]
            d[tag + "_radius"] = np.asarray(info.nerf_normalization["radius"])
    np.savez_compressed(os.path.join(HERE, "scene.npz"), **d)
    print("wrote", os.path.join(HERE, "scene.npz"), len(d), "arrays")


if __name__ == "__main__":
    main(sys.argv[1])
