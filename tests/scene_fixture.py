"""Datasets on disk, from a seed: COLMAP sparse models (binary and text), Blender transforms and Dust3r transforms with their
PNGs and point clouds. Test infrastructure, shared by tests/golden/make_golden_scene.py, tests/test_scene_*.py and
tools/run_scene.py. The writers follow COLMAP's published formats (https://colmap.github.io/format.html), independently of the
readers in c3dgs_amd/colmap.py.

    ring(n, ...)                       world-to-camera poses on an arc, looking at the origin
    write_colmap(root, cams, imgs, pts)   sparse/0/{cameras,images,points3D}.{bin,txt}
    write_blender(root, name, frames, head)   transforms_<name>.json
    write_png(path, array)             8-bit RGB / RGBA (16-bit greyscale for uint16 input)
    rendered_blender(root, ...)        GPU: a Blender set whose PNGs are renders of a hidden model by our own rasterizer
"""
import json
import os
import struct

import numpy as np


def rotmat2qvec(R):
    """(w, x, y, z) of a rotation whose 1 + trace is well away from 0."""
    w = np.sqrt(1.0 + R[0, 0] + R[1, 1] + R[2, 2]) / 2.0
    q = np.array([w, (R[2, 1] - R[1, 2]) / (4 * w), (R[0, 2] - R[2, 0]) / (4 * w), (R[1, 0] - R[0, 1]) / (4 * w)])
    return q / np.linalg.norm(q)


def ring(n, radius=4.0, arc=np.deg2rad(150.0), height=0.4, seed=0):
    """n world-to-camera (R, t) pairs (COLMAP axes: x right, y down, z forward) on an arc around the origin, looking at it. The
    arc keeps every rotation at 1 + trace >= 0.5 (the reference's mat_to_quat divides by sqrt(1 + trace))."""
    rng = np.random.default_rng(seed)
    out = []
    for k in range(n):
        a = -arc / 2 + arc * k / max(n - 1, 1)
        centre = np.array([radius * np.sin(a), height * np.cos(3 * a) + 0.05 * rng.standard_normal(), -radius * np.cos(a)])
        fwd = -centre / np.linalg.norm(centre)
        right = np.cross(np.array([0.0, 1.0, 0.0]), fwd)   # the world's y points down, like the cameras'
        right = right / np.linalg.norm(right)
        down = np.cross(fwd, right)
        R = np.stack([right, down, fwd])                    # rows: camera axes in world coordinates
        assert 1.0 + np.trace(R) >= 0.5 and np.linalg.det(R) > 0.99
        out.append((R, -R @ centre))
    return out


def write_png(path, a):
    from PIL import Image
    a = np.asarray(a)
    os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
    if a.dtype == np.uint16:
        Image.fromarray(a).save(path)                       # mode I;16
    elif a.ndim == 2:
        Image.fromarray(a.astype(np.uint8), "L").save(path)
    else:
        Image.fromarray(a.astype(np.uint8), "RGBA" if a.shape[2] == 4 else "RGB").save(path)


def pattern(H, W, seed, alpha=False):
    """A smooth colour ramp plus noise, uint8 [H][W][3|4]."""
    rng = np.random.default_rng(seed)
    y, x = np.mgrid[0:H, 0:W]
    img = np.stack([x * 255 // max(W - 1, 1), y * 255 // max(H - 1, 1), (x + y + seed) * 37 % 256], axis=2)
    img = np.clip(img + rng.integers(-20, 21, size=img.shape), 0, 255).astype(np.uint8)
    if alpha:
        img = np.concatenate([img, rng.integers(0, 256, size=(H, W, 1)).astype(np.uint8)], axis=2)
    return img


_MODEL_IDS = {"SIMPLE_PINHOLE": 0, "PINHOLE": 1, "SIMPLE_RADIAL": 2, "OPENCV": 4}


def write_colmap(root, cameras, images, points, binary=True, text=True):
    """cameras: [(id, model, width, height, params)], images: [(id, qvec, tvec, camera_id, name, [(x, y, point3D_id)])],
    points: [(id, xyz, rgb, error, [(image_id, point2D_idx)])] -> root/sparse/0/."""
    d = os.path.join(root, "sparse", "0")
    os.makedirs(d, exist_ok=True)
    if binary:
        with open(os.path.join(d, "cameras.bin"), "wb") as f:
            f.write(struct.pack("<Q", len(cameras)))
            for cid, model, w, h, params in cameras:
                f.write(struct.pack("<iiQQ", cid, _MODEL_IDS[model], w, h) + struct.pack(f"<{len(params)}d", *params))
        with open(os.path.join(d, "images.bin"), "wb") as f:
            f.write(struct.pack("<Q", len(images)))
            for iid, q, t, cid, name, obs in images:
                f.write(struct.pack("<I7dI", iid, *q, *t, cid) + name.encode("utf-8") + b"\0" + struct.pack("<Q", len(obs)))
                for x, y, pid in obs:
                    f.write(struct.pack("<ddq", x, y, pid))
        with open(os.path.join(d, "points3D.bin"), "wb") as f:
            f.write(struct.pack("<Q", len(points)))
            for pid, xyz, rgb, err, track in points:
                f.write(struct.pack("<Q3d3BdQ", pid, *xyz, *rgb, err, len(track)))
                for iid, k in track:
                    f.write(struct.pack("<II", iid, k))
    if text:
        with open(os.path.join(d, "cameras.txt"), "w") as f:
            f.write(f"# Camera list with one line of data per camera:\n#   CAMERA_ID, MODEL, WIDTH, HEIGHT, PARAMS[]\n# Number of cameras: {len(cameras)}\n")
            for cid, model, w, h, params in cameras:
                f.write(" ".join([str(cid), model, str(w), str(h)] + [repr(float(p)) for p in params]) + "\n")
        with open(os.path.join(d, "images.txt"), "w") as f:
            f.write("# Image list with two lines of data per image:\n#   IMAGE_ID, QW, QX, QY, QZ, TX, TY, TZ, CAMERA_ID, NAME\n#   POINTS2D[] as (X, Y, POINT3D_ID)\n")
            for iid, q, t, cid, name, obs in images:
                f.write(" ".join([str(iid)] + [repr(float(v)) for v in list(q) + list(t)] + [str(cid), name]) + "\n")
                f.write(" ".join(f"{float(x)!r} {float(y)!r} {pid}" for x, y, pid in obs) + "\n")
        with open(os.path.join(d, "points3D.txt"), "w") as f:
            f.write("# 3D point list with one line of data per point:\n#   POINT3D_ID, X, Y, Z, R, G, B, ERROR, TRACK[] as (IMAGE_ID, POINT2D_IDX)\n")
            for pid, xyz, rgb, err, track in points:
                f.write(" ".join([str(pid)] + [repr(float(v)) for v in xyz] + [str(int(v)) for v in rgb] + [repr(float(err))]
                                 + [f"{iid} {k}" for iid, k in track]) + "\n")


def colmap_dataset(root, seed=0, views=10, W=8, H=6, n_points=40, images=True):
    """A small COLMAP dataset: camera 1 PINHOLE W x H, camera 2 SIMPLE_PINHOLE 2W x 2H; image names whose sorted order differs
    from the file order; images with no, few and many observations; points with empty and long tracks.
    -> (cameras, images, points) as written."""
    rng = np.random.default_rng(seed)
    cameras = [(1, "PINHOLE", W, H, [1.2 * W, 1.1 * W, W / 2 + 0.25, H / 2 - 0.5]),
               (2, "SIMPLE_PINHOLE", 2 * W, 2 * H, [2.3 * W, float(W), float(H)])]
    order = rng.permutation(views)
    imgs = []
    for k, (R, t) in enumerate(ring(views, seed=seed)):
        obs = [(float(rng.uniform(0, W)), float(rng.uniform(0, H)), int(rng.integers(-1, n_points))) for _ in range((k * 3) % 7)]
        imgs.append((k + 1, rotmat2qvec(R).tolist(), t.tolist(), 1 + (k % 3 == 1), f"view_{order[k]:02d}.png", obs))
    points = []
    for p in range(n_points):
        track = [(int(rng.integers(1, views + 1)), int(rng.integers(0, 6))) for _ in range(p % 5)]
        points.append((p + 1, rng.uniform(-1, 1, 3).tolist(), rng.integers(0, 256, 3).tolist(), float(rng.uniform(0, 2)), track))
    write_colmap(root, cameras, imgs, points)
    if images:
        for iid, _, _, cid, name, _ in imgs:
            write_png(os.path.join(root, "images", name), pattern(H, W, seed + iid))
    return cameras, imgs, points


def blender_frames(poses, folder, names=None):
    """world-to-camera (R, t) in COLMAP axes -> frames with Blender camera-to-world matrices (y up, z back)."""
    frames = []
    for k, (R, t) in enumerate(poses):
        w2c = np.eye(4)
        w2c[:3, :3], w2c[:3, 3] = R, t
        c2w = np.linalg.inv(w2c)
        c2w[:3, 1:3] *= -1
        frames.append({"file_path": f"./{folder}/{names[k] if names else 'r_%d' % k}", "transform_matrix": c2w.tolist()})
    return frames


def write_blender(root, name, frames, head):
    os.makedirs(root, exist_ok=True)
    with open(os.path.join(root, f"transforms_{name}.json"), "w") as f:
        json.dump({**head, "frames": frames}, f, indent=1)


def write_point_ply(path, xyz, rgb):
    """x y z red green blue, the point-cloud PLY GaussianModel.load_ply reads."""
    from c3dgs_amd import ply
    xyz, rgb = np.asarray(xyz, dtype=np.float32), np.asarray(rgb, dtype=np.float32)
    ply.write_ply(path, {"x": xyz[:, 0], "y": xyz[:, 1], "z": xyz[:, 2], "red": rgb[:, 0], "green": rgb[:, 1], "blue": rgb[:, 2]})


def dust3r_dataset(root, seed=0, views=3, W=8, H=6):
    """transforms_dust3r.json (camera-to-world and a pixel intrinsic matrix per frame), scene.ply and the PNGs."""
    rng = np.random.default_rng(seed)
    frames = []
    for k, (R, t) in enumerate(ring(views, seed=seed)):
        w2c = np.eye(4)
        w2c[:3, :3], w2c[:3, 3] = R, t
        frames.append({"file_path": f"images/d_{k}.png", "transform_matrix": np.linalg.inv(w2c).tolist(),
                       "intrinsic_matrix": [[1.2 * W, 0.0, W / 2], [0.0, 1.2 * W, H / 2], [0.0, 0.0, 1.0]]})
        write_png(os.path.join(root, "images", f"d_{k}.png"), pattern(H, W, seed + k))
    with open(os.path.join(root, "transforms_dust3r.json"), "w") as f:
        json.dump({"frames": frames}, f)
    write_point_ply(os.path.join(root, "scene.ply"), rng.uniform(-1, 1, (30, 3)), rng.integers(0, 256, (30, 3)))


def rendered_blender(root, views=8, hold_every=4, W=64, H=48, focal=60.0, P_teacher=1500, keep_every=4, device="cuda", seed=31):
    """GPU. A Blender dataset whose ground truth is rendered from a hidden model with our own rasterizer: a synth-v1 teacher in
    front of `views` nearby cameras, every `hold_every`-th view in transforms_test.json, the rest in transforms_train.json,
    and every `keep_every`-th teacher position as points3d.ply. -> number of points written."""
    import torch
    from c3dgs_amd import scene as sc
    from c3dgs_amd.model import PipelineParams
    from tests import train_scene
    teacher, s = train_scene.teacher_model(P_teacher, W, H, focal, device, seed=seed)
    poses = []
    for k in range(views):
        a = 2 * np.pi * k / views
        c, sn = np.cos(0.03 * np.sin(a)), np.sin(0.03 * np.sin(a))
        R = np.array([[c, 0.0, sn], [0.0, 1.0, 0.0], [-sn, 0.0, c]])
        poses.append((R, np.array([0.25 * np.cos(a), 0.25 * np.sin(a), 0.0])))
    head = {"camera_angle_x": 2.0 * np.arctan(W / (2.0 * focal)), "w": W, "h": H}
    held = [k for k in range(views) if k % hold_every == 0]
    kept = [k for k in range(views) if k % hold_every != 0]
    write_blender(root, "train", blender_frames([poses[k] for k in kept], "train", [f"r_{k}" for k in kept]), head)
    write_blender(root, "test", blender_frames([poses[k] for k in held], "test", [f"r_{k}" for k in held]), head)
    bg = torch.zeros(3, device=device)
    for name in ("train", "test"):
        for info in sc.readCamerasFromTransforms(root, f"transforms_{name}.json", False):
            cam = sc.Camera(info.uid, info.extrinsic, info.intrinsic, H, W, info.image_name, info.image_path, info.uid,
                            data_device=device)
            with torch.no_grad():
                img = teacher.render(cam, PipelineParams(), bg)["render"].clamp(0, 1)
            write_png(info.image_path, (img.permute(1, 2, 0) * 255.0 + 0.5).to(torch.uint8).cpu().numpy())
    xyz = s["means3D"][::keep_every].numpy()
    rgb = np.clip((0.5 + 0.28209479177387814 * s["shs"][::keep_every, 0].numpy()) * 255.0, 0, 255).round()
    write_point_ply(os.path.join(root, "points3d.ply"), xyz, rgb)
    return xyz.shape[0]
