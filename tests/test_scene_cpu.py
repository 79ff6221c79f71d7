"""CPU: the dataset readers, CameraInfo, normalisation, Camera pose / intrinsics, loadCam's resolution rule and cameras.json
against tests/golden/scene.npz (what the reference returned for the fixtures under tests/golden/scene/, see
tests/golden/make_golden_scene.py), and the error paths."""
import json
import os

import numpy as np
import pytest

from tests import scene_fixture as sf

HERE = os.path.dirname(os.path.abspath(__file__))
FIX = os.path.join(HERE, "golden", "scene")
COLMAP = os.path.join(FIX, "colmap")
SPARSE = os.path.join(COLMAP, "sparse", "0")


@pytest.fixture(scope="module")
def G():
    return np.load(os.path.join(HERE, "golden", "scene.npz"))


@pytest.fixture()
def scene(monkeypatch):
    from c3dgs_amd import scene
    monkeypatch.setattr(scene, "INTRINSIC_DEVICE", "cpu")          # as the golden script places the reference's intrinsic
    return scene


def same(a, b):
    """Equal to the last bit, same dtype and shape."""
    a, b = np.asarray(a), np.asarray(b)
    return a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes()


@pytest.mark.parametrize("kind", ("binary", "text"))
def test_colmap_readers_match_the_reference(G, kind):
    from c3dgs_amd import colmap
    ext = {"binary": "bin", "text": "txt"}[kind]
    images = getattr(colmap, f"read_extrinsics_{kind}")(os.path.join(SPARSE, "images." + ext))
    cameras = getattr(colmap, f"read_intrinsics_{kind}")(os.path.join(SPARSE, "cameras." + ext))
    xyz, rgb, err = getattr(colmap, f"read_points3D_{kind}")(os.path.join(SPARSE, "points3D." + ext))
    assert list(images) == G["img_id"].tolist() and len(images) >= 9
    ims = list(images.values())
    assert [i.id for i in ims] == G["img_id"].tolist()
    assert same(np.array([i.qvec for i in ims]), G["img_qvec"]) and same(np.array([i.tvec for i in ims]), G["img_tvec"])
    assert [i.camera_id for i in ims] == G["img_camera_id"].tolist()
    assert [i.name for i in ims] == G["img_name"].tolist()
    assert sorted(i.name for i in ims) != [i.name for i in ims]                       # sorted order differs from file order
    assert [len(i.point3D_ids) for i in ims] == G["img_nobs"].tolist() and 0 in G["img_nobs"]
    assert all(i.xys.shape == (len(i.point3D_ids), 2) for i in ims)
    assert same(np.concatenate([i.xys for i in ims]), G["img_xys"])
    assert same(np.concatenate([i.point3D_ids for i in ims]), G["img_point3D_ids"])
    assert list(cameras) == G["cam_id"].tolist()
    cs = list(cameras.values())
    assert [c.model for c in cs] == G["cam_model"].tolist() and {c.model for c in cs} == {"PINHOLE", "SIMPLE_PINHOLE"}
    assert [[c.width, c.height] for c in cs] == G["cam_size"].tolist()
    assert [len(c.params) for c in cs] == G["cam_nparams"].tolist()
    assert same(np.concatenate([c.params for c in cs]), G["cam_params"])
    assert same(xyz, G["pts_xyz"]) and same(rgb, G["pts_rgb"]) and same(err, G["pts_error"])


def test_qvec2rotmat_operation_order():
    from c3dgs_amd.colmap import qvec2rotmat
    q = np.array([0.7926102, 0.0342281, 0.6081933, 0.0262642])
    q = q / np.linalg.norm(q)
    R = qvec2rotmat(q)
    w, x, y, z = q
    assert R[0, 0] == 1 - 2 * y ** 2 - 2 * z ** 2 and R[0, 2] == 2 * z * x + 2 * w * y and R[2, 1] == 2 * y * z + 2 * w * x
    assert np.allclose(R @ R.T, np.eye(3), rtol=0, atol=1e-12) and np.linalg.det(R) > 0.999


def _check_infos(G, tag, cams, root):
    assert [c.image_name for c in cams] == G[tag + "_name"].tolist(), tag
    assert [os.path.relpath(c.image_path, root).replace(os.sep, "/") for c in cams] == G[tag + "_path"].tolist(), tag
    assert [c.uid for c in cams] == G[tag + "_uid"].tolist(), tag
    assert [[c.width, c.height] for c in cams] == G[tag + "_size"].tolist(), tag
    if cams:
        assert same(np.array([c.extrinsic for c in cams]), G[tag + "_extrinsic"]), tag
        assert same(np.array([c.intrinsic for c in cams]), G[tag + "_intrinsic"]), tag


def _check_norm(G, tag, norm):
    assert same(norm["translate"], G[tag + "_translate"]), tag
    assert same(np.asarray(norm["radius"]), G[tag + "_radius"]), tag
    assert np.asarray(norm["radius"]).dtype == np.float32              # getWorld2View2 returns float32: the reference's quirk


@pytest.mark.parametrize("source", ("binary", "text"))
def test_colmap_scene_info_matches_the_reference(G, scene, source, tmp_path):
    root = COLMAP
    if source == "text":                                               # the same dataset with the text model alone
        cams, imgs, pts = sf.colmap_dataset(str(tmp_path), seed=0, images=False)
        for name in ("cameras.bin", "images.bin", "points3D.bin"):
            os.remove(tmp_path / "sparse" / "0" / name)
        root = str(tmp_path)
    for tag, ev, hold in (("colmap_all", False, 8), ("colmap_h8", True, 8), ("colmap_h3", True, 3)):
        info = scene.readColmapSceneInfo(root, None, ev, llffhold=hold)
        _check_infos(G, tag + "_train", info.train_cameras, root)
        _check_infos(G, tag + "_test", info.test_cameras, root)
        _check_norm(G, tag, info.nerf_normalization)
        assert info.ply_path == os.path.join(root, "sparse/0/points3D.ply")
        assert info.point_cloud.points.shape == (len(G["pts_xyz"]), 3)
        assert same(info.point_cloud.points, G["pts_xyz"].astype(np.float32))
        assert same(info.point_cloud.colors, G["pts_rgb"] / 255.0)
    assert len(G["colmap_h8_test_name"]) == 2 and len(G["colmap_h3_test_name"]) == 4 and len(G["colmap_all_test_name"]) == 0


def test_camera_pose_and_intrinsics_match_the_reference(G, scene):
    from c3dgs_amd.pipeline import ModelParams
    info = scene.readColmapSceneInfo(COLMAP, None, True)
    args = ModelParams(resolution=-1, data_device="cpu")
    cams = scene.cameraList_from_camInfos(info.train_cameras, 1.0, save_memory=False, args=args)
    assert all(c.extrinsic_vector.device.type == "cpu" and c.extrinsic_vector.dtype.is_floating_point for c in cams)
    assert same(np.stack([c.extrinsic_vector.numpy() for c in cams]), G["camera_extrinsic_vector"])
    assert same(np.stack([c.intrinsic.numpy() for c in cams]), G["camera_intrinsic"])
    assert [c.uid for c in cams] == G["camera_uid"].tolist() and [c.colmap_id for c in cams] == G["camera_colmap_id"].tolist()
    for c, ci in zip(cams, info.train_cameras):
        assert (float(c.intrinsic[0, 2]), float(c.intrinsic[1, 2])) == (ci.width, ci.height)
        assert (c.image_name, c.image_path, c.save_memory, c.flip, c.background) == (ci.image_name, ci.image_path, False, False, None)
        assert str(c.data_device) == "cpu"


def test_loadcam_resolution_rule(G, scene):
    from c3dgs_amd.pipeline import ModelParams
    info = scene.readColmapSceneInfo(COLMAP, None, True)
    by_size = {(ci.width, ci.height): ci for ci in info.train_cameras[:2]}
    by_size[(3200, 2133)] = info.train_cameras[0]._replace(width=3200, height=2133)
    seen = set()
    for w, h, res, rs, want_w, want_h in G["loadcam"].tolist():
        cam = scene.loadCam(ModelParams(resolution=int(res), data_device="cpu"), 0, by_size[(int(w), int(h))], rs)
        assert (cam.image_width, cam.image_height) == (int(want_w), int(want_h)), (w, h, res, rs)
        assert (int(cam.intrinsic[0, 2]), int(cam.intrinsic[1, 2])) == (int(want_w), int(want_h))
        seen.add((int(res), rs))
    assert seen == {(r, s) for r in (1, 2, 4, 8, -1, 400) for s in (1.0, 2.0)}
    wide = scene.loadCam(ModelParams(resolution=-1, data_device="cpu"), 0, by_size[(3200, 2133)], 1.0)
    assert (wide.image_width, wide.image_height) == (1600, 1066)       # the 1600-pixel cap


def test_cameras_json_matches_the_reference(G, scene):
    info = scene.readColmapSceneInfo(COLMAP, None, True)
    ours = [scene.camera_to_JSON(i, c) for i, c in enumerate(list(info.test_cameras) + list(info.train_cameras))]
    assert json.loads(json.dumps(ours)) == json.loads(str(G["cameras_json"]))


@pytest.mark.parametrize("name", ("blender_angle", "blender_focal", "blender_rgba"))
def test_blender_readers_match_the_reference(G, scene, name):
    root = os.path.join(FIX, name)
    for tag, ev in ((name + "_eval", True), (name + "_all", False)):
        info = scene.readNerfSyntheticInfo(root, False, ev)
        _check_infos(G, tag + "_train", info.train_cameras, root)
        _check_infos(G, tag + "_test", info.test_cameras, root)
        _check_norm(G, tag, info.nerf_normalization)
        assert info.point_cloud.points.shape == (25, 3)
    assert len(G[name + "_eval_test_name"]) == 2 and len(G[name + "_all_train_name"]) == 5
    # w, h, cx, cy persist across the frames once set: every frame carries the first frame's
    cams = scene.readCamerasFromTransforms(root, "transforms_train.json", False)
    assert {(c.width, c.height, c.intrinsic[0, 2], c.intrinsic[1, 2]) for c in cams} == {(8, 6, 4.0, 3.0)}


def test_blender_size_persists_from_the_first_frame(scene, tmp_path):
    """Only the FIRST image is opened when the head gives no size: a second frame of another size keeps the first one's."""
    frames = sf.blender_frames(sf.ring(2, radius=3.0), "train")
    sf.write_blender(str(tmp_path), "train", frames, {"camera_angle_x": 0.7})
    sf.write_png(str(tmp_path / "train" / "r_0.png"), sf.pattern(6, 8, 0))
    sf.write_png(str(tmp_path / "train" / "r_1.png"), sf.pattern(10, 20, 1))
    cams = scene.readCamerasFromTransforms(str(tmp_path), "transforms_train.json", False)
    assert [(c.width, c.height) for c in cams] == [(8, 6), (8, 6)]
    assert cams[1].intrinsic[0, 2] == 4.0 and cams[1].intrinsic[1, 2] == 3.0 and cams[1].intrinsic[0, 0] == 0.7


def test_dust3r_reader(scene, tmp_path):
    sf.dust3r_dataset(str(tmp_path), views=3)
    info = scene.readDustrInfo(str(tmp_path), False, True)
    assert len(info.train_cameras) == 3 and info.test_cameras == [] and info.point_cloud is None
    assert info.nerf_normalization == {"translate": [0.0, 0.0, 0.0], "radius": 1.0}
    c = info.train_cameras[1]
    assert (c.width, c.height, c.image_name) == (8, 6, "d_1") and c.intrinsic[0, 0] == scene.focal2fov(1.2 * 8, 8)
    assert set(scene.sceneLoadTypeCallbacks) == {"Colmap", "Blender", "Dust3r"}


def test_unsupported_camera_model_raises(scene, tmp_path):
    cams, imgs, pts = sf.colmap_dataset(str(tmp_path), seed=1, views=3, images=False)
    sf.write_colmap(str(tmp_path), [(1, "OPENCV", 8, 6, [9.0, 9.0, 4.0, 3.0, 0.1, 0.0, 0.0, 0.0]), cams[1]], imgs, pts)
    with pytest.raises(ValueError, match="OPENCV"):
        scene.readColmapSceneInfo(str(tmp_path), None, False)


def test_truncated_images_bin_raises_and_names_the_path(scene, tmp_path):
    from c3dgs_amd import colmap
    sf.colmap_dataset(str(tmp_path), seed=2, images=False)
    path = tmp_path / "sparse" / "0" / "images.bin"
    whole = path.read_bytes()
    for cut in (4, 8, 40, 75, len(whole) // 2, len(whole) - 1):
        path.write_bytes(whole[:cut])
        with pytest.raises(ValueError, match="images.bin"):
            colmap.read_extrinsics_binary(str(path))
    with pytest.raises(ValueError, match="images.bin"):               # present but unreadable: no quiet switch to the text model
        scene.readColmapSceneInfo(str(tmp_path), None, False)
    path.write_bytes(b"\xff" * 8 + whole[8:])                         # an absurd count
    with pytest.raises(ValueError, match="images.bin"):
        colmap.read_extrinsics_binary(str(path))
    for name, reader in (("cameras.bin", colmap.read_intrinsics_binary), ("points3D.bin", colmap.read_points3D_binary)):
        p = tmp_path / "sparse" / "0" / name
        p.write_bytes(p.read_bytes()[:-3])
        with pytest.raises(ValueError, match=name):
            reader(str(p))
    txt = tmp_path / "sparse" / "0" / "images.txt"
    txt.write_text("1 0.5 0.5 0.5\n\n")
    with pytest.raises(ValueError, match="images.txt"):
        colmap.read_extrinsics_text(str(txt))


class _Model:
    def load_ply(self, path):
        self.loaded = path

    def load(self, path, override_quantization=False):
        self.loaded = path


def test_unrecognised_directory_raises(scene, tmp_path):
    from c3dgs_amd.pipeline import ModelParams
    (tmp_path / "src").mkdir()
    args = ModelParams(source_path=str(tmp_path / "src"), model_path=str(tmp_path / "out"), data_device="cpu").extract()
    with pytest.raises(ValueError, match="scene type"):
        scene.Scene(args, _Model())


def test_scene_on_the_host_side(G, scene, tmp_path):
    """Everything of Scene that needs no GPU: detection, input.ply, cameras.json, split and order, extent, flip and background."""
    from c3dgs_amd.pipeline import ModelParams
    args = ModelParams(source_path=COLMAP, model_path=str(tmp_path / "out"), eval=True, data_device="cpu").extract()
    assert os.path.isabs(args.source_path) and (args.images, args.resolution, args.white_background, args.sh_degree) == ("images", -1, False, 3)
    m = _Model()
    s = scene.Scene(args, m, shuffle=False)
    assert s.kind == "Colmap" and len(s) == 10 and s.loaded_iter is None
    assert [c.image_name for c in s.getTrainCameras()] == G["colmap_h8_train_name"].tolist()
    assert [c.image_name for c in s.getTestCameras()] == G["colmap_h8_test_name"].tolist()
    assert s.getSomeCameras()[1] == "test"
    assert s.cameras_extent == G["colmap_h8_radius"] and m.spatial_lr_scale == s.cameras_extent
    assert m.loaded == os.path.join(COLMAP, "sparse/0/points3D.ply")
    assert open(tmp_path / "out" / "input.ply", "rb").read() == open(m.loaded, "rb").read()
    assert json.load(open(tmp_path / "out" / "cameras.json")) == json.loads(str(G["cameras_json"]))
    assert not any(c.flip for c in s.getTrainCameras()) and all(c.background is None for c in s.getTrainCameras())

    args = ModelParams(source_path=os.path.join(FIX, "blender_rgba"), model_path=str(tmp_path / "b"), white_background=True,
                       data_device="cpu").extract()
    s = scene.Scene(args, _Model(), shuffle=False, composite_background=True)
    assert s.kind == "Blender" and len(s.getTrainCameras()) == 5 and s.getSomeCameras()[1] == "train"
    assert all(c.background == [1.0, 1.0, 1.0] and not c.flip for c in s.getTrainCameras())

    sf.dust3r_dataset(str(tmp_path / "d3"))
    args = ModelParams(source_path=str(tmp_path / "d3"), model_path=str(tmp_path / "d"), data_device="cpu").extract()
    s = scene.Scene(args, _Model(), shuffle=False)
    assert s.kind == "Dust3r" and all(c.flip for c in s.getTrainCameras()) and s.cameras_extent == 1.0


def test_scene_shuffles_with_pythons_random(scene, tmp_path):
    import random
    from c3dgs_amd.pipeline import ModelParams
    args = ModelParams(source_path=COLMAP, model_path=str(tmp_path / "out"), data_device="cpu").extract()
    random.seed(4)
    got = [c.image_name for c in scene.Scene(args, _Model()).getTrainCameras()]
    names = sorted(got)
    random.seed(4)
    random.shuffle(names)
    assert got == names and got != sorted(got)


def test_search_for_max_iteration(scene, tmp_path):
    for it in (7, 30000, 120):
        (tmp_path / f"iteration_{it}").mkdir()
    assert scene.searchForMaxIteration(str(tmp_path)) == 30000


def test_store_and_fetch_ply_round_trip(scene, tmp_path):
    from c3dgs_amd import ply
    rng = np.random.default_rng(0)
    xyz, rgb = rng.uniform(-2, 2, (17, 3)), rng.integers(0, 256, (17, 3)).astype(np.float64)
    path = str(tmp_path / "p.ply")
    scene.storePly(path, xyz, rgb)
    head = open(path, "rb").read(300)
    assert b"property float nz\nproperty uchar red\n" in head and b"element vertex 17\n" in head
    v = ply.read_ply(path)
    assert v["red"].dtype == np.uint8 and v["x"].dtype == np.float32
    pc = scene.fetchPly(path)
    assert same(pc.points, xyz.astype(np.float32)) and same(pc.colors, rgb / 255.0) and not pc.normals.any()
