"""-m gpu: c3dgs_image_from_u8 against tests/image_ref.py bit for bit, Camera.original_image, Scene on the golden fixtures and
one end-to-end run (dataset on disk -> Scene -> pipeline.train -> render_and_eval).

The image path is pinned by our own restatement of OpenCV's documented INTER_LINEAR (tests/image_ref.py), not by cv2.resize.
"""
import ctypes as C
import itertools
import json
import os

import numpy as np
import pytest
import torch
from PIL import Image as PILImage

from tests import image_ref, scene_fixture as sf

pytestmark = pytest.mark.gpu
DEV = "cuda"
HERE = os.path.dirname(os.path.abspath(__file__))
FIX = os.path.join(HERE, "golden", "scene")
GUARD = 64                       # sentinel bytes / floats on each side of src / out
SENTINEL = -7.0
BGS = (None, (1.0, 1.0, 1.0), (0.1, 0.7, 0.33))


def run_kernel(hip, src, Hd, Wd, flip=0, bg=None, src_shift=0, out_shift=0, stream=None):
    """The C entry on `src` placed `src_shift` bytes and `out` placed `out_shift` floats into larger buffers filled with
    sentinels (so every alignment of both is reached); asserts the sentinels around `out` are untouched. -> float32 [3][Hd][Wd]"""
    from c3dgs_amd import _lib
    Hs, Ws, Cn = src.shape
    n_src, n_out = src.size, 3 * Hd * Wd
    sbuf = torch.full((GUARD + src_shift + n_src + GUARD,), 0xAB, dtype=torch.uint8, device=DEV)
    sbuf[GUARD + src_shift:GUARD + src_shift + n_src] = torch.from_numpy(src.reshape(-1)).to(DEV)
    obuf = torch.full((GUARD + out_shift + n_out + GUARD,), SENTINEL, dtype=torch.float32, device=DEV)
    bgt = torch.tensor(bg, dtype=torch.float32, device=DEV) if bg is not None else None
    s = stream if stream is not None else torch.cuda.current_stream()
    if stream is not None:
        stream.wait_stream(torch.cuda.current_stream())
    rc = _lib.lib().c3dgs_image_from_u8(Hs, Ws, Cn, sbuf.data_ptr() + GUARD + src_shift, flip, bgt.data_ptr() if bgt is not None else None,
                                        Hd, Wd, obuf.data_ptr() + 4 * (GUARD + out_shift), C.c_void_p(s.cuda_stream))
    _lib.check(rc)
    s.synchronize()
    host = obuf.cpu().numpy()
    lo = GUARD + out_shift
    assert (host[:lo] == SENTINEL).all() and (host[lo + n_out:] == SENTINEL).all(), "the kernel wrote outside out"
    assert (sbuf[:GUARD + src_shift] == 0xAB).all() and (sbuf[GUARD + src_shift + n_src:] == 0xAB).all()
    return host[lo:lo + n_out].reshape(3, Hd, Wd)


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


@pytest.mark.parametrize("shape", image_ref.SHAPES, ids=lambda s: "%dx%d-%dx%d" % (s[0] + s[1]))
def test_kernel_matches_the_restatement_bit_for_bit(hip, shape):
    (Hs, Ws), (Hd, Wd) = shape
    rng = np.random.default_rng(Hs * 1000 + Wd)
    k = 0
    for Cn in (3, 4):
        src = rng.integers(0, 256, size=(Hs, Ws, Cn), dtype=np.uint8)
        for flip, bg in itertools.product((0, 1), BGS if Cn == 4 else (None,)):
            want = image_ref.image_from_u8(src, Hd, Wd, flip, None if bg is None else np.array(bg, np.float32))
            got = run_kernel(hip, src, Hd, Wd, flip, bg, src_shift=k % 4, out_shift=(k // 2) % 4)   # every alignment of both
            diff = bits(got) != bits(want)
            assert not diff.any(), (shape, Cn, flip, bg, int(diff.sum()), float(np.abs(got - want).max()))
            k += 1


def test_every_byte_value_at_equal_size(hip):
    src = np.arange(256, dtype=np.uint8).reshape(16, 16, 1).repeat(3, axis=2)
    got = run_kernel(hip, src, 16, 16)
    assert np.array_equal(bits(got[1].ravel()), bits(np.arange(256, dtype=np.float32) / np.float32(255)))


@pytest.mark.parametrize("alpha", ("zero", "opaque", "random"))
def test_alpha_planes_and_black_background(hip, alpha):
    rng = np.random.default_rng(9)
    src = rng.integers(0, 256, size=(23, 37, 4), dtype=np.uint8)
    if alpha != "random":
        src[:, :, 3] = 0 if alpha == "zero" else 255
    for Hd, Wd in ((23, 37), (9, 16), (31, 53)):
        plain = run_kernel(hip, src, Hd, Wd)
        black = run_kernel(hip, src, Hd, Wd, bg=(0.0, 0.0, 0.0))
        assert np.array_equal(bits(plain), bits(black))
        assert np.array_equal(bits(plain), bits(image_ref.image_from_u8(src, Hd, Wd)))
        white = run_kernel(hip, src, Hd, Wd, bg=(1.0, 1.0, 1.0))
        if alpha == "zero":
            assert not plain.any() and (white == 1.0).all()
        if alpha == "opaque":
            assert np.array_equal(bits(white), bits(run_kernel(hip, np.ascontiguousarray(src[:, :, :3]), Hd, Wd)))


def test_repeatable_and_stream_independent(hip):
    rng = np.random.default_rng(11)
    src = rng.integers(0, 256, size=(143, 611, 4), dtype=np.uint8)
    a = run_kernel(hip, src, 71, 301, 1, (0.1, 0.7, 0.33))
    b = run_kernel(hip, src, 71, 301, 1, (0.1, 0.7, 0.33))
    c = run_kernel(hip, src, 71, 301, 1, (0.1, 0.7, 0.33), stream=torch.cuda.Stream())
    assert np.array_equal(bits(a), bits(b)) and np.array_equal(bits(a), bits(c))


def test_python_wrapper_validates(hip):
    from c3dgs_amd import image_io
    src = torch.zeros(4, 5, 3, dtype=torch.uint8, device=DEV)
    assert image_io.image_from_u8(src, 2, 3).shape == (3, 2, 3)
    with pytest.raises(ValueError):
        image_io.image_from_u8(src.cpu(), 2, 3)
    with pytest.raises(ValueError):
        image_io.image_from_u8(src.float(), 2, 3)
    with pytest.raises(RuntimeError, match="alpha"):
        image_io.image_from_u8(src, 2, 3, background=(1.0, 1.0, 1.0))
    with pytest.raises(RuntimeError, match="32768"):
        image_io.image_from_u8(src, 2, 40000)


# ------------------------------------------------------------------------------------------------ Camera.original_image
def _camera(path, h, w, **kw):
    from c3dgs_amd import scene
    return scene.Camera(0, np.eye(4), np.array([[0.8, 0, 4.0], [0, 0.6, 3.0], [0, 0, 1.0]]), h, w, "img", str(path), 0, **kw)


def test_original_image_caching_contract(hip, tmp_path, monkeypatch):
    from c3dgs_amd import image_io
    reads = []
    decode = image_io.decode_u8
    monkeypatch.setattr(image_io, "decode_u8", lambda p: (reads.append(p), decode(p))[1])
    src = sf.pattern(12, 20, 3, alpha=True)
    want = image_ref.image_from_u8(src, 9, 16)

    p = tmp_path / "keep.png"
    sf.write_png(str(p), src)
    cam = _camera(p, 9, 16, save_memory=False)
    assert not reads                                                  # nothing is read before the first access
    a = cam.original_image
    assert cam.original_image is a and cam._bytes is None             # the same object; the uint8 tensor is released
    assert a.shape == (3, 9, 16) and a.dtype == torch.float32 and a.device.type == "cuda"
    assert np.array_equal(bits(a.cpu().numpy()), bits(want)) and len(reads) == 1

    q = tmp_path / "lean.png"
    sf.write_png(str(q), src)
    cam = _camera(q, 9, 16, save_memory=True)
    a = cam.original_image
    os.remove(q)                                                      # the file is not read again
    b = cam.original_image
    assert a is not b and a.data_ptr() != b.data_ptr() and cam._image is None
    assert cam._bytes.dtype == torch.uint8 and tuple(cam._bytes.shape) == (12, 20, 4) and len(reads) == 2
    assert np.array_equal(bits(a.cpu().numpy()), bits(want)) and np.array_equal(bits(b.cpu().numpy()), bits(want))

    r = tmp_path / "host.png"
    sf.write_png(str(r), src)
    cam = _camera(r, 9, 16, data_device="cpu", flip=True, background=(1.0, 1.0, 1.0))
    img = cam.original_image
    assert img.device.type == "cpu" and cam.intrinsic.is_cuda and cam.extrinsic_vector.device.type == "cpu"
    assert np.array_equal(bits(img.numpy()), bits(image_ref.image_from_u8(src, 9, 16, 1, np.ones(3, np.float32))))
    rgb = tmp_path / "rgb.png"
    sf.write_png(str(rgb), src[:, :, :3])                             # a background is ignored without an alpha channel
    img = _camera(rgb, 12, 20, background=(1.0, 1.0, 1.0)).original_image
    assert np.array_equal(bits(img.cpu().numpy()), bits(image_ref.image_from_u8(src[:, :, :3], 12, 20)))


def test_original_image_refuses_other_modes(hip, tmp_path):
    sf.write_png(str(tmp_path / "g16.png"), np.full((6, 8), 40000, np.uint16))
    sf.write_png(str(tmp_path / "g8.png"), np.full((6, 8), 100, np.uint8))
    for name in ("g16.png", "g8.png"):
        with pytest.raises(ValueError, match=name):
            _camera(tmp_path / name, 6, 8).original_image


# ------------------------------------------------------------------------------------------------ Scene
def _model(quantization=False):
    from c3dgs_amd.model import GaussianModel
    return GaussianModel(3, quantization=quantization, device=DEV)


def _args(source, out, **kw):
    from c3dgs_amd.pipeline import ModelParams
    return ModelParams(source_path=str(source), model_path=str(out), **kw).extract()


def test_scene_on_the_golden_colmap_fixture(hip, tmp_path):
    from c3dgs_amd import scene
    G = np.load(os.path.join(HERE, "golden", "scene.npz"))
    root = os.path.join(FIX, "colmap")
    m = _model()
    s = scene.Scene(_args(root, tmp_path / "out", eval=True), m, shuffle=False)
    assert [c.image_name for c in s.getTrainCameras()] == G["colmap_h8_train_name"].tolist()
    assert [c.image_name for c in s.getTestCameras()] == G["colmap_h8_test_name"].tolist()
    assert len(s) == 10 and m._xyz.shape[0] == len(G["pts_xyz"])
    assert s.cameras_extent == G["colmap_h8_radius"] and m.spatial_lr_scale == s.cameras_extent
    assert os.path.getsize(tmp_path / "out" / "input.ply") > 0
    assert json.load(open(tmp_path / "out" / "cameras.json")) == json.loads(str(G["cameras_json"]))
    assert not any(c.flip for c in s.getTrainCameras() + s.getTestCameras())
    for cam in s.getTrainCameras():                                   # 8x6 files; the second camera model is 16x12
        img = cam.original_image
        assert tuple(img.shape) == (3, cam.image_height, cam.image_width) and img.is_cuda
        src = np.asarray(PILImage.open(cam.image_path))
        assert np.array_equal(bits(img.cpu().numpy()), bits(image_ref.image_from_u8(src, cam.image_height, cam.image_width)))
    assert {(c.image_width, c.image_height) for c in s.getTrainCameras()} == {(8, 6), (16, 12)}

    s.save(7)
    m2 = _model()
    s2 = scene.Scene(_args(root, tmp_path / "out", eval=True), m2, load_iteration=-1, shuffle=False)
    assert s2.loaded_iter == 7
    assert torch.equal(m2._xyz, m._xyz) and torch.equal(m2._opacity, m._opacity) and torch.equal(m2._features_dc, m._features_dc)
    assert torch.allclose(m2.get_scaling, m.get_scaling, rtol=1e-5, atol=0) and torch.allclose(m2.get_rotation, m.get_rotation, atol=1e-6)


def test_scene_on_the_golden_blender_fixtures_and_dust3r(hip, tmp_path):
    from c3dgs_amd import scene
    G = np.load(os.path.join(HERE, "golden", "scene.npz"))
    for name in ("blender_angle", "blender_rgba"):
        m = _model()
        s = scene.Scene(_args(os.path.join(FIX, name), tmp_path / name, eval=True, white_background=name == "blender_rgba"), m,
                        shuffle=False, composite_background=True)
        assert [c.image_name for c in s.getTrainCameras()] == G[name + "_eval_train_name"].tolist()
        assert [c.image_name for c in s.getTestCameras()] == G[name + "_eval_test_name"].tolist()
        assert m._xyz.shape[0] == 25 and s.cameras_extent == G[name + "_eval_radius"] == m.spatial_lr_scale
        assert os.path.exists(tmp_path / name / "input.ply") and os.path.exists(tmp_path / name / "cameras.json")
        assert not any(c.flip for c in s.getTrainCameras())
        cam = s.getTestCameras()[0]
        src = np.asarray(PILImage.open(cam.image_path))
        bg = np.ones(3, np.float32) if src.shape[2] == 4 else None
        assert src.shape[2] == (4 if name == "blender_rgba" else 3)
        assert np.array_equal(bits(cam.original_image.cpu().numpy()), bits(image_ref.image_from_u8(src, 6, 8, 0, bg)))
    sf.dust3r_dataset(str(tmp_path / "d3"))
    s = scene.Scene(_args(tmp_path / "d3", tmp_path / "d3out"), _model(), shuffle=False)
    assert s.kind == "Dust3r" and all(c.flip for c in s.getTrainCameras())
    cam = s.getTrainCameras()[1]
    src = np.asarray(PILImage.open(cam.image_path))
    assert np.array_equal(bits(cam.original_image.cpu().numpy()), bits(image_ref.image_from_u8(src, 6, 8, flip=1)))


def test_end_to_end_from_a_dataset_on_disk(hip, tmp_path):
    """Eight 64x48 views rendered from a hidden model, every fourth held out: Scene -> pipeline.train -> render_and_eval."""
    from c3dgs_amd import metrics, pipeline, scene
    from c3dgs_amd.model import PipelineParams
    from tests import train_scene
    n_points = sf.rendered_blender(str(tmp_path / "data"), views=8, hold_every=4, W=64, H=48)
    m = _model(quantization=True)
    s = scene.Scene(_args(tmp_path / "data", tmp_path / "out", eval=True), m, shuffle=False, save_memory=True)
    assert (len(s.getTrainCameras()), len(s.getTestCameras()), m._xyz.shape[0]) == (6, 2, n_points)
    assert [c.image_name for c in s.getTestCameras()] == ["r_0", "r_4"]
    bg = torch.zeros(3, device=DEV)
    before = metrics.render_and_eval(m, s.getTestCameras(), PipelineParams(), bg)["PSNR"]
    losses = []
    torch.manual_seed(0)
    n = pipeline.train(s, None, train_scene.schedule(120, densify=False), PipelineParams(), camera_stride=1, degree_up_iter=40,
                       log=lambda epoch, info: losses.append(info["ema_loss"]))
    after = metrics.render_and_eval(m, s.getTestCameras(), PipelineParams(), bg)["PSNR"]
    print(f"held-out PSNR {before:.2f} -> {after:.2f} dB after {n} iterations")
    assert n == 120 and len(losses) == 20 and np.isfinite(losses).all()
    assert np.isfinite([before, after]).all() and after > before
    s.save(n)
    assert os.path.exists(tmp_path / "out" / "point_cloud" / f"iteration_{n}" / "point_cloud.ply")
