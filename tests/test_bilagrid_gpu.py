"""-m gpu: per-image colour correction by bilateral grids (csrc/bilagrid.hip: c3dgs_bilagrid_slice / _slice_backward / _tv /
_tv_backward; c3dgs_amd.bilagrid; pipeline.train(bilagrid=...), pipeline.finetune(bilagrid=...)).

Reference: tests/bilagrid_ref.py, float64 (pinned by tests/test_bilagrid_ref_cpu.py). Bars: for each output, 4 x the distance of
the FLOAT32 grid_sample + autograd reference from the float64 one on the same case (reference against reference), floor 1e-6.
`out` and dL_drgb are measured rel-inf; each element of dL_dgrid, the total variation and each element of its gradient against
the sum of their contribution magnitudes. Every test prints what it measured in front of the assertion. Measured worst over all
cases (bar of that case): see README.md, "where it stands"."""
import random

import numpy as np
import pytest
import torch

from tests import bilagrid_ref as ref

pytestmark = pytest.mark.gpu
DEV = "cuda"
FLOOR = 1e-6
_ids = lambda v: "x".join(map(str, v)) if isinstance(v, tuple) else None     # noqa: E731


def rel_inf(a, b):
    return float(np.abs(a.astype(np.float64) - b).max() / max(np.abs(b).max(), 1e-30))


def scaled(a, b, mag):
    """max over the elements with contributions of |a - b| / (the sum of their magnitudes)"""
    live = mag > 0
    return float((np.abs(a.astype(np.float64) - b)[live] / mag[live]).max()) if live.any() else 0.0


def dev(x):
    return torch.from_numpy(np.ascontiguousarray(x, dtype=np.float32)).to(DEV)


def nan_like(shape):
    return torch.full(shape, float("nan"), dtype=torch.float32, device=DEV)


def k_slice(G, rgb):
    from c3dgs_amd import _lib
    _, L, Hg, Wg = G.shape
    _, H, W = rgb.shape
    out = nan_like(rgb.shape)
    _lib.check(_lib.lib().c3dgs_bilagrid_slice(H, W, L, Hg, Wg, G.data_ptr(), rgb.data_ptr(), out.data_ptr(), _lib.stream(G.device)))
    return out


def k_backward(G, rgb, dout, with_rgb=True):
    from c3dgs_amd import _lib
    _, L, Hg, Wg = G.shape
    _, H, W = rgb.shape
    n = _lib.lib().c3dgs_bilagrid_workspace_bytes(H, W, L, Hg, Wg)
    assert n >= 8192
    ws = torch.full((n // 4,), float("nan"), dtype=torch.float32, device=DEV)       # whatever the call reads it has written
    dG, drgb = nan_like(G.shape), (nan_like(rgb.shape) if with_rgb else None)
    _lib.check(_lib.lib().c3dgs_bilagrid_slice_backward(H, W, L, Hg, Wg, G.data_ptr(), rgb.data_ptr(), dout.data_ptr(), dG.data_ptr(),
                                                        _lib.ptr(drgb), ws.data_ptr(), _lib.stream(G.device)))
    return dG, drgb


def k_tv(X, dtv=None):
    from c3dgs_amd import _lib
    Cn, _, L, Hg, Wg = X.shape
    ws = torch.full((_lib.lib().c3dgs_bilagrid_workspace_bytes(1, 1, L, Hg, Wg) // 4,), float("nan"), dtype=torch.float32, device=DEV)
    out = nan_like((1,))
    _lib.check(_lib.lib().c3dgs_bilagrid_tv(Cn, L, Hg, Wg, X.data_ptr(), ws.data_ptr(), out.data_ptr(), _lib.stream(X.device)))
    if dtv is None:
        return out
    dX = nan_like(X.shape)
    _lib.check(_lib.lib().c3dgs_bilagrid_tv_backward(Cn, L, Hg, Wg, X.data_ptr(), dtv.data_ptr(), dX.data_ptr(), _lib.stream(X.device)))
    return out, dX


_case_cache = {}


def case(shape, hw):
    """The inputs of a (shape, size) pair and both references, computed once."""
    key = (shape, hw)
    if key not in _case_cache:
        seed = 1 + ref.CASES.index(key)
        G, rgb = ref.make_grid(*shape, seed=seed), ref.make_image(*hw, shape[0], seed=100 + seed)
        dout = (ref.hashed((3,) + hw, 200 + seed) - 0.5).astype(np.float32)
        dG64, drgb64, mag = ref.slice_backward_direct(G, rgb, dout)
        out32, dG32, drgb32 = ref.slice_grid_sample(G, rgb, dout, dtype=torch.float32)
        _case_cache[key] = dict(G=G, rgb=rgb, dout=dout, out64=ref.slice_direct(G, rgb), dG64=dG64, drgb64=drgb64, mag=mag,
                                out32=out32, dG32=dG32, drgb32=drgb32)
    return _case_cache[key]


@pytest.mark.parametrize("shape,hw", ref.CASES, ids=_ids)
def test_slice_and_its_backward_meet_the_bars(hip, shape, hw):
    c = case(shape, hw)
    assert not ref.offenders(c["rgb"], shape[0]).any()                    # the condition on the inputs, not a tolerance
    G, rgb, dout = dev(c["G"]), dev(c["rgb"]), dev(c["dout"])
    out = k_slice(G, rgb)
    dG, drgb = k_backward(G, rgb, dout)
    dG_only, none = k_backward(G, rgb, dout, with_rgb=False)
    out2 = k_slice(G, rgb)
    dG2, drgb2 = k_backward(G, rgb, dout)
    torch.cuda.synchronize()
    got = {"out": out.cpu().numpy(), "dG": dG.cpu().numpy(), "drgb": drgb.cpu().numpy()}
    for name, t in got.items():
        assert np.isfinite(t).all(), f"{name}: the NaN pre-fill is still there"
    fig = {"out": (rel_inf(got["out"], c["out64"]), rel_inf(c["out32"], c["out64"])),
           "drgb": (rel_inf(got["drgb"], c["drgb64"]), rel_inf(c["drgb32"], c["drgb64"])),
           "dG": (scaled(got["dG"], c["dG64"], c["mag"]), scaled(c["dG32"], c["dG64"], c["mag"]))}
    print("bilagrid", shape, hw, {k: "%.3g (float32 reference %.3g)" % v for k, v in fig.items()})
    for name, (mine, theirs) in fig.items():
        assert mine <= max(4 * theirs, FLOOR), (name, mine, theirs)
    assert not got["dG"][c["mag"] == 0].any(), "a vertex no pixel touches must receive exactly 0"
    if hw == (5, 3):
        assert (c["mag"] == 0).mean() > 0.5
    assert none is None and torch.equal(dG_only, dG), "dL_drgb = NULL changed dL_dgrid"
    assert torch.equal(out2, out) and torch.equal(dG2, dG) and torch.equal(drgb2, drgb), "a second call differs"


@pytest.mark.parametrize("hw", ref.SIZES, ids=_ids)
def test_identity_exposure_returns_the_image_bit_for_bit(hip, hw):
    rgb = dev(ref.make_image(*hw, 1, seed=9))
    out = k_slice(dev(ref.make_grid(1, 1, 1, seed=1, noise=0.0)), rgb)
    assert torch.equal(out, rgb)


@pytest.mark.parametrize("Cn", [1, 3])
@pytest.mark.parametrize("shape", ref.SHAPES, ids=_ids)
def test_tv_and_its_backward(hip, shape, Cn):
    X = np.stack([ref.make_grid(*shape, seed=40 + c) for c in range(Cn)])
    want, want32 = ref.tv(X), ref.tv(X, torch.float32)
    grad, mag = ref.tv_backward_direct(X)
    dtv = 0.73
    grad32 = ref.tv_backward_autograd(X, torch.float32)
    x, g = dev(X), dev(np.array([dtv]))
    out, dX = k_tv(x, g)
    out2, dX2 = k_tv(x, g)
    torch.cuda.synchronize()
    value, dXn = float(out[0]), dX.cpu().numpy()
    assert np.isfinite(value) and np.isfinite(dXn).all()
    if max(shape) == 1:
        assert value == 0.0 and want == 0.0 and not dXn.any()
    else:
        f_v = (abs(value - want) / want, abs(want32 - want) / want)
        f_g = (scaled(dXn, dtv * grad, dtv * mag), scaled(grad32, grad, mag))
        print("bilagrid tv", shape, Cn, "value %.3g (float32 reference %.3g), gradient %.3g (float32 reference %.3g)" % (f_v + f_g))
        assert f_v[0] <= max(4 * f_v[1], FLOOR) and f_g[0] <= max(4 * f_g[1], FLOOR)
    assert torch.equal(out2, out) and torch.equal(dX2, dX)


@pytest.mark.parametrize("shape,hw", [((8, 16, 16), (17, 33)), ((1, 1, 1), (70, 130)), ((3, 2, 5), (64, 64))], ids=_ids)
def test_autograd_through_the_module(hip, shape, hw):
    from c3dgs_amd.bilagrid import BilateralGrid, ExposureModel
    c, Cn, cam, tv_w = case(shape, hw), 3, 1, 2.5
    X = np.stack([ref.make_grid(*shape, seed=60 + k) for k in range(Cn)])
    X[cam] = c["G"]
    grids = ExposureModel(Cn) if shape == (1, 1, 1) else BilateralGrid(Cn, shape)
    assert grids.shape == shape and grids.grids.shape == (Cn, 12) + shape
    eye = torch.eye(3, 4, device=DEV).reshape(1, 12, 1, 1, 1).expand_as(grids.grids)
    assert torch.equal(grids.grids.detach(), eye)                         # the identity affine at every vertex
    with torch.no_grad():
        grids.grids.copy_(dev(X))
    image = dev(c["rgb"]).requires_grad_(True)
    out = grids.slice(image, cam)
    (out * dev(c["dout"])).sum().backward()
    slice_grad = grids.grids.grad.clone()
    assert not slice_grad[0].any() and not slice_grad[2].any(), "rows of other cameras must be exactly 0"
    (tv_w * grids.tv_loss()).backward()
    torch.cuda.synchronize()

    def composite(dG, tv_grad):
        e = tv_w * tv_grad
        e[cam] += dG
        return e
    tv64, tv_mag = ref.tv_backward_direct(X)
    want, mag = composite(c["dG64"], tv64), composite(c["mag"], tv_mag)
    want32 = composite(c["dG32"].astype(np.float64), ref.tv_backward_autograd(X, torch.float32).astype(np.float64))
    f_g = (scaled(grids.grids.grad.cpu().numpy(), want, mag), scaled(want32, want, mag))
    f_i = (rel_inf(image.grad.cpu().numpy(), c["drgb64"]), rel_inf(c["drgb32"], c["drgb64"]))
    print("bilagrid autograd", shape, hw, "grids.grad %.3g (float32 reference %.3g), image.grad %.3g (%.3g)" % (f_g + f_i))
    assert rel_inf(out.detach().cpu().numpy(), c["out64"]) <= max(4 * rel_inf(c["out32"], c["out64"]), FLOOR)
    assert f_g[0] <= max(4 * f_g[1], FLOOR) and f_i[0] <= max(4 * f_i[1], FLOOR)
    # an image that needs no gradient: the same grid gradient bits (the NULL dL_drgb path)
    grids.grids.grad = None
    (grids.slice(dev(c["rgb"]), cam) * dev(c["dout"])).sum().backward()
    assert torch.equal(grids.grids.grad, slice_grad)


def test_cpu_tensors_are_refused(hip):
    from c3dgs_amd.bilagrid import BilateralGrid
    grids = BilateralGrid(2, (2, 2, 2))
    with pytest.raises(RuntimeError, match="GPU tensor"):
        grids.slice(torch.zeros(3, 4, 4), 0)
    with pytest.raises(IndexError):
        grids.slice(torch.zeros(3, 4, 4, device=DEV), 2)
    with pytest.raises(RuntimeError, match="no CPU path"):
        BilateralGrid(2, (2, 2, 2), device="cpu")


def test_save_and_load_round_trip(hip, tmp_path):
    from c3dgs_amd.bilagrid import BilateralGrid

    class Cam:
        def __init__(self, name):
            self.image_name = name
    cams = [Cam("a_%02d" % k) for k in range(3)]
    grids = BilateralGrid(3, (3, 2, 5)).set_cameras(cams)
    with torch.no_grad():
        grids.grids.copy_(dev(np.stack([ref.make_grid(3, 2, 5, seed=70 + k) for k in range(3)])))
    path = str(tmp_path / "grids.npz")
    grids.save(path)
    with np.load(path) as z:
        assert sorted(z.files) == ["grids", "image_names"] and [str(s) for s in z["image_names"]] == ["a_00", "a_01", "a_02"]
    back = BilateralGrid(3, (3, 2, 5)).set_cameras(cams).load(path)
    assert torch.equal(back.grids.detach(), grids.grids.detach())
    with pytest.raises(ValueError, match="image names"):
        BilateralGrid(3, (3, 2, 5)).set_cameras(cams[::-1]).load(path)
    with pytest.raises(ValueError, match="holds"):
        BilateralGrid(3, (2, 2, 5)).set_cameras(cams).load(path)


# ------------------------------------------------------------------------------------------------ training
def _scene(tmp_dir, jitter):
    from tests import train_scene
    student, cams, extent = train_scene.make(tmp_dir, DEV)
    if jitter:
        ref.jitter_exposure(cams, jitter)

    class Scene:
        gaussians = student
        cameras_extent = extent

        def getTrainCameras(self):
            return cams
    return Scene(), student, cams


@pytest.fixture(scope="module")
def trained(hip, tmp_path_factory):
    """The toy scene with the --exposure-jitter 0.3 images, 400 iterations, no density control, every second camera: once
    without a grid and once with bilagrid=(1, 1, 1)."""
    from c3dgs_amd import pipeline
    from c3dgs_amd.model import PipelineParams
    from tests import train_scene
    runs = {}
    for name, kw in (("none", {}), ("exposure", dict(bilagrid=(1, 1, 1), bilagrid_tv=0))):
        scene, student, cams = _scene(tmp_path_factory.mktemp(name), 0.3)
        events = []
        torch.manual_seed(0)
        n = pipeline.train(scene, None, train_scene.schedule(400, densify=False), PipelineParams(), camera_stride=2, degree_up_iter=80,
                           log=lambda epoch, info: events.append(info), **kw)
        runs[name] = dict(iterations=n, events=events, cams=cams)
    return runs


def test_exposure_lowers_the_training_loss_under_exposure_jitter(trained):
    a, b = trained["none"]["events"][-1]["epoch_loss"], trained["exposure"]["events"][-1]["epoch_loss"]
    print("mean training loss over the last epoch, jitter 0.3: without a grid %.5f, bilagrid=(1, 1, 1) %.5f" % (a, b))
    assert trained["none"]["iterations"] == trained["exposure"]["iterations"] == 200
    assert "bilagrid" not in trained["none"]["events"][0]
    assert b < a


def test_only_the_visited_cameras_grids_move(trained):
    from c3dgs_amd.bilagrid import BilateralGrid
    events = trained["exposure"]["events"]
    grids = events[0]["bilagrid"]
    assert isinstance(grids, BilateralGrid) and grids.shape == (1, 1, 1) and grids.num_cameras == 8
    assert all("bilagrid" not in e for e in events[1:])
    eye = torch.eye(3, 4, device=DEV).reshape(12, 1, 1, 1)
    g = grids.grids.detach()
    for k in range(8):
        if k % 2:
            assert torch.equal(g[k], eye), f"camera {k} is skipped by camera_stride=2: its grid must stay the identity bit for bit"
        else:
            assert not torch.equal(g[k], eye) and torch.isfinite(g[k]).all(), f"camera {k} was trained: its grid must have moved"


def test_error_densification_with_a_grid_is_refused(hip, tmp_path):
    from c3dgs_amd import pipeline
    from c3dgs_amd.model import PipelineParams
    from tests import train_scene
    scene, _, _ = _scene(tmp_path, 0)
    with pytest.raises(ValueError, match="bilagrid"):
        pipeline.train(scene, None, train_scene.schedule(16), PipelineParams(), densify_by="error", error_threshold=1.0, bilagrid=(1, 1, 1))


def test_finetune_applies_the_grids_frozen(hip, tmp_path):
    from c3dgs_amd import pipeline
    from c3dgs_amd.bilagrid import BilateralGrid
    from c3dgs_amd.model import PipelineParams
    scene, student, cams = _scene(tmp_path, 0.3)
    grids = BilateralGrid(len(cams), (2, 2, 2))
    with torch.no_grad():
        grids.grids.copy_(dev(np.stack([ref.make_grid(2, 2, 2, seed=80 + k, noise=0.05) for k in range(len(cams))])))
    before = grids.grids.detach().clone()
    random.seed(3)
    torch.manual_seed(0)
    ema = pipeline.finetune(scene, pipeline._Dataset(), pipeline.OptimizationParams(), pipeline.CompressionParams(finetune_iterations=6),
                            PipelineParams(), bilagrid=grids)
    assert np.isfinite(ema)
    assert torch.equal(grids.grids.detach(), before) and grids.grids.requires_grad and grids.grids.grad is None
    with pytest.raises(ValueError, match="training cameras"):
        pipeline.finetune(scene, pipeline._Dataset(), pipeline.OptimizationParams(), pipeline.CompressionParams(finetune_iterations=2),
                          PipelineParams(), bilagrid=BilateralGrid(3, (1, 1, 1)))


# what ONE view of the default loop records (c3dgs_profile_read: stage -> launches), as the loop ran before the grids existed
DEFAULT_LOOP_STAGES = {"mark_visible": 1, "preprocess": 1, "depth_sort": 1, "scan": 1, "duplicate_with_keys": 1, "sort": 1,
                       "identify_ranges": 1, "render_forward": 1, "zero_partials": 1, "render_backward": 1, "backward_preprocess": 1,
                       "l1_ssim_forward": 1, "l1_ssim_backward": 1, "qat_observe": 6, "qat_codebooks": 3, "qat_points": 3,
                       "qat_points_backward": 1, "qat_codebooks_backward": 1, "adam_step": 1}


def _stages_of_train(tmp_dir, **kw):
    from c3dgs_amd import _lib, pipeline
    from c3dgs_amd.model import PipelineParams
    from tests import train_scene
    scene, _, _ = _scene(tmp_dir, 0)
    torch.manual_seed(0)
    _lib.profile_read()
    _lib.profile_enable(True)
    try:
        n = pipeline.train(scene, None, train_scene.schedule(16, densify=False), PipelineParams(), camera_stride=1, degree_up_iter=80, **kw)
        torch.cuda.synchronize()
        stages = {name: count for name, (_, count) in _lib.profile_read().items()}
    finally:
        _lib.profile_enable(False)
    return n, stages


def test_without_a_grid_the_loop_records_the_stages_it_always_did(hip, tmp_path_factory):
    n, plain = _stages_of_train(tmp_path_factory.mktemp("plain"), bilagrid=None)
    n2, with_grid = _stages_of_train(tmp_path_factory.mktemp("grid"), bilagrid=(2, 2, 2))
    print("train(bilagrid=None), %d views:" % n, plain)
    assert n == n2 == 16
    assert not [s for s in plain if s.startswith("bilagrid")]
    assert plain == {s: c * n for s, c in DEFAULT_LOOP_STAGES.items()}
    grid_only = {s: c for s, c in with_grid.items() if s.startswith("bilagrid")}
    assert grid_only == {"bilagrid_slice": n, "bilagrid_slice_backward": n, "bilagrid_gather": n, "bilagrid_fold": n,
                         "bilagrid_rgb_backward": n, "bilagrid_tv": n, "bilagrid_tv_backward": n}
    rest = {s: c for s, c in with_grid.items() if s not in grid_only}
    assert sorted(rest) == sorted(plain)
    assert rest["adam_step"] == plain["adam_step"] + n                    # the grids' own optimizer, one more step per view
