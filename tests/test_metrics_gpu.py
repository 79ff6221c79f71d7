"""-m gpu: the evaluation metrics (csrc/metrics.hip, c3dgs_amd.metrics) against the reference's own psnr / ssim
(tests/golden/metrics.npz), the float64 restatement (tests/metrics_ref.py) at full size, the fused loss kernel's SSIM,
and their determinism; then render_and_eval and run_vq(eval_cameras=...) end to end."""
import json
import os

import numpy as np
import pytest
import torch

from tests import metrics_ref as R
from tests import synth

pytestmark = pytest.mark.gpu
G = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
TAGS = ("rand", "batch", "gray", "tiny", "chw", "range", "same")
DEV = "cuda"


@pytest.fixture(scope="module")
def gold():
    return np.load(os.path.join(G, "metrics.npz"), allow_pickle=False)


def _pair(gold, tag):
    return torch.from_numpy(gold[f"{tag}_img"]).to(DEV), torch.from_numpy(gold[f"{tag}_gt"]).to(DEV)


def _inf_close(got, ref, atol):
    got, ref = np.asarray(got, np.float64).reshape(-1), np.asarray(ref, np.float64).reshape(-1)
    assert got.shape == ref.shape
    fin = np.isfinite(ref)
    assert np.array_equal(got[~fin], ref[~fin]), (got, ref)
    assert np.isfinite(got[fin]).all()
    np.testing.assert_allclose(got[fin], ref[fin], rtol=0, atol=atol)


@pytest.mark.parametrize("tag", TAGS)
def test_metrics_match_reference_golden(hip, gold, tag):
    from c3dgs_amd import metrics
    x, y = _pair(gold, tag)
    p = metrics.psnr(x, y)
    s = metrics.ssim(x, y)
    assert p.dtype == torch.float32 and p.shape == gold[f"{tag}_psnr32"].shape and s.dim() == 0 and s.dtype == torch.float32
    assert p.device.type == "cuda" and not p.requires_grad
    _inf_close(p.cpu().numpy(), gold[f"{tag}_psnr64"], 1e-5)            # dB
    _inf_close(p.cpu().numpy(), gold[f"{tag}_psnr32"], 1e-4)
    assert abs(float(s) - float(gold[f"{tag}_ssim64"])) <= 1e-6
    assert abs(float(s) - float(gold[f"{tag}_ssim32"])) <= 2e-6
    if x.dim() == 4:
        sn = metrics.ssim(x, y, size_average=False)
        assert sn.shape == (x.shape[0],)
        np.testing.assert_allclose(sn.cpu().numpy(), gold[f"{tag}_ssimN64"], rtol=0, atol=1e-6)
        np.testing.assert_allclose(sn.cpu().numpy(), gold[f"{tag}_ssimN32"], rtol=0, atol=2e-6)
        rows = metrics.image_metrics(x, y).cpu().numpy()
        np.testing.assert_allclose(rows[:, 0], gold[f"{tag}_mse64"], rtol=1e-6, atol=0)
        np.testing.assert_allclose(rows[:, 2], gold[f"{tag}_l164"], rtol=1e-6, atol=0)
    else:
        with pytest.raises(IndexError):
            metrics.ssim(x, y, size_average=False)


def test_metrics_input_handling(hip, gold):
    from c3dgs_amd import metrics
    x, y = _pair(gold, "rand")
    ref = metrics.image_metrics(x, y)
    # other dtypes and non-contiguous inputs are converted
    xt = x.double().transpose(2, 3).contiguous().transpose(2, 3)
    assert not xt.is_contiguous()
    assert torch.equal(metrics.image_metrics(xt, y), ref)
    with pytest.raises(RuntimeError, match="shape mismatch"):
        metrics.ssim(x, y[:, :, :10])
    with pytest.raises(NotImplementedError):
        metrics.ssim(x, y, window_size=7)
    with pytest.raises(RuntimeError, match="no CPU path"):
        metrics.psnr(x.cpu(), y.cpu())
    # rows land where `out` points, inside a larger table
    table = torch.full((3, 3), -1.0, dtype=torch.float64, device=DEV)
    metrics.image_metrics(x, y, out=table[1:2])
    assert torch.equal(table[1:2], ref) and (table[0] == -1).all() and (table[2] == -1).all()


def _fullsize_pairs():
    g = torch.Generator().manual_seed(7)
    H, W = 1080, 1920
    a = torch.rand(1, 3, H, W, generator=g)
    b = torch.rand(1, 3, H, W, generator=g)
    yy, xx = torch.meshgrid(torch.linspace(0, 1, H), torch.linspace(0, 1, W), indexing="ij")
    base = torch.stack([0.5 + 0.4 * torch.sin(12 * xx + 3 * yy), 0.5 + 0.4 * torch.cos(9 * yy - 2 * xx), xx * yy])[None]
    noisy = (base + 0.05 * torch.randn(base.shape, generator=g)).clamp(0, 1)
    return {"random": (a, b), "structured": (noisy, base)}


@pytest.mark.parametrize("kind", ["random", "structured"])
def test_fullsize_matches_restatement_and_loss_kernel(hip, kind):
    from c3dgs_amd import loss, metrics
    x, y = _fullsize_pairs()[kind]
    xd, yd = x.to(DEV), y.to(DEV)
    rows = metrics.image_metrics(xd, yd).cpu().numpy()[0]
    xn, yn = x.numpy(), y.numpy()
    mse = R.mse_rows(xn, yn)[0]
    assert abs(rows[0] - mse) <= 1e-6 * mse
    assert abs(rows[2] - R.l1_rows(xn, yn)[0]) <= 1e-6 * R.l1_rows(xn, yn)[0]
    assert abs(rows[1] - R.ssim_rows(xn, yn)[0]) <= 1e-6
    assert abs(float(metrics.psnr(xd, yd)) - R.psnr_rows(xn, yn)[0]) <= 1e-5
    # two independent kernels: the fused loss forward and the metrics pass. They agree to 2e-6 up to the one difference
    # of their inputs: loss.hip normalises its window by a running fp32 sum, 1 ulp below the reference's sum, which on
    # a smooth pair moves the mean SSIM by ~2e-5; each kernel is held to the restatement with its own window
    s_loss = float(loss.ssim(xd[0], yd[0]))
    s_loss_ref = R.ssim_rows(xn, yn, R.window(running_fp32_sum=True))[0]
    assert abs(s_loss - s_loss_ref) <= 2e-6
    assert abs(float(metrics.ssim(xd, yd)) - s_loss - (R.ssim_rows(xn, yn)[0] - s_loss_ref)) <= 2e-6


def test_batch_rows_equal_single_calls_and_are_deterministic(hip):
    from c3dgs_amd import metrics
    g = torch.Generator().manual_seed(11)
    gt = torch.rand(4, 3, 270, 480, generator=g)
    img = (gt + 0.1 * torch.randn(gt.shape, generator=g)).clamp(0, 1)
    x, y = img.to(DEV), gt.to(DEV)
    rows = metrics.image_metrics(x, y)
    again = metrics.image_metrics(x, y)
    assert torch.equal(rows.view(torch.int64), again.view(torch.int64))
    for n in range(4):
        single = metrics.image_metrics(x[n:n + 1], y[n:n + 1])
        assert torch.equal(rows[n:n + 1].view(torch.int64), single.view(torch.int64)), n


class _Cam:
    def __init__(self, intrinsic, ev):
        self.intrinsic, self.extrinsic_vector = intrinsic.to(DEV), ev.to(DEV)


def _model(sc):
    from c3dgs_amd.model import GaussianModel
    op = sc["opacities"].clamp(1e-6, 1 - 1e-6)
    norm = sc["scales"].norm(dim=1, keepdim=True)
    g = GaussianModel(3, quantization=True, device=DEV)
    g.set_tensors(xyz=sc["means3D"], features_dc=sc["shs"][:, :1], features_rest=sc["shs"][:, 1:], scaling=sc["scales"] / norm,
                  rotation=sc["rotations"], opacity=torch.log(op / (1 - op)), scaling_factor=torch.log(norm))
    g.spatial_lr_scale = 1.0
    return g


def _quantise(img):
    return img.mul(255).add_(0.5).clamp_(0, 255).permute(1, 2, 0).to("cpu", torch.uint8).numpy()


def test_render_and_eval(hip, tmp_path):
    from PIL import Image
    from c3dgs_amd import metrics
    from c3dgs_amd.model import PipelineParams
    W, H, P = 320, 200, 6000
    sc = synth.scene(P, W, H, 300.0, seed=5, sh_degree=3, scale_median=0.03)
    g = _model(sc)
    pert = dict(sc)
    gen = torch.Generator().manual_seed(6)
    pert["shs"] = sc["shs"] + 0.05 * torch.randn(sc["shs"].shape, generator=gen)
    gp = _model(pert)
    pipe, bg = PipelineParams(), torch.zeros(3, device=DEV)
    cams = []
    for k in range(4):
        intr, ev = synth.camera(W, H, 300.0, extrinsic_vector=(0.0, 0.02 * (k - 1.5), 0.0, 1.0, 0.0, 0.0, 0.0))
        cam = _Cam(intr, ev)
        with torch.no_grad():
            cam.original_image = gp.render(cam, pipe, bg)["render"].clone()
        cams.append(cam)
    with torch.no_grad():
        renders = [g.render(c, pipe, bg)["render"].clone() for c in cams]

    calls = []

    def lpips_fn(a, b):
        assert a.shape == (1, 3, H, W) and b.shape == (1, 3, H, W)
        calls.append(float((a - b).abs().mean()))
        return (a - b).abs().mean()

    out = metrics.render_and_eval(g, cams, pipe, bg, out_dir=str(tmp_path / "ev"), lpips_fn=lpips_fn)
    xs = [r.cpu().numpy()[None] for r in renders]
    ys = [c.original_image.cpu().numpy()[None] for c in cams]
    want_ssim = np.mean([R.ssim_rows(x, y)[0] for x, y in zip(xs, ys)])
    want_psnr = np.mean([R.psnr_rows(x, y)[0] for x, y in zip(xs, ys)])
    assert set(out) == {"SSIM", "PSNR", "LPIPS"}
    assert abs(out["SSIM"] - want_ssim) <= 1e-6
    assert abs(out["PSNR"] - want_psnr) <= 1e-4
    assert 15 < out["PSNR"] < 60 and 0.3 < out["SSIM"] < 1.0
    assert len(calls) == 4 and out["LPIPS"] == pytest.approx(np.mean(calls), rel=1e-6)
    for idx in range(4):
        got_r = np.asarray(Image.open(tmp_path / "ev" / "renders" / f"{idx:05d}.png"))
        got_g = np.asarray(Image.open(tmp_path / "ev" / "gt" / f"{idx:05d}.png"))
        assert np.array_equal(got_r, _quantise(renders[idx]))
        assert np.array_equal(got_g, _quantise(cams[idx].original_image))
    # without lpips_fn LPIPS is not computed, and without out_dir nothing is written
    again = metrics.render_and_eval(g, cams, pipe, bg)
    assert again["LPIPS"] is None and again["SSIM"] == out["SSIM"] and again["PSNR"] == out["PSNR"]


def test_run_vq_writes_results_json(hip, tmp_path):
    from c3dgs_amd import pipeline
    from c3dgs_amd.model import PipelineParams
    W, H, P = 320, 200, 6000
    sc = synth.scene(P, W, H, 300.0, seed=21, sh_degree=3, scale_median=0.03)
    g = _model(sc)
    pipe, bg = PipelineParams(), torch.zeros(3, device=DEV)
    cams = []
    for k in range(3):
        intr, ev = synth.camera(W, H, 300.0, extrinsic_vector=(0.0, 0.03 * (k - 1), 0.0, 1.0, 0.0, 0.0, 0.0))
        cam = _Cam(intr, ev)
        with torch.no_grad():
            cam.original_image = g.render(cam, pipe, bg)["render"].clone()
        cams.append(cam)
    comp = pipeline.CompressionParams(finetune_iterations=6, color_cluster_iterations=8, gaussian_cluster_iterations=8,
                                      color_codebook_size=64, gaussian_codebook_size=64, color_batch_size=2 ** 11,
                                      gaussian_batch_size=2 ** 11, output_vq=str(tmp_path / "vq"))
    timings, path = pipeline.run_vq(g, cams, pipeline.OptimizationParams(), pipe, comp, eval_cameras=cams)
    assert set(timings) == {"sensitivity_calculation", "clustering", "finetune", "encode", "total"}
    res = json.load(open(os.path.join(comp.output_vq, "results.json")))
    assert list(res) == ["ours_6"] and set(res["ours_6"]) == {"SSIM", "PSNR", "LPIPS", "size"}
    m = res["ours_6"]
    assert m["size"] == os.path.getsize(path) / 1024 ** 2
    assert m["PSNR"] > 25.0 and 0.5 < m["SSIM"] <= 1.0 and m["LPIPS"] is None
    for sub in ("renders", "gt"):
        d = os.path.join(comp.output_vq, "test", "ours_6", sub)
        assert sorted(os.listdir(d)) == [f"{i:05d}.png" for i in range(3)]
