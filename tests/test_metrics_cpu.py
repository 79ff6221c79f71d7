"""CPU: the float64 restatement of the evaluation metrics (tests/metrics_ref.py) against the reference's own psnr / ssim
(tests/golden/metrics.npz), the C-ABI validation of c3dgs_image_metrics without a device, and the no-CPU-path errors
of c3dgs_amd.metrics."""
import ctypes as C
import os

import numpy as np
import pytest
import torch

from tests import metrics_ref as R

G = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
TAGS = ("rand", "batch", "gray", "tiny", "chw", "range", "same")


@pytest.fixture(scope="module")
def gold():
    return np.load(os.path.join(G, "metrics.npz"), allow_pickle=False)


@pytest.fixture(scope="module")
def L():
    from c3dgs_amd import build, _lib
    build.build()
    return _lib.lib()


@pytest.mark.parametrize("tag", TAGS)
def test_restatement_matches_reference_fp64(gold, tag):
    x, y = gold[f"{tag}_img"], gold[f"{tag}_gt"]
    if x.ndim == 3:                       # psnr per channel, ssim over the whole [C,H,W]
        p, s = R.psnr_rows(x[:, None], y[:, None]), R.ssim_rows(x[None], y[None]).mean()
    else:
        p, s = R.psnr_rows(x, y), R.ssim_rows(x, y)
        np.testing.assert_allclose(s, gold[f"{tag}_ssimN64"], rtol=0, atol=1e-12)
        np.testing.assert_allclose(R.mse_rows(x, y), gold[f"{tag}_mse64"], rtol=1e-12, atol=0)
        np.testing.assert_allclose(R.l1_rows(x, y), gold[f"{tag}_l164"], rtol=1e-12, atol=0)
        s = s.mean()
    ref = gold[f"{tag}_psnr64"].reshape(-1)
    assert p.shape == ref.shape
    fin = np.isfinite(ref)
    assert np.array_equal(p[~fin], ref[~fin])
    np.testing.assert_allclose(p[fin], ref[fin], rtol=0, atol=1e-12)
    assert abs(s - float(gold[f"{tag}_ssim64"])) <= 1e-12


def test_fixture_covers_the_edge_cases(gold):
    assert gold["tiny_img"].shape[2] < 11 and gold["gray_img"].shape[2] < 11
    assert gold["range_img"].min() < 0 and gold["range_img"].max() > 1 and np.ptp(gold["range_gt"]) == 0
    assert np.isinf(gold["same_psnr32"]).all() and float(gold["same_ssim32"]) == 1.0
    assert gold["chw_psnr64"].shape == (3, 1) and gold["batch_ssimN64"].shape == (3,)


def test_image_metrics_validation_without_gpu(L):
    ws = C.c_void_p(64)                   # any non-null, 8-byte aligned address: validation fails before any launch
    img = C.c_void_p(4096)
    out = C.c_void_p(8192)
    need = L.c3dgs_image_metrics_ws_bytes(2, 3, 1080, 1920)
    assert need == 2 * 3 * 60 * 50 * 3 * 8                     # 32 x 22 tiles, three float64 partials each
    assert L.c3dgs_image_metrics_ws_bytes(1, 3, 5, 7) == 3 * 3 * 8
    assert L.c3dgs_image_metrics_ws_bytes(0, 3, 5, 7) == 0
    assert L.c3dgs_image_metrics_ws_bytes(2 ** 31 - 1, 2 ** 31 - 1, 2 ** 31 - 1, 2 ** 31 - 1) == 0
    for bad in ((0, 3, 8, 8), (1, 0, 8, 8), (1, 3, 0, 8), (1, 3, 8, -1)):
        assert L.c3dgs_image_metrics(*bad, img, img, ws, 1 << 20, out, None) == 1
        assert b"must be positive" in L.c3dgs_last_error()
    assert L.c3dgs_image_metrics(2 ** 31 - 1, 2 ** 31 - 1, 2 ** 31 - 1, 2 ** 31 - 1, img, img, ws, 1 << 20, out, None) == 1
    assert b"size overflow" in L.c3dgs_last_error()
    assert L.c3dgs_image_metrics(4096, 3, 1080, 1920, img, img, ws, 1 << 40, out, None) == 1
    assert b"size overflow" in L.c3dgs_last_error()
    for args in ((None, img, ws, out), (img, None, ws, out), (img, img, None, out), (img, img, ws, None)):
        a, b, w, o = args
        assert L.c3dgs_image_metrics(1, 3, 8, 8, a, b, w, 1 << 20, o, None) == 1
        assert b"are required" in L.c3dgs_last_error()
    assert L.c3dgs_image_metrics(1, 3, 8, 8, img, img, C.c_void_p(68), 1 << 20, out, None) == 1
    assert b"aligned" in L.c3dgs_last_error()
    assert L.c3dgs_image_metrics(2, 3, 1080, 1920, img, img, ws, need - 8, out, None) == 1
    assert b"ws too small" in L.c3dgs_last_error()


def test_metrics_have_no_cpu_path():
    from c3dgs_amd import metrics
    x, y = torch.rand(1, 3, 16, 16), torch.rand(1, 3, 16, 16)
    for fn in (metrics.psnr, metrics.ssim, metrics.image_metrics):
        with pytest.raises(RuntimeError, match="no CPU path"):
            fn(x, y)
    with pytest.raises(RuntimeError, match="shape mismatch"):
        metrics.psnr(x, y[..., :8])
    with pytest.raises(NotImplementedError):
        metrics.ssim(x, y, window_size=7)
