"""-m gpu: the binning stage at the tile-grid sizes where it changes behaviour, HIP against the oracle with the 8K test's bars
(tests/test_raster_gpu.py): bit-exact radii, sorted (tile << 32 | depth) keys, point list and ranges, image PSNR >= 80 dB,
and the flip-aware gradient bar.

| image (px)        | tiles              | what it pins                                                                      |
| 4096 x 4096       | 256 x 256 = 65,536 | 16-bit keys at their limit, sorted on 16 bits (higher_msb = 17); gathered rects  |
| 4080 x 4080       | 255 x 255 = 65,025 | the largest grid whose depth sort carries packed rectangles: coordinate 255      |
| 4112 x 4096       | 257 x 256 = 65,792 | the smallest grid with 32-bit tile keys                                           |
| 8192 x 8192       | 512 x 512 = 2^18   | 32-bit keys on 19 bits (three passes of 7 / 6 / 6 bits)                           |
| 1,048,560 x 16    | 65,535 x 1         | the widest grid the ABI admits: tiles_x^2 x tiles_y = 0.99997 x 2^32              |
| 524,288 x 48      | 32,768 x 3         | the emission's multiply-high divide with rows > 1 near its bound (0.75 x 2^32)    |
| 16 x 1,048,560    | 1 x 65,535         | the tallest grid: width-1 rectangles 65,535 tiles high                           |

Each scene is a few thousand Gaussians of synth-v1 plus a dozen screen-filling ones (faint, their rectangles reach every edge
of the grid), so the oracle's CPU render stays at seconds although the images hold 16-67 Mpixels. Measured per case on one
MI355X host, oracle included: 17 s for 4096 x 4096 and 4080 x 4080, 26 s for 65,535 x 1 and 1 x 65,535, 39 s for 32,768 x 3
(forward + backward, the oracle's float64 backward is most of it); under 2 s for 4112 x 4096 and 8192 x 8192, which check the
forward only (the 67-Mpixel oracle backward alone would take about a minute)."""
import numpy as np
import pytest
import torch

from tests import cases, fullsize, gpu_util, synth

pytestmark = pytest.mark.gpu

GRAD_TOL = 1e-4

# name -> (W, H, Gaussians, backward checked)
GRIDS = {
    "4096x4096": (4096, 4096, 2500, True),
    "4080x4080": (4080, 4080, 2500, True),
    "4112x4096": (4112, 4096, 4000, False),
    "8192x8192": (8192, 8192, 6000, False),
    "65535x1": (1_048_560, 16, 1500, True),
    "32768x3": (524_288, 48, 1500, True),
    "1x65535": (16, 1_048_560, 1500, True),
}


def _scene(W, H, P, seed):
    focal = max(W, H) / 1.6                                   # the long side spans tan(fov / 2) = 0.8, as at 1080p
    intr, ev = synth.camera(W, H, focal)
    sc = synth.scene(P, W, H, focal, seed=seed, scale_median=0.02)
    # a dozen screen-filling splats: sigma ~ 2.5-3 z world units = 2.5-3 focal pixels, several times the long side (1.6 focal),
    # so their rectangles reach every edge of the grid and their alpha stays far above 1/255 on the whole image (no blend
    # decision of theirs sits on the threshold, where an exp() ulp could flip it)
    sc["scales"][:12] = sc["means3D"][:12, 2:3] * torch.tensor([3.0, 2.5, 2.8])
    sc["opacities"][:12] = 0.05
    inp = dict(bg=torch.tensor([0.1, 0.0, 0.2]), means3D=sc["means3D"], opacities=sc["opacities"], shs=sc["shs"], colors_precomp=None,
               scales=sc["scales"], rotations=sc["rotations"], cov3D_precomp=None, scale_factors=None, sh_indices=None, g_indices=None,
               degree=3, scale_modifier=1.0, prefiltered=False, clamp_color=True)
    return inp, intr, ev


def _grid_property(name, st, u):
    """the grid property each case exists for must really hold"""
    gx, gy = (st.W + 15) // 16, (st.H + 15) // 16
    tiles = (st.keys_sorted >> np.uint64(32)).astype(np.int64)
    assert int(tiles[-1]) == gx * gy - 1                      # the last tile is reached: every key bit is in use
    rects = u["rects"][st.radii > 0]
    x0, y0, x1, y1 = (rects[:, i] for i in range(4))
    assert x1.max() == gx and y1.max() == gy and x0.min() == 0 and y0.min() == 0
    if name == "4096x4096":
        assert gx * gy == 65536 and gx > 255                  # 16-bit keys; the depth sort gathers the rectangles
    elif name == "4080x4080":
        assert gx == gy == 255 and x1.max() == 255 and y1.max() == 255
    elif name == "4112x4096":
        assert gx * gy == 65_792 and int(tiles.max()) > 65535
    elif name == "8192x8192":
        assert gx * gy == 1 << 18 and int(tiles.max()) >= 1 << 17
    elif name == "65535x1":
        assert (gx, gy) == (65535, 1) and gx * gx * gy > 0.9999 * 2.0 ** 32
        assert ((x0 == 0) & (x1 == 65535)).any()              # a rectangle 65,535 tiles wide
    elif name == "32768x3":
        assert (gx, gy) == (32768, 3)
        w, area = (x1 - x0).astype(np.int64), ((x1 - x0) * (y1 - y0)).astype(np.int64)
        assert int(((area - 1) * w).max()) >= 0.74 * 2.0 ** 32   # the divide's largest local x width: 0.75 x 2^32
    elif name == "1x65535":
        assert (gx, gy) == (1, 65535) and ((y0 == 0) & (y1 == 65535)).any()


@pytest.mark.parametrize("name", list(GRIDS))
def test_tile_grid_limit_matches_the_oracle(hip, orc, name):
    W, H, P, backward = GRIDS[name]
    inp, intr, ev = _scene(W, H, P, seed=91)
    cam = orc.camera(intr.numpy(), ev.numpy())
    st = cases.oracle_forward(inp, cam)
    fw = gpu_util.hip_forward(inp, cam, False)
    u = gpu_util.unpack(fw)
    assert u["num_rendered"] == st.num_rendered and st.num_rendered > 0
    np.testing.assert_array_equal(u["radii"], st.radii)
    np.testing.assert_array_equal(u["keys_sorted"], st.keys_sorted)
    np.testing.assert_array_equal(u["point_list"], st.point_list)
    np.testing.assert_array_equal(u["ranges"], st.ranges)
    assert gpu_util.psnr(u["out_color"], st.out_color) >= 80.0
    _grid_property(name, st, u)
    if backward:
        dL = synth.grad_image(W, H).numpy()
        ref = orc.rasterize_backward(st, dL)
        got = gpu_util.hip_backward(fw, dL)
        fullsize.check_grads(st, u, got, ref, GRAD_TOL, name)
