"""-m gpu: the compact per-tile lists the forward writes for the backward (render.hip, c3dgs_get_compact_layout).

Of the list entries a tile visits, only those whose quadrant mask is non-zero can reach a pixel of the tile; the forward
writes exactly those -- Gaussian id `cid`, mask `cqm` -- densely from the start of the tile's own segment, and per pixel / per
tile the 1-based COMPACT index of the last contributor (`n_contrib_c`, `tile_used_c`). The backward walks nothing else. All
checks on the lists are integer / exact:
  * per tile, cid[range.x : range.x + tile_used_c] is a subsequence, in order, of point_list[range.x : range.x + tile_used],
    and cqm is a non-zero 4-bit mask on all of it;
  * per pixel with n_contrib > 0: cid[range.x + n_contrib_c - 1] == point_list[range.x + n_contrib - 1]; n_contrib == 0 goes
    with n_contrib_c == 0; tile_used / tile_used_c are the tile maxima;
  * every entry of the visited prefix that is NOT in the compact list blends nowhere: in float64, from the oracle's means2D /
    conic_opacity, opacity * exp(power) < 1/255 at all 256 pixels of its tile. No tolerance and no exemption: the cull is
    conservative by 1e-4 relative + 1e-4 absolute in the exponent, far above the float32 error of the per-pixel test;
  * gradients against the oracle at the bar of tests/test_raster_gpu.py, and the non-indexed backward bitwise reproducible.

The full-HD scene (synth_300k: the indexed synth-v1 view tools/list_liveness.py counts, 39.7 % of its visited entries dead) takes
~60x the blend decisions of the small views; a few of them flip on a rounding of the exponent, so it is held to the repository's
full-HD bars (tests/test_fullsize_gpu.py): every flip proven inside the fp32 band, 1e-4 for everything that shares no tile with
a flipped pixel, 1e-3 overall. All other scenes are held to check_grads at the bar of tests/test_raster_gpu.py -- except
needles_long (tests/cases.py: EDGE_GAUSSIAN_CASES), where the reference's own fp32 formula leaves that bar: its gradients are held
to the float64 truth at max(1e-4, 4 x the oracle's own deviation), as in tests/test_edge_gaussians_gpu.py. The list checks are
the same exact ones on every scene: a needle's quadrant cull, and the saturated tiles of opaque_big, get no tolerance either.
"""
import ctypes as C

import numpy as np
import pytest
import torch

from tests import cases, fullsize, gpu_util, synth
from tests.test_fullsize_gpu import GRAD_TOL as FULL_HD_TOL, GRAD_TOL_FLIPPED as FULL_HD_TOL_FLIPPED, MAX_FLIPPED_FRACTION

pytestmark = pytest.mark.gpu

GRAD_TOL = 1e-4          # tests/test_raster_gpu.py


def _plain_inputs(sc, bg=(0.0, 0.0, 0.0)):
    return dict(bg=torch.tensor(bg), means3D=sc["means3D"], opacities=sc["opacities"], shs=sc["shs"], colors_precomp=None,
                scales=sc["scales"], rotations=sc["rotations"], cov3D_precomp=None, scale_factors=None, sh_indices=None,
                g_indices=None, degree=3, scale_modifier=1.0, prefiltered=False, clamp_color=True)


def _scene(name):
    """-> (inputs, cam, indexed)"""
    from oracle import oracle as orc
    if name in ("indexed", "odd_size", "needles_long", "opaque_big"):    # odd_size: 203 x 131 pixels, not a multiple of 16
        return cases.make_case(name)
    if name == "synth_300k":                             # synth-v1 at 1920x1080, indexed: the bench workload's shape at a tenth of its size
        inp, intr, ev, indexed = fullsize.config_inputs("config3_3M_indexed", P=300_000)
        return inp, orc.camera(intr.numpy(), ev.numpy()), indexed
    if name == "synth_small":                            # synth-v1, the same Gaussians per pixel, on 1/16 of the pixels
        inp, intr, ev, indexed = fullsize.config_inputs("config2_1M_fwd", P=18_750, W=480, H=270, focal=300.0)
        return inp, orc.camera(intr.numpy(), ev.numpy()), indexed
    if name == "dense":                                  # opaque splats stacked deep: tiles saturate long before their lists end
        W, H, focal = 250, 190, 160.0
        intr, ev = synth.camera(W, H, focal)
        sc = synth.scene(40_000, W, H, focal, seed=21, scale_median=0.12)
        sc["opacities"] = (0.55 + 0.4 * torch.rand(sc["opacities"].shape, generator=torch.Generator().manual_seed(22))).float()
        return _plain_inputs(sc, (0.1, 0.2, 0.3)), orc.camera(intr.numpy(), ev.numpy()), False
    if name == "huge_faint":
        # 700 screen-filling splats too faint to blend anywhere (opacity 0.003 < 1/255) in front of, and 300 faint-but-visible ones
        # (opacity 0.02: footprint far inside the 3-sigma rectangle) among, an ordinary scene: every tile's list starts with whole
        # rounds of 256 dead positions. 211 x 149 pixels: not a multiple of 16.
        W, H, focal = 211, 149, 140.0
        intr, ev = synth.camera(W, H, focal)
        sc = synth.scene(6000, W, H, focal, seed=31, scale_median=0.05, zmin=4.0, zmax=12.0)
        sc["means3D"][:700, 2] = torch.linspace(2.0, 3.0, 700)
        sc["means3D"][:700, :2] *= 0.2
        sc["scales"][:1000] = 8.0
        sc["opacities"][:700] = 0.003
        sc["opacities"][700:1000] = 0.02
        return _plain_inputs(sc), orc.camera(intr.numpy(), ev.numpy()), False
    raise KeyError(name)


def _compact(fw, u):
    """The library's compact arrays as numpy: cid, cqm (R each), n_contrib_c (H*W), tile_used_c (T)."""
    from c3dgs_amd import _lib
    R, W, H = fw["num_rendered"], fw["W"], fw["H"]
    T = ((W + 15) // 16) * ((H + 15) // 16)
    cl = _lib.CompactLayout()
    assert _lib.lib().c3dgs_get_compact_layout(R, W, H, C.byref(cl)) == 0
    il = _lib.ImageLayout()
    _lib.lib().c3dgs_get_image_layout(W, H, C.byref(il))
    b, img = fw["binning"], fw["img"]
    assert cl.cid + 4 * R <= b.numel() and cl.cqm + R <= cl.cid
    assert il.tile_order + 4 * T <= cl.tile_used_c and cl.tile_used_c + 4 * T <= cl.n_contrib_c and cl.n_contrib_c + 4 * W * H <= img.numel()
    tile_used = gpu_util._view(img, il.tile_used, T, torch.int32).cpu().numpy().astype(np.int64)
    return dict(cid=gpu_util._view(b, cl.cid, R, torch.int32).cpu().numpy().view(np.uint32),
                cqm=gpu_util._view(b, cl.cqm, R, torch.uint8).cpu().numpy(),
                n_contrib_c=gpu_util._view(img, cl.n_contrib_c, W * H, torch.int32).cpu().numpy().astype(np.int64),
                tile_used_c=gpu_util._view(img, cl.tile_used_c, T, torch.int32).cpu().numpy().astype(np.int64),
                tile_used=tile_used)


def _tile_max(per_pixel, W, H):
    gx, gy = (W + 15) // 16, (H + 15) // 16
    pad = np.zeros((gy * 16, gx * 16), np.int64)
    pad[:H, :W] = per_pixel.reshape(H, W)
    return pad.reshape(gy, 16, gx, 16).max(axis=(1, 3)).reshape(-1)


def _check_lists(fw, u, st):
    """-> statistics dict; asserts the three list properties of the module docstring."""
    W, H = fw["W"], fw["H"]
    gx = (W + 15) // 16
    c = _compact(fw, u)
    rg = u["ranges"].astype(np.int64)
    T = rg.shape[0]
    n = rg[:, 1] - rg[:, 0]
    nc = u["n_contrib"].astype(np.int64)
    ncc = c["n_contrib_c"]
    pl = u["point_list"].astype(np.int64)
    used, used_c = c["tile_used"], c["tile_used_c"]
    # tile maxima, and the compact list is never longer than the visited prefix
    np.testing.assert_array_equal(used, _tile_max(nc, W, H))
    np.testing.assert_array_equal(used_c, _tile_max(ncc, W, H))
    assert (used <= n).all() and (used_c <= used).all()
    assert ((used_c == 0) == (used == 0)).all()
    # visited prefix and compact list, flattened: (tile, position) / (tile, compact index)
    v_tile = np.repeat(np.arange(T), used)
    v_pos = np.arange(used.sum()) - np.repeat(np.cumsum(used) - used, used)
    v_id = pl[rg[v_tile, 0] + v_pos]
    c_tile = np.repeat(np.arange(T), used_c)
    c_idx = np.arange(used_c.sum()) - np.repeat(np.cumsum(used_c) - used_c, used_c)
    c_id = c["cid"].astype(np.int64)[rg[c_tile, 0] + c_idx]
    c_qm = c["cqm"][rg[c_tile, 0] + c_idx]
    assert ((c_qm >= 1) & (c_qm <= 15)).all()
    # subsequence in order: a Gaussian occurs at most once per tile, so every compact entry has ONE position in the visited
    # prefix of its tile, and those positions must increase strictly along the compact list
    v_key = v_tile * (1 << 32) + v_id
    assert np.unique(v_key).size == v_key.size
    order = np.argsort(v_key, kind="stable")
    at = np.searchsorted(v_key[order], c_tile * (1 << 32) + c_id)
    assert (at < v_key.size).all()
    hit = order[np.minimum(at, v_key.size - 1)]
    assert (v_key[hit] == c_tile * (1 << 32) + c_id).all(), "a compact entry is not in the visited prefix of its tile"
    c_pos = v_pos[hit]
    same_tile = c_tile[1:] == c_tile[:-1]
    assert (c_pos[1:][same_tile] > c_pos[:-1][same_tile]).all(), "compact entries out of list order"
    # per pixel: the compact index names the same last contributor as the position
    py, px = np.divmod(np.arange(W * H), W)
    p_tile = (py // 16) * gx + px // 16
    assert ((ncc == 0) == (nc == 0)).all()
    has = nc > 0
    a = c["cid"].astype(np.int64)[rg[p_tile[has], 0] + ncc[has] - 1]
    np.testing.assert_array_equal(a, pl[rg[p_tile[has], 0] + nc[has] - 1])
    # dropped entries blend nowhere in their tile (float64, the oracle's per-Gaussian values)
    live = np.zeros(v_key.size, bool)
    live[hit] = True
    dead = np.nonzero(~live)[0]
    m = st.means2D.astype(np.float64)
    co = st.conic_opacity.astype(np.float64)
    ox, oy = np.meshgrid(np.arange(16.0), np.arange(16.0))
    ox, oy = ox.reshape(1, -1), oy.reshape(1, -1)
    worst, bad = 0.0, 0
    for s0 in range(0, dead.size, 50_000):
        d = dead[s0:s0 + 50_000]
        g, t = v_id[d], v_tile[d]
        dx = m[g, 0][:, None] - ((t % gx) * 16.0)[:, None] - ox
        dy = m[g, 1][:, None] - ((t // gx) * 16.0)[:, None] - oy
        pw = -0.5 * (co[g, 0][:, None] * dx * dx + co[g, 2][:, None] * dy * dy) - co[g, 1][:, None] * dx * dy
        with np.errstate(over="ignore"):
            al = np.where(pw > 0, 0.0, co[g, 3][:, None] * np.exp(np.minimum(pw, 0.0)))
        worst = max(worst, float(al.max()))
        bad += int((al >= 1.0 / 255.0).sum())
    stats = dict(visited=int(v_key.size), compact=int(c_id.size), dropped=int(dead.size), max_alpha_x255=worst * 255.0,
                 rounds=int(((used + 255) // 256).sum()), rounds_c=int(((used_c + 255) // 256).sum()),
                 listed=int(n.sum()), first_live_pos_max=int(c_pos[c_idx == 0].max()) if c_id.size else 0)
    print(stats)
    assert bad == 0, f"{bad} (pixel, dropped entry) pairs reach alpha >= 1/255; largest alpha x 255 = {worst * 255.0}"
    return stats


@pytest.mark.parametrize("name", ["indexed", "odd_size", "synth_small", "synth_300k", "dense", "huge_faint", "needles_long", "opaque_big"])
def test_compact_lists_and_gradients(hip, orc, name):
    inp, cam, indexed = _scene(name)
    st = cases.oracle_forward(inp, cam)
    fw = gpu_util.hip_forward(inp, cam, indexed)
    u = gpu_util.unpack(fw)
    np.testing.assert_array_equal(u["point_list"], st.point_list)
    np.testing.assert_array_equal(u["ranges"], st.ranges)
    s = _check_lists(fw, u, st)
    assert s["compact"] > 0
    if name.startswith("synth"):                          # a sizeable share of what the tiles visit is dead (39.7 % at full HD)
        assert s["dropped"] > (0.3 if name == "synth_300k" else 0.1) * s["visited"]
    if name == "dense":
        assert s["visited"] < 0.25 * s["listed"]           # the tiles saturate long before their lists end
    if name in cases.EDGE_GAUSSIAN_CASES:
        cases.edge_guard(name, st)
        assert s["dropped"] > 0                             # the cull has something to be wrong about
    if name == "huge_faint":
        assert s["first_live_pos_max"] >= 512 and s["rounds_c"] < s["rounds"]     # whole rounds of dead positions exist
    dL = synth.grad_image(cam["W"], cam["H"]).numpy()
    got = gpu_util.hip_backward(fw, dL)
    if name == "synth_300k":                              # full HD: the bars of tests/test_fullsize_gpu.py
        flipped = fullsize.flipped_pixels(u, st)
        assert flipped.sum() <= max(2, int(MAX_FLIPPED_FRACTION * cam["W"] * cam["H"])), int(flipped.sum())
        proof = fullsize.prove_flips(u, st, flipped)
        assert proof["outside_band"] == 0 and proof["oracle_outside_band"] == 0, proof
        errs, clean, _ = fullsize.grad_errors(st, flipped, got, orc.rasterize_backward(st, dL))
        print(int(flipped.sum()), "flipped pixels; rel-inf overall", errs, "away from them", clean)
        assert set(errs) >= {"dL_dmeans2D", "dL_dcolors", "dL_dopacity", "dL_dmeans3D", "dL_dsh", "dL_dscales", "dL_dscale_factors",
                             "dL_drotations"}
        for k in errs:
            assert clean[k] <= FULL_HD_TOL, f"{k}: rel-inf {clean[k]:.3e} away from the flipped pixels"
            assert errs[k] <= FULL_HD_TOL_FLIPPED, f"{k}: rel-inf {errs[k]:.3e} overall"
    elif name == "needles_long":                          # the oracle itself is off 1e-4 here: float64 truth, 4 x its deviation
        e = cases.edge_reference(name)
        np.testing.assert_array_equal(e["st"].point_list, st.point_list)
        fullsize.check_grads(st, u, got, e["ref"], GRAD_TOL, name, target=e["truth"], tols=fullsize.truth_tols(e["d_ref"], GRAD_TOL, 4.0))
    else:
        fullsize.check_grads(st, u, got, orc.rasterize_backward(st, dL), GRAD_TOL, name)
    again = gpu_util.hip_backward(fw, dL)
    # no float atomics on the non-indexed path, nor on these three tensors of the indexed one: bitwise reproducible
    for k in (got if not indexed else ("dL_dmeans3D", "dL_dopacity", "dL_dscale_factors")):
        np.testing.assert_array_equal(got[k].view(np.uint32), again[k].view(np.uint32))
    # the backward has not disturbed what it walked
    c2 = _compact(fw, u)
    np.testing.assert_array_equal(c2["tile_used_c"], _tile_max(c2["n_contrib_c"], cam["W"], cam["H"]))
