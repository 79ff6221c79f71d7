"""-m gpu: per-Gaussian error scores of a finished forward (csrc/render_error.hip: c3dgs_render_error, c3dgs_error_map_l1,
c3dgs_error_accumulate) and what is built on them (settings.error_target, GaussianModel.render(error_target=), add_error_stats,
error_stats, densify_and_prune(scores=), train(densify_by="error")).

On every scene of tests/depth_ref.py and on `long_run` (one faint screen-filling Gaussian in front of 300 small ones on a
272 x 272 image: its run of 17 x 17 = 289 slots takes two trips of stage B's whole-wave fold, which no other scene has):
  1. against the float64 walk of tests/error_ref.py under the standard map: a Gaussian is exempt if render_contrib's `hits`
     differs from the walk's, at most max(2, 2e-5 P) are; every other row within 1e-4 relative (the bar weight_sum is held to;
     tests/test_error_ref_cpu.py: an fp32 evaluation with the kernel's arithmetic stays within 1.19e-5). Rows of culled and of
     never-blended Gaussians are exact zero bits.
  2. identities: a map of ones gives render_contrib's weight_sum bit for bit, a map of zeros zero bits, twice the map twice
     the bits.
  3. against the product backward: precomputed colours, image gradient (map, 0, 0): dL_dcolors[:, 0] equals err_sum to rel-inf
     1e-4 (1e-3 on `deep` and `huge_faint`).
  4. map addressing: a one-hot map on `odd_size` at a pixel of a ragged edge tile; conservation under the standard map.
  5. reproducible, independent of the backward, guards intact, exact zeros where nothing is blended.
Then error_map_l1, error_accumulate, the settings / autograd layer, the model, densification by score and the sort time-out."""
import ctypes as C
import functools
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from tests import cases, contrib_ref, depth_ref, error_ref, gpu_util, synth

pytestmark = pytest.mark.gpu

GUARD_BITS = 0xC0E80000                    # float32 -7.25: what the outputs and their guard elements hold before a call
WS_GUARD = 4096                            # bytes behind the workspace, filled with 0xA5
SCATTERED = ("dL_dsh", "dL_dscales", "dL_drotations")      # indexed backward: float atomics into the codebook gradients
GRAD_TOL = 1e-4                            # tests/test_raster_gpu.py: what it holds those three to between two runs
SCENES = list(depth_ref.SCENES) + ["long_run"]


def _scene(name):
    """-> (inputs, cam, indexed); computed once per process, not to be modified."""
    return error_ref.long_run_scene() if name == "long_run" else depth_ref.scene(name)


def _state(name):
    return error_ref.long_run_state() if name == "long_run" else depth_ref.oracle_state(name)


@functools.lru_cache(maxsize=None)
def _reference(name):
    """the float64 walk under the standard map: computed once, shared, not to be modified"""
    st = _state(name)
    return error_ref.walk(st, st.W, st.H, error_ref.standard_map(st.H, st.W))


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def _stream():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def _render_error(fw, emap):
    """c3dgs_render_error on the buffers of forward `fw` under `emap` (numpy fp32 [H, W]) into an int32-viewed [P + 1] buffer
    pre-filled with GUARD_BITS (element P: the guard) and a workspace of exactly c3dgs_error_workspace_bytes followed by a guard
    region. Both guards are checked. -> float32 numpy [P]."""
    from c3dgs_amd import _lib
    L = _lib.lib()
    P, W, H, R = int(fw["radii"].numel()), fw["W"], fw["H"], fw["num_rendered"]
    assert emap.dtype == np.float32 and emap.shape == (H, W)
    fill = int(np.uint32(GUARD_BITS).view(np.int32))
    out = torch.full((P + 1,), fill, dtype=torch.int32, device="cuda")
    nbytes = int(L.c3dgs_error_workspace_bytes(P, R))
    ws = torch.full((nbytes + WS_GUARD,), 0xA5, dtype=torch.uint8, device="cuda")
    assert ws.data_ptr() % 256 == 0
    m = torch.from_numpy(np.ascontiguousarray(emap)).cuda()
    ptr = lambda t: t.data_ptr() if t is not None and t.numel() else None      # noqa: E731
    rc = L.c3dgs_render_error(P, W, H, R, ptr(fw["geom"]), ptr(fw["binning"]), ptr(fw["img"]), ws.data_ptr(), m.data_ptr(),
                              out.data_ptr(), _stream())
    _lib.check(rc)
    torch.cuda.synchronize()
    assert bool((ws[nbytes:] == 0xA5).all()), "the guard region behind the workspace was written"
    o = out.cpu().numpy().view(np.uint32)
    assert o[-1] == GUARD_BITS, "the guard element behind the output was written"
    return o[:-1].view(np.float32)


def _contrib(fw):
    """render_contrib of the same forward -> (weight_sum f32, hits u32) numpy"""
    from c3dgs_amd import rasterizer as rz
    ws, _, hits = rz._C.render_contrib(int(fw["radii"].numel()), fw["W"], fw["H"], fw["num_rendered"], fw["geom"], fw["binning"], fw["img"])
    return ws.cpu().numpy(), hits.cpu().numpy().view(np.uint32)


# ---------------------------------------------------------------------------------------------------------------- 1
@pytest.mark.parametrize("name", SCENES)
def test_scores_against_the_float64_walk(hip, orc, name):
    """Measured on an MI355X, over the eight scenes: 0 Gaussians exempt; largest relative difference of err_sum against the walk
    1.2e-5 (`needles_long`; 3.9e-6 on `opaque_big`, 2.5e-6 on `huge_faint`, 1.5e-6 on `deep`, below 1e-6 elsewhere). The test
    prints each figure before it asserts."""
    inp, cam, indexed = _scene(name)
    W, H = cam["W"], cam["H"]
    fw = gpu_util.hip_forward(inp, cam, indexed)
    u = gpu_util.unpack(fw)
    P = int(fw["radii"].numel())
    assert fw["num_rendered"] > 0
    e = error_ref.standard_map(H, W)
    err = _render_error(fw, e)
    _, hits = _contrib(fw)
    assert np.isfinite(err).all()
    # what the scenes are there for
    if name in ("indexed", "odd_size", "huge_faint", "deep"):
        assert (hits[256:] > 0).any(), "no blended Gaussian beyond the first 256-Gaussian scan group"
    if name == "deep":
        from tests.test_compact_lists_gpu import _compact
        assert _compact(fw, u)["tile_used_c"].max() > 256, "no tile with two batches of compact entries"
    if name == "odd_size":
        assert W % 16 != 0 and H % 16 != 0
    if name == "long_run":
        assert ((u["tiles_touched"] > 256) & (hits > 0)).any(), "no blended Gaussian whose run takes two trips of the whole-wave fold"
        assert hits[0] == W * H                                  # the screen-filling one is blended at every pixel

    check_scores(name, u, err, hits)


def check_scores(name, u, err, hits, ref=None):
    """err_sum under the standard map and the hits of the same forward (unpacked: `u`) against the float64 walk (`ref`: error_ref.walk
    of another scene's oracle state under the map in use): the bar of test_scores_against_the_float64_walk, shared with
    tests/test_scratch_poison_gpu.py and tests/test_call_sequence_gpu.py"""
    P = int(u["radii"].size)
    ref = _reference(name) if ref is None else ref
    same = hits.astype(np.int64) == ref.hits
    exempt = int((~same).sum())
    d = np.abs(err.astype(np.float64)[same] - ref.err_sum[same]) / np.where(ref.err_sum[same] > 0, ref.err_sum[same], 1.0)
    rel = float(d.max()) if d.size else 0.0
    print(name, "GPU vs float64 walk: Gaussians whose hits differ:", exempt, "of", P, "; largest relative difference of err_sum %.3g" % rel,
          "; blended pairs", int(ref.hits.sum()))
    assert exempt <= contrib_ref.exemption_cap(P)
    assert rel <= 1e-4
    dead = u["radii"] == 0
    assert (_bits(err)[dead] == 0).all()
    assert (_bits(err)[hits == 0] == 0).all()
    assert (err[hits > 0] > 0).all()                            # the map is bounded away from zero


# ---------------------------------------------------------------------------------------------------------------- 2
@pytest.mark.parametrize("name", SCENES)
def test_identities(hip, name):
    inp, cam, indexed = _scene(name)
    W, H = cam["W"], cam["H"]
    fw = gpu_util.hip_forward(inp, cam, indexed)
    wsum, hits = _contrib(fw)
    assert (hits > 0).any()
    np.testing.assert_array_equal(_bits(_render_error(fw, np.ones((H, W), np.float32))), _bits(wsum))
    assert (_bits(_render_error(fw, np.zeros((H, W), np.float32))) == 0).all()
    e = error_ref.standard_map(H, W)
    once, twice = _render_error(fw, e), _render_error(fw, (e * np.float32(2)).astype(np.float32))
    np.testing.assert_array_equal(_bits(twice), _bits((once * np.float32(2)).astype(np.float32)))
    assert not np.array_equal(_bits(once), _bits(wsum))


# ---------------------------------------------------------------------------------------------------------------- 3
@pytest.mark.parametrize("name", SCENES)
def test_scores_against_the_product_backward(hip, orc, name):
    """Measured on an MI355X: rel-inf 6.6e-7 at most (`huge_faint`; 6.1e-7 on `deep`, 1.3e-7 on `needles_long`, below 1e-7
    elsewhere). Printed before the assertion."""
    inp, cam, indexed = _scene(name)
    W, H = cam["W"], cam["H"]
    fw = gpu_util.hip_forward(inp, cam, indexed)
    P = int(fw["radii"].numel())
    g = torch.Generator().manual_seed(5)
    inp_c = dict(inp)
    inp_c.update(shs=None, sh_indices=None, colors_precomp=torch.rand(P, 3, generator=g).float(), bg=torch.zeros(3))
    fc = gpu_util.hip_forward(inp_c, cam, indexed)
    np.testing.assert_array_equal(gpu_util.unpack(fc)["n_contrib"], gpu_util.unpack(fw)["n_contrib"])      # the colours change no decision
    e = error_ref.standard_map(H, W)
    err = _render_error(fc, e)
    np.testing.assert_array_equal(_bits(err), _bits(_render_error(fw, e)))                  # ... and so no score
    grad = np.zeros((3, H, W), np.float32)
    grad[0] = e
    gc = gpu_util.hip_backward(fc, grad)
    d = gpu_util.rel_inf(err, gc["dL_dcolors"][:, 0])
    print(name, "err_sum vs dL_dcolors[:, 0] of the product backward under (map, 0, 0): rel-inf %.3g" % d)
    assert d <= (1e-3 if name in ("deep", "huge_faint") else 1e-4)


# ---------------------------------------------------------------------------------------------------------------- 4
def _edge_pixel(st, W, H):
    """a pixel of a ragged edge tile (the corner tile first) at which the float64 walk blends at least three Gaussians and takes
    no decision within 1e-3 relative of its threshold"""
    gx, gy = (W + 15) // 16, (H + 15) // 16
    assert W % 16 and H % 16
    corner = [(y, x) for y in range((gy - 1) * 16, H) for x in range((gx - 1) * 16, W)]
    right = [(y, x) for y in range(0, (gy - 1) * 16) for x in range((gx - 1) * 16, W)]
    for y, x in corner + right:
        ids, T, margin = error_ref.pixel_trace(st, W, H, y * W + x)
        if ids.size >= 3 and margin > 1e-3:
            return y, x, ids, T
    raise AssertionError("no suitable pixel in a ragged edge tile")


def test_map_addressing_one_hot_and_conservation(hip, orc):
    """Measured on an MI355X: the pixel is (0, 192) of tile (0, 12), 4 Gaussians, their sum within 1.8e-8 of 1 - final_T;
    conservation under the standard map within 1.8e-9."""
    name = "odd_size"
    inp, cam, indexed = _scene(name)
    W, H = cam["W"], cam["H"]
    st = _state(name)
    y, x, ids, T64 = _edge_pixel(st, W, H)
    fw = gpu_util.hip_forward(inp, cam, indexed)
    u = gpu_util.unpack(fw)
    hot = np.zeros((H, W), np.float32)
    hot[y, x] = 1.0
    err = _render_error(fw, hot)
    np.testing.assert_array_equal(np.nonzero(err)[0], np.sort(ids))
    blended = 1.0 - float(u["final_T"].reshape(H, W)[y, x])
    total = float(err.astype(np.float64).sum())
    print("one-hot map at pixel (%d, %d) of tile (%d, %d): %d Gaussians, sum %.9g, 1 - final_T %.9g, relative difference %.3g; float64 walk 1 - T %.9g"
          % (y, x, y // 16, x // 16, ids.size, total, blended, abs(total - blended) / blended, 1.0 - T64))
    assert abs(total - blended) <= 1e-5 * blended
    # conservation under the standard map: sum_g err_sum = sum_pix e (1 - final_T)
    e = error_ref.standard_map(H, W)
    err = _render_error(fw, e)
    total = float(err.astype(np.float64).sum())
    want = float((e.astype(np.float64).ravel() * (1.0 - u["final_T"].astype(np.float64))).sum())
    print("conservation: sum of err_sum %.9g, sum of e (1 - final_T) %.9g, relative difference %.3g" % (total, want, abs(total - want) / want))
    assert abs(total - want) <= 1e-5 * want


# ---------------------------------------------------------------------------------------------------------------- 5
@pytest.mark.parametrize("name", ["indexed", "odd_size", "long_run"])
def test_reproducible_and_independent_of_the_backward(hip, name):
    inp, cam, indexed = _scene(name)
    W, H = cam["W"], cam["H"]
    e = error_ref.standard_map(H, W)
    grad = synth.grad_image(W, H).numpy()
    g_plain = gpu_util.hip_backward(gpu_util.hip_forward(inp, cam, indexed), grad)             # a forward that never saw render_error
    fw = gpu_util.hip_forward(inp, cam, indexed)
    first = _render_error(fw, e)
    np.testing.assert_array_equal(_bits(first), _bits(_render_error(fw, e)))
    g_after = gpu_util.hip_backward(fw, grad)
    for k in g_plain:
        if indexed and k in SCATTERED:                          # the order of the atomic adds is not fixed
            assert gpu_util.rel_inf(g_after[k], g_plain[k]) <= GRAD_TOL, k
        else:
            np.testing.assert_array_equal(_bits(g_plain[k]), _bits(g_after[k]), err_msg=k)
    np.testing.assert_array_equal(_bits(first), _bits(_render_error(fw, e)))                   # the same after the backward


@pytest.mark.parametrize("name", ["empty", "all_behind"])
def test_nothing_to_blend_gives_exact_zeros(hip, name):
    inp, cam, indexed = cases.make_case(name)
    fw = gpu_util.hip_forward(inp, cam, indexed)
    P = int(fw["radii"].numel())
    assert fw["num_rendered"] == 0 and (P == 0) == (name == "empty")
    err = _render_error(fw, error_ref.standard_map(cam["H"], cam["W"]))
    assert err.shape == (P,) and (_bits(err) == 0).all()


# ---------------------------------------------------------------------------------------------------------------- 6
def _l1_numpy(img, gt):
    acc = np.abs(img[0] - gt[0]).astype(np.float32)
    for c in range(1, img.shape[0]):
        acc = (acc + np.abs(img[c] - gt[c]).astype(np.float32)).astype(np.float32)
    return (acc / np.float32(img.shape[0])).astype(np.float32)


# (C, H, W, offsets of img / gt / out in floats): every shape on aligned bases; at 64 x 48, where aligned bases take the 16-byte
# path, also with all three bases, and with the image alone, 4 bytes off
L1_CASES = [(c, h, w, (0, 0, 0)) for c in (1, 3) for h, w in ((1, 1), (5, 3), (33, 17), (64, 48))] + \
    [(3, 64, 48, (1, 1, 1)), (1, 64, 48, (1, 1, 1)), (3, 64, 48, (1, 0, 0))]


@pytest.mark.parametrize("Cn,H,W,offset", L1_CASES)
def test_error_map_l1_bit_equal_to_numpy(hip, Cn, H, W, offset):
    from c3dgs_amd import _lib
    g = torch.Generator().manual_seed(11 + Cn + H)
    n = Cn * H * W
    img, gt = torch.rand(n, generator=g) * 2 - 0.5, torch.rand(n, generator=g)
    bufs = []
    for src, off in ((img, offset[0]), (gt, offset[1])):
        b = torch.zeros(n + 1, device="cuda")
        b[off:off + n] = src.cuda()
        bufs.append(b[off:off + n])
    fill = int(np.uint32(GUARD_BITS).view(np.int32))
    out = torch.full((H * W + 2,), fill, dtype=torch.int32, device="cuda")
    o = out[offset[2]:offset[2] + H * W]
    assert all((t.data_ptr() % 16 == 4 * k) for t, k in zip(bufs + [o], offset))
    _lib.check(_lib.lib().c3dgs_error_map_l1(Cn, H, W, bufs[0].data_ptr(), bufs[1].data_ptr(), o.data_ptr(), _stream()))
    torch.cuda.synchronize()
    got = out.cpu().numpy().view(np.uint32)
    want = _l1_numpy(img.numpy().reshape(Cn, H, W), gt.numpy().reshape(Cn, H, W))
    np.testing.assert_array_equal(got[offset[2]:offset[2] + H * W], _bits(want).ravel())
    assert got[offset[2] + H * W] == GUARD_BITS and (offset[2] == 0 or got[0] == GUARD_BITS), "a word beside the output was written"


def test_error_map_l1_binding(hip):
    from c3dgs_amd import rasterizer as rz
    g = torch.Generator().manual_seed(3)
    img, gt = torch.rand(3, 33, 17, generator=g), torch.rand(3, 33, 17, generator=g)
    out = rz._C.error_map_l1(img.cuda(), gt.cuda())
    assert out.shape == (33, 17) and out.dtype == torch.float32
    np.testing.assert_array_equal(_bits(out.cpu().numpy()), _bits(_l1_numpy(img.numpy(), gt.numpy())))
    for bad in (gt[:, :, :16].cuda(), gt.double().cuda(), gt):
        with pytest.raises(RuntimeError):
            rz._C.error_map_l1(img.cuda(), bad)


# ---------------------------------------------------------------------------------------------------------------- 7
def test_error_accumulate_against_numpy(hip):
    from c3dgs_amd import _lib, rasterizer as rz
    L = _lib.lib()
    inp, _, indexed = depth_ref.scene("indexed")
    W, H, focal = 200, 136, 125.0
    evs = [(0.05, -0.03, 0.02, 0.99, 0.1, -0.05, 0.2), (0.0, 0.0, 0.0, 1.0, -0.3, 0.1, 0.0), (-0.04, 0.06, 0.0, 0.99, 0.2, 0.2, -0.4)]
    P = int(inp["means3D"].shape[0])
    emap = torch.from_numpy(error_ref.standard_map(H, W)).cuda()
    views = []
    for ev in evs:
        fw = gpu_util.hip_forward(inp, cases._cam(W, H, focal, ev)[0], indexed)
        views.append(rz._C.render_error(P, W, H, fw["num_rendered"], fw["geom"], fw["binning"], fw["img"], emap))
    assert all(int((v > 0).sum()) > 100 for v in views)
    g = torch.Generator().manual_seed(9)
    for mapped in (False, True):
        acc_max, acc_sum = torch.zeros(P, device="cuda"), torch.zeros(P, device="cuda")
        want_max, want_sum = np.zeros(P, np.float32), np.zeros(P, np.float32)
        touched = np.zeros(P, bool)
        for es in views:
            if mapped:       # a model of P rows of which a random 70 % are "visible": the view's rows are those, in order
                vis = torch.rand(P, generator=g) < 0.7
                rows = vis.nonzero().squeeze(1)
                rank = (torch.cumsum(vis.to(torch.int32), 0) - vis.to(torch.int32)).to(torch.int32)
                s = es[rows.cuda()].contiguous()
                visible, rank_d = vis.to(torch.uint8).cuda(), rank.cuda()
                rc = L.c3dgs_error_accumulate(P, int(rows.numel()), visible.data_ptr(), rank_d.data_ptr(), s.data_ptr(),
                                              acc_max.data_ptr(), acc_sum.data_ptr(), _stream())
                sel = vis.numpy()
            else:
                s = es
                rc = L.c3dgs_error_accumulate(P, P, None, None, s.data_ptr(), acc_max.data_ptr(), acc_sum.data_ptr(), _stream())
                sel = np.ones(P, bool)
            _lib.check(rc)
            sn = s.cpu().numpy()
            want_max[sel] = np.maximum(want_max[sel], sn)
            want_sum[sel] = want_sum[sel] + sn                  # one fp32 add per view, in view order
            touched |= sel
        torch.cuda.synchronize()
        np.testing.assert_array_equal(_bits(acc_max.cpu().numpy()), _bits(want_max))
        np.testing.assert_array_equal(_bits(acc_sum.cpu().numpy()), _bits(want_sum))
        assert not mapped or not touched.all()                  # some rows were visible in no view: left alone (zero bits above)
    # rows not visible keep what they held; a NaN row of a timed-out view propagates
    acc_max, acc_sum = torch.full((4,), 3.0, device="cuda"), torch.full((4,), 5.0, device="cuda")
    row = torch.tensor([float("nan"), 7.0], device="cuda")
    visible, rank = torch.tensor([1, 0, 1, 0], dtype=torch.uint8, device="cuda"), torch.tensor([0, 9, 1, 9], dtype=torch.int32, device="cuda")
    _lib.check(L.c3dgs_error_accumulate(4, 2, visible.data_ptr(), rank.data_ptr(), row.data_ptr(), acc_max.data_ptr(), acc_sum.data_ptr(), _stream()))
    torch.cuda.synchronize()
    am, asum = acc_max.cpu().numpy(), acc_sum.cpu().numpy()
    assert np.isnan(am[0]) and np.isnan(asum[0])
    assert am[1] == 3.0 and asum[1] == 5.0 and am[3] == 3.0 and asum[3] == 5.0
    assert am[2] == 7.0 and asum[2] == 12.0


# ---------------------------------------------------------------------------------------------------------------- 8
def _settings(hip, intr, ev, **kw):
    return hip.GaussianRasterizationSettings(intrinsic=intr.cuda(), extrinsic_vector=ev.cuda(), bg=torch.tensor((0.2, 0.4, 0.1), device="cuda"),
                                             scale_modifier=1.0, sh_degree=3, prefiltered=False, debug=False, clamp_color=True, **kw)


def test_settings_tuple_is_unchanged(hip):
    intr, ev = synth.camera(75, 50, 60.0)
    gt = torch.rand(3, 50, 75).cuda()
    plain, scored = _settings(hip, intr, ev), _settings(hip, intr, ev, error_target=gt)
    assert plain.error_target is None and scored.error_target is gt
    assert plain._fields == scored._fields and plain._fields[-1] == "depth" and "error_target" not in plain._fields
    assert len(plain) == len(scored) == 9
    assert tuple(plain[3:]) == tuple(scored[3:])
    same = plain._replace()
    assert same == plain and plain._replace(error_target=gt) == plain                   # equality is the tuple's: the elements alone
    intrinsic, extrinsic_vector, bg, scale_modifier, sh_degree, prefiltered, debug, clamp_color, depth = scored          # unpacks as before
    r = scored._replace(depth=True, contrib=True)
    assert r.error_target is gt and r.depth is True and r.contrib is True
    assert scored._replace(error_target=None).error_target is None and scored._replace(error_target=None).contrib is False
    assert plain._replace(sh_degree=2).error_target is None


@pytest.mark.parametrize("indexed", [False, True])
def test_settings_error_target_through_the_autograd_functions(hip, indexed, monkeypatch):
    from c3dgs_amd import rasterizer as rz
    P, W, H, focal = 1500, 75, 50, 60.0
    intr, ev = synth.camera(W, H, focal, extrinsic_vector=(0.05, -0.03, 0.02, 0.99, 0.1, -0.05, 0.2))
    sc = synth.scene(P, W, H, focal, seed=17, scale_median=0.08)
    names = ("means3D", "opacities", "shs", "scales", "rotations") + (("scale_factors",) if indexed else ())
    if indexed:
        sc = synth.index_scene(sc, shs_extra=32, gs_extra=32)
    gt = torch.rand(3, H, W, generator=torch.Generator().manual_seed(2)).cuda()

    seen = []
    entry = "rasterize_gaussians_indexed" if indexed else "rasterize_gaussians"
    real = getattr(rz._C, entry)

    def spy(*a):
        out = real(*a)
        seen.append(out)
        return out
    monkeypatch.setattr(rz._C, entry, spy)

    def run(loss, **kw):
        leaves = {k: sc[k].cuda().requires_grad_() for k in names}
        means2D = torch.zeros_like(leaves["means3D"], requires_grad=True)
        rs = _settings(hip, intr, ev, **kw)
        if indexed:
            out = hip.GaussianRasterizerIndexed(rs)(means3D=leaves["means3D"], means2D=means2D, opacities=leaves["opacities"],
                                                    sh_indices=sc["sh_indices"].cuda(), g_indices=sc["g_indices"].cuda(), shs=leaves["shs"],
                                                    scales=leaves["scales"], scale_factors=leaves["scale_factors"],
                                                    rotations=leaves["rotations"], extrinsic_vector=ev.cuda())
        else:
            out = hip.GaussianRasterizer(rs)(means3D=leaves["means3D"], means2D=means2D, opacities=leaves["opacities"], shs=leaves["shs"],
                                             scales=leaves["scales"], rotations=leaves["rotations"], extrinsic_vector=ev.cuda())
        loss(out).backward()
        torch.cuda.synchronize()
        return out, {k: v.grad.clone() for k, v in leaves.items()}

    plain, g0 = run(lambda o: o[0].sum())
    assert len(plain) == 2                                      # no target: exactly what there was
    only, g1 = run(lambda o: o[0].sum() + o[2].sum(), error_target=gt)
    assert len(only) == 3
    R, color, _, geom, binning, img = seen[-1]
    want = rz._C.render_error(P, W, H, R, geom, binning, img, rz._C.error_map_l1(color, gt))
    full, g2 = run(lambda o: o[0].sum() + o[8].sum(), depth=True, contrib=True, error_target=gt)
    assert len(full) == 9                                       # three maps, three contrib rows, then err_sum
    R, _, _, geom, binning, img = seen[-1]
    want_depth = rz._C.render_depth(P, W, H, R, geom, binning, img)
    want_contrib = rz._C.render_contrib(P, W, H, R, geom, binning, img)
    for t, w in zip(full[2:5], want_depth):
        assert t.shape == (H, W) and torch.equal(t.view(torch.int32), w.view(torch.int32))
    for t, w in zip(full[5:8], want_contrib):
        assert t.shape == (P,) and torch.equal(t.view(torch.int32), w.view(torch.int32))
    for t in (only[2], full[8]):
        assert t.shape == (P,) and t.dtype == torch.float32 and not t.requires_grad
        assert torch.equal(t.view(torch.int32), want.view(torch.int32))
    assert int((only[2] > 0).sum()) > 100
    for out in (only, full):
        assert torch.equal(out[0].view(torch.int32), plain[0].view(torch.int32)) and torch.equal(out[1], plain[1])
    # no gradient through the score: the parameter gradients are those of image.sum() alone
    for gx in (g1, g2):
        for k in g0:
            assert torch.equal(g0[k].view(torch.int32), gx[k].view(torch.int32)) or \
                (indexed and torch.allclose(g0[k], gx[k], rtol=1e-5, atol=1e-6 * float(g0[k].abs().max()))), k
    for bad in (gt[:, :, :W - 1].contiguous(), gt.double(), gt.cpu(), gt[0]):
        with pytest.raises(RuntimeError):
            run(lambda o: o[0].sum(), error_target=bad)


# ---------------------------------------------------------------------------------------------------------------- 9
class _Cam:
    def __init__(self, intrinsic, ev, target=None):
        self.intrinsic, self.extrinsic_vector = intrinsic.cuda(), ev.cuda()
        self.original_image = target


_EVS = [(0, 0, 0, 1, 0, 0, 0), (0.02, -0.03, 0.0, 1.0, 0.4, 0.1, 0.3), (-0.03, 0.02, 0.01, 1.0, -0.5, -0.2, -0.2)]
MW, MH, MFOCAL = 90, 60, 80.0


def _dense_model(sc, quantization=False):
    from c3dgs_amd.model import GaussianModel
    m = GaussianModel(3, quantization=quantization, device="cuda")
    op = sc["opacities"].clamp(1e-6, 1 - 1e-6)
    norm = sc["scales"].norm(dim=1, keepdim=True)
    m.set_tensors(xyz=sc["means3D"], features_dc=sc["shs"][:, :1], features_rest=sc["shs"][:, 1:], scaling=sc["scales"] / norm,
                  rotation=sc["rotations"], opacity=torch.log(op / (1 - op)), scaling_factor=torch.log(norm))
    return m


def _model(path, quantization=False, behind_fraction=0.2):
    from c3dgs_amd.model import GaussianModel
    sc = synth.scene(2000, W=MW, H=MH, focal=MFOCAL, seed=23, scale_median=0.06, behind_fraction=behind_fraction)
    if path != "fused_indexed":
        return _dense_model(sc, quantization)
    m = GaussianModel(3, quantization=quantization, device="cuda")
    m.set_tensors(**synth.raw_params(synth.index_scene(sc, seed=24, shs_extra=32, gs_extra=32)))
    return m


def _cams():
    g = torch.Generator().manual_seed(77)
    return [_Cam(*synth.camera(MW, MH, MFOCAL, extrinsic_vector=ev), target=torch.rand(3, MH, MW, generator=g).cuda()) for ev in _EVS]


@pytest.mark.parametrize("path,gather", [("fused_indexed", True), ("composed", True), ("composed", False)])
def test_model_render_error_target(hip, path, gather):
    from c3dgs_amd import rasterizer as rz
    from c3dgs_amd.model import PipelineParams
    m = _model(path)
    P = m._xyz.shape[0]
    cam, bg = _cams()[0], torch.zeros(3, device="cuda")
    before = m.render(cam, PipelineParams(), bg, gather_visible=gather)
    assert set(before) == {"render", "viewspace_points", "visibility_filter", "radii", "visible"}        # today's keys, exactly
    out = m.render(cam, PipelineParams(), bg, gather_visible=gather, error_target=cam.original_image, return_depth=True)
    assert set(out) == set(before) | {"error_sum", "error_rank", "depth", "alpha", "median_depth"}
    if gather:                                                  # model row -> row of the scores, for the visible ones
        vis = out["visible"]
        assert out["error_rank"].dtype == torch.int32 and torch.equal(out["error_rank"][vis].long(), torch.arange(int(vis.sum()), device="cuda"))
    else:
        assert out["error_rank"] is None
    rows = out["radii"].shape[0]
    assert rows == (int(out["visible"].sum()) if gather else P) and (not gather or rows < P)
    es = out["error_sum"]
    assert es.shape == (rows,) and es.dtype == torch.float32 and not es.requires_grad
    assert bool((es[out["radii"] == 0] == 0).all()) and int((es > 0).sum()) > 100
    # conservation through the model: sum_g error_sum = sum_pix e alpha, e the map of this very render
    emap = rz._C.error_map_l1(out["render"].detach(), cam.original_image)
    total, want = float(es.double().sum()), float((emap.double() * out["alpha"].double()).sum())
    assert abs(total - want) <= 1e-5 * want
    out["render"].sum().backward()
    assert all(p.grad is not None and torch.isfinite(p.grad).all() for p in m.parameters())


def test_model_error_sum_agrees_between_the_gathered_and_the_full_call(hip):
    """the same model, camera and target with and without the gather of the visible rows: the rasterizer sees the same visible
    Gaussians in the same order, so a Gaussian's score has the same bits under both row numberings"""
    from c3dgs_amd.model import PipelineParams
    m = _model("composed")
    cam, bg = _cams()[1], torch.zeros(3, device="cuda")
    with torch.no_grad():
        a = m.render(cam, PipelineParams(), bg, gather_visible=True, error_target=cam.original_image)
        b = m.render(cam, PipelineParams(), bg, gather_visible=False, error_target=cam.original_image)
    assert torch.equal(a["render"].view(torch.int32), b["render"].view(torch.int32))
    vis = a["visible"].bool()
    full = torch.zeros(m._xyz.shape[0], device="cuda")
    full[vis] = a["error_sum"][a["error_rank"][vis].long()]
    assert int((full > 0).sum()) > 100
    assert torch.equal(full.view(torch.int32), b["error_sum"].view(torch.int32))


@pytest.mark.parametrize("path", ["fused_indexed", "composed"])
def test_error_stats_equal_the_views_folded_by_hand(hip, path):
    from c3dgs_amd.model import PipelineParams
    m = _model(path)
    P = m._xyz.shape[0]
    cams, bg = _cams(), torch.zeros(3, device="cuda")
    st = m.error_stats(cams, PipelineParams(), bg)
    assert set(st) == {"error_max", "error_sum"} and not any(t.requires_grad for t in st.values())
    emax, esum = np.zeros(P, np.float32), np.zeros(P, np.float32)
    with torch.no_grad():
        for cam in cams:
            out = m.render(cam, PipelineParams(), bg, error_target=cam.original_image)
            vis = out["visible"].cpu().numpy().astype(bool)
            s = out["error_sum"].cpu().numpy()
            emax[vis] = np.maximum(emax[vis], s)
            esum[vis] = esum[vis] + s
    np.testing.assert_array_equal(_bits(st["error_max"].cpu().numpy()), _bits(emax))
    np.testing.assert_array_equal(_bits(st["error_sum"].cpu().numpy()), _bits(esum))
    assert (emax > 0).sum() > 100 and (emax == 0).sum() > 100 and (esum >= emax).all()


@pytest.mark.parametrize("path", ["fused_indexed", "composed"])
def test_error_stats_leave_the_observers_alone(hip, path):
    from c3dgs_amd.model import PipelineParams
    m = _model(path, quantization=True, behind_fraction=0.0)
    cams, bg = _cams(), torch.zeros(3, device="cuda")
    with torch.no_grad():
        m.render(cams[0], PipelineParams(), bg)                 # the observers have seen something
        m._opacity += 1.0                                       # ... and the next getter call would move the opacity observer
        state = m._fq_state.clone()
    st = m.error_stats(cams, PipelineParams(), bg)
    assert float(st["error_max"].max()) > 0
    assert torch.equal(m._fq_state.view(torch.int32), state.view(torch.int32))
    with torch.no_grad():
        m.render(cams[0], PipelineParams(), bg)
    assert not torch.equal(m._fq_state.view(torch.int32), state.view(torch.int32)), "a render moved no observer: nothing was protected"


def test_add_error_stats_folds_and_does_not_allocate(hip):
    m = _model("composed")
    P = m._xyz.shape[0]
    g = torch.Generator().manual_seed(13)
    rows = [torch.rand(P, generator=g).cuda() * 10.0 ** (k % 5 - 2) for k in range(9)]
    vis = (torch.rand(P, generator=g) < 0.6)
    rank = (torch.cumsum(vis.to(torch.int32), 0) - vis.to(torch.int32)).to(torch.int32).cuda()
    vis_d = vis.cuda()
    short = [r[vis_d].contiguous() for r in rows]
    n0 = None
    for k in range(9):
        if k == 1:                                              # after the first call, which creates the accumulators
            n0 = torch.cuda.memory_stats()["num_device_alloc"]
        if k % 2:
            m.add_error_stats(short[k], vis_d, rank)
        else:
            m.add_error_stats(rows[k])
    assert torch.cuda.memory_stats()["num_device_alloc"] == n0
    emax, esum = np.zeros(P, np.float32), np.zeros(P, np.float32)
    v = vis.numpy()
    for k in range(9):
        if k % 2:
            s = short[k].cpu().numpy()
            emax[v] = np.maximum(emax[v], s)
            esum[v] = esum[v] + s
        else:
            s = rows[k].cpu().numpy()
            emax, esum = np.maximum(emax, s), (esum + s).astype(np.float32)
    np.testing.assert_array_equal(_bits(m.error_max.cpu().numpy()), _bits(emax))
    np.testing.assert_array_equal(_bits(m.error_sum_acc.cpu().numpy()), _bits(esum))
    with pytest.raises(RuntimeError):
        m.add_error_stats(rows[0], vis_d, None)
    with pytest.raises(RuntimeError):
        m.add_error_stats(short[1])


# ---------------------------------------------------------------------------------------------------------------- 10
def _hidden_setup():
    """-> (model of the base scene, [camera whose target is the hidden scene's render], bg)"""
    from c3dgs_amd.model import PipelineParams
    base, hidden = error_ref.hidden_scene()
    m, teacher = _dense_model(base), _dense_model(hidden)
    intr, ev = synth.camera(error_ref.HIDDEN_W, error_ref.HIDDEN_H, error_ref.HIDDEN_FOCAL)
    bg = torch.zeros(3, device="cuda")
    cam = _Cam(intr, ev)
    with torch.no_grad():
        cam.original_image = teacher.render(cam, PipelineParams(), bg)["render"].clone()
    return m, base, [cam], bg


def test_top_scores_lie_where_the_image_is_wrong(hip):
    """Chosen on the CPU: under the float64 walk with the oracle's two images, 92 % of the top 5 % of the scores have their
    centre inside the region that holds 17 % of all centres. Measured on an MI355X: 0.920 inside, 0.080 outside."""
    from c3dgs_amd.model import PipelineParams
    m, base, cams, bg = _hidden_setup()
    s = m.error_stats(cams, PipelineParams(), bg)["error_max"].cpu().numpy()
    inside = error_ref.in_region(base["means3D"]).numpy()
    k = int(0.05 * s.size)
    top = np.argsort(-s, kind="stable")[:k]
    f_in = float(inside[top].mean())
    print("top 5 %% of the scores (%d rows): %.3f inside the region, %.3f outside; the region holds %.3f of all centres; lowest top score %.4g"
          % (k, f_in, 1 - f_in, float(inside.mean()), float(s[top].min())))
    assert s[top].min() > 0
    assert f_in >= 0.8 and f_in >= 4 * (1 - f_in) and inside.mean() < 0.25


def test_densify_and_prune_by_scores(hip):
    from c3dgs_amd import _lib
    from c3dgs_amd.model import PipelineParams
    m, base, cams, bg = _hidden_setup()
    m.percent_dense, extent = 0.01, 5.0
    P = m._xyz.shape[0]
    s = m.error_stats(cams, PipelineParams(), bg)["error_max"]
    thr = float(np.sort(s.cpu().numpy())[-P // 20])             # the 5 % of the test above
    with torch.no_grad():
        big = m.get_scaling.detach().amax(dim=1) > m.percent_dense * extent
    sel = s >= thr
    want_clone, want_split = (sel & ~big).nonzero().squeeze(1), (sel & big).nonzero().squeeze(1)
    assert want_clone.numel() > 5 and want_split.numel() > 5
    m.add_error_stats(s)                                        # accumulators exist and hold something
    src, kind, draw_row, (kept, clones, S, CK) = m.densify_and_prune(thr, 0.0, extent, None, scores=s)
    assert (clones, S, CK) == (want_clone.numel(), want_split.numel(), want_split.numel()) and kept == P - S
    assert torch.equal(src[kind == 1].long().sort().values, want_clone)
    assert torch.equal(src[kind == 2].long().unique(), want_split)
    assert m._xyz.shape[0] == kept + clones + 2 * CK
    # the error accumulators start again at the new length
    assert m.error_max.shape == (m._xyz.shape[0],) and not bool(m.error_max.any()) and not bool(m.error_sum_acc.any())
    with pytest.raises(RuntimeError):
        m.densify_and_prune(thr, 0.0, extent, None, scores=s)   # the old length
    assert _lib.ROW_CLONE == 2


def test_scores_of_a_gradient_run_give_the_gradient_plan(hip):
    base, _ = error_ref.hidden_scene()
    g = torch.Generator().manual_seed(8)
    P = base["means3D"].shape[0]
    accum = (torch.rand(P, 1, generator=g) * 1e-3).cuda()
    denom = torch.randint(0, 4, (P, 1), generator=g).float().cuda()         # zeros among them: 0 / 0 rows
    plans = []
    for by_score in (False, True):
        m = _dense_model(base)
        m.percent_dense = 0.01
        m.xyz_gradient_accum, m.denom, m.max_radii2D = accum.clone(), denom.clone(), torch.zeros(P, device="cuda")
        torch.manual_seed(4)
        if by_score:
            plans.append(m.densify_and_prune(0.0002, 0.005, 5.0, None, scores=(accum / denom).reshape(P)))
        else:
            plans.append(m.densify_and_prune(0.0002, 0.005, 5.0, None))
    (s0, k0, d0, t0), (s1, k1, d1, t1) = plans
    assert t0 == t1 and t0[1] > 0 and t0[2] > 0
    assert torch.equal(s0, s1) and torch.equal(k0, k1) and torch.equal(d0, d1)


def _train_scene(tmp_path):
    from tests import train_scene
    student, cams, extent = train_scene.make(tmp_path, "cuda")

    class Scene:
        gaussians = student
        cameras_extent = extent

        def getTrainCameras(self):
            return cams
    return student, cams, Scene()


def _three_epochs():
    """24 iterations over 8 views: epochs 0, 1, 2; one densification, behind epoch 2"""
    from c3dgs_amd.pipeline import OptimizationParams
    return OptimizationParams(iterations=24, position_lr_max_steps=24, densify_from_iter=0, densification_interval=1,
                              opacity_reset_interval=24, densify_until_iter=24)


def test_train_densifies_by_error(hip, tmp_path, monkeypatch):
    from c3dgs_amd import pipeline
    from c3dgs_amd.model import GaussianModel, PipelineParams
    student, cams, scene = _train_scene(tmp_path)
    P0 = student._xyz.shape[0]
    with pytest.raises(ValueError):
        pipeline.train(scene, None, _three_epochs(), PipelineParams(), camera_stride=1, densify_by="error")
    with pytest.raises(ValueError):
        pipeline.train(scene, None, _three_epochs(), PipelineParams(), camera_stride=1, densify_by="colour")
    # the threshold: the median positive score of the untrained student over the training views (its scale follows the
    # resolution and the scene, there is no default)
    s = student.error_stats(cams, PipelineParams(), torch.zeros(3, device="cuda"))["error_max"]
    thr = float(s[s > 0].median())
    calls = []
    real = GaussianModel.densify_and_prune

    def spy(self, *a, **kw):
        calls.append((a[0], kw["scores"].clone(), self.max_radii2D.clone()))
        return real(self, *a, **kw)
    monkeypatch.setattr(GaussianModel, "densify_and_prune", spy)
    events = []
    torch.manual_seed(0)
    n = pipeline.train(scene, None, _three_epochs(), PipelineParams(), camera_stride=1, degree_up_iter=80, densify_by="error",
                       error_threshold=thr, log=lambda e, i: events.append((e, i)))
    dens = [i["densified"] for _, i in events if i["densified"] is not None]
    print("train(densify_by='error', error_threshold=%.4g): rows %d -> %d, densifications %s" % (thr, P0, student._xyz.shape[0], dens))
    assert n == 24 and len(events) == 3 and len(dens) >= 1 and len(calls) == len(dens)
    rows, (kept, clones, S, CK) = dens[0]
    assert clones + S > 0 and student._xyz.shape[0] == kept + clones + 2 * CK
    thr_used, scores, max_radii = calls[0]
    assert thr_used == thr and scores.shape == (P0,) and float(scores.max()) > thr and bool((max_radii > 0).any())
    assert clones + S <= int((scores >= thr).sum())             # what was selected, less the clones the opacity prune took
    for p in student.parameters():
        assert p.shape[0] == student._xyz.shape[0] and bool(torch.isfinite(p).all())
    assert student.error_max.shape == (student._xyz.shape[0],) and not bool(student.error_max.any())


def test_train_by_gradient_is_the_loop_it_was(hip, tmp_path, monkeypatch):
    """densify_by="grad" and the call without the new arguments: the same final count and ema_loss for a fixed seed, no render
    with an error target, no densification by scores, no error accumulators."""
    from c3dgs_amd import pipeline
    from c3dgs_amd.model import GaussianModel, PipelineParams
    seen = []
    real_render, real_densify = GaussianModel.render, GaussianModel.densify_and_prune

    def render(self, *a, **kw):
        seen.append(("render", tuple(sorted(kw))))
        return real_render(self, *a, **kw)

    def densify(self, *a, **kw):
        seen.append(("densify", len(a), tuple(sorted(kw))))
        return real_densify(self, *a, **kw)
    results = []
    for k, extra in enumerate((dict(), dict(densify_by="grad"))):
        (tmp_path / str(k)).mkdir()
        student, cams, scene = _train_scene(tmp_path / str(k))
        events = []
        with monkeypatch.context() as mp:
            mp.setattr(GaussianModel, "render", render)
            mp.setattr(GaussianModel, "densify_and_prune", densify)
            torch.manual_seed(0)
            pipeline.train(scene, None, _three_epochs(), PipelineParams(), camera_stride=1, degree_up_iter=80,
                           log=lambda e, i: events.append((e, dict(i))), **extra)
        assert getattr(student, "error_max", None) is None
        results.append((student._xyz.shape[0], events[-1][1]["ema_loss"], [i["densified"] for _, i in events]))
    assert set(seen) == {("render", ("clamp_color", "cov3d", "gather_visible")), ("densify", 4, ())}
    print("train by gradient, default call and densify_by='grad':", results)
    assert results[0] == results[1] and results[0][2][-1] is not None


# ---------------------------------------------------------------------------------------------------------------- 11
_TIMEOUT_CHILD = r"""
import ctypes as C, numpy as np, torch, sys
from tests import gpu_util, synth
from oracle import oracle as orc
from c3dgs_amd import _lib, rasterizer as rz
assert _lib.LIB_PATH.endswith("libc3dgs_hip_spin1.so"), _lib.LIB_PATH
intr, ev = synth.camera(640, 360, 400.0)
cam = orc.camera(intr.numpy(), ev.numpy())
sc = synth.scene(400_000, 640, 360, 400.0, seed=3, scale_median=0.02)
inp = dict(bg=torch.zeros(3), means3D=sc["means3D"], opacities=sc["opacities"], shs=sc["shs"], scales=sc["scales"],
           rotations=sc["rotations"], degree=3, clamp_color=True)
fw = gpu_util.hip_forward(inp, cam, False)           # look-backs give up: the forward's image is NaN
torch.cuda.synchronize()
assert torch.isnan(fw["color"]).all(), "a forward whose sort timed out must return a NaN image"
emap = torch.full((360, 640), 0.5, device="cuda")
es = rz._C.render_error(int(fw["radii"].numel()), 640, 360, fw["num_rendered"], fw["geom"], fw["binning"], fw["img"], emap)
torch.cuda.synchronize()
assert es.shape == (400_000,) and torch.isnan(es).all(), "scores of a forward whose sort timed out must be NaN"
print("NAN_ROWS")
"""


def test_sort_timeout_gives_nan_rows():
    """With the `spin1` variant of the library, started the way tests/test_render_contrib_gpu.py::test_sort_timeout_gives_nan_rows
    starts its child: the forward's image is NaN, every err_sum row is NaN."""
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    lib = os.path.join(root, "c3dgs_amd", "libc3dgs_hip_spin1.so")
    if not os.path.exists(lib):
        from c3dgs_amd import build
        build.build_variant("spin1")
    r = subprocess.run([sys.executable, "-c", _TIMEOUT_CHILD], cwd=root, env=dict(os.environ, C3DGS_LIB_PATH=lib),
                       capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    assert "NAN_ROWS" in r.stdout, r.stdout
