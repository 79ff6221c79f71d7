"""-m gpu: the depth-distortion map and its gradient (csrc/render_distortion.hip, csrc/render_maps_backward.hip;
GaussianRasterizationSettings(distortion=), GaussianModel.render(distortion=), pipeline.train(lambda_dist=)).

  forward    on tests/depth_ref.py's scenes, raw and ndc(0.2, 100): against the float64 prefix formula of tests/distortion_ref.py on
             the oracle's forward (tied to the brute-force double sum with |.| by tests/test_distortion_ref_cpu.py), the skip
             decisions replayed from the fp32 formula and a pair whose fp32 alpha is within 4e-6 of 1/255 free to go either way, as
             tests/depth_grad_ref.py does for the depth gradients. Pixels where the HIP forward and the oracle disagree on
             n_contrib are skipped, at most depth_ref.exemption_cap of them; on the rest |got - ref| <= smax 2e-5 + 1e-4 |ref|
             (tests/test_render_depth_gpu.py's depth bar with s for z), for the moment too. Two calls: the same bits.
  truth      every leaf gradient against the float64 reference (autograd over the walk's pairs, or the closed form under the
             replayed decisions), rel-inf <= 1e-4, with gL alone and with gD, gA, gL together.
  opt-in     distortion=False is today's call, bit for bit; with it the other outputs keep their bits; a loss that ignores the map
             gives depth_grad's backward, bits and stage counts; a three-map backward replays the blend once.
  edges, model, driver.

Measured on an MI355X (from this file's prints): see FORWARD_MEASURED and TRUTH_MEASURED below."""
import functools

import numpy as np
import pytest
import torch

from tests import cases, depth_grad_ref as dgr, depth_ref, distortion_ref as dr, gpu_util, synth
from tests.test_depth_grad_gpu import (CASE_CAMERA, LEAF_KEYS, TRUTH_NAMES, _Cam, _maps, _module_scene, _run, _run_module, _same,
                                       _settings, _worst)
from tests.test_pose_grad_gpu import _stage_counts

pytestmark = pytest.mark.gpu

FORWARD_MEASURED = ("largest error over its bar, distortion / moment: raw indexed 3.3e-3 / 2.3e-3, odd_size 3.0e-3 / 2.6e-3, opaque_big 2.9e-3 / "
                    "4.0e-3, needles_long 3.0e-2 / 2.6e-1, huge_faint 5.1e-3 / 3.1e-3, deep 2.0e-3 / 1.8e-3, one_pixel 0 / 0; ndc indexed 5.3e-4 / "
                    "9.5e-3, odd_size 5.8e-4 / 6.0e-3, opaque_big 5.2e-4 / 4.5e-3, needles_long 3.5e-3 / 3.2e-1, huge_faint 4.6e-4 / 7.4e-4, deep "
                    "3.5e-4 / 3.4e-3, one_pixel 0 / 1.1e-4")
TRUTH_MEASURED = ("worst leaf rel-inf, gL alone / three maps: raw tiny 2.7e-6 / 1.9e-6, indexed 2.1e-5 / 7.9e-6, odd_size 1.3e-5 / 7.2e-6, "
                  "cov_precomp 1.8e-5 / 8.5e-6, colors_precomp 1.8e-5 / 8.5e-6; ndc tiny 1.2e-5 / 1.9e-6, indexed 1.2e-5 / 4.6e-6, odd_size 1.8e-5 / "
                  "6.8e-6, cov_precomp 1.9e-5 / 5.1e-6, colors_precomp 1.8e-5 / 1.3e-5; train: mean distortion of the held view 1.070 without "
                  "the term, 0.912 with lambda_dist = 1")

MODE_NAMES = ("raw", "ndc")


def _dev(x):
    return None if x is None else torch.from_numpy(np.ascontiguousarray(x, dtype=np.float32)).cuda()


def _render(fw, mode):
    from c3dgs_amd import rasterizer
    P = int(fw["radii"].numel())
    d, m = rasterizer._C.render_distortion(P, fw["W"], fw["H"], fw["num_rendered"], fw["geom"], fw["binning"], fw["img"], mode)
    return d, m


def _backward(fw, dL_dout, gD=None, gA=None, gL=None, moment=None, mode=None):
    """_C.rasterize_gaussians_backward(_indexed) on the buffers of forward `fw` with the three maps. numpy or None in (`moment`: the
    device tensor of _render). -> {name: numpy}"""
    from c3dgs_amd import rasterizer
    a = fw["args"]
    kw = dict(dL_ddepth=_dev(gD), dL_dalpha=_dev(gA))
    if gL is not None:
        kw.update(dL_ddistortion=_dev(gL), moment=moment, near_far=mode)
    if fw["indexed"]:
        (bg, means3D, colors, opac, scales, sf, rot, smod, cov3D, view, proj, tfx, tfy, H, W, sh, deg, campos, shi, gi, pre, dbg, clamp) = a
        out = rasterizer._C.rasterize_gaussians_backward_indexed(
            bg, means3D, fw["radii"], colors, scales, sf, rot, smod, cov3D, view, proj, tfx, tfy, _dev(dL_dout), sh, deg, campos,
            fw["geom"], fw["num_rendered"], fw["binning"], fw["img"], False, shi, gi, **kw)
        names = ("dL_dmeans2D", "dL_dcolors", "dL_dopacity", "dL_dmeans3D", "dL_dcov3D", "dL_dsh", "dL_dscales", "dL_dscale_factors",
                 "dL_drotations")
    else:
        (bg, means3D, colors, opac, scales, rot, smod, cov3D, view, proj, tfx, tfy, H, W, sh, deg, campos, pre, dbg, clamp) = a
        out = rasterizer._C.rasterize_gaussians_backward(
            bg, means3D, fw["radii"], colors, scales, rot, smod, cov3D, view, proj, tfx, tfy, _dev(dL_dout), sh, deg, campos,
            fw["geom"], fw["num_rendered"], fw["binning"], fw["img"], False, **kw)
        names = ("dL_dmeans2D", "dL_dcolors", "dL_dopacity", "dL_dmeans3D", "dL_dcov3D", "dL_dsh", "dL_dscales", "dL_drotations")
    torch.cuda.synchronize()
    return {n: o.detach().cpu().numpy() for n, o in zip(names, out)}


# ---------------------------------------------------------------------------------------------------------------- forward
@functools.lru_cache(maxsize=None)
def _forward_reference(name, mode_name):
    """once per process, shared, not to be modified"""
    inp, cam, _ = depth_ref.scene(name)
    return dr.forward_candidates(depth_ref.oracle_state(name), cam["W"], cam["H"], dr.MODES[mode_name])


def check_forward(name, mode_name, u, st, dist, moment, refs=None):
    """the forward bar for the two maps of scene `name` (its forward unpacked: `u`, its oracle state: `st`); shared with
    tests/test_distortion_poison_gpu.py"""
    refs = _forward_reference(name, mode_name) if refs is None else refs
    W, H = st.W, st.H
    skip = (u["n_contrib"].astype(np.int64) != st.n_contrib.astype(np.int64)).reshape(H, W)
    print(f"{name} {mode_name}: pixels skipped (HIP forward and oracle disagree on n_contrib): {int(skip.sum())}; admissible references: "
          f"{len(refs)}")
    assert skip.sum() <= depth_ref.exemption_cap(W * H)
    smax = refs[0]["smax"]
    assert 0 < smax < 1e4
    for key, got in (("distortion", dist), ("moment", moment)):
        assert np.isfinite(got).all(), key
        over = np.min([np.abs(got - r[key]) / (smax * 2e-5 + 1e-4 * np.abs(r[key])) for r in refs], axis=0)
        over[skip] = 0.0
        err = np.min([np.abs(got - r[key]) for r in refs], axis=0)
        err[skip] = 0.0
        print(f"{name} {mode_name}: {key} largest error {float(err.max()):.3e}, largest error over its bar {float(over.max()):.3e}, "
              f"smax {smax:.4f}, largest value {float(np.abs(refs[0][key]).max()):.4e}")
        assert (over <= 1.0).all(), (key, int((over > 1.0).sum()), float(over.max()))
        # only the pixel of an ambiguous pair may need another reference than the first, the fp32 decisions as they are
        first = np.abs(got - refs[0][key]) / (smax * 2e-5 + 1e-4 * np.abs(refs[0][key]))
        first[skip] = 0.0
        needs_flip = set(np.nonzero(first.reshape(-1) > 1.0)[0].tolist())
        print(f"{name} {mode_name}: {key} pixels that match only a flipped reference: {sorted(needs_flip)}; ambiguous pixels: "
              f"{refs[0]['ambiguous_pixels']}")
        assert needs_flip <= set(refs[0]["ambiguous_pixels"]), (key, sorted(needs_flip), refs[0]["ambiguous_pixels"])
    assert (dist >= 0).all()


@pytest.mark.parametrize("mode_name", MODE_NAMES)
@pytest.mark.parametrize("name", depth_ref.SCENES)
def test_forward_against_the_float64_prefix_formula(hip, orc, name, mode_name):
    inp, cam, indexed = depth_ref.scene(name)
    st = depth_ref.oracle_state(name)
    fw = gpu_util.hip_forward(inp, cam, indexed)
    u = gpu_util.unpack(fw)
    mode = dr.MODES[mode_name]
    d, m = _render(fw, mode)
    d2, m2 = _render(fw, mode)
    assert torch.equal(d.view(torch.int32), d2.view(torch.int32)) and torch.equal(m.view(torch.int32), m2.view(torch.int32))
    dist, moment = d.cpu().numpy().astype(np.float64), m.cpu().numpy().astype(np.float64)
    check_forward(name, mode_name, u, st, dist, moment)
    if name == "one_pixel":
        assert not dist.any() and moment.max() > 0
    else:
        assert dist.max() > 0
    if mode_name == "raw":
        # the moment of the raw mode is the depth map, to the rounding of two different summation orders: the depth map's own bar
        depth = hip.rasterizer._C.render_depth(st.P, cam["W"], cam["H"], fw["num_rendered"], fw["geom"], fw["binning"], fw["img"])[0]
        z = u["depths"][u["radii"] > 0]
        diff = np.abs(moment - depth.cpu().numpy().astype(np.float64))
        print(f"{name}: raw moment against the depth map, largest difference {float(diff.max()):.3e}")
        assert (diff <= float(z.max()) * 2e-5 + 1e-4 * np.abs(moment)).all()
    # valid behind the backward as well, with the same bits
    gpu_util.hip_backward(fw, synth.grad_image(cam["W"], cam["H"]).numpy())
    d3, m3 = _render(fw, mode)
    assert torch.equal(d.view(torch.int32), d3.view(torch.int32)) and torch.equal(m.view(torch.int32), m3.view(torch.int32))


# ---------------------------------------------------------------------------------------------------------------- backward truth
TRUTH_CASES = ["tiny", "indexed", "odd_size", "cov_precomp", "colors_precomp"]


def _best(got, cands, names_of, label):
    per_candidate = []
    for want in cands:
        ref = {k: want[v].reshape(got[k].shape) for k, v in names_of.items() if v in want and k in got}
        per_candidate.append((max(gpu_util.rel_inf(got[k], ref[k]) for k in ref), ref))
    print(f"{label}: worst rel-inf per admissible reference:", ["%.3e" % e for e, _ in per_candidate])
    return min(per_candidate, key=lambda t: t[0])[1]


@pytest.mark.parametrize("three", [False, True], ids=["gL", "gD+gA+gL"])
@pytest.mark.parametrize("mode_name", MODE_NAMES)
@pytest.mark.parametrize("name", TRUTH_CASES)
def test_truth_float64(hip, name, mode_name, three):
    st, inp, cam, indexed = dgr.black_state(name)
    W, H = cam["W"], cam["H"]
    mode = dr.MODES[mode_name]
    replayed, amb, cands = dr.candidates(name, mode_name, three)
    gL = dr.gl_map(W, H)
    gD, gA = (dgr.hashed_map(W, H, 1), dgr.hashed_map(W, H, 2)) if three else (None, None)
    fw = gpu_util.hip_forward(inp, cam, indexed)
    u = gpu_util.unpack(fw)
    differ = int((u["n_contrib"].astype(np.int64) != st.n_contrib.astype(np.int64)).sum())
    print(f"truth {name}: pixels where the HIP forward and the oracle disagree on n_contrib: {differ}; replayed {replayed}; ambiguous {amb}")
    assert differ <= depth_ref.exemption_cap(W * H)
    _, moment = _render(fw, mode)
    got = _backward(fw, None, gD, gA, gL, moment, mode)
    label = f"truth {name} {mode_name} {'three maps' if three else 'gL alone'}"
    ref = _best(got, cands, TRUTH_NAMES, label)
    assert "dL_dmeans3D" in ref and "dL_dopacity" in ref and ("dL_dcov3D" in ref) == (name == "cov_precomp")
    worst = _worst(got, ref, tuple(ref), 1e-4, label + ":")
    print(f"{label}: worst rel-inf {worst:.3e}")
    assert not got["dL_dcolors"].any() and not got["dL_dsh"].any()              # the maps do not depend on the colours
    if three:
        # the sum of the references: depth_grad_ref's for (gD, gA) plus this file's for gL alone, where no decision is replayed
        r0, a0, alone = dr.candidates(name, mode_name, False)
        if not r0 and not a0:
            both = dgr.truth(name)[2]
            for k, v in TRUTH_NAMES.items():
                if k in ref and v in both:
                    total = both[v].reshape(ref[k].shape) + alone[0][v].reshape(ref[k].shape)
                    assert gpu_util.rel_inf(ref[k], total) <= 1e-8, k


@pytest.mark.parametrize("mode_name", MODE_NAMES)
@pytest.mark.parametrize("name", ["tiny", "indexed"])
def test_truth_through_the_autograd_modules(hip, orc, name, mode_name):
    """param.grad end to end: settings with distortion=, the loss (depth gD).sum() + (alpha gA).sum() + (distortion gL).sum()"""
    st, inp, cam, indexed = dgr.black_state(name)
    W, H, focal = CASE_CAMERA[name]
    mode = dr.MODES[mode_name]
    _, _, cands = dr.candidates(name, mode_name, True)
    intr, ev = synth.camera(W, H, focal, extrinsic_vector=(0.05, -0.03, 0.02, 0.99, 0.1, -0.05, 0.2))
    rs = hip.GaussianRasterizationSettings(intrinsic=intr.cuda(), extrinsic_vector=ev.cuda(), bg=inp["bg"].cuda(),
                                           scale_modifier=float(inp["scale_modifier"]), sh_degree=int(inp["degree"]), prefiltered=False,
                                           debug=False, clamp_color=bool(inp["clamp_color"]), distortion=True if mode is None else mode)
    leaves = {k: inp[k].cuda().requires_grad_() for k in LEAF_KEYS if inp.get(k) is not None}
    means2D = torch.zeros_like(leaves["means3D"], requires_grad=True)
    kw = dict(means3D=leaves["means3D"], means2D=means2D, opacities=leaves["opacities"], shs=leaves.get("shs"),
              colors_precomp=leaves.get("colors_precomp"), scales=leaves.get("scales"), rotations=leaves.get("rotations"),
              cov3D_precomp=leaves.get("cov3D_precomp"), extrinsic_vector=ev.cuda())
    if indexed:
        rast = hip.GaussianRasterizerIndexed(rs)
        kw.update(sh_indices=inp["sh_indices"].cuda(), g_indices=inp["g_indices"].cuda(), scale_factors=leaves.get("scale_factors"))
    else:
        rast = hip.GaussianRasterizer(rs)
    image, radii, depth, alpha, median, distortion = rast(**kw)
    assert distortion.requires_grad and depth.requires_grad and alpha.requires_grad and not median.requires_grad
    tD, tA, tL = (_dev(m) for m in (dgr.hashed_map(W, H, 1), dgr.hashed_map(W, H, 2), dr.gl_map(W, H)))
    ((depth * tD).sum() + (alpha * tA).sum() + (distortion * tL).sum()).backward()
    torch.cuda.synchronize()
    got = {k: v.grad.cpu().numpy() for k, v in leaves.items() if k not in ("shs", "colors_precomp")}
    got["means2D"] = means2D.grad.cpu().numpy()
    ref = _best(got, cands, {k: k for k in got}, f"modules {name} {mode_name}")
    worst = _worst(got, ref, tuple(ref), 1e-4, f"modules {name} {mode_name}:")
    print(f"modules {name} {mode_name}: worst rel-inf {worst:.3e}")


# ---------------------------------------------------------------------------------------------------------------- opt-in and bits
def _bits_equal(a, b):
    return torch.equal(a.view(torch.int32), b.view(torch.int32)) if a.dtype == torch.float32 else torch.equal(a, b)


@pytest.mark.parametrize("indexed", [False, True])
def test_opt_in_and_bits(hip, indexed):
    sc, intr, ev, W, H = _module_scene(indexed)
    gD, gA = (torch.from_numpy(m).cuda() for m in _maps(W, H))
    gL = _dev(dr.gl_map(W, H))
    wimg = synth.grad_image(W, H).cuda()
    rs = _settings(hip, intr, ev, distortion=dr.NDC)
    ndc32 = tuple(float(np.float32(v)) for v in dr.NDC)          # the settings keep the pair as the fp32 values the library receives
    assert rs.distortion == ndc32 and rs.depth_grad is False and "distortion" not in rs._fields and len(rs) == 9
    assert rs._replace(scale_modifier=2.0).distortion == ndc32 and rs._replace(distortion=False).distortion is False
    assert _settings(hip, intr, ev).distortion is False and _settings(hip, intr, ev, distortion=True).distortion is True
    # 1e-50 underflows to 0 in fp32, and 1 + 1e-9 rounds to 1: in order as doubles, not as the floats the library receives
    for bad in ((0.0, 1.0), (2.0, 1.0), (1.0,), "ndc", (1e-50, 1.0), (1.0, 1.0 + 1e-9)):
        with pytest.raises(ValueError):
            _settings(hip, intr, ev, distortion=bad)

    image_loss = lambda o: (o[0] * wimg).sum()                                          # noqa: E731
    maps_loss = lambda o: (o[2] * gD).sum() + (o[3] * gA).sum()                         # noqa: E731
    three_loss = lambda o: maps_loss(o) + (o[-1] * gL).sum()                            # noqa: E731
    # distortion=False: today's outputs and gradients, bit for bit
    plain, g_plain = _run(hip, sc, intr, ev, indexed, image_loss)
    off, g_off = _run(hip, sc, intr, ev, indexed, image_loss, distortion=False)
    assert len(plain) == len(off) == 2
    for a, b in zip(off, plain):
        assert _bits_equal(a, b)
    for k in g_plain:
        assert _same(g_off[k], g_plain[k], indexed, k), k
    # with it: the image, depth, alpha and median bits are depth_grad's; the map is the last output and differentiable
    ref_out, g_ref_img = _run(hip, sc, intr, ev, indexed, image_loss, depth_grad=True)
    for mode in (True, dr.NDC):
        (out, g_img), counts_img = _stage_counts(hip, lambda: _run(hip, sc, intr, ev, indexed, image_loss, distortion=mode))
        assert len(out) == 6 and len(ref_out) == 5
        for a, b in zip(out[:5], ref_out):
            assert _bits_equal(a, b)
        assert out[5].requires_grad and out[2].requires_grad and out[3].requires_grad and not out[4].requires_grad
        assert out[5].shape == (H, W) and float(out[5].detach().min()) >= 0 and float(out[5].detach().max()) > 0
        # a loss that ignores the distortion output: today's backward bits and stage counts
        for k in g_plain:
            assert _same(g_img[k], g_plain[k], indexed, k), k
        assert counts_img.get("render_distortion") == 1 and "render_distortion_backward" not in counts_img
        assert "render_depth_backward" not in counts_img
    (_, g_ref_maps), counts_ref = _stage_counts(hip, lambda: _run(hip, sc, intr, ev, indexed, maps_loss, depth_grad=True))
    (_, g_maps), counts_maps = _stage_counts(hip, lambda: _run(hip, sc, intr, ev, indexed, maps_loss, distortion=True))
    for k in g_ref_maps:
        assert _same(g_maps[k], g_ref_maps[k], indexed, k), k
    extra = {k: v for k, v in counts_maps.items() if counts_ref.get(k) != v}
    assert extra == {"render_distortion": 1}, (counts_maps, counts_ref)
    assert counts_maps.get("render_depth_backward") == 1
    # the three-map backward: ONE replay of the blend for the maps
    (_, g_three), counts_three = _stage_counts(hip, lambda: _run(hip, sc, intr, ev, indexed, three_loss, distortion=True))
    assert counts_three.get("render_distortion_backward") == 1 and "render_depth_backward" not in counts_three
    assert counts_three.get("depth_backward_fold") == 1 and "render_backward" not in counts_three
    (_, g_all), counts_all = _stage_counts(hip, lambda: _run(hip, sc, intr, ev, indexed, lambda o: image_loss(o) + three_loss(o),
                                                               distortion=True))
    assert counts_all.get("render_distortion_backward") == 1 and "render_depth_backward" not in counts_all
    assert counts_all.get("render_backward") == 1
    # image + three maps = image-only + three-maps-only, to the re-association of two fp32 addends (tests/test_depth_grad_gpu.py)
    for k in g_plain:
        want = (g_img[k].double() + g_three[k].double()).cpu().numpy()
        e = gpu_util.rel_inf(g_all[k].cpu().numpy(), want)
        print(f"image + three maps against the sum, {'indexed' if indexed else 'plain'}, {k}: rel-inf {e:.3e}")
        assert e <= 1e-5, (k, e)
    # the distortion term is there: the three-map gradients differ from the two-map ones
    assert not torch.equal(g_three["opacities"], g_maps["opacities"]) and not g_three["shs"].any()
    # two runs of the same backward: equal bits (non-indexed: no atomics anywhere)
    _, g_again = _run(hip, sc, intr, ev, indexed, three_loss, distortion=True)
    for k in g_three:
        assert _same(g_again[k], g_three[k], indexed, k), k


@pytest.mark.parametrize("indexed", [False, True])
def test_pose_gradient_with_distortion_is_refused(hip, indexed):
    sc, intr, ev, W, H = _module_scene(indexed, P=64)
    rs = _settings(hip, intr, ev, distortion=True)
    cls = hip.GaussianRasterizerIndexed if indexed else hip.GaussianRasterizer
    for oc in ((True, "exact") if indexed else ("exact",)):
        with pytest.raises(ValueError, match="distortion"):
            cls(rs, optimize_camera=oc)
        rast = cls(_settings(hip, intr, ev), optimize_camera=oc)
        rast.raster_settings = rs                               # swapped in behind the constructor: refused at the call
        with pytest.raises(ValueError, match="distortion"):
            _run_module(rast, sc, ev, indexed)
    cls(rs, optimize_camera=False)


# ---------------------------------------------------------------------------------------------------------------- edges
@pytest.mark.parametrize("name", ["all_behind", "one_tile"])
def test_edges_nothing_visible_and_one_tile(hip, orc, name):
    """all_behind: R == 0, zero maps without a launch, every gradient an exact zero. one_tile (9 x 5 pixels): narrower than a wave's
    pixel block; forward and gradients against the float64 reference."""
    inp, cam, indexed = cases.make_case(name)
    W, H = cam["W"], cam["H"]
    gL = dr.gl_map(W, H)
    fw = gpu_util.hip_forward(inp, cam, indexed)
    if name == "all_behind":
        assert fw["num_rendered"] == 0
        (d, m), counts = _stage_counts(hip, lambda: _render(fw, None))
        assert not d.any() and not m.any() and "render_distortion" not in counts
        got = _backward(fw, None, None, None, gL, m, None)
        for k, v in got.items():
            assert not v.any(), k
        return
    st, inp_b, _, _ = dgr.black_state(name)
    for mode_name in MODE_NAMES:
        mode = dr.MODES[mode_name]
        d, m = _render(fw, mode)
        refs = dr.forward_candidates(st, W, H, mode)
        check_forward(name, mode_name, gpu_util.unpack(fw), st, d.cpu().numpy().astype(np.float64), m.cpu().numpy().astype(np.float64), refs)
        _, _, cands = dr.candidates(name, mode_name, False)
        got = _backward(fw, None, None, None, gL, m, mode)
        ref = _best(got, cands, TRUTH_NAMES, f"one_tile {mode_name}")
        _worst(got, ref, tuple(ref), 1e-4, f"one_tile {mode_name}:")


def test_edges_no_gaussians_and_a_single_one(hip, orc):
    from c3dgs_amd import rasterizer
    # P == 0: zeros, no blend launch
    empty = torch.empty(0, dtype=torch.uint8, device="cuda")
    (d, m), counts = _stage_counts(hip, lambda: rasterizer._C.render_distortion(0, 40, 24, 0, empty, empty, empty, dr.NDC))
    assert d.shape == (24, 40) and not d.any() and not m.any() and "render_distortion" not in counts
    # a single Gaussian: no pair, a zero map. Its gradients are exact zeros in float64 (tests/test_distortion_ref_cpu.py); fp32 leaves
    # the round-off of the backward's pivot, a few ulp of s <= 4 times w |gL| <= 1, held to 1e-6 where a wrong term would be of order 1
    inp, cam, indexed = depth_ref.scene("one_pixel")
    fw = gpu_util.hip_forward(inp, cam, indexed)
    assert fw["num_rendered"] == 1
    for mode in (None, dr.NDC):
        d, m = _render(fw, mode)
        assert not d.any() and float(m.max()) > 0
        got = _backward(fw, None, None, None, np.ones((1, 1)), m, mode)
        for k, v in got.items():
            assert np.isfinite(v).all() and np.abs(v).max() <= 1e-6, (k, float(np.abs(v).max()))
    with pytest.raises(RuntimeError, match="moment"):
        _backward(fw, None, None, None, np.ones((1, 1)), None, None)


# ---------------------------------------------------------------------------------------------------------------- model and driver
def _model_for(path, sc):
    from c3dgs_amd.model import GaussianModel
    m = GaussianModel(3, quantization=True, device="cuda")
    if path == "fused_indexed":
        m.set_tensors(**synth.raw_params(synth.index_scene(sc, seed=24, shs_extra=32, gs_extra=32)))
    else:
        op = sc["opacities"].clamp(1e-6, 1 - 1e-6)
        m.set_tensors(xyz=sc["means3D"], features_dc=sc["shs"][:, :1], features_rest=sc["shs"][:, 1:],
                      scaling=sc["scales"] / sc["scales"].norm(dim=1, keepdim=True), rotation=sc["rotations"],
                      opacity=torch.log(op / (1 - op)), scaling_factor=torch.log(sc["scales"].norm(dim=1, keepdim=True)))
    return m


def _module_level_call(hip, m, cam, bg, distortion, antialiasing):
    """The rasterizer MODULE on the model's own activated tensors, gathered to the visible rows as the reference's render() gathers
    them: what GaussianModel.render(distortion=) has to equal, whichever of its two paths it takes.
    -> (color, radii, depth, alpha, median, distortion)"""
    from c3dgs_amd.model import ColorMode
    indexed = m.color_index_mode == ColorMode.ALL_INDEXED and m.is_gaussian_indexed
    rs = hip.GaussianRasterizationSettings(intrinsic=cam.intrinsic, extrinsic_vector=cam.extrinsic_vector, bg=bg, scale_modifier=1.0,
                                           sh_degree=m.active_sh_degree, prefiltered=False, debug=False, clamp_color=True,
                                           distortion=distortion, antialiasing=antialiasing)
    rast = (hip.GaussianRasterizerIndexed if indexed else hip.GaussianRasterizer)(rs)
    means3D, opacity = m.get_xyz, m.get_opacity
    screen = torch.zeros_like(means3D, requires_grad=True)
    rows = rast.markVisible(means3D, extrinsic_vector=cam.extrinsic_vector).nonzero(as_tuple=False).squeeze(1)
    pick = lambda t: t.index_select(0, rows)                                            # noqa: E731
    if indexed:
        return rast(means3D=pick(means3D), means2D=pick(screen), shs=m._get_features_raw, sh_indices=pick(m._feature_indices),
                    g_indices=pick(m._gaussian_indices), opacities=pick(opacity), scales=m.get_scaling_normalized,
                    scale_factors=pick(m.get_scaling_factor), rotations=m._rotation_post_activation,
                    extrinsic_vector=cam.extrinsic_vector)
    return rast(means3D=pick(means3D), means2D=pick(screen), shs=pick(m.get_features), opacities=pick(opacity),
                scales=pick(m.get_scaling), rotations=pick(m.get_rotation), extrinsic_vector=cam.extrinsic_vector)


@pytest.mark.parametrize("path,antialiasing", [("fused_indexed", False), ("composed", False), ("fused_indexed", True)],
                         ids=["fused_indexed", "composed", "fused_indexed-antialiased"])
def test_model_render_distortion(hip, path, antialiasing):
    """GaussianModel.render(distortion=(near, far)) against the module-level call on the model's own activated tensors: the same
    distortion, depth and alpha bits, and every parameter's gradient under a loss on the distortion map within the file's bar.
    Three models of the same tensors, one per render, so that every getter's observer sees its first call in each."""
    from c3dgs_amd.model import PipelineParams
    W, H, focal = 90, 60, 80.0
    sc = synth.scene(2000, W=W, H=H, focal=focal, seed=23, scale_median=0.06)
    m, twin, third = (_model_for(path, sc) for _ in range(3))
    intr, ev = synth.camera(W, H, focal)
    cam, bg = _Cam(intr, ev), torch.zeros(3, device="cuda")
    kw = dict(antialiasing=antialiasing)
    base = third.render(cam, PipelineParams(), bg, depth_grad=True, **kw)
    out = m.render(cam, PipelineParams(), bg, distortion=dr.NDC, **kw)
    assert set(out) == set(base) | {"distortion"}
    for k in ("render", "depth", "alpha", "median_depth"):
        assert torch.equal(out[k].view(torch.int32), base[k].view(torch.int32)), k
    assert out["distortion"].requires_grad and out["depth"].requires_grad and not out["median_depth"].requires_grad
    assert out["distortion"].shape == (H, W) and float(out["distortion"].detach().max()) > 0
    # the module-level call: the same maps, bit for bit
    ref = _module_level_call(hip, twin, cam, bg, dr.NDC, antialiasing)
    assert len(ref) == 6 and torch.equal(ref[1] > 0, out["visibility_filter"])
    for k, r in (("render", ref[0]), ("depth", ref[2]), ("alpha", ref[3]), ("median_depth", ref[4]), ("distortion", ref[5])):
        assert torch.equal(out[k].view(torch.int32), r.view(torch.int32)), k
    # ... and the mode reached the rasterizer: the raw map of the same tensors is another map
    raw = _module_level_call(hip, third, cam, bg, True, antialiasing)[5]
    assert float((raw.detach() - out["distortion"].detach()).abs().max()) > 10 * float(out["distortion"].detach().max())
    gL = _dev(dr.gl_map(W, H))
    (out["distortion"] * gL).sum().backward()
    (ref[5] * gL).sum().backward()
    torch.cuda.synchronize()
    worst = 0.0
    for k, (p, q) in enumerate(zip(m.parameters(), twin.parameters())):
        assert p.grad is not None and q.grad is not None and bool(torch.isfinite(p.grad).all()), k
        if float(q.grad.abs().max()) == 0:
            assert not bool(p.grad.any()), k                    # the colours: the map does not depend on them
            continue
        e = gpu_util.rel_inf(p.grad.cpu().numpy(), q.grad.cpu().numpy())
        print(f"model {path}{' antialiased' if antialiasing else ''}: parameter {k} {tuple(p.shape)} rel-inf to the module-level call {e:.3e}")
        worst = max(worst, e)
        assert e <= 1e-4, (k, e)
    print(f"model {path}{' antialiased' if antialiasing else ''}: worst rel-inf {worst:.3e}")
    assert float(m._xyz.grad.abs().max()) > 0 and float(m._opacity.grad.abs().max()) > 0
    assert float(twin._xyz.grad.abs().max()) > 0 and float(twin._opacity.grad.abs().max()) > 0
    pose = _Cam(intr, ev)
    pose.extrinsic_vector.requires_grad_()
    with pytest.raises(ValueError, match="distortion"):
        m.render(pose, PipelineParams(), bg, distortion=True)


def test_finetune_with_the_distortion_term(hip, tmp_path):
    """finetune(lambda_dist=0) is today's loop, stage for stage and bit for bit; with a weight the term is there from
    `dist_from_iter` on, one forward replay and one three-map backward replay per view; a negative weight is refused."""
    import random
    from c3dgs_amd import pipeline
    from c3dgs_amd.model import PipelineParams
    from tests import train_scene

    def run(k, **kw):
        (tmp_path / str(k)).mkdir()
        student, cams, _ = train_scene.make(tmp_path / str(k), "cuda", W=96, H=64, focal=90.0, views=4)

        class Scene:
            gaussians = student

            def getTrainCameras(self):
                return cams
        random.seed(3)
        torch.manual_seed(0)
        ema, counts = _stage_counts(hip, lambda: pipeline.finetune(Scene(), pipeline._Dataset(), pipeline.OptimizationParams(),
                                                                   pipeline.CompressionParams(finetune_iterations=6), PipelineParams(), **kw))
        assert np.isfinite(ema)
        return [p.detach().clone() for p in student.parameters()], counts, Scene()

    p0, c0, _ = run(0)
    p1, c1, _ = run(1, lambda_dist=0.0, dist_near_far=dr.NDC, dist_from_iter=2)
    assert c1 == c0 and "render_distortion" not in c0, (c1, c0)
    for a, b in zip(p0, p1):
        assert torch.equal(a.view(torch.int32), b.view(torch.int32))
    p2, c2, scene = run(2, lambda_dist=1.0, dist_near_far=dr.NDC, dist_from_iter=2)
    assert c2.get("render_distortion") == 4 and c2.get("render_distortion_backward") == 4 and "render_depth_backward" not in c2
    assert all(bool(torch.isfinite(p).all()) for p in p2) and any(not torch.equal(a, b) for a, b in zip(p0, p2))
    for bad in (dict(lambda_dist=-1.0), dict(lambda_dist=1.0, dist_near_far=(5.0, 1.0))):
        with pytest.raises(ValueError):
            pipeline.finetune(scene, pipeline._Dataset(), pipeline.OptimizationParams(), pipeline.CompressionParams(finetune_iterations=2),
                              PipelineParams(), **bad)


def test_train_with_the_distortion_term(hip, tmp_path):
    """A few epochs on the toy scene: lambda_dist = 0 is the default loop (stage counts and final parameters); with the term the
    run is finite and the mean distortion of a held view ends below the plain run's."""
    from c3dgs_amd import pipeline
    from c3dgs_amd.model import PipelineParams
    from tests import train_scene
    W, H, focal = 160, 112, 150.0

    def make(k):
        (tmp_path / str(k)).mkdir()
        student, cams, extent = train_scene.make(tmp_path / str(k), "cuda", W=W, H=H, focal=focal)

        class Scene:
            gaussians = student
            cameras_extent = extent

            def getTrainCameras(self):
                return cams[:-1]
        return student, Scene(), cams[-1]

    opt = lambda: train_scene.schedule(35, densify=False)       # noqa: E731
    bg = torch.zeros(3, device="cuda")

    def held(student, cam):
        with torch.no_grad():
            return float(student.render(cam, PipelineParams(), bg, distortion=True)["distortion"].mean())

    finals, counts, dists = [], [], []
    for k, kw in enumerate((dict(), dict(lambda_dist=0.0, dist_near_far=dr.NDC, dist_from_iter=3), dict(lambda_dist=1.0, dist_from_iter=7))):
        student, scene, held_cam = make(k)
        torch.manual_seed(0)
        losses = []
        n, c = _stage_counts(hip, lambda: pipeline.train(scene, None, opt(), PipelineParams(), camera_stride=1,
                                                         log=lambda e, i: losses.append(i["ema_loss"]), **kw))
        assert n == 35 and len(losses) == 5 and all(np.isfinite(v) for v in losses)
        finals.append([p.detach().clone() for p in student.parameters()])
        counts.append(c)
        dists.append(held(student, held_cam))
        for p in student.parameters():
            assert bool(torch.isfinite(p).all())
    # lambda_dist == 0: the default loop, launch for launch and bit for bit
    assert counts[1] == counts[0], (counts[1], counts[0])
    assert "render_distortion" not in counts[0] and "render_distortion_backward" not in counts[0]
    for a, b in zip(finals[0], finals[1]):
        assert torch.equal(a.view(torch.int32), b.view(torch.int32))
    # with the term: from iteration 7 on, one forward replay and one backward replay per view
    assert counts[2].get("render_distortion") == 35 - 7 and counts[2].get("render_distortion_backward") == 35 - 7
    assert "render_depth_backward" not in counts[2]
    print(f"mean distortion of the held view: lambda_dist=0 {dists[0]:.6e}, lambda_dist=1 {dists[2]:.6e}")
    assert dists[2] < dists[0]
    with pytest.raises(ValueError):
        pipeline.train(scene, None, opt(), PipelineParams(), camera_stride=1, lambda_dist=-1.0)
    with pytest.raises(ValueError):
        pipeline.train(scene, None, opt(), PipelineParams(), camera_stride=1, lambda_dist=1.0, dist_near_far=(5.0, 1.0))
