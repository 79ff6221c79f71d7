"""-m gpu: gradients through the depth and alpha maps (csrc/render_maps_backward.hip; GaussianRasterizationSettings(depth_grad=True),
GaussianModel.render(depth_grad=True), pipeline.train(lambda_depth=, lambda_alpha=)).

  identity   By linearity the map gradients equal the PRODUCT backward's on the same scene with colours (z, 1, 0), a black
             background and the image gradient (gD, gA, 0), where dL/dz is that backward's dL_dcolors[:, 0]; z is built in fp32
             torch from means3D and the view matrix, so that means3D receives the z-term. Every gradient tensor, means2D
             included, rel-inf (max abs difference over the reference's max abs) <= 1e-4: the bar of the contrib, error and
             pose tests. Both maps, then each alone (the NULL-map paths), on both rasterizers (a non-indexed scene goes to the
             indexed one with identity indices).
  truth      end to end against the float64 autograd of tests/depth_grad_ref.py (dense_render on the oracle's lists), rel-inf
             <= 1e-4, the pose test's end-to-end bar; also with cov3D_precomp and with colors_precomp. The 1/255 skip is the
             forward's decision, replayed and not re-decided: where the float64 reference decides a pair otherwise than the fp32
             formula (one pair on odd_size, alpha64 / thr - 1 = -3.4e-6, worth 1.9e-3 of dL_dmeans3D: the CPU oracle's own backward
             is that far from the float64 autograd there), the reference is the float64 closed form under the fp32 decisions
             (tests/depth_grad_ref.py: candidates; tied to the autograd at 1e-8 by tests/test_depth_grad_ref_cpu.py), every
             tensor at the same bar; a pair whose fp32 alpha is within 4e-6 of the threshold may go either way.
             The same cases once more through GaussianRasterizer / GaussianRasterizerIndexed with leaf tensors and the loss
             (depth gD).sum() + (alpha gA).sum(): every leaf's .grad against the same reference at the same bar.
  opt-in     depth_grad's forward outputs are depth=True's bits; a loss on the image alone gives the plain settings' bits;
             image + maps = image-only + maps-only to rel-inf 1e-5 (two fp32 addends, re-associated); two runs are bit-equal on
             the non-indexed path; median does not require grad.
  edges, model, driver.

Measured on an MI355X (from this file's prints): see IDENTITY_MEASURED, TRUTH_MEASURED and SUM_MEASURED below."""
import functools

import numpy as np
import pytest
import torch

from tests import cases, depth_grad_ref as dgr, depth_ref, error_ref, gpu_util, synth

pytestmark = pytest.mark.gpu

IDENTITY_MEASURED = ("worst tensor, both maps or one, plain and indexed alike: indexed 8.1e-8, odd_size 1.5e-8, opaque_big 5.3e-8, "
                     "needles_long 2.2e-8, huge_faint 1.2e-7, deep 0, one_pixel 0, one_tile (signed maps) 1.2e-8, long_run 0")
TRUTH_MEASURED = ("tiny 6.0e-7, indexed 4.6e-6 (one pair replayed; 7.3e-4 under the other decision of its one ambiguous pair), "
                  "odd_size 6.8e-6 (one pair replayed; 1.9e-3 against the float64 reference's own decision), cov_precomp 5.1e-6, "
                  "colors_precomp 6.1e-6")
SUM_MEASURED = "image + maps against image-only + maps-only: plain 1.2e-6, indexed 3.6e-7"

GRADS = ("dL_dmeans2D", "dL_dopacity", "dL_dmeans3D", "dL_dcov3D", "dL_dscales", "dL_drotations", "dL_dscale_factors")


def _maps(W, H, signed=False):
    return dgr.hashed_map(W, H, 1, signed).astype(np.float32), dgr.hashed_map(W, H, 2, signed).astype(np.float32)


def _backward(fw, dL_dout, gD=None, gA=None):
    """_C.rasterize_gaussians_backward(_indexed) on the buffers of forward `fw` (gpu_util.hip_backward with the two maps).
    dL_dout / gD / gA: numpy or None. -> {name: numpy}"""
    from c3dgs_amd import rasterizer
    dev = lambda x: None if x is None else torch.from_numpy(np.ascontiguousarray(x)).cuda()      # noqa: E731
    a = fw["args"]
    kw = dict(dL_ddepth=dev(gD), dL_dalpha=dev(gA))
    if fw["indexed"]:
        (bg, means3D, colors, opac, scales, sf, rot, smod, cov3D, view, proj, tfx, tfy, H, W, sh, deg, campos, shi, gi, pre, dbg, clamp) = a
        out = rasterizer._C.rasterize_gaussians_backward_indexed(
            bg, means3D, fw["radii"], colors, scales, sf, rot, smod, cov3D, view, proj, tfx, tfy, dev(dL_dout), sh, deg, campos,
            fw["geom"], fw["num_rendered"], fw["binning"], fw["img"], False, shi, gi, **kw)
        names = ("dL_dmeans2D", "dL_dcolors", "dL_dopacity", "dL_dmeans3D", "dL_dcov3D", "dL_dsh", "dL_dscales", "dL_dscale_factors",
                 "dL_drotations")
    else:
        (bg, means3D, colors, opac, scales, rot, smod, cov3D, view, proj, tfx, tfy, H, W, sh, deg, campos, pre, dbg, clamp) = a
        out = rasterizer._C.rasterize_gaussians_backward(
            bg, means3D, fw["radii"], colors, scales, rot, smod, cov3D, view, proj, tfx, tfy, dev(dL_dout), sh, deg, campos,
            fw["geom"], fw["num_rendered"], fw["binning"], fw["img"], False, **kw)
        names = ("dL_dmeans2D", "dL_dcolors", "dL_dopacity", "dL_dmeans3D", "dL_dcov3D", "dL_dsh", "dL_dscales", "dL_drotations")
    torch.cuda.synchronize()
    return {n: o.detach().cpu().numpy() for n, o in zip(names, out)}


def _lift(inp):
    """a non-indexed scene for the indexed rasterizer: identity indices, unit scale factors"""
    P = inp["means3D"].shape[0]
    ar = torch.arange(P, dtype=torch.int64)
    return dict(inp, sh_indices=ar.clone() if inp.get("shs") is not None else None,
                g_indices=ar.clone() if inp.get("scales") is not None else None,
                scale_factors=torch.ones(P, 1) if inp.get("scales") is not None else None)


def _colour_coded(inp, cam):
    """-> (the scene with colours (z, 1, 0) over a black background, fn(dL_dcolors) -> the z-term of dL_dmeans3D): z in fp32
    torch from means3D and the view matrix, element by element in xform4x3's order"""
    m = inp["means3D"].clone().requires_grad_()
    v = torch.from_numpy(np.asarray(cam["viewmatrix"], np.float32).reshape(4, 4))
    z = m[:, 0] * v[0, 2] + m[:, 1] * v[1, 2] + m[:, 2] * v[2, 2] + v[3, 2]
    col = torch.stack([z, torch.ones_like(z), torch.zeros_like(z)], 1)
    d = dict(inp, shs=None, sh_indices=None, colors_precomp=col.detach().contiguous(), bg=torch.zeros(3))

    def z_term(dL_dcolors):
        m.grad = None
        col.backward(torch.from_numpy(np.ascontiguousarray(dL_dcolors)), retain_graph=True)
        return m.grad.numpy().copy()
    return d, z_term


def _reference(fz, z_term, gD, gA, H, W):
    """the product backward of the colour-coded forward `fz` under the image gradient (gD, gA, 0), the z-term added"""
    zero = np.zeros((H, W), np.float32)
    dL = np.stack([zero if gD is None else gD, zero if gA is None else gA, zero])
    ref = gpu_util.hip_backward(fz, dL)
    ref = dict(ref, dL_dz=ref["dL_dcolors"][:, 0].copy())
    ref["dL_dmeans3D"] = ref["dL_dmeans3D"] + z_term(ref["dL_dcolors"])
    return ref


def _worst(got, ref, names, bar, label):
    worst = 0.0
    for k in names:
        if k not in ref or ref[k] is None or ref[k].size == 0:
            continue
        assert np.isfinite(got[k]).all(), k
        e = gpu_util.rel_inf(got[k], ref[k]) if np.abs(ref[k]).max() > 0 else float(np.abs(got[k]).max())
        print(label, k, "rel-inf %.3e" % e, "reference max %.3e" % float(np.abs(ref[k]).max()))
        worst = max(worst, e)
        assert e <= bar, (label, k, e)
    return worst


CASES = [(name, ix) for name in depth_ref.SCENES for ix in ((True,) if name == "indexed" else (False, True))]
# tests/error_ref.py's scene: a Gaussian over 17 x 17 tiles, i.e. a run of 289 slots (two trips of the fold's whole-wave path)
CASES += [("long_run", False), ("long_run", True)]


@pytest.mark.parametrize("name,as_indexed", CASES, ids=[f"{n}-{'indexed' if i else 'plain'}" for n, i in CASES])
def test_identity_with_the_colour_coded_product_backward(hip, name, as_indexed):
    inp, cam, indexed = error_ref.long_run_scene() if name == "long_run" else depth_ref.scene(name)
    if as_indexed and not indexed:
        inp = _lift(inp)
    W, H = cam["W"], cam["H"]
    gD, gA = _maps(W, H)
    fw = gpu_util.hip_forward(inp, cam, as_indexed)
    assert fw["num_rendered"] > 0
    inp_z, z_term = _colour_coded(inp, cam)
    fz = gpu_util.hip_forward(inp_z, cam, as_indexed)
    np.testing.assert_array_equal(gpu_util.unpack(fz)["n_contrib"], gpu_util.unpack(fw)["n_contrib"])     # the colours change no decision
    names = GRADS if as_indexed else tuple(g for g in GRADS if g != "dL_dscale_factors")
    zero_img = np.zeros((3, H, W), np.float32)
    worst = 0.0
    for label, d, a in (("both", gD, gA), ("depth only", gD, None), ("alpha only", None, gA)):
        ref = _reference(fz, z_term, d, a, H, W)
        got = _backward(fw, zero_img, d, a)
        assert np.abs(ref["dL_dopacity"]).max() > 0 and np.abs(ref["dL_dmeans2D"]).max() > 0 or name == "one_pixel"
        worst = max(worst, _worst(got, ref, names, 1e-4, f"identity {name} {label}:"))
        # the colour part of a map-only backward is exactly zero
        for k in ("dL_dcolors", "dL_dsh"):
            assert not got[k].any(), k
        if label == "both":
            # without an image gradient at all (NULL dL_dout_color: no colour blend launch) the values are the same: a zero image
            # gradient only adds exact zeros to the same sums (the codebook scatter-adds of the indexed path are float atomics
            # in no fixed order: tests/test_render_depth_gpu.py's bar for them)
            alone = _backward(fw, None, d, a)
            _worst(alone, got, names, 1e-5 if as_indexed else 0.0, f"identity {name} no image gradient:")
            if not as_indexed:                                  # no atomics on this path: bit for bit, run to run
                again = _backward(fw, zero_img, d, a)
                for k in names:
                    np.testing.assert_array_equal(got[k].view(np.uint32), again[k].view(np.uint32), err_msg=k)
    print(f"identity {name} {'indexed' if as_indexed else 'plain'}: worst rel-inf {worst:.3e}")


@functools.lru_cache(maxsize=None)
def _truth_case(name):
    """black_state + truth + candidates of tests/depth_grad_ref.py for a scene of depth_ref.SCENES or a case of tests/cases.py: once
    per process"""
    st, inp, cam, indexed = dgr.black_state(name)
    gD, gA, _ = dgr.truth(name)
    replayed, amb, cands = dgr.candidates(name)
    return st, inp, cam, indexed, gD, gA, (replayed, amb), cands


TRUTH_NAMES = {"dL_dmeans3D": "means3D", "dL_dmeans2D": "means2D", "dL_dopacity": "opacities", "dL_dscales": "scales",
               "dL_drotations": "rotations", "dL_dscale_factors": "scale_factors", "dL_dcov3D": "cov3D_precomp"}


@pytest.mark.parametrize("name", ["tiny", "indexed", "odd_size", "cov_precomp", "colors_precomp"])
def test_truth_float64_autograd(hip, name):
    st, inp, cam, indexed, gD, gA, amb, cands = _truth_case(name)
    W, H = cam["W"], cam["H"]
    fw = gpu_util.hip_forward(inp, cam, indexed)
    u = gpu_util.unpack(fw)
    differ = int((u["n_contrib"].astype(np.int64) != st.n_contrib.astype(np.int64)).sum())
    print(f"truth {name}: pixels where the HIP forward and the oracle disagree on n_contrib: {differ}")
    assert differ <= depth_ref.exemption_cap(W * H)
    got = _backward(fw, None, gD.astype(np.float32), gA.astype(np.float32))
    print(f"truth {name}: pairs (pixel, list position) decided by the fp32 formula against float64: {amb[0]}; fp32 alpha within "
          f"{dgr.EXP_BAND} of 1/255: {amb[1]}; admissible references: {len(cands)}")
    per_candidate = []
    for want in cands:
        ref = {k: want[v].reshape(got[k].shape) for k, v in TRUTH_NAMES.items() if v in want and k in got}
        assert "dL_dmeans3D" in ref and "dL_dopacity" in ref and ("dL_dcov3D" in ref) == (name == "cov_precomp")
        per_candidate.append((max(gpu_util.rel_inf(got[k], ref[k]) for k in ref), ref))
    print(f"truth {name}: worst rel-inf per admissible reference:", ["%.3e" % e for e, _ in per_candidate])
    worst, ref = min(per_candidate, key=lambda t: t[0])
    worst = _worst(got, ref, tuple(ref), 1e-4, f"truth {name}:")
    print(f"truth {name}: worst rel-inf {worst:.3e}")
    if name == "colors_precomp":
        assert not got["dL_dcolors"].any()                      # the maps do not depend on the colours
    if name in ("tiny", "cov_precomp", "colors_precomp"):       # no pair near the threshold: the float64 autograd itself
        assert amb == ([], []) and len(cands) == 1 and cands[0] is dgr.truth(name)[2]


# (W, H, focal) of the cases of tests/cases.py the truth tests use; their pose is make_case's default
CASE_CAMERA = {"tiny": (48, 32, 40.0), "indexed": (200, 136, 125.0), "odd_size": (203, 131, 125.0), "cov_precomp": (200, 136, 125.0),
               "colors_precomp": (200, 136, 125.0)}
LEAF_KEYS = ("means3D", "opacities", "shs", "colors_precomp", "scales", "scale_factors", "rotations", "cov3D_precomp")


@pytest.mark.parametrize("name", ["tiny", "indexed", "odd_size", "cov_precomp", "colors_precomp"])
def test_truth_through_the_autograd_modules(hip, orc, name):
    """param.grad end to end: the case through GaussianRasterizer / GaussianRasterizerIndexed with leaf tensors, settings with
    depth_grad=True and the loss (depth gD).sum() + (alpha gA).sum(), gD and gA different hashed maps; every leaf's .grad against
    the float64 reference of test_truth_float64_autograd at the same bar, 1e-4. A swap of the two maps between the autograd
    outputs and the library, or the loss of one, leaves that bar by orders of magnitude (asserted on the reference)."""
    st, inp, cam, indexed, gD, gA, amb, cands = _truth_case(name)
    W, H, focal = CASE_CAMERA[name]
    intr, ev = synth.camera(W, H, focal, extrinsic_vector=(0.05, -0.03, 0.02, 0.99, 0.1, -0.05, 0.2))
    same = orc.camera(intr.numpy(), ev.numpy())
    for k in ("viewmatrix", "projmatrix", "campos"):            # the case's own camera
        np.testing.assert_array_equal(np.asarray(same[k]), np.asarray(cam[k]))
    assert (same["W"], same["H"]) == (cam["W"], cam["H"]) and not np.array_equal(gD, gA)
    rs = hip.GaussianRasterizationSettings(intrinsic=intr.cuda(), extrinsic_vector=ev.cuda(), bg=inp["bg"].cuda(),
                                           scale_modifier=float(inp["scale_modifier"]), sh_degree=int(inp["degree"]), prefiltered=False,
                                           debug=False, clamp_color=bool(inp["clamp_color"]), depth_grad=True)
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
    image, radii, depth, alpha, median = rast(**kw)
    tD, tA = torch.from_numpy(gD.astype(np.float32)).cuda(), torch.from_numpy(gA.astype(np.float32)).cuda()
    ((depth * tD).sum() + (alpha * tA).sum()).backward()
    torch.cuda.synchronize()
    got = {k: v.grad.cpu().numpy() for k, v in leaves.items() if k not in ("shs", "colors_precomp")}
    got["means2D"] = means2D.grad.cpu().numpy()
    for k in ("shs", "colors_precomp"):                          # the maps do not depend on the colours
        if k in leaves:
            assert leaves[k].grad is None or not bool(leaves[k].grad.any()), k
    per_candidate = []
    for want in cands:
        ref = {k: want[k].reshape(got[k].shape) for k in got}
        per_candidate.append((max(gpu_util.rel_inf(got[k], ref[k]) for k in ref), ref))
    print(f"modules {name}: worst rel-inf per admissible reference:", ["%.3e" % e for e, _ in per_candidate])
    worst, ref = min(per_candidate, key=lambda t: t[0])
    assert set(ref) >= {"means3D", "means2D", "opacities"} and ("cov3D_precomp" in ref) == (name == "cov_precomp")
    worst = _worst(got, ref, tuple(ref), 1e-4, f"modules {name}:")
    print(f"modules {name}: worst rel-inf {worst:.3e}")
    # what a swap of the maps would give, in float64: far outside the bar, so the comparison above tells them apart
    swapped = dgr.restated(st, inp, gA, gD, fp32=bool(amb[0] or amb[1]))
    apart = dgr.rel_inf(swapped["opacities"], ref["opacities"].reshape(swapped["opacities"].shape))
    print(f"modules {name}: dL_dopacity with gD and gA swapped, rel-inf to the reference: {apart:.3e}")
    assert apart > 1e-2


# ---------------------------------------------------------------------------------------------------------------- Python layer
def _settings(hip, intr, ev, **kw):
    base = dict(intrinsic=intr.cuda(), extrinsic_vector=ev.cuda(), bg=torch.tensor((0.2, 0.4, 0.1), device="cuda"), scale_modifier=1.0,
                sh_degree=3, prefiltered=False, debug=False, clamp_color=True)
    return hip.GaussianRasterizationSettings(**base, **kw)


def _module_scene(indexed, P=1500, W=75, H=50, focal=60.0):
    ev_t = (0.05, -0.03, 0.02, 0.99, 0.1, -0.05, 0.2)
    intr, ev = synth.camera(W, H, focal, extrinsic_vector=ev_t)
    sc = synth.scene(P, W, H, focal, seed=17, scale_median=0.08)
    if indexed:
        sc = synth.index_scene(sc, shs_extra=32, gs_extra=32)
    return sc, intr, ev, W, H


def _run(hip, sc, intr, ev, indexed, loss, optimize_camera=False, **skw):
    names = ("means3D", "opacities", "shs", "scales", "rotations") + (("scale_factors",) if indexed else ())
    leaves = {k: sc[k].cuda().requires_grad_() for k in names}
    means2D = torch.zeros_like(leaves["means3D"], requires_grad=True)
    rs = _settings(hip, intr, ev, **skw)
    if indexed:
        rast = hip.GaussianRasterizerIndexed(rs, optimize_camera=optimize_camera)
        out = rast(means3D=leaves["means3D"], means2D=means2D, opacities=leaves["opacities"], sh_indices=sc["sh_indices"].cuda(),
                   g_indices=sc["g_indices"].cuda(), shs=leaves["shs"], scales=leaves["scales"],
                   scale_factors=leaves["scale_factors"], rotations=leaves["rotations"], extrinsic_vector=ev.cuda())
    else:
        rast = hip.GaussianRasterizer(rs, optimize_camera=optimize_camera)
        out = rast(means3D=leaves["means3D"], means2D=means2D, opacities=leaves["opacities"], shs=leaves["shs"],
                   scales=leaves["scales"], rotations=leaves["rotations"], extrinsic_vector=ev.cuda())
    loss(out).backward()
    torch.cuda.synchronize()
    g = {k: (torch.zeros_like(v) if v.grad is None else v.grad.clone()) for k, v in leaves.items()}
    g["means2D"] = torch.zeros_like(means2D) if means2D.grad is None else means2D.grad.clone()
    return out, g


def _same(a, b, indexed, k):
    """bit for bit; on the indexed path the codebook scatter-adds are float atomics, so the bar of tests/test_render_depth_gpu.py"""
    if torch.equal(a.view(torch.int32), b.view(torch.int32)):
        return True
    return indexed and torch.allclose(a, b, rtol=1e-5, atol=1e-6 * float(b.abs().max()))


@pytest.mark.parametrize("indexed", [False, True])
def test_opt_in_and_bits(hip, indexed):
    sc, intr, ev, W, H = _module_scene(indexed)
    gD, gA = (torch.from_numpy(m).cuda() for m in _maps(W, H))
    wimg = synth.grad_image(W, H).cuda()
    rs = _settings(hip, intr, ev, depth_grad=True)
    assert rs.depth_grad is True and rs.depth is False and "depth_grad" not in rs._fields and rs._fields[-1] == "depth"
    assert rs._replace(scale_modifier=2.0).depth_grad is True and rs._replace(depth_grad=False).depth_grad is False
    assert rs == rs._replace(depth_grad=False) and _settings(hip, intr, ev).depth_grad is False and len(rs) == 9

    image_loss = lambda o: (o[0] * wimg).sum()                                          # noqa: E731
    maps_loss = lambda o: (o[2] * gD).sum() + (o[3] * gA).sum()                         # noqa: E731
    plain, g_plain = _run(hip, sc, intr, ev, indexed, image_loss)
    fwd, g_depth_settings = _run(hip, sc, intr, ev, indexed, image_loss, depth=True)
    out, g_img = _run(hip, sc, intr, ev, indexed, image_loss, depth_grad=True)
    assert len(plain) == 2 and len(fwd) == 5 and len(out) == 5
    # the forward outputs are depth=True's, bit for bit; depth and alpha are differentiable, median and radii are not
    for a, b in zip(out, fwd):
        assert torch.equal(a.view(torch.int32), b.view(torch.int32)) if a.dtype == torch.float32 else torch.equal(a, b)
    assert out[2].requires_grad and out[3].requires_grad and not out[4].requires_grad and not out[1].requires_grad
    assert not fwd[2].requires_grad and not fwd[3].requires_grad
    # a loss on the image alone: the plain settings' gradients
    for k in g_plain:
        assert _same(g_img[k], g_plain[k], indexed, k), k
    # maps of zeros: the image-only values
    _, g_zero = _run(hip, sc, intr, ev, indexed, lambda o: image_loss(o) + (o[2] * 0).sum() + (o[3] * 0).sum(), depth_grad=True)
    for k in g_plain:
        assert torch.equal(g_zero[k], g_plain[k]) or _same(g_zero[k], g_plain[k], True, k), k
    # image + maps = image-only + maps-only
    _, g_maps = _run(hip, sc, intr, ev, indexed, maps_loss, depth_grad=True)
    _, g_both = _run(hip, sc, intr, ev, indexed, lambda o: image_loss(o) + maps_loss(o), depth_grad=True)
    worst = 0.0
    for k in g_plain:
        want = (g_img[k].double() + g_maps[k].double()).cpu().numpy()
        e = gpu_util.rel_inf(g_both[k].cpu().numpy(), want)
        print(f"image + maps against the sum, {'indexed' if indexed else 'plain'}, {k}: rel-inf {e:.3e}")
        worst = max(worst, e)
        assert e <= 1e-5, (k, e)
    assert float(g_maps["means3D"].abs().max()) > 0 and float(g_maps["opacities"].abs().max()) > 0
    assert not g_maps["shs"].any()                              # the maps do not depend on the colours
    print(f"image + maps against the sum, {'indexed' if indexed else 'plain'}: worst rel-inf {worst:.3e}")
    # two runs of the same backward: equal bits (non-indexed: no atomics anywhere)
    _, g_again = _run(hip, sc, intr, ev, indexed, lambda o: image_loss(o) + maps_loss(o), depth_grad=True)
    for k in g_both:
        assert _same(g_again[k], g_both[k], indexed, k), k


@pytest.mark.parametrize("indexed", [False, True])
def test_pose_gradient_with_depth_grad_is_refused(hip, indexed):
    sc, intr, ev, W, H = _module_scene(indexed, P=64)
    rs = _settings(hip, intr, ev, depth_grad=True)
    cls = hip.GaussianRasterizerIndexed if indexed else hip.GaussianRasterizer
    for oc in ((True, "exact") if indexed else ("exact",)):
        with pytest.raises(ValueError, match="depth_grad"):
            cls(rs, optimize_camera=oc)
        rast = cls(_settings(hip, intr, ev), optimize_camera=oc)
        rast.raster_settings = rs                               # swapped in behind the constructor: refused at the call
        with pytest.raises(ValueError, match="depth_grad"):
            _run_module(rast, sc, ev, indexed)
    cls(rs, optimize_camera=False)


def _run_module(rast, sc, ev, indexed):
    kw = dict(means3D=sc["means3D"].cuda(), means2D=torch.zeros(sc["means3D"].shape, device="cuda"), opacities=sc["opacities"].cuda(),
              shs=sc["shs"].cuda(), scales=sc["scales"].cuda(), rotations=sc["rotations"].cuda(), extrinsic_vector=ev.cuda())
    if indexed:
        kw.update(sh_indices=sc["sh_indices"].cuda(), g_indices=sc["g_indices"].cuda(), scale_factors=sc["scale_factors"].cuda())
    return rast(**kw)


@pytest.mark.parametrize("name", ["all_behind", "one_tile"])
def test_edges_nothing_visible_and_one_tile(hip, name):
    """all_behind: R == 0, every gradient an exact zero. one_tile (9 x 5 pixels): narrower than a wave's pixel block."""
    inp, cam, indexed = cases.make_case(name)
    W, H = cam["W"], cam["H"]
    gD, gA = _maps(W, H, signed=True)
    fw = gpu_util.hip_forward(inp, cam, indexed)
    got = _backward(fw, None, gD, gA)
    if name == "all_behind":
        assert fw["num_rendered"] == 0
        for k, v in got.items():
            assert not v.any(), k
        return
    inp_z, z_term = _colour_coded(inp, cam)
    fz = gpu_util.hip_forward(inp_z, cam, indexed)
    ref = _reference(fz, z_term, gD, gA, H, W)
    _worst(got, ref, tuple(g for g in GRADS if g != "dL_dscale_factors"), 1e-4, f"identity {name} signed maps:")


# ---------------------------------------------------------------------------------------------------------------- model and driver
class _Cam:
    def __init__(self, intrinsic, ev):
        self.intrinsic, self.extrinsic_vector = intrinsic.cuda(), ev.cuda()


@pytest.mark.parametrize("path", ["fused_indexed", "composed"])
def test_model_render_depth_grad(hip, path):
    from c3dgs_amd.model import GaussianModel, PipelineParams
    W, H, focal = 90, 60, 80.0
    sc = synth.scene(2000, W=W, H=H, focal=focal, seed=23, scale_median=0.06)
    m = GaussianModel(3, quantization=True, device="cuda")
    if path == "fused_indexed":
        m.set_tensors(**synth.raw_params(synth.index_scene(sc, seed=24, shs_extra=32, gs_extra=32)))
    else:
        op = sc["opacities"].clamp(1e-6, 1 - 1e-6)
        m.set_tensors(xyz=sc["means3D"], features_dc=sc["shs"][:, :1], features_rest=sc["shs"][:, 1:],
                      scaling=sc["scales"] / sc["scales"].norm(dim=1, keepdim=True), rotation=sc["rotations"],
                      opacity=torch.log(op / (1 - op)), scaling_factor=torch.log(sc["scales"].norm(dim=1, keepdim=True)))
    intr, ev = synth.camera(W, H, focal)
    cam, bg = _Cam(intr, ev), torch.zeros(3, device="cuda")
    plain = m.render(cam, PipelineParams(), bg, return_depth=True)
    assert not plain["depth"].requires_grad and not plain["alpha"].requires_grad           # return_depth alone stays as it is
    out = m.render(cam, PipelineParams(), bg, depth_grad=True)
    assert set(out) == set(plain)
    for k in ("depth", "alpha", "median_depth"):
        assert torch.equal(out[k].view(torch.int32), plain[k].view(torch.int32)), k
    assert out["depth"].requires_grad and out["alpha"].requires_grad and not out["median_depth"].requires_grad
    (out["depth"].sum() + out["alpha"].sum()).backward()
    torch.cuda.synchronize()
    for p in m.parameters():
        assert p.grad is not None and bool(torch.isfinite(p.grad).all())
    assert float(m._xyz.grad.abs().max()) > 0 and float(m._opacity.grad.abs().max()) > 0
    pose = _Cam(intr, ev)
    pose.extrinsic_vector.requires_grad_()
    with pytest.raises(ValueError, match="depth_grad"):
        m.render(pose, PipelineParams(), bg, depth_grad=True)


def test_train_with_depth_and_alpha_terms(hip, tmp_path):
    """A few dozen iterations on the toy scene with the teacher's own maps as targets: finite throughout. The same call with both
    lambdas at 0 is today's run: the same final parameters as the call without the options, bit for bit."""
    from c3dgs_amd import pipeline
    from c3dgs_amd.model import PipelineParams
    from tests import train_scene
    W, H, focal = 160, 112, 150.0

    def make(k, targets):
        (tmp_path / str(k)).mkdir()
        student, cams, extent = train_scene.make(tmp_path / str(k), "cuda", W=W, H=H, focal=focal)
        if targets:
            teacher, _ = train_scene.teacher_model(4000, W, H, focal, "cuda")
            bg = torch.zeros(3, device="cuda")
            with torch.no_grad():
                for cam in cams:
                    t = teacher.render(cam, PipelineParams(), bg, return_depth=True)
                    cam.alpha_target, cam.depth_target = t["alpha"].clone(), (t["depth"] / t["alpha"].clamp(min=1e-6)) * (t["alpha"] > 0.5)

        class Scene:
            gaussians = student
            cameras_extent = extent

            def getTrainCameras(self):
                return cams
        return student, Scene()

    opt = lambda: train_scene.schedule(32, densify=False)       # noqa: E731
    finals = []
    for k, kw in enumerate((dict(), dict(lambda_depth=0.0, lambda_alpha=0.0))):
        student, scene = make(k, targets=True)                  # the targets are attached, and ignored
        torch.manual_seed(0)
        assert pipeline.train(scene, None, opt(), PipelineParams(), camera_stride=1, **kw) == 32
        finals.append([p.detach().clone() for p in student.parameters()])
    for a, b in zip(*finals):
        assert torch.equal(a.view(torch.int32), b.view(torch.int32))

    student, scene = make(2, targets=True)
    losses = []
    torch.manual_seed(0)
    n = pipeline.train(scene, None, opt(), PipelineParams(), camera_stride=1, lambda_depth=0.1, lambda_alpha=0.1,
                       log=lambda e, i: losses.append(i["ema_loss"]))
    assert n == 32 and len(losses) == 4 and all(np.isfinite(v) for v in losses)
    for p in student.parameters():
        assert bool(torch.isfinite(p).all())
    moved = any(not torch.equal(a, b) for a, b in zip(finals[0], [p.detach() for p in student.parameters()]))
    assert moved                                                # the two terms reached the parameters
    with pytest.raises(ValueError):
        pipeline.train(scene, None, opt(), PipelineParams(), camera_stride=1, lambda_depth=-1.0)
