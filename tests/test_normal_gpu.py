"""-m gpu: the normal maps (csrc/normals.hip, csrc/render_normal.hip, csrc/render_maps_backward.hip;
GaussianRasterizationSettings(normal=), c3dgs_amd.normals, GaussianModel.render(normal=), pipeline.train(lambda_normal=)).

  forward    on tests/depth_ref.py's seven scenes: the per-Gaussian normals against the float64 definition (16 x 2^-24 per
             component; a sign-ambiguous Gaussian, |cos| < 1e-5, hands its sign to the reference), the map against the float64 sum
             over the oracle's blended pairs, the skip decisions replayed from the fp32 formula and a pair whose fp32 alpha is within
             4e-6 of 1/255 free to go either way, as tests/depth_grad_ref.py does. Pixels where the HIP forward and the oracle
             disagree on n_contrib are skipped, at most depth_ref.exemption_cap of them; on the rest, per component,
             |got - ref| <= 2e-5 + 1e-4 |ref|. Two calls: the same bits. Without the oracle: the product's own colour forward with
             colors_precomp = n, a black background and no clamp, to the same bar.
  truth      every leaf gradient against the float64 closed form of tests/normal_ref.py (tied to autograd by
             tests/test_normal_ref_cpu.py), rel-inf <= 1e-4, under gN alone, gD + gA + gN, and gD + gA + gL + gN raw and ndc.
  one recurrence   a map whose incoming gradient is all zero changes no gradient: the replay's four instances agree as floats.
  opt-in     normal=False is today's call, bit for bit; with it the other outputs keep their bits; a loss that ignores the map gives
             the other settings' backward, bits and stage counts; a four-map backward replays the blend once and folds once more.
  refusals, edges, the stencil, model and drivers.

Measured on an MI355X (from this file's prints): see MEASURED below."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from tests import depth_grad_ref as dgr, depth_ref, distortion_ref as dr, gpu_util, normal_ref as nr, synth
from tests.test_depth_grad_gpu import TRUTH_NAMES, _Cam, _lift, _maps, _module_scene, _run, _run_module, _same, _settings, _worst
from tests.test_distortion_gpu import _best, _bits_equal, _model_for
from tests.test_pose_grad_gpu import _stage_counts

pytestmark = pytest.mark.gpu

MEASURED = ("gaussian_normals: largest component error 3.0 x 2^-24 on every scene (the fp32 restatement's figure, bar 16); normal map, largest "
            "error over its bar: indexed 7.7e-3, odd_size 9.4e-3, opaque_big 7.9e-3, needles_long 0.32, huge_faint 1.2e-2, deep 6.3e-3, "
            "one_pixel 1.0e-3, and bit-equal to the colour forward with colors_precomp = n on all seven; worst leaf rel-inf, gN / gD+gA+gN / "
            "all four raw / all four ndc: tiny 2.1e-6 / 1.4e-6 / 1.2e-6 / 7.4e-7, indexed 1.6e-5 / 4.8e-6 / 8.2e-6 / 4.8e-6, odd_size 2.5e-5 / "
            "4.9e-6 / 4.8e-6 / 4.9e-6, colors_precomp 1.7e-5 / 6.7e-6 / 8.8e-6 / 6.4e-6 (bar 1e-4); four maps against three + one at most "
            "6.4e-7; depth_to_normal: restatement's worst 0.409 x 2^-24 max(fx, fy), k = 1.635, GPU's worst 0.407; backward: restatement "
            "1.46e-6, bar 5.8e-6, GPU's worst 1.46e-6; train on the toy scene, 35 iterations, lambda_normal = 1 from iteration 7: "
            "normal-consistency error of the held view 0.582 against 1.056 without the term (a run that also frees scales and rotations "
            "against one that does not), 0.581 with filter_3d next to it; render(normal=True) with a 3D filter: every map bit-equal to "
            "the module-level call, dL/d_rotation within 8.7e-8 (fused indexed) and 0 (composed)")


def _dev(x):
    return None if x is None else torch.from_numpy(np.ascontiguousarray(x, dtype=np.float32)).cuda()


def _geometry(fw):
    """(means3D, scales, rotations, g_indices | None, viewmatrix) of a gpu_util forward"""
    a = fw["args"]
    if fw["indexed"]:
        return a[1], a[4], a[6], a[19], a[9]
    return a[1], a[4], a[5], None, a[8]


def _normals(fw):
    from c3dgs_amd import rasterizer
    return rasterizer._C.gaussian_normals(*_geometry(fw))


def _render(fw, normals):
    from c3dgs_amd import rasterizer
    return rasterizer._C.render_normal(int(fw["radii"].numel()), fw["W"], fw["H"], fw["num_rendered"], fw["geom"], fw["binning"],
                                       fw["img"], normals)


def _backward(fw, dL_dout, gN=None, normals=None, gD=None, gA=None, gL=None, moment=None, mode=None):
    """_C.rasterize_gaussians_backward(_indexed) on the buffers of forward `fw` with the maps' gradients. numpy or None in (`moment`,
    `normals`: device tensors). -> {name: numpy}"""
    from c3dgs_amd import rasterizer
    a = fw["args"]
    kw = dict(dL_ddepth=_dev(gD), dL_dalpha=_dev(gA))
    if gL is not None:
        kw.update(dL_ddistortion=_dev(gL), moment=moment, near_far=mode)
    if gN is not None:
        kw.update(dL_dnormal=_dev(gN), normals=normals)
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
def check_gaussian_normals(label, inp, viewmatrix, buf):
    """the [P, 4] buffer against the float64 definition -> the reference, with the signs of sign-ambiguous Gaussians adopted"""
    ref = nr.gaussian_normals(inp, viewmatrix)
    sg, amb = nr.adopt_ambiguous_signs(ref, buf[:, 3])
    assert amb.size <= 1, amb
    if amb.size:
        ref = nr.gaussian_normals(inp, viewmatrix, sigma=sg)
    worst32, bar = nr.gaussian_normals_bar()
    err = float(np.abs(buf[:, :3].astype(np.float64) - ref["n"]).max()) if buf.size else 0.0
    print(f"{label}: gaussian_normals largest component error {err:.3e} = {err / nr.U:.2f} x 2^-24 (bar {bar / nr.U:.1f} x 2^-24; the fp32 "
          f"restatement's worst {worst32 / nr.U:.2f}); sign-ambiguous Gaussians {amb.tolist()}")
    assert np.isfinite(buf).all() and err <= bar
    np.testing.assert_array_equal(buf[:, 3], ref["sigma"] * (ref["m"] + 1))
    return ref


def check_forward(label, u, st, got, n64):
    """the map's bar on a scene (its forward unpacked: `u`, its oracle state: `st`); shared with tests/test_normal_poison_gpu.py"""
    W, H = st.W, st.H
    refs = nr.normal_map_candidates(st, W, H, n64)
    skip = (u["n_contrib"].astype(np.int64) != st.n_contrib.astype(np.int64)).reshape(H, W)
    print(f"{label}: pixels skipped (HIP forward and oracle disagree on n_contrib): {int(skip.sum())}; admissible references: {len(refs)}")
    assert skip.sum() <= depth_ref.exemption_cap(W * H)
    assert np.isfinite(got).all()
    over = np.min([np.abs(got - r["normal"]) / (2e-5 + 1e-4 * np.abs(r["normal"])) for r in refs], axis=0)
    over[:, skip] = 0.0
    print(f"{label}: normal map largest error over its bar {float(over.max()):.3e}, largest value {float(np.abs(refs[0]['normal']).max()):.4f}")
    assert (over <= 1.0).all(), (int((over > 1.0).sum()), float(over.max()))
    first = np.abs(got - refs[0]["normal"]) / (2e-5 + 1e-4 * np.abs(refs[0]["normal"]))
    first[:, skip] = 0.0
    needs_flip = set(np.nonzero((first > 1.0).any(0).reshape(-1))[0].tolist())
    assert needs_flip <= set(refs[0]["ambiguous_pixels"]), (sorted(needs_flip), refs[0]["ambiguous_pixels"])
    return float(over.max())


@pytest.mark.parametrize("name", depth_ref.SCENES)
def test_forward_against_the_float64_sum(hip, orc, name):
    inp, cam, indexed = depth_ref.scene(name)
    st = depth_ref.oracle_state(name)
    fw = gpu_util.hip_forward(inp, cam, indexed)
    u = gpu_util.unpack(fw)
    nb = _normals(fw)
    assert tuple(nb.shape) == (st.P, 4) and torch.equal(nb.view(torch.int32), _normals(fw).view(torch.int32))
    ref = check_gaussian_normals(name, inp, cam["viewmatrix"], nb.cpu().numpy())
    N = _render(fw, nb)
    assert tuple(N.shape) == (3, cam["H"], cam["W"]) and torch.equal(N.view(torch.int32), _render(fw, nb).view(torch.int32))
    got = N.cpu().numpy().astype(np.float64)
    check_forward(name, u, st, got, ref["n"])
    assert np.abs(got).max() > 0.05
    # without the oracle: the product's own colour forward with the normals as colours
    col = gpu_util.hip_forward(dict(inp, shs=None, sh_indices=None,
                                    colors_precomp=nb[:, :3].contiguous().cpu(), bg=torch.zeros(3), clamp_color=False), cam, indexed)
    np.testing.assert_array_equal(gpu_util.unpack(col)["n_contrib"], u["n_contrib"])
    c = col["color"].cpu().numpy().astype(np.float64)
    e = np.abs(got - c) / (2e-5 + 1e-4 * np.abs(c))
    print(f"{name}: against the colour forward with colors_precomp = n: largest error over the bar {float(e.max()):.3e}; bit-equal: "
          f"{bool(torch.equal(N.view(torch.int32), col['color'].view(torch.int32)))}")
    assert (e <= 1.0).all()
    # valid behind the backward as well, with the same bits
    gpu_util.hip_backward(fw, synth.grad_image(cam["W"], cam["H"]).numpy())
    assert torch.equal(N.view(torch.int32), _render(fw, nb).view(torch.int32))


def test_gaussian_normals_through_identity_indices(hip):
    """a plain scene lifted to the indexed entry: the same buffer, bit for bit; and a codebook with repeated rows"""
    inp, cam, _ = depth_ref.scene("odd_size")
    plain = _normals(gpu_util.hip_forward(inp, cam, False))
    lifted = _normals(gpu_util.hip_forward(_lift(inp), cam, True))
    assert torch.equal(plain.view(torch.int32), lifted.view(torch.int32))
    from c3dgs_amd import rasterizer
    P = inp["means3D"].shape[0]
    gi = (torch.arange(P) % 7).cuda()
    view = torch.from_numpy(np.asarray(cam["viewmatrix"], np.float32)).cuda()
    buf = rasterizer._C.gaussian_normals(inp["means3D"].cuda(), inp["scales"][:7].cuda().contiguous(), inp["rotations"][:7].cuda().contiguous(),
                                         gi, view)
    check_gaussian_normals("odd_size, 7-row codebook", dict(inp, scales=inp["scales"][:7], rotations=inp["rotations"][:7],
                                                             g_indices=gi.cpu()), cam["viewmatrix"], buf.cpu().numpy())


# ---------------------------------------------------------------------------------------------------------------- backward truth
TRUTH_CASES = ["tiny", "indexed", "odd_size", "colors_precomp"]
COMBOS = [("gN", "raw"), ("gD+gA+gN", "raw"), ("gD+gA+gL+gN", "raw"), ("gD+gA+gL+gN", "ndc")]


def _truth_inputs(name, combo, mode_name, fw):
    st, inp, cam, indexed = dgr.black_state(name)
    W, H = cam["W"], cam["H"]
    nb = _normals(fw)
    ref = check_gaussian_normals(f"truth {name}", inp, cam["viewmatrix"], nb.cpu().numpy())
    gN = nr.gn_map(W, H)
    gD, gA = (dgr.hashed_map(W, H, 1), dgr.hashed_map(W, H, 2)) if "gD" in combo else (None, None)
    gL = dr.gl_map(W, H) if "gL" in combo else None
    replayed, amb, cands = nr.candidates(name, combo, mode_name, sigma=ref["sigma"])
    return nb, gN, gD, gA, gL, (replayed, amb), cands


@pytest.mark.parametrize("combo,mode_name", COMBOS, ids=[f"{c}-{m}" for c, m in COMBOS])
@pytest.mark.parametrize("name", TRUTH_CASES)
def test_truth_float64(hip, name, combo, mode_name):
    st, inp, cam, indexed = dgr.black_state(name)
    W, H = cam["W"], cam["H"]
    mode = dr.MODES[mode_name]
    fw = gpu_util.hip_forward(inp, cam, indexed)
    u = gpu_util.unpack(fw)
    differ = int((u["n_contrib"].astype(np.int64) != st.n_contrib.astype(np.int64)).sum())
    nb, gN, gD, gA, gL, (replayed, amb), cands = _truth_inputs(name, combo, mode_name, fw)
    print(f"truth {name}: pixels where the HIP forward and the oracle disagree on n_contrib: {differ}; replayed {replayed}; ambiguous {amb}")
    assert differ <= depth_ref.exemption_cap(W * H)
    moment = None
    if gL is not None:
        from c3dgs_amd import rasterizer
        moment = rasterizer._C.render_distortion(st.P, W, H, fw["num_rendered"], fw["geom"], fw["binning"], fw["img"], mode)[1]
    got = _backward(fw, None, gN, nb, gD, gA, gL, moment, mode)
    label = f"truth {name} {combo} {mode_name}"
    ref = _best(got, cands, TRUTH_NAMES, label)
    assert {"dL_dmeans3D", "dL_dopacity", "dL_dscales", "dL_drotations"} <= set(ref)
    worst = _worst(got, ref, tuple(ref), 1e-4, label + ":")
    print(f"{label}: worst rel-inf {worst:.3e}")
    assert not got["dL_dcolors"].any() and not got["dL_dsh"].any()              # the maps do not depend on the colours
    if combo == "gN":
        assert np.abs(got["dL_drotations"]).max() > 0 and np.abs(got["dL_dscales"]).max() > 0 and np.abs(got["dL_dmeans3D"]).max() > 0
        # the share of the rotations that comes through n, not through w: the reference's chain of dL/dn, well above the bar
        q, _, gi = nr._rows(inp)
        ng = nr.gaussian_normals(inp, cam["viewmatrix"])
        chain = nr.normal_chain(q, ng["m"], ng["sigma"], cam["viewmatrix"], cands[0]["n"])
        if gi is not None:
            rows = np.zeros_like(ref["dL_drotations"], dtype=np.float64)
            np.add.at(rows, gi, chain)
            chain = rows
        share = float(np.abs(chain).max() / np.abs(ref["dL_drotations"]).max())
        print(f"{label}: largest element of the chain through n over the largest of dL_drotations: {share:.3e}")
        assert share > 1e-2


@pytest.mark.parametrize("name", ["tiny", "indexed"])
def test_truth_through_the_autograd_modules(hip, orc, name):
    """param.grad end to end: settings with normal=True and distortion=NDC, the loss over all four maps"""
    from tests.test_depth_grad_gpu import CASE_CAMERA, LEAF_KEYS
    st, inp, cam, indexed = dgr.black_state(name)
    W, H, focal = CASE_CAMERA[name]
    intr, ev = synth.camera(W, H, focal, extrinsic_vector=(0.05, -0.03, 0.02, 0.99, 0.1, -0.05, 0.2))
    rs = hip.GaussianRasterizationSettings(intrinsic=intr.cuda(), extrinsic_vector=ev.cuda(), bg=inp["bg"].cuda(),
                                           scale_modifier=float(inp["scale_modifier"]), sh_degree=int(inp["degree"]), prefiltered=False,
                                           debug=False, clamp_color=bool(inp["clamp_color"]), distortion=dr.NDC, normal=True)
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
    image, radii, depth, alpha, median, distortion, normal = rast(**kw)
    assert normal.requires_grad and distortion.requires_grad and depth.requires_grad and not median.requires_grad
    assert tuple(normal.shape) == (3, H, W)
    tD, tA, tL, tN = (_dev(m) for m in (dgr.hashed_map(W, H, 1), dgr.hashed_map(W, H, 2), dr.gl_map(W, H), nr.gn_map(W, H)))
    ((depth * tD).sum() + (alpha * tA).sum() + (distortion * tL).sum() + (normal * tN).sum()).backward()
    torch.cuda.synchronize()
    got = {k: v.grad.cpu().numpy() for k, v in leaves.items() if k not in ("shs", "colors_precomp")}
    got["means2D"] = means2D.grad.cpu().numpy()
    _, _, cands = nr.candidates(name, "gD+gA+gL+gN", "ndc")
    ref = _best(got, cands, {k: k for k in got}, f"modules {name}")
    worst = _worst(got, ref, tuple(ref), 1e-4, f"modules {name}:")
    print(f"modules {name}: worst rel-inf {worst:.3e}")


# ---------------------------------------------------------------------------------------------------------------- one recurrence
@pytest.mark.parametrize("name", ["deep", "odd_size"])
def test_a_map_with_a_zero_gradient_adds_exact_zeros(hip, name):
    """The four instances of render_maps_backward_kernel are one recurrence. With contraction off a map whose incoming gradient is
    all zero contributes exact zeros to every sum, so the instance that carries the map returns what the instance without it
    returns: equal as floats (-0 == +0), every tensor, through the C entry. An all-zero dL_dnormal (with the real normals) against
    no dL_dnormal, with and without the distortion gradient (ndc); an all-zero dL_ddistortion (with the forward's real moment,
    ndc) against none, with and without the normal gradient. dL_drotations receives only the exact zeros of the fold. `deep` walks
    three and more batches of 256 per tile, where the double-buffered hit bits are reused."""
    from c3dgs_amd import rasterizer
    inp, cam, indexed = depth_ref.scene(name)
    W, H = cam["W"], cam["H"]
    fw = gpu_util.hip_forward(inp, cam, indexed)
    nb = _normals(fw)
    moment = rasterizer._C.render_distortion(int(fw["radii"].numel()), W, H, fw["num_rendered"], fw["geom"], fw["binning"], fw["img"],
                                             dr.NDC)[1]
    assert float(moment.abs().max()) > 0 and float(nb[:, :3].abs().max()) > 0
    gD, gA, gL, gN = dgr.hashed_map(W, H, 1), dgr.hashed_map(W, H, 2), dr.gl_map(W, H), nr.gn_map(W, H)
    zN, zL = np.zeros((3, H, W), np.float32), np.zeros((H, W), np.float32)
    dist = dict(moment=moment, mode=dr.NDC)
    pairs = {
        "zero gN beside gD+gA": (dict(), dict(gN=zN, normals=nb)),
        "zero gN beside gD+gA+gL": (dict(gL=gL, **dist), dict(gL=gL, gN=zN, normals=nb, **dist)),
        "zero gL beside gD+gA": (dict(), dict(gL=zL, **dist)),
        "zero gL beside gD+gA+gN": (dict(gN=gN, normals=nb), dict(gN=gN, normals=nb, gL=zL, **dist)),
    }
    for label, (without, with_zero) in pairs.items():
        want = _backward(fw, None, gD=gD, gA=gA, **without)
        got = _backward(fw, None, gD=gD, gA=gA, **with_zero)
        assert np.abs(want["dL_dmeans3D"]).max() > 0 and np.abs(want["dL_dopacity"]).max() > 0
        for k in want:
            assert np.isfinite(got[k]).all(), (label, k)
            differ = np.nonzero(got[k].reshape(-1) != want[k].reshape(-1))[0]
            print(f"{name}, {label}: {k}: {differ.size} of {got[k].size} elements differ")
            assert np.array_equal(got[k], want[k]), (label, k, differ[:8].tolist())


# ---------------------------------------------------------------------------------------------------------------- opt-in and bits
@pytest.mark.parametrize("indexed", [False, True])
def test_opt_in_and_bits(hip, indexed):
    sc, intr, ev, W, H = _module_scene(indexed)
    gD, gA = (torch.from_numpy(m).cuda() for m in _maps(W, H))
    gL, gN = _dev(dr.gl_map(W, H)), _dev(nr.gn_map(W, H))
    wimg = synth.grad_image(W, H).cuda()
    rs = _settings(hip, intr, ev, normal=True)
    assert rs.normal is True and rs.depth_grad is False and "normal" not in rs._fields and len(rs) == 9
    assert rs._replace(scale_modifier=2.0).normal is True and rs._replace(normal=False).normal is False
    assert _settings(hip, intr, ev).normal is False

    image_loss = lambda o: (o[0] * wimg).sum()                                          # noqa: E731
    maps_loss = lambda o: (o[2] * gD).sum() + (o[3] * gA).sum()                         # noqa: E731
    # normal=False: today's outputs and gradients, bit for bit
    plain, g_plain = _run(hip, sc, intr, ev, indexed, image_loss)
    off, g_off = _run(hip, sc, intr, ev, indexed, image_loss, normal=False)
    assert len(plain) == len(off) == 2
    for a, b in zip(off, plain):
        assert _bits_equal(a, b)
    for k in g_plain:
        assert _same(g_off[k], g_plain[k], indexed, k), k
    # with it: the image, depth, alpha and median bits are depth_grad's; the map is the last output and differentiable
    ref_out, _ = _run(hip, sc, intr, ev, indexed, image_loss, depth_grad=True)
    (out, g_img), counts_img = _stage_counts(hip, lambda: _run(hip, sc, intr, ev, indexed, image_loss, normal=True))
    assert len(ref_out) == 5 and len(out) == 6 and tuple(out[-1].shape) == (3, H, W)
    for a, b in zip(out[:5], ref_out):
        assert _bits_equal(a, b)
    assert out[-1].requires_grad and out[2].requires_grad and out[3].requires_grad and not out[4].requires_grad
    assert counts_img.get("gaussian_normals") == 1 and counts_img.get("render_normal") == 1
    # a loss on the image alone: the plain settings' gradients and launches in the backward
    for k in g_plain:
        assert _same(g_img[k], g_plain[k], indexed, k), k
    for stage in ("render_normal_backward", "normal_backward_fold", "render_depth_backward", "depth_backward_fold"):
        assert stage not in counts_img, stage
    # a loss on depth and alpha alone: depth_grad's backward, bits and stage counts
    (_, g_ref_maps), counts_ref = _stage_counts(hip, lambda: _run(hip, sc, intr, ev, indexed, maps_loss, depth_grad=True))
    (_, g_maps), counts_maps = _stage_counts(hip, lambda: _run(hip, sc, intr, ev, indexed, maps_loss, normal=True))
    for k in g_ref_maps:
        assert _same(g_maps[k], g_ref_maps[k], indexed, k), k
    extra_fw = {"gaussian_normals": 1, "render_normal": 1}
    assert counts_maps == {**counts_ref, **extra_fw}, (counts_maps, counts_ref)
    assert counts_maps.get("render_depth_backward") == 1 and "render_normal_backward" not in counts_maps
    # with distortion next to it: the distortion map keeps its place in front of the normal map and its bits, and a loss that
    # ignores the normal map is the distortion settings' backward
    dist_loss = lambda o, at: maps_loss(o) + (o[at] * gL).sum()                        # noqa: E731
    (d_out, g_ref3), counts_ref3 = _stage_counts(hip, lambda: _run(hip, sc, intr, ev, indexed, lambda o: dist_loss(o, -1),
                                                                   distortion=dr.NDC))
    (b_out, g3), counts3 = _stage_counts(hip, lambda: _run(hip, sc, intr, ev, indexed, lambda o: dist_loss(o, -2), distortion=dr.NDC,
                                                           normal=True))
    assert len(b_out) == 7 and _bits_equal(b_out[-2], d_out[-1]) and _bits_equal(b_out[-1], out[-1])
    for k in g_ref3:
        assert _same(g3[k], g_ref3[k], indexed, k), k
    assert counts3 == {**counts_ref3, **extra_fw}, (counts3, counts_ref3)
    # all four maps: ONE replay in the backward, in the place of the other two, and one extra fold
    four_loss = lambda o: dist_loss(o, -2) + (o[-1] * gN).sum()                       # noqa: E731
    (_, g4), counts4 = _stage_counts(hip, lambda: _run(hip, sc, intr, ev, indexed, four_loss, distortion=dr.NDC, normal=True))
    assert counts4.get("render_normal_backward") == 1 and counts4.get("normal_backward_fold") == 1
    assert counts4.get("depth_backward_fold") == 1
    assert "render_depth_backward" not in counts4 and "render_distortion_backward" not in counts4 and "render_backward" not in counts4
    want4 = dict(counts3, render_normal_backward=1, normal_backward_fold=1)
    want4.pop("render_distortion_backward")
    assert counts4 == want4, (counts4, want4)
    # four maps = three maps + the normal map alone, to the re-association of fp32 addends
    (_, gn), _ = _stage_counts(hip, lambda: _run(hip, sc, intr, ev, indexed, lambda o: (o[-1] * gN).sum(), normal=True))
    worst = 0.0
    for k in g4:
        want = (g3[k].double() + gn[k].double()).cpu().numpy()
        e = gpu_util.rel_inf(g4[k].cpu().numpy(), want)
        print(f"four maps against three + one, {'indexed' if indexed else 'plain'}, {k}: rel-inf {e:.3e}")
        worst = max(worst, e)
        assert e <= 1e-5, (k, e)
    assert float(gn["rotations"].abs().max()) > 0 and not gn["shs"].any()
    # two runs of the same backward: equal bits (non-indexed: no atomics anywhere)
    _, g_again = _run(hip, sc, intr, ev, indexed, four_loss, distortion=dr.NDC, normal=True)
    for k in g4:
        assert _same(g_again[k], g4[k], indexed, k), k


# ---------------------------------------------------------------------------------------------------------------- refusals
@pytest.mark.parametrize("indexed", [False, True])
def test_refusals(hip, indexed):
    sc, intr, ev, W, H = _module_scene(indexed, P=64)
    rs = _settings(hip, intr, ev, normal=True)
    cls = hip.GaussianRasterizerIndexed if indexed else hip.GaussianRasterizer
    for oc in ((True, "exact") if indexed else ("exact",)):
        with pytest.raises(ValueError, match="normal"):
            cls(rs, optimize_camera=oc)
        rast = cls(_settings(hip, intr, ev), optimize_camera=oc)
        rast.raster_settings = rs                               # swapped in behind the constructor: refused at the call
        with pytest.raises(ValueError, match="normal"):
            _run_module(rast, sc, ev, indexed)
    rast = cls(rs, optimize_camera=False)
    kw = dict(means3D=sc["means3D"].cuda(), means2D=torch.zeros(sc["means3D"].shape, device="cuda"), opacities=sc["opacities"].cuda(),
              shs=sc["shs"].cuda(), cov3D_precomp=torch.eye(3).reshape(-1)[[0, 1, 2, 4, 5, 8]].repeat(64, 1).cuda() * 0.01,
              extrinsic_vector=ev.cuda())
    if indexed:
        kw.update(sh_indices=sc["sh_indices"].cuda(), g_indices=sc["g_indices"].cuda())
    with pytest.raises(ValueError, match="covariance"):
        rast(**kw)


def test_model_refuses_a_pose_that_requires_grad(hip):
    from c3dgs_amd.model import PipelineParams
    W, H, focal = 90, 60, 80.0
    m = _model_for("composed", synth.scene(500, W=W, H=H, focal=focal, seed=23, scale_median=0.06))
    intr, ev = synth.camera(W, H, focal)
    pose = _Cam(intr, ev)
    pose.extrinsic_vector.requires_grad_()
    with pytest.raises(ValueError, match="normal"):
        m.render(pose, PipelineParams(), torch.zeros(3, device="cuda"), normal=True)
    with pytest.raises(ValueError, match="covariance"):
        m.render(_Cam(intr, ev), PipelineParams(), torch.zeros(3, device="cuda"), normal=True, cov3d=m.get_covariance().detach())


# ---------------------------------------------------------------------------------------------------------------- edges
def test_edges(hip, orc):
    from c3dgs_amd import normals, rasterizer
    # P == 0: zeros, no launch
    empty = torch.empty(0, dtype=torch.uint8, device="cuda")
    nb0 = torch.empty((0, 4), device="cuda")
    N, counts = _stage_counts(hip, lambda: rasterizer._C.render_normal(0, 40, 24, 0, empty, empty, empty, nb0))
    assert tuple(N.shape) == (3, 24, 40) and not N.any() and "render_normal" not in counts
    z3 = torch.empty((0, 3), device="cuda")
    assert tuple(rasterizer._C.gaussian_normals(z3, z3, torch.empty((0, 4), device="cuda"), None, torch.eye(4).cuda()).shape) == (0, 4)
    # one_pixel: one Gaussian, one pixel
    inp, cam, indexed = depth_ref.scene("one_pixel")
    fw = gpu_util.hip_forward(inp, cam, indexed)
    nb = _normals(fw)
    got = _backward(fw, None, np.ones((3, 1, 1)), nb)
    for k, v in got.items():
        assert np.isfinite(v).all(), k
    assert np.abs(got["dL_drotations"]).max() > 0
    # a 2 x 2 image: depth_to_normal is all zero, and so is its gradient
    intr2, _ = synth.camera(2, 2, 2.0)
    z = torch.full((2, 2), 3.0, device="cuda", requires_grad=True)
    n2 = normals.depth_to_normal(z, intr2)
    assert tuple(n2.shape) == (3, 2, 2) and not n2.any()
    n2.sum().backward()
    assert not z.grad.any()
    # degenerate quaternions. The zero quaternion's rotation matrix is the identity as preprocess builds it (1 - 2 (..) = 1), so
    # its normal is an axis like any other; (0, 0, 0.5, 0.5) makes column 0 vanish exactly: the zero normal, finite gradients
    sc = synth.scene(6, 48, 32, 40.0, seed=2, scale_median=0.3)
    sc["scales"] = torch.tensor([[0.1, 0.3, 0.4]]).repeat(6, 1)          # m = 0 everywhere
    sc["rotations"][0] = torch.zeros(4)
    sc["rotations"][1] = torch.tensor([0.0, 0.0, 0.5, 0.5])
    intr, ev = synth.camera(48, 32, 40.0)
    cam = orc.camera(intr.numpy(), ev.numpy())
    inp = dict(bg=torch.zeros(3), means3D=sc["means3D"], opacities=sc["opacities"], shs=sc["shs"], scales=sc["scales"],
               rotations=sc["rotations"], degree=3, clamp_color=True)
    fw = gpu_util.hip_forward(inp, cam, False)
    nb = _normals(fw)
    buf = nb.cpu().numpy()
    check_gaussian_normals("degenerate quaternions", inp, cam["viewmatrix"], buf)
    assert not buf[1, :3].any() and abs(float(np.sqrt((buf[0, :3].astype(np.float64) ** 2).sum())) - 1.0) < 1e-3
    N = _render(fw, nb)
    assert bool(torch.isfinite(N).all())
    got = _backward(fw, None, nr.gn_map(48, 32), nb)
    for k, v in got.items():
        assert np.isfinite(v).all(), k


_TIMEOUT_CHILD = r"""
import numpy as np, torch
from tests import gpu_util, synth
from oracle import oracle as orc
from c3dgs_amd import _lib, rasterizer as rz
assert _lib.LIB_PATH.endswith("libc3dgs_hip_spin1.so"), _lib.LIB_PATH
W, H = 640, 360
intr, ev = synth.camera(W, H, 400.0)
cam = orc.camera(intr.numpy(), ev.numpy())
sc = synth.scene(400_000, W, H, 400.0, seed=3, scale_median=0.02)
inp = dict(bg=torch.zeros(3), means3D=sc["means3D"], opacities=sc["opacities"], shs=sc["shs"], scales=sc["scales"],
           rotations=sc["rotations"], degree=3, clamp_color=True)
fw = gpu_util.hip_forward(inp, cam, False)           # look-backs give up: the forward's image is NaN
torch.cuda.synchronize()
assert torch.isnan(fw["color"]).all(), "a forward whose sort timed out must return a NaN image"
a = fw["args"]
nb = rz._C.gaussian_normals(a[1], a[4], a[5], None, a[8])
assert bool(torch.isfinite(nb).all())                # per Gaussian: no list is read
N = rz._C.render_normal(int(fw["radii"].numel()), W, H, fw["num_rendered"], fw["geom"], fw["binning"], fw["img"], nb)
torch.cuda.synchronize()
assert N.shape == (3, H, W) and torch.isnan(N).all(), "the normal map of a forward whose sort timed out must be NaN"
(bg, means3D, colors, opac, scales, rot, smod, cov3D, view, proj, tfx, tfy, H_, W_, sh, deg, campos, pre, dbg, clamp) = a
# the maps' replay walks nothing, and the folds would write NaN into the rows of the LISTED Gaussians; but a timed-out forward leaves
# tile_used_c = 0, so no pass flags a slot and nothing is listed (with or without an image gradient): that branch of the folds is
# not reachable from a real time-out. What must hold is that no row holds finite garbage: every rotation and mean row is NaN or
# exactly zero
out = rz._C.rasterize_gaussians_backward(bg, means3D, fw["radii"], colors, scales, rot, smod, cov3D, view, proj, tfx, tfy, None, sh, deg,
                                         campos, fw["geom"], fw["num_rendered"], fw["binning"], fw["img"], False,
                                         dL_dnormal=torch.ones((3, H, W), device="cuda"), normals=nb)
torch.cuda.synchronize()
for rows in (out[7], out[3]):
    assert bool((torch.isnan(rows) | (rows == 0)).all()), "a row of a timed-out backward must be NaN or zero"
print("rotation rows that are NaN:", int(torch.isnan(out[7]).any(1).sum()))
print("NAN_NORMALS")
"""


def test_sort_timeout_gives_nan(hip):
    """With the `spin1` variant of the library, started the way tests/test_render_depth_gpu.py::test_sort_timeout_gives_nan_maps starts
    its child: a NaN normal map; the backward leaves no finite garbage (its rows are NaN or zero)"""
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    lib = os.path.join(root, "c3dgs_amd", "libc3dgs_hip_spin1.so")
    if not os.path.exists(lib):
        from c3dgs_amd import build
        build.build_variant("spin1")
    r = subprocess.run([sys.executable, "-c", _TIMEOUT_CHILD], cwd=root, env=dict(os.environ, C3DGS_LIB_PATH=lib),
                       capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    assert "NAN_NORMALS" in r.stdout, r.stdout


# ---------------------------------------------------------------------------------------------------------------- the stencil
def _intrinsic_for(W, H, tfx, tfy):
    """an intrinsic whose field of view gives these tangents (the reference's layout: [0, 0] = FoVx, [1, 1] = FoVy, [0, 2] = W, [1, 2] = H)"""
    intr = torch.zeros(3, 3)
    intr[0, 0], intr[1, 1], intr[0, 2], intr[1, 2] = 2 * np.arctan(tfx), 2 * np.arctan(tfy), W, H
    return intr


def test_depth_to_normal_against_float64(hip):
    from c3dgs_amd import normals
    from c3dgs_amd.rasterizer import _intrinsic_scalars
    (wf, k), (wb, bar_b) = nr.stencil_bars()["forward"], nr.stencil_bars()["backward"]
    worst_f = worst_b = 0.0
    for label, z64, tfx, tfy in nr.stencil_inputs():
        H, W = z64.shape
        intr = _intrinsic_for(W, H, tfx, tfy)
        tfx32, tfy32 = _intrinsic_scalars(intr)[0][:2]            # the tangents the library receives
        z = torch.from_numpy(z64.astype(np.float32)).cuda().requires_grad_()
        n = normals.depth_to_normal(z, intr)
        again = normals.depth_to_normal(z, intr)
        assert torch.equal(n.view(torch.int32), again.view(torch.int32))
        ref = nr.depth_to_normal(z64, tfx32, tfy32)
        unit = nr.U * max(W / (2 * tfx32), H / (2 * tfy32))
        e = float(np.abs(n.detach().cpu().numpy().astype(np.float64) - ref).max()) / unit
        g = nr.gn_map(W, H)
        (n * _dev(g)).sum().backward()
        eb = dgr.rel_inf(z.grad.cpu().numpy(), nr.depth_to_normal_backward(z64, g, tfx32, tfy32))
        print(f"stencil {label}: forward error {e:.3f} x 2^-24 max(fx, fy) (bar k = {k:.3f}, restatement {wf:.3f}); backward rel-inf "
              f"{eb:.3e} (bar {bar_b:.3e}, restatement {wb:.3e})")
        worst_f, worst_b = max(worst_f, e), max(worst_b, eb)
        assert e <= k and eb <= bar_b, (label, e, eb)
        nn = n.detach().cpu().numpy()
        assert not nn[:, 0].any() and not nn[:, -1].any() and not nn[:, :, 0].any() and not nn[:, :, -1].any()
    print(f"stencil: worst forward {worst_f:.3f} x 2^-24 max(fx, fy), worst backward rel-inf {worst_b:.3e}")


def test_normal_consistency_composes(hip):
    """the term on a rasterizer's maps against its float64 restatement on the same maps; gradients reach all three maps"""
    from c3dgs_amd import normals
    sc, intr, ev, W, H = _module_scene(False)
    out, _ = _run(hip, sc, intr, ev, False, lambda o: o[0].sum() * 0, normal=True)
    maps = [o.detach().clone().requires_grad_() for o in (out[2], out[3], out[-1])]
    loss = normals.normal_consistency(*maps, intr)
    loss.backward()
    from c3dgs_amd.rasterizer import _intrinsic_scalars
    tfx, tfy = _intrinsic_scalars(intr)[0][:2]
    m64 = [o.detach().cpu().double().requires_grad_() for o in maps]
    want = nr.normal_consistency(*m64, tfx, tfy)
    want.backward()
    loss, want = loss.detach(), want.detach()
    print(f"normal_consistency: {float(loss):.6f} against float64 {float(want):.6f}; gradient to the normal map rel-inf "
          f"{gpu_util.rel_inf(maps[2].grad.cpu().numpy(), m64[2].grad.numpy()):.3e}")
    # a mean over the pixels of products of two vectors of length <= 1: the fp32 stencil on a rendered depth / alpha is the only
    # source of error that is not a rounding of the result, and where alpha is next to nothing its z is noise in both precisions
    assert abs(float(loss) - float(want)) <= 1e-3
    assert 0.0 < float(loss) < 2.0
    for t in maps:
        assert t.grad is not None and bool(torch.isfinite(t.grad).all())


# ---------------------------------------------------------------------------------------------------------------- model and drivers
def _module_level_call(hip, m, cam, bg, filtered=False, **skw):
    """The rasterizer MODULE on the model's own activated tensors, gathered to the visible rows as render() gathers them. `filtered`:
    the model has a 3D filter; the module then blends filter3d.apply's covariance and opacity, with the model's scales and rotations
    beside the covariance as the normals' axes."""
    from c3dgs_amd.model import ColorMode
    indexed = m.color_index_mode == ColorMode.ALL_INDEXED and m.is_gaussian_indexed
    rs = hip.GaussianRasterizationSettings(intrinsic=cam.intrinsic, extrinsic_vector=cam.extrinsic_vector, bg=bg, scale_modifier=1.0,
                                           sh_degree=m.active_sh_degree, prefiltered=False, debug=False, clamp_color=True, **skw)
    rast = (hip.GaussianRasterizerIndexed if indexed else hip.GaussianRasterizer)(rs)
    means3D, opacity = m.get_xyz, m.get_opacity
    screen = torch.zeros_like(means3D, requires_grad=True)
    rows = rast.markVisible(means3D, extrinsic_vector=cam.extrinsic_vector).nonzero(as_tuple=False).squeeze(1)
    pick = lambda t: t.index_select(0, rows)                                            # noqa: E731
    if indexed:
        scales, rotations, factors = m.get_scaling_normalized, m._rotation_post_activation, m.get_scaling_factor
        cov = None
        if filtered:
            from c3dgs_amd import filter3d
            cov, opacity = filter3d.apply(opacity, scales, rotations, m.filter_3D, 1.0, scale_factors=factors, g_indices=m._gaussian_indices)
        return rast(means3D=pick(means3D), means2D=pick(screen), shs=m._get_features_raw, sh_indices=pick(m._feature_indices),
                    g_indices=pick(m._gaussian_indices), opacities=pick(opacity), scales=scales,
                    scale_factors=None if filtered else pick(factors), rotations=rotations,
                    cov3D_precomp=pick(cov) if filtered else None, extrinsic_vector=cam.extrinsic_vector)
    scales, rotations = m.get_scaling, m.get_rotation
    cov = None
    if filtered:
        from c3dgs_amd import filter3d
        cov, opacity = filter3d.apply(opacity, scales, rotations, m.filter_3D, 1.0)
    return rast(means3D=pick(means3D), means2D=pick(screen), shs=pick(m.get_features), opacities=pick(opacity),
                scales=pick(scales), rotations=pick(rotations), cov3D_precomp=pick(cov) if filtered else None,
                extrinsic_vector=cam.extrinsic_vector)


@pytest.mark.parametrize("path,antialiasing,filtered", [("fused_indexed", False, False), ("composed", False, False),
                                                        ("composed", True, False), ("fused_indexed", False, True),
                                                        ("composed", False, True)],
                         ids=["fused_indexed", "composed", "composed-antialiased", "fused_indexed-filtered", "composed-filtered"])
def test_model_render_normal(hip, path, antialiasing, filtered):
    """GaussianModel.render(normal=True, distortion=) against the module-level call on the model's own activated tensors: the same
    bits in every map; gradients reach the rotations. `filtered`: with a 3D filter, where the rasterizer blends the filtered
    covariance and the normals come from the model's own (unfiltered) axes: the normal map's per-Gaussian normals are those of the
    unfiltered model"""
    from c3dgs_amd.model import PipelineParams
    W, H, focal = 90, 60, 80.0
    sc = synth.scene(2000, W=W, H=H, focal=focal, seed=23, scale_median=0.06)
    m, twin = (_model_for(path, sc) for _ in range(2))
    intr, ev = synth.camera(W, H, focal)
    cam, bg = _Cam(intr, ev), torch.zeros(3, device="cuda")
    if filtered:
        for model in (m, twin):
            assert bool(model.compute_3D_filter([cam]).any()) and float(model.filter_3D.max()) > 0
    out = m.render(cam, PipelineParams(), bg, normal=True, distortion=dr.NDC, antialiasing=antialiasing)
    ref = _module_level_call(hip, twin, cam, bg, filtered=filtered, normal=True, distortion=dr.NDC, antialiasing=antialiasing)
    assert tuple(out["normal"].shape) == (3, H, W) and out["normal"].requires_grad
    for key, r in (("depth", ref[2]), ("alpha", ref[3]), ("distortion", ref[-2]), ("normal", ref[-1])):
        assert torch.equal(out[key].view(torch.int32), r.view(torch.int32)), key
    from c3dgs_amd import normals
    normals.normal_consistency(out["depth"], out["alpha"], out["normal"], cam.intrinsic).backward()
    torch.cuda.synchronize()
    for p in m.parameters():
        assert p.grad is None or bool(torch.isfinite(p.grad).all())
    assert float(m._rotation.grad.abs().max()) > 0 and float(m._xyz.grad.abs().max()) > 0
    if filtered:
        # the gradient of a loss on the normal map alone reaches the model's rotations through the axes beside the covariance: the
        # same values as through the module-level call (its rotations are the twin's activated ones, so compare at the parameter)
        tN = _dev(nr.gn_map(W, H))
        grads = []
        for model, normal_map in ((m, None), (twin, ref[-1])):
            model._rotation.grad = None
            if normal_map is None:
                normal_map = model.render(cam, PipelineParams(), bg, normal=True)["normal"]
            (normal_map * tN).sum().backward()
            grads.append(model._rotation.grad.detach().cpu().numpy().copy())
        e = gpu_util.rel_inf(grads[0], grads[1])
        print(f"model {path} filtered: dL/d_rotation under a loss on the normal map, render() against the module-level call: {e:.3e}")
        assert np.abs(grads[1]).max() > 0 and e <= 1e-4


def test_finetune_with_the_normal_term(hip, tmp_path):
    """finetune(lambda_normal=0) is today's loop, stage for stage and bit for bit; with a weight the term is there from
    `normal_from_iter` on; with lambda_dist next to it the backward still replays the blend once per view"""
    import random
    from c3dgs_amd import pipeline
    from c3dgs_amd.model import PipelineParams
    from tests import train_scene

    def run(k, with_filter=False, **kw):
        (tmp_path / str(k)).mkdir()
        student, cams, _ = train_scene.make(tmp_path / str(k), "cuda", W=96, H=64, focal=90.0, views=4)
        if with_filter:
            student.compute_3D_filter(cams)

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
    p1, c1, _ = run(1, lambda_normal=0.0, normal_from_iter=2)
    assert c1 == c0 and "render_normal" not in c0 and "gaussian_normals" not in c0, (c1, c0)
    for a, b in zip(p0, p1):
        assert torch.equal(a.view(torch.int32), b.view(torch.int32))
    p2, c2, scene = run(2, lambda_normal=0.5, normal_from_iter=2, lambda_dist=1.0, dist_near_far=dr.NDC, dist_from_iter=2)
    assert c2.get("render_normal") == 4 and c2.get("render_normal_backward") == 4 and c2.get("normal_backward_fold") == 4
    assert c2.get("depth_to_normal") == 4 and c2.get("depth_to_normal_backward") == 4
    assert "render_depth_backward" not in c2 and "render_distortion_backward" not in c2
    assert all(bool(torch.isfinite(p).all()) for p in p2) and any(not torch.equal(a, b) for a, b in zip(p0, p2))
    with pytest.raises(ValueError):
        pipeline.finetune(scene, pipeline._Dataset(), pipeline.OptimizationParams(), pipeline.CompressionParams(finetune_iterations=2),
                          PipelineParams(), lambda_normal=-1.0)
    # on a model with a 3D filter: the same launches for the term, on top of the filtered loop's
    p3, c3, _ = run(3, with_filter=True)
    p4, c4, _ = run(4, with_filter=True, lambda_normal=0.5, normal_from_iter=2)
    for stage in ("render_normal", "render_normal_backward", "normal_backward_fold", "depth_to_normal", "depth_to_normal_backward"):
        assert c4.get(stage) == 4 and stage not in c3, (stage, c4.get(stage))
    assert all(bool(torch.isfinite(p).all()) for p in p4) and any(not torch.equal(a, b) for a, b in zip(p3, p4))


def test_train_with_the_normal_term(hip, tmp_path):
    """A few epochs on the toy scene of the distortion driver test, same seed: lambda_normal = 0 is the default loop (stage counts
    and final parameters); with the term the run is finite and the normal-consistency error of a held view is printed next to the
    plain run's and asserted lower."""
    from c3dgs_amd import normals, pipeline
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
            o = student.render(cam, PipelineParams(), bg, normal=True)
            return float(normals.normal_consistency(o["depth"], o["alpha"], o["normal"], cam.intrinsic))

    finals, counts, errs = [], [], []
    for k, kw in enumerate((dict(), dict(lambda_normal=0.0, normal_from_iter=3), dict(lambda_normal=1.0, normal_from_iter=7))):
        student, scene, held_cam = make(k)
        torch.manual_seed(0)
        losses = []
        n, c = _stage_counts(hip, lambda: pipeline.train(scene, None, opt(), PipelineParams(), camera_stride=1,
                                                         log=lambda e, i: losses.append(i["ema_loss"]), **kw))
        assert n == 35 and len(losses) == 5 and all(np.isfinite(v) for v in losses)
        finals.append([p.detach().clone() for p in student.parameters()])
        counts.append(c)
        errs.append(held(student, held_cam))
        for p in student.parameters():
            assert bool(torch.isfinite(p).all())
    assert counts[1] == counts[0], (counts[1], counts[0])
    assert "render_normal" not in counts[0] and "render_normal_backward" not in counts[0]
    for a, b in zip(finals[0], finals[1]):
        assert torch.equal(a.view(torch.int32), b.view(torch.int32))
    assert counts[2].get("render_normal") == 35 - 7 and counts[2].get("render_normal_backward") == 35 - 7
    assert "render_depth_backward" not in counts[2]
    print(f"normal-consistency error of the held view: lambda_normal=0 {errs[0]:.6e}, lambda_normal=1 {errs[2]:.6e}")
    assert errs[2] < errs[0]
    # with the 3D filter next to the term: the filtered covariance is blended, the normals come from the unfiltered axes
    student, scene, held_cam = make(3)
    torch.manual_seed(0)
    n, c = _stage_counts(hip, lambda: pipeline.train(scene, None, opt(), PipelineParams(), camera_stride=1, lambda_normal=1.0,
                                                     normal_from_iter=7, filter_3d=True, filter_3d_interval=10))
    assert n == 35 and c.get("render_normal") == 35 - 7 and c.get("render_normal_backward") == 35 - 7
    for p in student.parameters():
        assert bool(torch.isfinite(p).all())
    print(f"normal-consistency error of the held view, lambda_normal=1 with the 3D filter: {held(student, held_cam):.6e}")
    with pytest.raises(ValueError):
        pipeline.train(scene, None, opt(), PipelineParams(), camera_stride=1, lambda_normal=-1.0)
