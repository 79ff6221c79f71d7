"""-m gpu: antialiased rasterization (csrc/aa_opacity.hip; GaussianRasterizationSettings(antialiasing=True), _C.aa_opacity,
_C.aa_opacity_backward, GaussianModel.render(antialiasing=), PipelineParams(antialiasing=)).

  rho          _C.aa_opacity against tests/aa_ref.py in float64 on the same fp32 inputs, every case: per row at most
               max(1e-6, 4 x the float32 restatement's deviation of that case) (aa_ref.f32_deviation: reference against
               reference; the kernel may round and associate differently from torch over roughly 40 operations, hence the 4).
               Every rho finite, exactly 1 behind the near plane, exactly sqrt(0.000025f) at the floor, o' = o rho bit for bit.
  forward      GaussianRasterizer(antialiasing=True) = the plain rasterizer fed _C.aa_opacity's o', bit for bit: image, radii, the
               depth / alpha / median maps, the contribution rows and the error scores; both rasterizers. Radii also equal the
               plain render's with the raw opacities.
  backward     _C.aa_opacity_backward alone on preset outputs (hashed g' in dL_dopacity, hashed non-zero values elsewhere: the
               kernel adds, it does not overwrite) against the float64 autograd of sum o rho g' through aa_ref, added to the
               presets: per tensor rel-inf (max |x - ref| / max |ref|) at most max(1e-5, 4 x the float32 restatement's deviation
               for that case and tensor). Rows with radii == 0 untouched, bit for bit. Every output pointer NULL in turn.
  composition  param.grad through the modules with antialiasing=True against the plain modules fed
               o (rho_ref + (rho_kernel - rho_ref).detach()), rho_ref = aa_ref in float64 on the device tensors: the forward's
               bits and blend decisions are the same and autograd supplies the chain through rho. rel-inf 1e-4 per tensor.
  model, refusals, the unchanged default.

Measured on an MI355X (from this file's prints): see RHO_MEASURED, BACKWARD_MEASURED, COMPOSITION_MEASURED below."""
import numpy as np
import pytest
import torch

from tests import aa_ref, gpu_util, synth

pytestmark = pytest.mark.gpu

RHO_MEASURED = ("worst row |rho - rho64| (float32 restatement of the same case): floor 1.0e-6 (1.0e-6), needles 2.4e-4 (2.4e-4: D0 cancels), "
                "clamped 7.3e-7 (7.3e-7), behind 9.3e-7 (9.3e-7), indexed 5.2e-7 (5.5e-7), indexed_scale_mod 5.4e-7 (5.4e-7), "
                "cov_precomp 9.2e-7 (9.8e-7)")
BACKWARD_MEASURED = ("worst tensor other than dL_dopacity, over the NULL patterns: floor 5.8e-8, needles 5.8e-8, clamped 4.4e-8, behind 6.3e-8, "
                     "indexed 2.8e-7, indexed_scale_mod 4.0e-7 (the atomically added codebook rows, worst of two runs; dL_dscale_factors 8.5e-8), "
                     "cov_precomp 6.6e-8; dL_dopacity = rho g' "
                     "carries the fp32 rho: 3.2e-7 .. 8.0e-7, needles 2.0e-4 (float32 restatement 2.1e-4)")
COMPOSITION_MEASURED = ("worst tensor: floor 4.6e-8, needles 4.5e-8, clamped 4.5e-8, indexed 4.0e-7, indexed_scale_mod 3.8e-7, cov_precomp "
                        "4.0e-8, indexed + depth_grad 2.9e-7 (indexed: worst of two runs, atomic adds). With the chain through rho in fp32 (before it went to double) needles "
                        "stood at 2.7e-3 on scales and 3.3e-4 on rotations")

EV = (0.05, -0.03, 0.02, 0.99, 0.1, -0.05, 0.2)       # cases.make_case's pose; every aa case is 200 x 136 at focal 125
W, H, FOCAL = 200, 136, 125.0
GRAD_OF = {"dL_dopacity": "opacities", "dL_dmeans3D": "means3D", "dL_dscales": "scales", "dL_drotations": "rotations",
           "dL_dscale_factors": "scale_factors"}


def _dev(x, dtype=None):
    if x is None:
        return None
    t = torch.as_tensor(np.ascontiguousarray(x)) if isinstance(x, np.ndarray) else x
    return t.to(device="cuda", dtype=dtype if dtype is not None else t.dtype).contiguous()


def _proj_inputs(c):
    """the positional arguments of _C.aa_opacity behind (means3D, opacities) and in front of the gradient tensors"""
    inp, cam = c["inp"], c["cam"]
    return (_dev(inp["scales"]), _dev(inp["rotations"]), _dev(inp["scale_factors"]), _dev(inp["g_indices"]),
            _dev(inp["cov3D_precomp"]), float(inp["scale_modifier"]), _dev(np.asarray(cam["viewmatrix"], np.float32)),
            cam["tan_fovx"], cam["tan_fovy"], cam["H"], cam["W"])


def _kernel_rho(hip, c):
    from c3dgs_amd import rasterizer
    inp = c["inp"]
    o, rho = rasterizer._C.aa_opacity(_dev(inp["means3D"]), _dev(inp["opacities"]), *_proj_inputs(c))
    torch.cuda.synchronize()
    return o, rho


# ---------------------------------------------------------------------------------------------------------------- 1. rho
@pytest.mark.parametrize("name", aa_ref.AA_CASES)
def test_rho_and_compensated_opacity(hip, name):
    c = aa_ref.aa_case(name)
    t, inp = c["t"], c["inp"]
    o_k, rho_k = _kernel_rho(hip, c)
    assert o_k.shape == inp["opacities"].shape and rho_k.shape == (inp["means3D"].shape[0],)
    o_k, rho_k = o_k.cpu().numpy().reshape(-1), rho_k.cpu().numpy()
    assert np.isfinite(rho_k).all()
    dev = aa_ref.f32_deviation(name)["rho"]
    bar = max(1e-6, 4 * dev)
    err = np.abs(rho_k.astype(np.float64) - t["rho"])
    print(f"rho {name}: worst row {err.max():.3e}, on visible rows {err[c['radii'] > 0].max():.3e}; float32 restatement {dev:.3e}, bar {bar:.3e}")
    assert err.max() <= bar, (name, float(err.max()), bar)
    # behind the near plane: exactly 1
    assert (rho_k[t["behind"]] == 1.0).all()
    # at the floor: exactly sqrt(0.000025f). Rows whose float64 r lies within 1e-3 of the floor may round to either side in fp32
    # (continuous there: they are held by the bar above)
    floor = t["floor"] & (t["r"] < aa_ref.R_FLOOR * (1 - 1e-3))
    print(f"rho {name}: floor rows {int(t['floor'].sum())}, of them clear of the threshold {int(floor.sum())}")
    assert (rho_k[floor] == aa_ref.RHO_FLOOR32).all()
    assert (rho_k >= aa_ref.RHO_FLOOR32).all() and (rho_k <= 1.0).all()
    if name == "floor":
        assert int(floor.sum()) >= 10
    if name == "behind":
        assert int(t["behind"].sum()) >= 10
    # o' = o rho, one fp32 multiplication
    want = inp["opacities"].numpy().reshape(-1) * rho_k
    np.testing.assert_array_equal(o_k.view(np.uint32), want.view(np.uint32))
    # without the optional output: the same o'
    from c3dgs_amd import rasterizer
    o2, none = rasterizer._C.aa_opacity(_dev(inp["means3D"]), _dev(inp["opacities"]), *_proj_inputs(c), rho=False)
    assert none is None and torch.equal(o2.cpu().reshape(-1), torch.from_numpy(o_k))


# ---------------------------------------------------------------------------------------------------------------- 2. forward
def _settings(hip, inp, **kw):
    intr, ev = synth.camera(W, H, FOCAL, extrinsic_vector=EV)
    rs = hip.GaussianRasterizationSettings(intrinsic=intr.cuda(), extrinsic_vector=ev.cuda(), bg=inp["bg"].cuda(),
                                           scale_modifier=float(inp["scale_modifier"]), sh_degree=int(inp["degree"]), prefiltered=False,
                                           debug=False, clamp_color=bool(inp["clamp_color"]), **kw)
    return rs, ev.cuda()


LEAF_KEYS = ("means3D", "opacities", "shs", "scales", "scale_factors", "rotations", "cov3D_precomp")


def _module_call(hip, c, rs, ev, leaves, means2D=None, opacities=None):
    inp = c["inp"]
    kw = dict(means3D=leaves["means3D"], means2D=means2D if means2D is not None else torch.zeros_like(leaves["means3D"]),
              opacities=leaves["opacities"] if opacities is None else opacities, shs=leaves.get("shs"), scales=leaves.get("scales"),
              rotations=leaves.get("rotations"), cov3D_precomp=leaves.get("cov3D_precomp"), extrinsic_vector=ev)
    if c["indexed"]:
        kw.update(sh_indices=inp["sh_indices"].cuda(), g_indices=inp["g_indices"].cuda(), scale_factors=leaves.get("scale_factors"))
        return hip.GaussianRasterizerIndexed(rs)(**kw)
    return hip.GaussianRasterizer(rs)(**kw)


def _same_camera(orc, c):
    intr, ev = synth.camera(W, H, FOCAL, extrinsic_vector=EV)
    same = orc.camera(intr.numpy(), ev.numpy())
    for k in ("viewmatrix", "projmatrix", "campos"):
        np.testing.assert_array_equal(np.asarray(same[k]), np.asarray(c["cam"][k]))
    assert (same["W"], same["H"]) == (c["cam"]["W"], c["cam"]["H"]) == (W, H)


@pytest.mark.parametrize("name", ["floor", "indexed_scale_mod", "cov_precomp"])
def test_forward_is_the_plain_rasterizer_on_the_compensated_opacity(hip, orc, name):
    c = aa_ref.aa_case(name)
    _same_camera(orc, c)
    inp = c["inp"]
    gt = synth.grad_image(W, H, seed=5).abs().clamp(0, 1).cuda().contiguous()
    extra = dict(depth=True, contrib=True, error_target=gt)
    leaves = {k: inp[k].cuda() for k in LEAF_KEYS if inp.get(k) is not None}
    with torch.no_grad():
        rs_aa, ev = _settings(hip, inp, antialiasing=True, **extra)
        rs, _ = _settings(hip, inp, **extra)
        assert rs_aa.antialiasing is True and rs.antialiasing is False
        got = _module_call(hip, c, rs_aa, ev, leaves)
        o_k, _ = _kernel_rho(hip, c)
        want = _module_call(hip, c, rs, ev, leaves, opacities=o_k)
        raw = _module_call(hip, c, rs, ev, leaves)
    torch.cuda.synchronize()
    names = ("image", "radii", "depth", "alpha", "median", "contrib_sum", "contrib_max", "contrib_hits", "error_sum")
    assert len(got) == len(want) == len(names)
    for k, a, b in zip(names, got, want):
        assert a.dtype == b.dtype and a.shape == b.shape, k
        assert torch.equal(a.view(torch.int32), b.view(torch.int32)) if a.dtype == torch.float32 else torch.equal(a, b), k
    assert torch.equal(got[1], raw[1])                                  # radii do not depend on the opacity
    np.testing.assert_array_equal(got[1].cpu().numpy(), c["radii"])     # ... and are the oracle's
    assert not torch.equal(got[0], raw[0])                              # the compensation is visible
    assert float(got[3].sum()) < float(raw[3].sum())                    # and only ever takes opacity away


# ---------------------------------------------------------------------------------------------------------------- 3. backward kernel
def _presets(c, term, salt0):
    """hashed, non-zero starting values of every output, scaled to the size of what the kernel adds"""
    inp = c["inp"]
    P = inp["means3D"].shape[0]
    shapes = dict(dL_dmeans3D=(P, 3), dL_dcov3D=(P, 6))
    if inp.get("scales") is not None:
        shapes.update(dL_dscales=tuple(inp["scales"].shape), dL_drotations=tuple(inp["rotations"].shape))
    if inp.get("g_indices") is not None:
        shapes["dL_dscale_factors"] = (P, 1)
    out = {}
    for salt, (k, shp) in enumerate(sorted(shapes.items())):
        ref = term[_term_key(c, k)]
        scale = 0.5 * max(float(np.abs(ref).max()), 1e-30)
        out[k] = (aa_ref.hashed(int(np.prod(shp)), salt0 + salt) * scale).astype(np.float32).reshape(shp)
    return out


def _term_key(c, k):
    if k == "dL_dcov3D":
        return "cov3D_precomp" if c["inp"].get("cov3D_precomp") is not None else "cov3D"
    return GRAD_OF[k]


@pytest.mark.parametrize("name", aa_ref.AA_CASES)
def test_backward_kernel_alone(hip, name):
    from c3dgs_amd import rasterizer
    c = aa_ref.aa_case(name)
    inp, cam = c["inp"], c["cam"]
    P = inp["means3D"].shape[0]
    fw = gpu_util.hip_forward(inp, cam, c["indexed"])
    radii = fw["radii"]
    vis = radii.cpu().numpy() > 0
    np.testing.assert_array_equal(radii.cpu().numpy(), c["radii"])
    gp = aa_ref.hashed(P, 11).astype(np.float32)                                    # the rasterizer's dL/do', hashed
    rho64, term = aa_ref.vjp(inp, cam, gp.astype(np.float64), torch.float64, rows=vis)
    dev = aa_ref.f32_deviation(name)
    presets = _presets(c, term, 20)
    cov_form = inp.get("cov3D_precomp") is not None
    optional = [k for k in presets if not (cov_form and k == "dL_dcov3D")]
    worst = {}
    for absent in [None] + optional:                                                # every optional output NULL in turn
        g = {k: _dev(v.copy()) for k, v in presets.items() if k != absent}
        g["dL_dopacity"] = _dev(gp.copy()).reshape(P, 1)
        rasterizer._C.aa_opacity_backward(_dev(inp["means3D"]), _dev(inp["opacities"]), radii, *_proj_inputs(c), g["dL_dopacity"],
                                          dL_dmeans3D=g.get("dL_dmeans3D"), dL_dcov3D=g.get("dL_dcov3D"),
                                          dL_dscales=g.get("dL_dscales"), dL_drotations=g.get("dL_drotations"),
                                          dL_dscale_factors=g.get("dL_dscale_factors"))
        torch.cuda.synchronize()
        for k, t in g.items():
            got = t.cpu().numpy()
            assert np.isfinite(got).all(), (absent, k)
            if k == "dL_dopacity":
                want = np.where(vis, rho64 * gp, gp).reshape(P, 1)
                start = gp.reshape(P, 1)
            else:
                want = presets[k].astype(np.float64) + term[_term_key(c, k)].reshape(presets[k].shape)
                start = presets[k]
            e = gpu_util.rel_inf(got, want)
            bar = max(1e-5, 4 * dev[_term_key(c, k) if k != "dL_dopacity" else "opacities"])
            if absent is None:
                print(f"backward {name} {k}: rel-inf {e:.3e}, float32 restatement {dev[_term_key(c, k) if k != 'dL_dopacity' else 'opacities']:.3e}, "
                      f"bar {bar:.3e}; the kernel's share of the result {np.abs(want - start).max() / np.abs(want).max():.2f}")
            worst[k] = max(worst.get(k, 0.0), e)
            assert e <= bar, (name, absent, k, e, bar)
            if got.shape[0] == P and not (k in ("dL_dscales", "dL_drotations") and c["indexed"]):
                # rows with radii == 0: untouched, bit for bit
                np.testing.assert_array_equal(got[~vis].view(np.uint32), start[~vis].view(np.uint32), err_msg=f"{absent} {k}")
            if absent is None and k != "dL_dopacity":
                assert np.abs(got - start).max() > 0, k                             # something was added
    print(f"backward {name}: worst rel-inf over the NULL patterns", {k: "%.3e" % v for k, v in worst.items()})


# ---------------------------------------------------------------------------------------------------------------- 4. composition
def _leaves(c):
    inp = c["inp"]
    lv = {k: inp[k].cuda().requires_grad_() for k in LEAF_KEYS if inp.get(k) is not None}
    lv["means2D"] = torch.zeros_like(lv["means3D"], requires_grad=True)
    return lv


def _compose(hip, c, depth_grad=False):
    """-> (grads through the antialiased module, grads through the plain module fed o (rho_ref + (rho_kernel - rho_ref).detach()))"""
    from c3dgs_amd import rasterizer
    inp, cam = c["inp"], c["cam"]
    P = inp["means3D"].shape[0]
    dL = synth.grad_image(W, H).cuda()
    gD, gA = (torch.from_numpy(aa_ref.hashed(W * H, s, signed=False).astype(np.float32).reshape(H, W)).cuda() for s in (31, 32))

    def loss(out):
        val = (out[0] * dL).sum()
        if depth_grad:
            val = val + (out[2] * gD).sum() + (out[3] * gA).sum()
        return val
    skw = dict(depth_grad=True) if depth_grad else {}
    grads, images = [], []
    for mode in ("antialiased", "composed"):
        lv = _leaves(c)
        m2 = lv.pop("means2D")
        if mode == "antialiased":
            rs, ev = _settings(hip, inp, antialiasing=True, **skw)
            out = _module_call(hip, c, rs, ev, lv, means2D=m2)
        else:
            rs, ev = _settings(hip, inp, **skw)
            with torch.no_grad():
                rho_k = rasterizer._C.aa_opacity(lv["means3D"], lv["opacities"], lv.get("scales"), lv.get("rotations"),
                                                 lv.get("scale_factors"), _dev(inp["g_indices"]), lv.get("cov3D_precomp"),
                                                 float(inp["scale_modifier"]), _dev(np.asarray(cam["viewmatrix"], np.float32)),
                                                 cam["tan_fovx"], cam["tan_fovy"], H, W)[1]
            ref_lv = {k: lv[k].double() for k in aa_ref.LEAVES if k in lv}
            rho_ref = aa_ref.rho(ref_lv, inp, cam).float()
            rho = rho_ref + (rho_k - rho_ref).detach()
            assert torch.equal(rho.detach(), rho_k)                                 # the forward's bits
            out = _module_call(hip, c, rs, ev, lv, means2D=m2, opacities=lv["opacities"] * rho.reshape(P, 1))
        loss(out).backward()
        torch.cuda.synchronize()
        lv["means2D"] = m2
        grads.append({k: (torch.zeros_like(v) if v.grad is None else v.grad).cpu().numpy() for k, v in lv.items()})
        images.append(out[0].detach())
    assert torch.equal(images[0].view(torch.int32), images[1].view(torch.int32))     # same forward, same blend decisions
    return grads


def _check_composition(label, got, want):
    worst = 0.0
    for k in want:
        assert np.isfinite(got[k]).all(), k
        e = gpu_util.rel_inf(got[k], want[k])
        print(f"composition {label} {k}: rel-inf {e:.3e}, reference max {np.abs(want[k]).max():.3e}")
        worst = max(worst, e)
    print(f"composition {label}: worst rel-inf {worst:.3e}")
    for k in want:
        assert gpu_util.rel_inf(got[k], want[k]) <= 1e-4, (label, k)
    assert np.abs(want["opacities"]).max() > 0 and np.abs(want["means3D"]).max() > 0


@pytest.mark.parametrize("name", ["floor", "needles", "clamped", "indexed", "indexed_scale_mod", "cov_precomp"])
def test_composition_end_to_end(hip, orc, name):
    """Measured on an MI355X: see COMPOSITION_MEASURED."""
    c = aa_ref.aa_case(name)
    _same_camera(orc, c)
    got, want = _compose(hip, c)
    _check_composition(name, got, want)


def test_composition_with_depth_grad(hip, orc):
    c = aa_ref.aa_case("indexed")
    _same_camera(orc, c)
    got, want = _compose(hip, c, depth_grad=True)
    _check_composition("indexed + depth_grad", got, want)
    plain, _ = _compose(hip, c)
    assert gpu_util.rel_inf(got["opacities"], plain["opacities"]) > 1e-3           # the maps' loss reached the opacity through rho


# ---------------------------------------------------------------------------------------------------------------- 5. model
class _Cam:
    def __init__(self, intrinsic, ev):
        self.intrinsic, self.extrinsic_vector = intrinsic.cuda(), ev.cuda()


def _model(path):
    from c3dgs_amd.model import GaussianModel
    Wm, Hm, focal = 90, 60, 80.0
    sc = synth.scene(2000, W=Wm, H=Hm, focal=focal, seed=23, scale_median=0.06)
    sc["scales"][:400] *= 0.02                                                     # floor rows: specks far below a pixel
    m = GaussianModel(3, quantization=True, device="cuda")
    if path == "fused_indexed":
        m.set_tensors(**synth.raw_params(synth.index_scene(sc, seed=24, shs_extra=32, gs_extra=32)))
    else:
        op = sc["opacities"].clamp(1e-6, 1 - 1e-6)
        m.set_tensors(xyz=sc["means3D"], features_dc=sc["shs"][:, :1], features_rest=sc["shs"][:, 1:],
                      scaling=sc["scales"] / sc["scales"].norm(dim=1, keepdim=True), rotation=sc["rotations"],
                      opacity=torch.log(op / (1 - op)), scaling_factor=torch.log(sc["scales"].norm(dim=1, keepdim=True)))
    intr, ev = synth.camera(Wm, Hm, focal)
    return m, intr, ev


@pytest.mark.parametrize("path", ["fused_indexed", "composed"])
def test_model_render(hip, path):
    from c3dgs_amd.model import PipelineParams
    m, intr, ev = _model(path)
    cam, bg = _Cam(intr, ev), torch.zeros(3, device="cuda")
    assert PipelineParams().antialiasing is False and PipelineParams(False, False, False, True).antialiasing is True
    plain = m.render(cam, PipelineParams(), bg)
    by_pipe = m.render(cam, PipelineParams(antialiasing=True), bg)
    by_arg = m.render(cam, PipelineParams(), bg, antialiasing=True)
    off = m.render(cam, PipelineParams(antialiasing=True), bg, antialiasing=False)
    assert set(by_pipe) == set(plain)
    assert torch.equal(by_pipe["render"].view(torch.int32), by_arg["render"].view(torch.int32))
    assert torch.equal(off["render"].view(torch.int32), plain["render"].view(torch.int32))
    assert torch.equal(by_pipe["radii"], plain["radii"])
    assert not torch.equal(by_pipe["render"], plain["render"])
    by_pipe["render"].sum().backward()
    torch.cuda.synchronize()
    for p in m.parameters():
        assert p.grad is not None and bool(torch.isfinite(p.grad).all())
    assert float(m._xyz.grad.abs().max()) > 0 and float(m._opacity.grad.abs().max()) > 0
    pose = _Cam(intr, ev)
    pose.extrinsic_vector.requires_grad_()
    with pytest.raises(ValueError, match="antialiasing"):
        m.render(pose, PipelineParams(antialiasing=True), bg)
    with pytest.raises(ValueError, match="antialiasing"):
        m.render(pose, PipelineParams(), bg, antialiasing=True)


# ---------------------------------------------------------------------------------------------------------------- 6. refusals, default
def _small(indexed, P=1500):
    Ws, Hs, focal = 75, 50, 60.0
    intr, ev = synth.camera(Ws, Hs, focal, extrinsic_vector=EV)
    sc = synth.scene(P, Ws, Hs, focal, seed=17, scale_median=0.08)
    if indexed:
        sc = synth.index_scene(sc, shs_extra=32, gs_extra=32)
    return sc, intr, ev, Ws, Hs


def _small_settings(hip, intr, ev, **kw):
    return hip.GaussianRasterizationSettings(intrinsic=intr.cuda(), extrinsic_vector=ev.cuda(), bg=torch.tensor((0.2, 0.4, 0.1), device="cuda"),
                                             scale_modifier=1.0, sh_degree=3, prefiltered=False, debug=False, clamp_color=True, **kw)


def _small_run(hip, sc, rs, ev, indexed, wimg, optimize_camera=False, grad=True):
    names = ("means3D", "opacities", "shs", "scales", "rotations") + (("scale_factors",) if indexed else ())
    leaves = {k: sc[k].cuda().requires_grad_(grad) for k in names}
    means2D = torch.zeros_like(leaves["means3D"], requires_grad=grad)
    kw = dict(means3D=leaves["means3D"], means2D=means2D, opacities=leaves["opacities"], shs=leaves["shs"], scales=leaves["scales"],
              rotations=leaves["rotations"], extrinsic_vector=ev.cuda())
    if indexed:
        rast = hip.GaussianRasterizerIndexed(rs, optimize_camera=optimize_camera)
        kw.update(sh_indices=sc["sh_indices"].cuda(), g_indices=sc["g_indices"].cuda(), scale_factors=leaves["scale_factors"])
    else:
        rast = hip.GaussianRasterizer(rs, optimize_camera=optimize_camera)
    out = rast(**kw)
    if grad:
        (out[0] * wimg).sum().backward()
    torch.cuda.synchronize()
    leaves["means2D"] = means2D
    return out, {k: (None if v.grad is None else v.grad.clone()) for k, v in leaves.items()}


@pytest.mark.parametrize("indexed", [False, True])
def test_pose_gradient_with_antialiasing_is_refused(hip, indexed):
    sc, intr, ev, Ws, Hs = _small(indexed, P=64)
    rs = _small_settings(hip, intr, ev, antialiasing=True)
    cls = hip.GaussianRasterizerIndexed if indexed else hip.GaussianRasterizer
    wimg = synth.grad_image(Ws, Hs).cuda()
    for oc in ((True, "exact") if indexed else ("exact",)):
        with pytest.raises(ValueError, match="antialiasing"):
            cls(rs, optimize_camera=oc)
        rast = cls(_small_settings(hip, intr, ev), optimize_camera=oc)
        rast.raster_settings = rs                               # swapped in behind the constructor: refused at the call
        with pytest.raises(ValueError, match="antialiasing"):
            kw = dict(means3D=sc["means3D"].cuda(), means2D=torch.zeros(sc["means3D"].shape, device="cuda"),
                      opacities=sc["opacities"].cuda(), shs=sc["shs"].cuda(), scales=sc["scales"].cuda(),
                      rotations=sc["rotations"].cuda(), extrinsic_vector=ev.cuda())
            if indexed:
                kw.update(sh_indices=sc["sh_indices"].cuda(), g_indices=sc["g_indices"].cuda(), scale_factors=sc["scale_factors"].cuda())
            rast(**kw)
    cls(rs, optimize_camera=False)
    assert wimg.shape == (3, Hs, Ws)


def test_refine_poses_refuses(hip, tmp_path):
    from c3dgs_amd import pipeline
    from c3dgs_amd.model import PipelineParams
    from tests import train_scene
    teacher, _ = train_scene.teacher_model(500, 64, 48, 60.0, "cuda")
    intr, ev = synth.camera(64, 48, 60.0)
    cam = train_scene.Cam(intr, ev, "cuda")
    with torch.no_grad():
        cam.original_image = teacher.render(cam, PipelineParams(), torch.zeros(3, device="cuda"))["render"].clone()
    with pytest.raises(ValueError, match="antialiasing"):
        pipeline.refine_poses([cam], teacher, PipelineParams(antialiasing=True), torch.zeros(3, device="cuda"), 2)


@pytest.mark.parametrize("indexed", [False, True])
def test_flag_off_is_the_parent(hip, indexed):
    """antialiasing=False: the outputs and gradients of the call without the keyword, bit for bit, and no aa_* stage is launched"""
    from c3dgs_amd import _lib
    sc, intr, ev, Ws, Hs = _small(indexed)
    wimg = synth.grad_image(Ws, Hs).cuda()
    rs_plain, rs_off, rs_on = (_small_settings(hip, intr, ev, **kw) for kw in (dict(), dict(antialiasing=False), dict(antialiasing=True)))
    assert rs_off.antialiasing is False and "antialiasing" not in rs_off._fields and rs_off._fields[-1] == "depth" and len(rs_off) == 9
    assert rs_on._replace(scale_modifier=2.0).antialiasing is True and rs_on._replace(antialiasing=False).antialiasing is False
    assert rs_on == rs_on._replace(antialiasing=False)             # an attribute beside the tuple, like contrib and depth_grad
    _lib.profile_enable(True)
    try:
        _lib.profile_read()
        out_a, g_a = _small_run(hip, sc, rs_plain, ev, indexed, wimg)
        out_b, g_b = _small_run(hip, sc, rs_off, ev, indexed, wimg)
        stages_off = _lib.profile_read()
        out_c, g_c = _small_run(hip, sc, rs_on, ev, indexed, wimg)
        stages_on = _lib.profile_read()
    finally:
        _lib.profile_enable(False)
    assert not [s for s in stages_off if s.startswith("aa_")], stages_off
    assert stages_off["preprocess"][1] == 2 and stages_off["backward_preprocess"][1] == 2
    assert stages_on["aa_opacity"][1] == 1 and stages_on["aa_opacity_backward"][1] == 1
    assert {s: n for s, (_, n) in stages_on.items() if not s.startswith("aa_")} == {s: n // 2 for s, (_, n) in stages_off.items()}
    assert len(out_a) == len(out_b) == 2
    assert torch.equal(out_a[0].view(torch.int32), out_b[0].view(torch.int32)) and torch.equal(out_a[1], out_b[1])
    for k in g_a:
        a, b = g_a[k], g_b[k]
        same = torch.equal(a.view(torch.int32), b.view(torch.int32))
        if not same and indexed and k in ("shs", "scales", "rotations"):
            # the indexed backward's codebook scatter-adds are float atomics in no fixed order: tests/test_render_depth_gpu.py's bar
            same = torch.allclose(a, b, rtol=1e-5, atol=1e-6 * float(b.abs().max()))
        assert same, k
    assert torch.equal(out_c[1], out_a[1]) and not torch.equal(out_c[0], out_a[0])
    assert not torch.equal(g_c["opacities"], g_a["opacities"])


def test_train_three_epochs_with_the_flag(hip, tmp_path):
    from c3dgs_amd import pipeline
    from c3dgs_amd.model import PipelineParams
    from tests import train_scene
    Wt, Ht, focal = 160, 112, 150.0
    losses = {}
    for flag in (False, True):
        d = tmp_path / str(int(flag))
        d.mkdir()
        student, cams, extent = train_scene.make(d, "cuda", W=Wt, H=Ht, focal=focal)

        class Scene:
            gaussians = student
            cameras_extent = extent

            def getTrainCameras(self):
                return cams
        log = []
        torch.manual_seed(0)
        n = pipeline.train(Scene(), None, train_scene.schedule(24, densify=False), PipelineParams(antialiasing=flag), camera_stride=1,
                           log=lambda e, i: log.append(i["ema_loss"]))
        assert n == 24 and len(log) == 3 and all(np.isfinite(v) for v in log)
        for p in student.parameters():
            assert bool(torch.isfinite(p).all())
        losses[flag] = log
    print("three epochs on the toy scene, ema loss without / with antialiasing:", losses[False], losses[True])
    assert losses[True] != losses[False]
