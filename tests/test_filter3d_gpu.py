"""-m gpu: the 3D smoothing filter (csrc/filter3d.hip; c3dgs_amd/filter3d.py, GaussianModel.compute_3D_filter / render,
pipeline.train(filter_3d=)).

  filter     filter3d.compute against tests/filter3d_ref.py: filter_np in float32, bit for bit (every operation of the kernel is a
             single IEEE fp32 operation that NumPy repeats; no operation had to be excused), and a second call bit-identical.
  apply      filter3d.apply against the float64 restatement, per tensor rel-inf at most max(1e-6, 4 x the float32
             restatement's own distance from float64 on the same preset) (filter3d_ref.f32_deviation: reference against reference,
             1e-7 .. 4e-7 on every preset, so the floor governs); f == 0 rows return Sigma and o bit for bit; the visible / rank
             form returns the rows of the plain form bit for bit.
  backward   c3dgs_filter3d_apply_backward alone on hashed gradients, every output NULL in turn, the same rule (floor 1e-5 on
             the atomically added codebook rows); rows whose gradients are both zero keep their bits.
  forward    render() with a filter = the plain rasterizer fed the kernel's (Sigma', o'), bit for bit, both rasterizers.
  model      selections carry the filter, created rows make render() raise, npz / ply round trips, fuse_filter, refusals.
  training   the compute stage is recorded where train(filter_3d=True) says it runs -- before the first iteration, at the interval,
             behind every densification by gradient or by error and every MCMC refinement that changed rows; filter_3d=False
             records no filter3d stage.
  cov3d=     a caller's covariance: cov3d + f^2 I and dL/dcov3d = dL/dSigma' bit for bit.
  compress   the sensitivity pass, run_vq and finetune (with its own pruning) on a filtered model.
  float64    gradients through filter3d.apply and GaussianRasterizer against float64 autograd of dense_render on (Sigma'_ref, o'_ref)."""
import ctypes as C

import numpy as np
import pytest
import torch

from tests import aa_ref, synth
from tests import filter3d_ref as ref

pytestmark = pytest.mark.gpu

PRESETS = ("floor", "needles", "clamped", "behind", "indexed", "indexed_scale_mod")
EV = (0.05, -0.03, 0.02, 0.99, 0.1, -0.05, 0.2)


def _bits(t):
    return t.contiguous().view(torch.int32) if t.dtype == torch.float32 else t


def _compute(xyz, table):
    from c3dgs_amd import filter3d
    f, seen = filter3d.compute(torch.from_numpy(xyz).cuda(), torch.from_numpy(table).cuda())
    torch.cuda.synchronize()
    return f.cpu().numpy(), seen.cpu().numpy()


# ---------------------------------------------------------------------------------------------------------------- 1. the filter
@pytest.mark.parametrize("C", [1, 2, 7])
@pytest.mark.parametrize("P", [1, 63, 64, 65, 257, 1025, 5000])
def test_filter_is_the_float32_restatement(hip, P, C):
    """the kernel reads the table by scalar loads, one camera per iteration: there is no camera-chunk boundary to straddle"""
    xyz, table = ref.ring_scene(P, C, seed=P + C)           # cameras of two sizes and C focal lengths in one table
    want, seen_w, _ = ref.filter_np(xyz, table)
    got, seen_g = _compute(xyz, table)
    assert got.dtype == np.float32 and got.shape == (P,)
    np.testing.assert_array_equal(seen_g, seen_w)
    np.testing.assert_array_equal(got.view(np.uint32), want.view(np.uint32))
    again, _ = _compute(xyz, table)
    np.testing.assert_array_equal(again.view(np.uint32), got.view(np.uint32))
    if P == 5000:
        assert 0 < seen_w.sum() < P                            # rows seen by nobody take the fallback


def test_filter_seen_by_nobody_and_the_near_plane(hip):
    xyz, table = ref.ring_scene(257, 3)
    got, seen = _compute(xyz + np.float32(100.0), table)
    assert not seen.any() and (got == 0).all()
    # points exactly at z = 0.2 under an identity camera: the test is z > 0.2
    table = np.zeros((1, 16), np.float32)
    table[0, [0, 5, 10]] = 1.0
    table[0, 12:] = (60.0, 60.0, 64.0, 48.0)
    z = np.float32(0.2)
    xyz = np.zeros((130, 3), np.float32)
    xyz[:, 2] = z
    xyz[65:, 2] = np.nextafter(z, np.float32(1.0))
    want, seen_w, _ = ref.filter_np(xyz, table)
    got, seen = _compute(xyz, table)
    assert not seen[:65].any() and seen[65:].all()
    np.testing.assert_array_equal(seen, seen_w)
    np.testing.assert_array_equal(got.view(np.uint32), want.view(np.uint32))


def test_camera_table_reads_the_cameras(hip):
    from c3dgs_amd import filter3d, rasterizer
    intr, ev = synth.camera(90, 60, 80.0, extrinsic_vector=EV)
    cam = _Cam(intr, ev)
    t = filter3d.camera_table([cam, _Cam(*synth.camera(64, 48, 50.0))], "cuda").cpu().numpy()
    view = rasterizer.camera_matrices(cam.intrinsic, cam.extrinsic_vector, "cuda")[0].cpu().numpy()       # transposed
    np.testing.assert_array_equal(t[0, :12].reshape(3, 4), view.T[:3])
    assert abs(t[0, 12] - 80.0) < 1e-4 and abs(t[0, 13] - 80.0) < 1e-4 and tuple(t[0, 14:]) == (90.0, 60.0)    # FoV is stored in fp32
    assert abs(t[1, 12] - 50.0) < 1e-4 and abs(t[1, 13] - 50.0) < 1e-4 and tuple(t[1, 14:]) == (64.0, 48.0)
    with pytest.raises(ValueError):
        filter3d.camera_table([], "cuda")


# ---------------------------------------------------------------------------------------------------------------- 2. apply
def _cuda(a):
    return {k: (v.cuda() if torch.is_tensor(v) else v) for k, v in a.items()}


def _apply(a, f=None, **kw):
    from c3dgs_amd import filter3d
    with torch.no_grad():
        out = filter3d.apply(a["opacities"], a["scales"], a["rotations"], a["f"] if f is None else f, a["scale_modifier"],
                             scale_factors=a["scale_factors"], g_indices=a["g_indices"], **kw)
    torch.cuda.synchronize()
    return out


def _bar(dev, floor):
    return max(floor, 4 * dev)


@pytest.mark.parametrize("name", PRESETS)
def test_apply_outputs(hip, name):
    a = ref.apply_inputs(name)
    dev = ref.f32_deviation(name)
    d = lambda t: None if t is None else t.double()           # noqa: E731
    with torch.no_grad():
        cov64, o64 = ref.apply(d(a["opacities"]), d(a["scales"]), d(a["rotations"]), d(a["f"]), a["scale_modifier"],
                               d(a["scale_factors"]), a["g_indices"])
    g = _cuda(a)
    cov, o = _apply(g)
    assert cov.shape == cov64.shape and o.shape == a["opacities"].shape
    e_cov, e_o = ref.relinf(cov.cpu(), cov64), ref.relinf(o.cpu(), o64)
    print(f"apply {name}: cov3D' {e_cov:.3e} (float32 restatement {dev['cov3D']:.3e}), o' {e_o:.3e} ({dev['opacity']:.3e})")
    assert e_cov <= _bar(dev["cov3D"], 1e-6) and e_o <= _bar(dev["opacity"], 1e-6)
    # f == 0: Sigma and o bit for bit (Sigma: what the kernel gives with no filter anywhere)
    zero = a["f"] == 0
    assert int(zero.sum()) >= 10 and int((a["f"] > 10 * a["f"].median()).sum()) >= 10
    cov0, o0 = _apply(g, f=torch.zeros_like(g["f"]))
    assert torch.equal(_bits(o0), _bits(g["opacities"]))
    assert torch.equal(_bits(cov[zero.cuda()]), _bits(cov0[zero.cuda()])) and torch.equal(_bits(o[zero.cuda()]), _bits(g["opacities"][zero.cuda()]))
    assert not torch.equal(cov[~zero.cuda()], cov0[~zero.cuda()])
    # the visible / rank form: the subset's rows are the plain form's rows
    n = o.shape[0]
    vis = torch.as_tensor(aa_ref.hashed(n, 17) > -0.3).cuda()
    rank = (torch.cumsum(vis, 0, dtype=torch.int32) - vis.to(torch.int32)).contiguous()
    sub = dict(g, opacities=g["opacities"][vis].contiguous())
    if a["g_indices"] is not None:
        sub.update(g_indices=g["g_indices"][vis].contiguous(), scale_factors=g["scale_factors"][vis].contiguous())
    else:
        sub.update(scales=g["scales"][vis].contiguous(), rotations=g["rotations"][vis].contiguous())
    cov_v, o_v = _apply(sub, visible=vis.to(torch.uint8), rank=rank)
    assert torch.equal(_bits(cov_v), _bits(cov[vis])) and torch.equal(_bits(o_v), _bits(o[vis]))


# ---------------------------------------------------------------------------------------------------------------- 3. backward alone
OUTPUTS = ("dL_dopacity", "dL_dscales", "dL_drotations", "dL_dscale_factors")
KEY_OF = dict(dL_dopacity="opacities", dL_dscales="scales", dL_drotations="rotations", dL_dscale_factors="scale_factors")


@pytest.mark.parametrize("name", PRESETS)
def test_backward_kernel_alone(hip, name):
    from c3dgs_amd import _lib, filter3d
    a = ref.apply_inputs(name)
    indexed = a["g_indices"] is not None
    n = a["opacities"].shape[0]
    d_cov = torch.as_tensor(aa_ref.hashed(6 * n, 11)).reshape(n, 6).float()
    gp = torch.as_tensor(aa_ref.hashed(n, 13)).float()
    dead = torch.zeros(n, dtype=torch.bool)
    dead[3::5] = True                                          # both gradients zero: the kernel does not touch these rows
    d_cov[dead], gp[dead] = 0, 0
    d_cov[1::5] = 0                                            # only g'
    gp[2::5] = 0                                               # only dL_dcov3D
    want = ref.autograd_backward(a["opacities"], a["scales"], a["rotations"], a["f"], d_cov, gp, a["scale_modifier"],
                                 a["scale_factors"], a["g_indices"])
    dev = ref.f32_deviation(name)
    g = _cuda(a)
    r, t, _ = filter3d._rows(g["opacities"], g["scales"], g["rotations"], g["f"], g["scale_modifier"], g["scale_factors"],
                             g["g_indices"], None, None)
    d_cov_g, gp_g = d_cov.cuda().contiguous(), gp.cuda().contiguous()
    names = [o for o in OUTPUTS if indexed or o != "dL_dscale_factors"]
    for skip in [None] + names:
        outs, preset = {}, {}
        for o in names:
            if o == skip:
                continue
            like = g[KEY_OF[o]]
            atomic = indexed and o in ("dL_dscales", "dL_drotations")
            preset[o] = torch.zeros_like(like) if atomic else torch.as_tensor(
                aa_ref.hashed(like.numel(), 23 + len(o)).reshape(like.shape)).float().cuda()
            outs[o] = preset[o].clone()
        gr = _lib.Filter3DGrads(dL_dcov3D=d_cov_g.data_ptr(), dL_dopacity_out=gp_g.data_ptr(), **{o: v.data_ptr() for o, v in outs.items()})
        _lib.check(_lib.lib().c3dgs_filter3d_apply_backward(C.byref(r), C.byref(gr), None))
        torch.cuda.synchronize()
        for o, got in outs.items():
            w = want[KEY_OF[o]]
            atomic = indexed and o in ("dL_dscales", "dL_drotations")
            if atomic:
                e = ref.relinf(got.cpu(), w)
            else:
                live = ~dead
                assert torch.equal(_bits(got.cpu()[dead]), _bits(preset[o].cpu()[dead])), (o, "rows without a gradient were written")
                e = ref.relinf(got.cpu()[live], w.reshape(got.shape)[live])
            bar = _bar(dev["d_" + KEY_OF[o]], 1e-5 if atomic else 1e-6)
            if skip is None:
                print(f"backward {name} {o}: rel-inf {e:.3e} (float32 restatement {dev['d_' + KEY_OF[o]]:.3e}), bar {bar:.1e}")
            assert e <= bar, (name, o, skip, e, bar)


# ---------------------------------------------------------------------------------------------------------------- 4. forward identity
class _Cam:
    def __init__(self, intrinsic, ev):
        self.intrinsic, self.extrinsic_vector = intrinsic.cuda(), ev.cuda()


WM, HM, FOCAL = 90, 60, 80.0


def _cams():
    poses = (EV, (0, 0, 0, 1, 0, 0, 0), (-0.04, 0.06, 0.0, 0.99, -0.2, 0.1, 0.4))
    return [_Cam(*synth.camera(WM, HM, FOCAL * (1 + 0.2 * k), extrinsic_vector=ev)) for k, ev in enumerate(poses)]


def _model(path, P=2000, quantization=False):
    from c3dgs_amd.model import GaussianModel
    sc = synth.scene(P, W=WM, H=HM, focal=FOCAL, seed=23, scale_median=0.06)
    sc["scales"][:400] *= 0.02                                                     # specks far below the filter
    m = GaussianModel(3, quantization=quantization, device="cuda")
    if path == "fused_indexed":
        m.set_tensors(**synth.raw_params(synth.index_scene(sc, seed=24, shs_extra=32, gs_extra=32)))
    else:
        op = sc["opacities"].clamp(1e-6, 1 - 1e-6)
        m.set_tensors(xyz=sc["means3D"], features_dc=sc["shs"][:, :1], features_rest=sc["shs"][:, 1:],
                      scaling=sc["scales"] / sc["scales"].norm(dim=1, keepdim=True), rotation=sc["rotations"],
                      opacity=torch.log(op / (1 - op)), scaling_factor=torch.log(sc["scales"].norm(dim=1, keepdim=True)))
    return m


@pytest.mark.parametrize("path", ["fused_indexed", "composed"])
def test_render_is_the_plain_rasterizer_on_the_filtered_inputs(hip, path):
    from c3dgs_amd import filter3d
    from c3dgs_amd.model import PipelineParams
    m = _model(path)
    cams = _cams()
    cam, bg, pipe = cams[0], torch.tensor((0.2, 0.4, 0.1), device="cuda"), PipelineParams()
    seen = m.compute_3D_filter(cams)
    assert m.filter_3D.shape == (2000,) and m.filter_3D.dtype == torch.float32 and not m.filter_3D.requires_grad
    assert bool(seen.any()) and float(m.filter_3D.min()) > 0
    gt = synth.grad_image(WM, HM, seed=5).abs().clamp(0, 1).cuda().contiguous()
    extra = dict(return_depth=True, return_contrib=True, error_target=gt)
    with torch.no_grad():
        got = m.render(cam, pipe, bg, gather_visible=False, **extra)
        plain = m.clear_3D_filter() or m.render(cam, pipe, bg, gather_visible=False)
        m.compute_3D_filter(cams)
        rs = hip.GaussianRasterizationSettings(intrinsic=cam.intrinsic, extrinsic_vector=cam.extrinsic_vector, bg=bg, scale_modifier=1.0,
                                               sh_degree=m.active_sh_degree, prefiltered=False, debug=False, clamp_color=True,
                                               depth=True, contrib=True, error_target=gt)
        means2D = torch.zeros_like(m._xyz)
        if path == "fused_indexed":
            cov, o = filter3d.apply(m.get_opacity, m.get_scaling_normalized, m._rotation_post_activation, m.filter_3D, 1.0,
                                    scale_factors=m.get_scaling_factor, g_indices=m._gaussian_indices)
            want = hip.GaussianRasterizerIndexed(rs)(means3D=m.get_xyz, means2D=means2D, opacities=o, shs=m._get_features_raw,
                                                     sh_indices=m._feature_indices, g_indices=m._gaussian_indices, cov3D_precomp=cov,
                                                     extrinsic_vector=cam.extrinsic_vector)
            rows = got["visible"]
        else:
            cov, o = filter3d.apply(m.get_opacity, m.get_scaling, m.get_rotation, m.filter_3D, 1.0)
            want = hip.GaussianRasterizer(rs)(means3D=m.get_xyz, means2D=means2D, opacities=o, shs=m.get_features, cov3D_precomp=cov,
                                              extrinsic_vector=cam.extrinsic_vector)
            rows = torch.ones(2000, dtype=torch.bool, device="cuda")
    torch.cuda.synchronize()
    keys = ("render", "radii", "depth", "alpha", "median_depth", "contrib_sum", "contrib_max", "contrib_hits", "error_sum")
    assert len(want) == len(keys)
    for k, b in zip(keys, want):
        a = got[k]
        if a.shape != b.shape:                                 # the fused path's per-Gaussian rows are the visible subset
            b = b[rows]
        assert a.dtype == b.dtype and a.shape == b.shape, k
        assert torch.equal(_bits(a), _bits(b)), k
    assert not torch.equal(got["render"], plain["render"])     # the filter is visible


# ---------------------------------------------------------------------------------------------------------------- 5. gradients end to end
@pytest.mark.parametrize("path,mode", [("fused_indexed", "antialiasing"), ("composed", "depth_grad"), ("fused_indexed", "depth_grad"),
                                       ("composed", "antialiasing")])
def test_param_grad_through_render(hip, path, mode):
    """param.grad through GaussianModel.render with a filter against the plain rasterizer modules fed (Sigma', o') whose VALUES are
    the kernel's and whose DERIVATIVES are float64 autograd of tests/filter3d_ref.py: apply (x_ref + (x_kernel - x_ref).detach()),
    so the rasterizer's forward and blend decisions are the same and autograd supplies the chain through the filter. rel-inf 1e-4
    per tensor, the bar of the depth-gradient and antialiasing tests. The rasterizer's own backward is on both sides here;
    test_gradients_against_dense_render holds the whole chain, rasterizer included, to float64."""
    from c3dgs_amd import filter3d
    from c3dgs_amd.model import PipelineParams
    m = _model(path)
    cams = _cams()
    cam, bg = cams[0], torch.tensor((0.2, 0.4, 0.1), device="cuda")
    m.compute_3D_filter(cams)
    kw = dict(antialiasing=True) if mode == "antialiasing" else dict(depth_grad=True)
    dL = synth.grad_image(WM, HM).cuda()
    gD, gA = (torch.from_numpy(aa_ref.hashed(WM * HM, s, signed=False).astype(np.float32).reshape(HM, WM)).cuda() for s in (31, 32))

    def loss(image, depth=None, alpha=None):
        val = (image * dL).sum()
        return val + (depth * gD).sum() + (alpha * gA).sum() if mode == "depth_grad" else val
    grads = []
    for which in ("render", "reference"):
        m.zero_grad()
        if which == "render":
            out = m.render(cam, PipelineParams(), bg, gather_visible=False, **kw)
            loss(out["render"], out.get("depth"), out.get("alpha")).backward()
        else:
            f = m.filter_3D
            rs = hip.GaussianRasterizationSettings(intrinsic=cam.intrinsic, extrinsic_vector=cam.extrinsic_vector, bg=bg, scale_modifier=1.0,
                                                   sh_degree=m.active_sh_degree, prefiltered=False, debug=False, clamp_color=True, **kw)
            means2D = torch.zeros_like(m._xyz)
            if path == "fused_indexed":
                o_in, sc, rt, sf, gi = m.get_opacity, m.get_scaling_normalized, m._rotation_post_activation, m.get_scaling_factor, m._gaussian_indices
            else:
                o_in, sc, rt, sf, gi = m.get_opacity, m.get_scaling, m.get_rotation, None, None
            with torch.no_grad():
                cov_k, o_k = filter3d.apply(o_in, sc, rt, f, 1.0, scale_factors=sf, g_indices=gi)
            cov_r, o_r = ref.apply(o_in.double().reshape(-1), sc.double(), rt.double(), f.double(), 1.0,
                                   None if sf is None else sf.double().reshape(-1), gi)
            cov_r, o_r = cov_r.float(), o_r.float().reshape(o_k.shape)
            cov, o = cov_r + (cov_k - cov_r).detach(), o_r + (o_k - o_r).detach()
            assert torch.equal(_bits(cov.detach()), _bits(cov_k)) and torch.equal(_bits(o.detach()), _bits(o_k))
            if path == "fused_indexed":
                out = hip.GaussianRasterizerIndexed(rs)(means3D=m.get_xyz, means2D=means2D, opacities=o, shs=m._get_features_raw,
                                                        sh_indices=m._feature_indices, g_indices=gi, cov3D_precomp=cov,
                                                        extrinsic_vector=cam.extrinsic_vector)
            else:
                out = hip.GaussianRasterizer(rs)(means3D=m.get_xyz, means2D=means2D, opacities=o, shs=m.get_features, cov3D_precomp=cov,
                                                 extrinsic_vector=cam.extrinsic_vector)
            loss(out[0], *(out[2:4] if mode == "depth_grad" else ())).backward()
        torch.cuda.synchronize()
        grads.append({k: getattr(m, k).grad.detach().cpu().clone() for k in ("_xyz", "_opacity", "_scaling", "_scaling_factor", "_rotation",
                                                                            "_features_dc", "_features_rest")})
    got, want = grads
    for k in want:
        assert bool(torch.isfinite(got[k]).all()), k
        e = ref.relinf(got[k], want[k])
        print(f"param.grad {path} {mode} {k}: rel-inf {e:.3e}, reference max {float(want[k].abs().max()):.3e}")
        assert e <= 1e-4, (path, mode, k, e)
    assert float(want["_scaling"].abs().max()) > 0 and float(want["_opacity"].abs().max()) > 0


# ---------------------------------------------------------------------------------------------------------------- 6. the model
def test_refusals(hip):
    from c3dgs_amd import pipeline
    from c3dgs_amd.model import PipelineParams
    m = _model("composed", P=300)
    cams = _cams()
    bg = torch.zeros(3, device="cuda")
    m.compute_3D_filter(cams)
    with pytest.raises(NotImplementedError, match="3D filter"):
        m.render(cams[0], PipelineParams(compute_cov3D_python=True), bg)
    pose = _Cam(*synth.camera(WM, HM, FOCAL))
    pose.extrinsic_vector.requires_grad_()
    with pytest.raises(ValueError, match="3D filter"):
        m.render(pose, PipelineParams(), bg)
    pose.original_image = torch.zeros(3, HM, WM, device="cuda")
    with pytest.raises(ValueError, match="3D filter"):
        pipeline.refine_poses([pose], m, PipelineParams(), bg, 1)
    m.clear_3D_filter()
    assert m.filter_3D is None
    m.render(cams[0], PipelineParams(), bg, cov3d=m.get_covariance().detach())


def test_selections_carry_the_filter_and_new_rows_drop_it(hip):
    from c3dgs_amd.model import PipelineParams
    cams, bg = _cams(), torch.zeros(3, device="cuda")
    m = _model("composed", P=500)
    m.compute_3D_filter(cams)
    f0 = m.filter_3D.clone()
    mask = torch.as_tensor(aa_ref.hashed(500, 3) > 0).cuda()
    m.prune_points(mask)
    assert torch.equal(m.filter_3D, f0[~mask])
    keep = torch.as_tensor(aa_ref.hashed(int((~mask).sum()), 4) > -0.5).cuda()
    f1 = m.filter_3D.clone()
    m.mask_splats(keep)
    assert torch.equal(m.filter_3D, f1[keep])
    xyz, f2 = m._xyz.detach().clone(), m.filter_3D.clone()
    m._sort_morton()
    back = (m._xyz.detach()[:, None, :] == xyz[None, :, :]).all(2).float().argmax(1)        # positions are distinct
    assert torch.equal(m.filter_3D, f2[back])
    m.render(cams[0], PipelineParams(), bg)
    # rows are created: the filter goes and render() refuses until it is computed again
    m.densify_and_clone(selected_pts_mask=torch.arange(5, device="cuda"))
    assert m.filter_3D is None
    with pytest.raises(RuntimeError, match="compute_3D_filter"):
        m.render(cams[0], PipelineParams(), bg)
    m.compute_3D_filter(cams)
    assert m.filter_3D.shape[0] == m._xyz.shape[0]
    m.render(cams[0], PipelineParams(), bg)
    # an indexed model
    mi = _model("fused_indexed", P=500)
    mi.compute_3D_filter(cams)
    fi = mi.filter_3D.clone()
    mi.prune_points_indexed(mask)
    assert torch.equal(mi.filter_3D, fi[~mask])
    stats = mi.contribution_stats(cams, PipelineParams(), bg)
    fj, gone = mi.filter_3D.clone(), stats["views"] < 1
    assert mi.prune_by_contribution(stats) == int(gone.sum())
    assert torch.equal(mi.filter_3D, fj[~gone])
    mi.render(cams[0], PipelineParams(), bg)


@pytest.mark.parametrize("path", ["fused_indexed", "composed"])
def test_npz_and_ply_round_trips(hip, path, tmp_path):
    from c3dgs_amd.model import GaussianModel, PipelineParams
    cams, bg = _cams(), torch.zeros(3, device="cuda")
    m = _model(path, P=600)
    # the opacity keeps its 8-bit fake-quantiser even with quantization=False (as in the reference); for fuse_filter it would
    # quantise o in one model and the baked o' in the other, a step of ~1/255 that is no property of the filter: off in both
    m.opacity_qa.disable_fake_quant()
    m.opacity_qa.disable_observer()
    m.save_npz(str(tmp_path / "plain.npz"))
    m.compute_3D_filter(cams)
    with torch.no_grad():
        want = m.render(cams[0], PipelineParams(), bg)["render"]
    for half in (False, True):
        m.save_npz(str(tmp_path / "f.npz"), half_precision=half)
        keys = list(np.load(str(tmp_path / "f.npz")).keys())
        assert keys[-1] == "filter_3D" and np.load(str(tmp_path / "f.npz"))["filter_3D"].dtype == (np.float16 if half else np.float32)
        m2 = GaussianModel(3, quantization=False, device="cuda").load_npz(str(tmp_path / "f.npz"))
        assert torch.equal(m2.filter_3D, m.filter_3D.half().float() if half else m.filter_3D)
    f = m.filter_3D.clone()
    m.clear_3D_filter()
    m.save_npz(str(tmp_path / "cleared.npz"))
    # no filter: the file of a model that never had one, member for member (the zip container stamps each member with the time of writing)
    members = lambda p: [(k, v.dtype, v.shape, v.tobytes()) for k, v in np.load(str(p)).items()]      # noqa: E731
    assert members(tmp_path / "cleared.npz") == members(tmp_path / "plain.npz")
    assert "filter_3D" not in np.load(str(tmp_path / "plain.npz")).keys()
    m.filter_3D = f
    m.save_ply(str(tmp_path / "f.ply"))
    m3 = GaussianModel(3, quantization=False, device="cuda").load_ply(str(tmp_path / "f.ply"))
    assert torch.equal(m3.filter_3D, m.filter_3D)
    m.save_ply(str(tmp_path / "fused.ply"), fuse_filter=True)
    m4 = GaussianModel(3, quantization=False, device="cuda").load_ply(str(tmp_path / "fused.ply"))
    assert m4.filter_3D is None
    m4.active_sh_degree = m.active_sh_degree
    m4.opacity_qa.disable_fake_quant()
    m4.opacity_qa.disable_observer()
    from c3dgs_amd import filter3d
    with torch.no_grad():
        got = m4.render(cams[0], PipelineParams(), bg)["render"]
        o_in, sc, rt = m.get_opacity, m.get_scaling, m.get_rotation
        cov_f, o_f = filter3d.apply(o_in, sc, rt, m.filter_3D, 1.0)
        cov64, o64 = ref.apply(o_in.double().reshape(-1), sc.double(), rt.double(), m.filter_3D.double())
        cov32, o32 = ref.apply(o_in.reshape(-1), sc, rt, m.filter_3D)
        cov_l, o_l = m4.get_covariance(), m4.get_opacity
    # the render of the baked model against the filtered one, held to the apply bar as rel-inf on the image (the bar's floor, 1e-6:
    # both renders blend the same Gaussians from inputs that agree to that bar; measured on an MI355X: 1.6e-7 / 1.9e-7)
    e_img = ref.relinf(got, want)
    print(f"fuse_filter {path}: image rel-inf {e_img:.3e}, max |image difference| {float((got - want).abs().max()):.3e}")
    assert e_img <= 1e-6, (path, e_img)
    # and the rasterizer's inputs, the apply bar: 4 x the float32 restatement's distance from float64 on this scene, at least 1e-6
    for what, a, b, b32, b64 in (("cov3D'", cov_l, cov_f, cov32, cov64), ("o'", o_l.reshape(-1), o_f.reshape(-1), o32, o64)):
        e, bar = ref.relinf(a, b), max(1e-6, 4 * ref.relinf(b32, b64))
        print(f"fuse_filter {path} {what}: rel-inf {e:.3e}, bar {bar:.1e}")
        assert e <= bar, (what, e, bar)


# ---------------------------------------------------------------------------------------------------------------- 7. training
def _train(tmp_path, iterations=24, densify=False, log=None, **kw):
    from c3dgs_amd import _lib, pipeline
    from c3dgs_amd.model import PipelineParams
    from tests import train_scene
    student, cams, extent = train_scene.make(tmp_path, "cuda", W=160, H=112, focal=150.0)

    class Scene:
        gaussians = student
        cameras_extent = extent

        def getTrainCameras(self):
            return cams
    torch.manual_seed(0)
    _lib.profile_enable(True)
    try:
        _lib.profile_read()
        n = pipeline.train(Scene(), None, train_scene.schedule(iterations, densify=densify), PipelineParams(), camera_stride=1,
                           log=log, **kw)
        stages = _lib.profile_read()
    finally:
        _lib.profile_enable(False)
    assert n == iterations
    return student, stages


def test_train_computes_the_filter_where_it_says(hip, tmp_path):
    student, stages = _train(tmp_path, filter_3d=True, filter_3d_interval=10)
    # before the first iteration, and in front of iterations 10 and 20; no step of this schedule changes rows
    assert stages["filter3d_compute"][1] == 3
    assert stages["filter3d_apply"][1] == 24 and stages["filter3d_apply_backward"][1] == 24
    assert student.filter_3D is not None and student.filter_3D.shape[0] == student._xyz.shape[0]
    for p in student.parameters():
        assert bool(torch.isfinite(p).all())


def test_train_without_the_flag_is_the_default_path(hip, tmp_path):
    student, stages = _train(tmp_path)
    assert not [s for s in stages if s.startswith("filter3d")], stages
    assert student.filter_3D is None
    assert stages["preprocess"][1] == 24


@pytest.mark.parametrize("mode", ["grad", "error", "mcmc"])
def test_train_recomputes_the_filter_after_every_step_that_changes_rows(hip, tmp_path, mode):
    """80 iterations = 10 epochs of 8 views with density control (tests/train_scene.py: schedule): the filter is computed before
    the first iteration, in front of iteration 50 (the interval) and once behind every epoch whose density step changed rows --
    densify_and_prune by gradient or by error always rebuilds the scene; an MCMC refinement that neither relocated nor added a
    row changes nothing -- and every render in between goes through (render() raises on a stale filter)."""
    events = []
    kw = dict(grad={}, error=dict(densify_by="error", error_threshold=1.5), mcmc=dict(strategy="mcmc", cap_max=700))[mode]
    student, stages = _train(tmp_path, iterations=80, densify=True, log=lambda e, i: events.append(i), filter_3d=True,
                             filter_3d_interval=50, **kw)
    if mode == "mcmc":
        changed = sum(1 for i in events if i["mcmc"] and (i["mcmc"][0] or i["mcmc"][1]))
    else:
        changed = sum(1 for i in events if i["densified"] is not None)
    print(f"train {mode}: {changed} row-changing steps, rows {student._xyz.shape[0]}, stages {stages['filter3d_compute']}")
    assert changed >= 3
    assert stages["filter3d_compute"][1] == 1 + 1 + changed
    assert stages["filter3d_apply"][1] == 80
    assert student.filter_3D is not None and student.filter_3D.shape[0] == student._xyz.shape[0] and not student._filter_3D_stale
    assert student._xyz.shape[0] != 500 or mode == "mcmc"
    for p in student.parameters():
        assert bool(torch.isfinite(p).all())


# ---------------------------------------------------------------------------------------------------------------- 8. a caller's covariance
@pytest.mark.parametrize("name", ["floor", "indexed_scale_mod"])
def test_apply_with_a_callers_covariance(hip, name):
    """cov3d + (scale_modifier f)^2 I bit for bit (one fp32 product and one add per diagonal element), o' as without it, and the
    gradients: dL/dcov3d is dL/dSigma' itself, the opacity takes coef g', scales and rotations receive nothing through Sigma"""
    from c3dgs_amd import filter3d
    a = ref.apply_inputs(name)
    g = _cuda(a)
    n = a["opacities"].shape[0]
    cov_in = torch.as_tensor(aa_ref.hashed(6 * n, 41)).reshape(n, 6).float().cuda().requires_grad_()
    o_in = g["opacities"].clone().requires_grad_()
    sc_in = g["scales"].clone().requires_grad_()
    cov, o = filter3d.apply(o_in, sc_in, None, g["f"], g["scale_modifier"], scale_factors=g["scale_factors"], g_indices=g["g_indices"],
                            cov3d=cov_in)
    _, o_plain = _apply(g)
    assert torch.equal(_bits(o.detach()), _bits(o_plain))
    sm = torch.tensor(g["scale_modifier"], dtype=torch.float32, device="cuda")
    mf = sm * g["f"]
    want = cov_in.detach().clone()
    want[:, [0, 3, 5]] += torch.where(g["f"] == 0, torch.zeros_like(mf), mf * mf)[:, None]
    assert torch.equal(_bits(cov.detach()), _bits(want))
    d_cov = torch.as_tensor(aa_ref.hashed(6 * n, 11)).reshape(n, 6).float().cuda()
    gp = torch.as_tensor(aa_ref.hashed(n, 13)).float().cuda()
    ((cov * d_cov).sum() + (o * gp).sum()).backward()
    torch.cuda.synchronize()
    assert torch.equal(_bits(cov_in.grad), _bits(d_cov))
    ref_g = ref.autograd_backward(a["opacities"], a["scales"], a["rotations"], a["f"], torch.zeros(n, 6), gp.cpu(), a["scale_modifier"],
                                  a["scale_factors"], a["g_indices"])
    dev = ref.f32_deviation(name)
    assert ref.relinf(o_in.grad.cpu(), ref_g["opacities"]) <= _bar(dev["d_opacities"], 1e-6)
    assert ref.relinf(sc_in.grad.cpu(), ref_g["scales"]) <= _bar(dev["d_scales"], 1e-5 if a["g_indices"] is not None else 1e-6)


# ---------------------------------------------------------------------------------------------------------------- 9. the compression run
def _vq_model(P=6000, W=320, H=200):
    from c3dgs_amd.model import GaussianModel, PipelineParams
    sc = synth.scene(P, W, H, 300.0, seed=21, sh_degree=3, scale_median=0.03)
    op = sc["opacities"].clamp(1e-6, 1 - 1e-6)
    norm = sc["scales"].norm(dim=1, keepdim=True)
    g = GaussianModel(3, quantization=True, device="cuda")
    g.set_tensors(xyz=sc["means3D"], features_dc=sc["shs"][:, :1], features_rest=sc["shs"][:, 1:], scaling=sc["scales"] / norm,
                  rotation=sc["rotations"], opacity=torch.log(op / (1 - op)), scaling_factor=torch.log(norm))
    g.spatial_lr_scale = 1.0
    cams = [_Cam(*synth.camera(W, H, 300.0, extrinsic_vector=(0.0, 0.03 * (k - 1), 0.0, 1.0, 0.0, 0.0, 0.0))) for k in range(3)]
    g.compute_3D_filter(cams)
    pipe, bg = PipelineParams(), torch.zeros(3, device="cuda")
    for cam in cams:
        with torch.no_grad():
            cam.original_image = g.render(cam, pipe, bg)["render"].clone()
    return g, cams, pipe, bg


def test_sensitivity_pass_on_a_filtered_model(hip):
    """calc_importance_experimental hands render() its covariance leaf; with a filter the leaf enters Sigma' = cov3d + f^2 I, so
    cov_grad is still the gradient with respect to the model's covariance. Against the same pass with the filter cleared the
    gradients differ (the filter is in the render) and stay of the same order"""
    from c3dgs_amd import _lib, sensitivity
    g, cams, pipe, bg = _vq_model(P=3000)
    _lib.profile_enable(True)
    try:
        _lib.profile_read()
        imp, cov_grad = sensitivity.calc_importance_experimental(g, cams, pipe, use_gt=False)
        stages = _lib.profile_read()
    finally:
        _lib.profile_enable(False)
    assert stages["filter3d_apply"][1] == 3 and stages["filter3d_apply_backward"][1] == 3
    assert imp.shape == (3000, 48) and cov_grad.shape == (3000, 6)
    assert bool(torch.isfinite(imp).all()) and bool(torch.isfinite(cov_grad).all()) and float(cov_grad.abs().max()) > 0
    f = g.filter_3D
    g.clear_3D_filter()
    imp0, cov_grad0 = sensitivity.calc_importance_experimental(g, cams, pipe, use_gt=False)
    g.filter_3D = f
    assert not torch.equal(cov_grad, cov_grad0)
    ratio = float(cov_grad.abs().sum() / cov_grad0.abs().sum())
    print(f"sensitivity with / without the filter: sum |cov_grad| ratio {ratio:.3f}")
    assert 0.1 < ratio < 10.0


def test_run_vq_and_finetune_on_a_filtered_model(hip, tmp_path):
    """train -> compress is the product's main flow: run_vq (sensitivity, prune + VQ, fine-tune, npz) on a model that carries a
    filter keeps it through the pruning and the indexing, writes it, and the file loads into a model that renders close to the
    filtered original; finetune's own pruning re-measures it"""
    import os
    from c3dgs_amd import _lib, pipeline
    from c3dgs_amd.model import GaussianModel
    P = 6000
    g, cams, pipe, bg = _vq_model(P)
    comp = pipeline.CompressionParams(finetune_iterations=6, color_cluster_iterations=8, gaussian_cluster_iterations=8,
                                      color_codebook_size=64, gaussian_codebook_size=64, color_batch_size=2 ** 11,
                                      gaussian_batch_size=2 ** 11, output_vq=str(tmp_path / "vq"))
    timings, path = pipeline.run_vq(g, cams, pipeline.OptimizationParams(), pipe, comp)
    assert os.path.isfile(path) and g.is_color_indexed and g.is_gaussian_indexed
    assert g.filter_3D is not None and g.filter_3D.shape[0] == g._xyz.shape[0] <= P
    assert "filter_3D" in np.load(path).keys()
    back = GaussianModel(3, quantization=True, device="cuda").load_npz(path)
    assert back.filter_3D is not None and back.filter_3D.shape[0] == back._xyz.shape[0]
    with torch.no_grad():
        a = back.render(cams[1], pipe, bg)["render"]
    mse = float(((a - cams[1].original_image) ** 2).mean())
    assert -10 * np.log10(mse) > 25.0, mse                      # tests/test_model_gpu.py's bar for the same run without a filter
    # finetune with its own pruning: the survivors carry their values and the scene is measured again behind each prune
    comp2 = pipeline.CompressionParams(finetune_iterations=6, output_vq=str(tmp_path / "vq2"))
    _lib.profile_enable(True, only="filter3d_compute")
    try:
        _lib.profile_read()
        pipeline.finetune(pipeline._SceneView(back, cams, 0), pipeline._Dataset(), pipeline.OptimizationParams(), comp2, pipe,
                          prune_interval=2, prune_min_opacity=0.02)
        stages = _lib.profile_read()
    finally:
        _lib.profile_enable(False)
    assert stages["filter3d_compute"][1] == 2                   # iterations 2 and 4 (none behind the last iteration)
    assert back.filter_3D.shape[0] == back._xyz.shape[0]


# ---------------------------------------------------------------------------------------------------------------- 10. float64 dense render
def test_gradients_against_dense_render(hip, orc):
    """Gradients of sum(image x dL) with respect to the rasterizer's leaves through filter3d.apply and GaussianRasterizer, against
    float64 autograd of tests/dense_ref.py: dense_render on (Sigma'_ref, o'_ref) = tests/filter3d_ref.py: apply in float64, on the
    tile lists the CPU oracle builds for the fp32 (Sigma'_ref, o'_ref). rel-inf 1e-4 per tensor."""
    from c3dgs_amd import filter3d
    from tests import cases, dense_ref
    inp, cam, indexed = cases.make_case("tiny")
    assert not indexed
    P, sm = inp["means3D"].shape[0], float(inp["scale_modifier"])
    f = ref.hashed_filter(P, float(inp["scales"].median()))
    f[5::11] = 3.0 * float(inp["scales"].median())              # f >> s rows that still leave something to see
    dL = synth.grad_image(cam["W"], cam["H"])
    lv = dense_ref.leaves_of(inp)
    cov64, o64 = ref.apply(lv["opacities"].reshape(-1), lv["scales"], lv["rotations"], f.double(), sm)
    st = cases.oracle_forward(dict(inp, cov3D_precomp=cov64.detach().float(), opacities=o64.detach().float().reshape(P, 1),
                                   scales=None, rotations=None), cam)
    assert int((np.asarray(st.radii) > 0).sum()) >= 10
    img64 = dense_ref.dense_render(st, dict(means3D=lv["means3D"], means2D=lv["means2D"], opacities=o64, shs=lv["shs"], cov3D_precomp=cov64))
    (img64 * dL.double()).sum().backward()
    intr, ev = synth.camera(cam["W"], cam["H"], 40.0, extrinsic_vector=EV)
    same = orc.camera(intr.numpy(), ev.numpy())
    np.testing.assert_array_equal(np.asarray(same["viewmatrix"]), np.asarray(cam["viewmatrix"]))
    rs = hip.GaussianRasterizationSettings(intrinsic=intr.cuda(), extrinsic_vector=ev.cuda(), bg=inp["bg"].cuda(), scale_modifier=sm,
                                           sh_degree=int(inp["degree"]), prefiltered=False, debug=False, clamp_color=bool(inp["clamp_color"]))
    names = ("means3D", "opacities", "shs", "scales", "rotations")
    gl = {k: inp[k].cuda().requires_grad_() for k in names}
    cov, o = filter3d.apply(gl["opacities"], gl["scales"], gl["rotations"], f.cuda(), sm)
    out = hip.GaussianRasterizer(rs)(means3D=gl["means3D"], means2D=torch.zeros_like(gl["means3D"], requires_grad=True), opacities=o,
                                     shs=gl["shs"], cov3D_precomp=cov, extrinsic_vector=ev.cuda())
    (out[0] * dL.cuda()).sum().backward()
    torch.cuda.synchronize()
    e_img = ref.relinf(out[0].detach().cpu(), img64.detach())
    print(f"dense_render image rel-inf {e_img:.3e}")
    for k in names:
        e = ref.relinf(gl[k].grad.cpu(), lv[k].grad.reshape(gl[k].shape))
        print(f"dense_render {k}: rel-inf {e:.3e}, reference max {float(lv[k].grad.abs().max()):.3e}")
        assert e <= 1e-4, (k, e)
    assert float(lv["scales"].grad.abs().max()) > 0 and float(lv["rotations"].grad.abs().max()) > 0
