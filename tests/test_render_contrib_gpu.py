"""-m gpu: per-Gaussian blend statistics of a finished forward (csrc/render_contrib.hip: c3dgs_render_contrib,
c3dgs_contrib_accumulate) and what is built on them (settings.contrib, GaussianModel.render(return_contrib=True),
contribution_stats, prune_by_contribution, finetune(prune_min_views=...)).

On every scene of tests/depth_ref.py and on tests/error_ref.py's `long_run`:
  1. against the float64 walk of tests/contrib_ref.py: a Gaussian is exempt if its `hits` differs from the walk's, at most
     max(2, 2e-5 P) are (tests/test_contrib_ref_cpu.py: the reference side needs none); every other row has equal hits and
     weight_sum, weight_max within 1e-4 relative (the project's gradient bar; about 9x the spread between the walk and an
     fp32 evaluation with the kernel's exponent rounding, 1.15e-5, which leaves room for the fp32 summation). Rows with
     radii == 0 are exact zeros.
  2. against the product backward: the same scene with colors_precomp and an all-ones image gradient; dL_dcolors[:, 0] equals
     weight_sum to rel-inf 1e-4 (1e-3 on `deep` and `huge_faint`: the bar DESIGN.md section 2 gives deep lists, where the backward
     rebuilds T by divisions).
  3. conservation, in float64: sum_g weight_sum = sum_pix (1 - final_T) within 1e-5 relative; hits.sum() > 0;
     weight_max <= 0.99; weight_max <= weight_sum.
  4. all three outputs bit-identical on a second call and after hip_backward on the same buffers; the backward's gradients after
     a render_contrib call are bit-identical to those of a forward that never saw one (of an indexed scene the three
     codebook gradients, scatter-added with float atomics, to rel-inf 1e-4 as in tests/test_raster_gpu.py); a NULL output leaves the other two unchanged; a guard element behind every [P] output and
     a guard region behind the workspace stay intact.
Then empty inputs, the sort time-out, c3dgs_contrib_accumulate, the Python layer and pruning."""
import ctypes as C
import functools
import os
import random
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


def _render_contrib(fw, want=(True, True, True)):
    """c3dgs_render_contrib on the buffers of forward `fw` into three int32-viewed [P + 1] buffers pre-filled with GUARD_BITS
    (element P: the guard) and a workspace of exactly c3dgs_contrib_workspace_bytes followed by a guard region.
    -> list of uint32 numpy [P + 1] (None where the output was passed as NULL)."""
    from c3dgs_amd import _lib
    L = _lib.lib()
    P, W, H, R = int(fw["radii"].numel()), fw["W"], fw["H"], fw["num_rendered"]
    fill = int(np.uint32(GUARD_BITS).view(np.int32))
    bufs = [torch.full((P + 1,), fill, dtype=torch.int32, device="cuda") if w else None for w in want]
    nbytes = int(L.c3dgs_contrib_workspace_bytes(P, R))
    ws = torch.full((nbytes + WS_GUARD,), 0xA5, dtype=torch.uint8, device="cuda")
    assert ws.data_ptr() % 256 == 0
    ptr = lambda t: t.data_ptr() if t is not None and t.numel() else None      # noqa: E731
    rc = L.c3dgs_render_contrib(P, W, H, R, ptr(fw["geom"]), ptr(fw["binning"]), ptr(fw["img"]), ws.data_ptr(),
                                *[ptr(b) for b in bufs], C.c_void_p(torch.cuda.current_stream().cuda_stream))
    _lib.check(rc)
    torch.cuda.synchronize()
    assert bool((ws[nbytes:] == 0xA5).all()), "the guard region behind the workspace was written"
    return [None if b is None else b.cpu().numpy().view(np.uint32) for b in bufs]


def _stats(fw):
    """-> (weight_sum f32 [P], weight_max f32 [P], hits u32 [P]); the guards are checked"""
    out = _render_contrib(fw)
    for b in out:
        assert b[-1] == GUARD_BITS, "the guard element behind an output was written"
    return out[0][:-1].view(np.float32), out[1][:-1].view(np.float32), out[2][:-1]


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def _scene(name):
    """-> (inputs, cam, indexed); computed once per process, not to be modified."""
    return error_ref.long_run_scene() if name == "long_run" else depth_ref.scene(name)


@functools.lru_cache(maxsize=None)
def _reference(name):
    st = error_ref.long_run_state() if name == "long_run" else depth_ref.oracle_state(name)
    return contrib_ref.walk(st, st.W, st.H)


def check_against_walk(name, u, wsum, wmax, hits, ref=None):
    """the three rows of scene `name` (its forward unpacked: `u`) against the float64 walk (`ref`: contrib_ref.walk of another
    scene's oracle state): point 1 of the module's list, shared with tests/test_scratch_poison_gpu.py and
    tests/test_call_sequence_gpu.py"""
    P = int(u["radii"].size)
    ref = _reference(name) if ref is None else ref
    exempt, rel_sum, rel_max = contrib_ref.compare(wsum, wmax, hits, ref, name + " GPU vs float64 walk:")
    assert exempt <= contrib_ref.exemption_cap(P)
    assert rel_sum <= 1e-4 and rel_max <= 1e-4
    dead = u["radii"] == 0
    assert (_bits(wsum)[dead] == 0).all() and (_bits(wmax)[dead] == 0).all() and (hits[dead] == 0).all()
    never = hits == 0
    assert (_bits(wsum)[never] == 0).all() and (_bits(wmax)[never] == 0).all()


@pytest.mark.parametrize("name", list(depth_ref.SCENES) + ["long_run"])
def test_statistics_replay_the_forward(hip, orc, name):
    """Measured on an MI355X, over the seven scenes of tests/depth_ref.py: 0 Gaussians exempt; largest relative difference against
    the walk 1.15e-5 for weight_sum (`needles_long`; 2.5e-6 on `huge_faint`, 1.5e-6 on `deep`) and 4.3e-6 for weight_max;
    weight_sum against dL_dcolors[:, 0] of the product backward rel-inf 6.2e-7 at most (`huge_faint`; 5.7e-7 on `deep`, 1.2e-7
    elsewhere); conservation within 8.7e-9. `long_run` (tests/error_ref.py: the one scene with a blended Gaussian over more than
    256 slots, i.e. two trips of stage B's whole-wave fold) puts weight_max and hits through that fold: 0 of 301 exempt, 2.8e-7 and 2.6e-7 against
    the walk, 1.1e-9 against the product backward.
    The test prints each figure before it asserts."""
    inp, cam, indexed = _scene(name)
    W, H = cam["W"], cam["H"]
    fw = gpu_util.hip_forward(inp, cam, indexed)
    u = gpu_util.unpack(fw)
    P = int(fw["radii"].numel())
    assert fw["num_rendered"] > 0
    wsum, wmax, hits = _stats(fw)
    assert np.isfinite(wsum).all() and np.isfinite(wmax).all()
    if name in ("indexed", "odd_size", "huge_faint", "deep"):
        assert (hits[256:] > 0).any(), "no blended Gaussian beyond the first 256-Gaussian scan group"
    if name == "long_run":
        assert ((u["tiles_touched"] > 256) & (hits > 0)).any(), "no blended Gaussian whose run takes two trips of the whole-wave fold"

    # 1. against the float64 walk
    check_against_walk(name, u, wsum, wmax, hits)

    # 2. against the product backward: dL_dcolors of an all-ones image gradient
    g = torch.Generator().manual_seed(5)
    inp_c = dict(inp)
    inp_c.update(shs=None, sh_indices=None, colors_precomp=torch.rand(P, 3, generator=g).float(), bg=torch.zeros(3))
    fc = gpu_util.hip_forward(inp_c, cam, indexed)
    np.testing.assert_array_equal(gpu_util.unpack(fc)["n_contrib"], u["n_contrib"])          # the colours change no decision
    gc = gpu_util.hip_backward(fc, np.ones((3, H, W), np.float32))
    err = gpu_util.rel_inf(wsum, gc["dL_dcolors"][:, 0])
    print(name, "weight_sum vs dL_dcolors[:, 0] of the product backward: rel-inf %.3g" % err)
    assert err <= (1e-3 if name in ("deep", "huge_faint") else 1e-4)

    # 3. conservation
    total, blended = float(wsum.astype(np.float64).sum()), float((1.0 - u["final_T"].astype(np.float64)).sum())
    print(name, "sum of weight_sum %.9g, sum of 1 - final_T %.9g, relative difference %.3g" % (total, blended, abs(total - blended) / blended))
    assert abs(total - blended) <= 1e-5 * blended
    assert int(hits.astype(np.int64).sum()) > 0
    assert wmax.max() <= np.float32(0.99) and (wmax <= wsum).all()      # 0.99: the alpha cap, an fp32 constant (w = alpha T, T <= 1)

    # 4. reproducible; independent of the backward, and the backward of it
    grad = synth.grad_image(W, H).numpy()
    g_plain = gpu_util.hip_backward(gpu_util.hip_forward(inp, cam, indexed), grad)             # a forward that never saw render_contrib
    for a, b in zip((wsum, wmax, hits), _stats(fw)):
        np.testing.assert_array_equal(_bits(a), _bits(b))
    g_after = gpu_util.hip_backward(fw, grad)
    for k in g_plain:
        if indexed and k in SCATTERED:                          # the order of the atomic adds is not fixed
            assert gpu_util.rel_inf(g_after[k], g_plain[k]) <= GRAD_TOL, k
        else:
            np.testing.assert_array_equal(_bits(g_plain[k]), _bits(g_after[k]), err_msg=k)
    for a, b in zip((wsum, wmax, hits), _stats(fw)):
        np.testing.assert_array_equal(_bits(a), _bits(b))
    for k in range(3):                                         # NULL outputs: the other two unchanged, guards intact
        out = _render_contrib(fw, [j != k for j in range(3)])
        assert out[k] is None
        for j in range(3):
            if j != k:
                assert out[j][-1] == GUARD_BITS
                np.testing.assert_array_equal(out[j][:-1], _bits((wsum, wmax, hits)[j]))


@pytest.mark.parametrize("name", ["empty", "all_behind"])
def test_nothing_to_blend_gives_exact_zeros(hip, name):
    inp, cam, indexed = cases.make_case(name)
    fw = gpu_util.hip_forward(inp, cam, indexed)
    P = int(fw["radii"].numel())
    assert fw["num_rendered"] == 0 and (P == 0) == (name == "empty")
    for m in _stats(fw):
        assert m.shape == (P,) and (_bits(m) == 0).all()
    for k in range(3):
        out = _render_contrib(fw, [j == k for j in range(3)])
        assert (out[k][:-1] == 0).all() and out[k][-1] == GUARD_BITS


# ---------------------------------------------------------------------------------------------------------------- accumulate
def _three_views():
    inp, _, indexed = depth_ref.scene("indexed")
    W, H, focal = 200, 136, 125.0
    evs = [(0.05, -0.03, 0.02, 0.99, 0.1, -0.05, 0.2), (0.0, 0.0, 0.0, 1.0, -0.3, 0.1, 0.0), (-0.04, 0.06, 0.0, 0.99, 0.2, 0.2, -0.4)]
    return inp, indexed, W, H, [cases._cam(W, H, focal, ev) for ev in evs]


def test_contrib_accumulate_against_numpy(hip):
    from c3dgs_amd import _lib, rasterizer as rz
    L = _lib.lib()
    inp, indexed, W, H, cams = _three_views()
    P = int(inp["means3D"].shape[0])
    stream = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    views = []
    for cam, _, _ in cams:
        fw = gpu_util.hip_forward(inp, cam, indexed)
        views.append(rz._C.render_contrib(P, W, H, fw["num_rendered"], fw["geom"], fw["binning"], fw["img"]))
    assert all(int((v[2] > 0).sum()) > 100 for v in views)
    g = torch.Generator().manual_seed(9)
    for mapped in (False, True):
        acc = [torch.zeros(P, dtype=torch.float32, device="cuda"), torch.zeros(P, dtype=torch.float32, device="cuda"),
               torch.zeros(P, dtype=torch.int64, device="cuda"), torch.zeros(P, dtype=torch.int32, device="cuda")]
        want = [np.zeros(P, np.float32), np.zeros(P, np.float32), np.zeros(P, np.int64), np.zeros(P, np.uint32)]
        for ws, wm, h in views:
            if mapped:       # a model of P rows of which a random 70 % are "visible": the view's rows are those, in order
                vis = torch.rand(P, generator=g) < 0.7
                rows = vis.nonzero().squeeze(1)
                rank = (torch.cumsum(vis.to(torch.int32), 0) - vis.to(torch.int32)).to(torch.int32)
                s, m, hh = (t[rows.cuda()].contiguous() for t in (ws, wm, h))
                visible, rank_d = vis.to(torch.uint8).cuda(), rank.cuda()
                rc = L.c3dgs_contrib_accumulate(P, int(rows.numel()), visible.data_ptr(), rank_d.data_ptr(), s.data_ptr(), m.data_ptr(),
                                                hh.data_ptr(), *[a.data_ptr() for a in acc], stream)
                sel = vis.numpy()
            else:
                s, m, hh = ws, wm, h
                rc = L.c3dgs_contrib_accumulate(P, P, None, None, s.data_ptr(), m.data_ptr(), hh.data_ptr(), *[a.data_ptr() for a in acc], stream)
                sel = np.ones(P, bool)
            _lib.check(rc)
            sn, mn, hn = s.cpu().numpy(), m.cpu().numpy(), hh.cpu().numpy().view(np.uint32)
            want[0][sel] = want[0][sel] + sn                    # one fp32 add per view, in view order
            want[1][sel] = np.maximum(want[1][sel], mn)
            want[2][sel] += hn.astype(np.int64)
            want[3][sel] += (hn > 0).astype(np.uint32)
        torch.cuda.synchronize()
        got = [a.cpu().numpy() for a in acc]
        np.testing.assert_array_equal(_bits(got[0]), _bits(want[0]))
        np.testing.assert_array_equal(_bits(got[1]), _bits(want[1]))
        np.testing.assert_array_equal(got[2], want[2])
        np.testing.assert_array_equal(got[3].view(np.uint32), want[3])
        assert want[3].max() == 3 and want[3].min() == 0
    # NaN rows of a timed-out view propagate
    nan = torch.full((4,), float("nan"), device="cuda")
    acc = [torch.ones(4, device="cuda"), torch.ones(4, device="cuda"), torch.zeros(4, dtype=torch.int64, device="cuda"),
           torch.zeros(4, dtype=torch.int32, device="cuda")]
    _lib.check(L.c3dgs_contrib_accumulate(4, 4, None, None, nan.data_ptr(), nan.data_ptr(), torch.zeros(4, dtype=torch.int32, device="cuda").data_ptr(),
                                          *[a.data_ptr() for a in acc], stream))
    torch.cuda.synchronize()
    assert torch.isnan(acc[0]).all() and torch.isnan(acc[1]).all() and int(acc[2].sum()) == 0 and int(acc[3].sum()) == 0


# ---------------------------------------------------------------------------------------------------------------- Python layer
def _settings(hip, intr, ev, **kw):
    return hip.GaussianRasterizationSettings(intrinsic=intr.cuda(), extrinsic_vector=ev.cuda(), bg=torch.tensor((0.2, 0.4, 0.1), device="cuda"),
                                             scale_modifier=1.0, sh_degree=3, prefiltered=False, debug=False, clamp_color=True, **kw)


@pytest.mark.parametrize("indexed", [False, True])
def test_settings_contrib_through_the_autograd_functions(hip, indexed, monkeypatch):
    from c3dgs_amd import rasterizer as rz
    P, W, H, focal = 1500, 75, 50, 60.0
    intr, ev = synth.camera(W, H, focal, extrinsic_vector=(0.05, -0.03, 0.02, 0.99, 0.1, -0.05, 0.2))
    sc = synth.scene(P, W, H, focal, seed=17, scale_median=0.08)
    names = ("means3D", "opacities", "shs", "scales", "rotations") + (("scale_factors",) if indexed else ())
    if indexed:
        sc = synth.index_scene(sc, shs_extra=32, gs_extra=32)
    assert _settings(hip, intr, ev).contrib is False and _settings(hip, intr, ev, contrib=True).contrib is True

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
    assert len(plain) == 2                                      # contrib=False: exactly what there was
    only, g1 = run(lambda o: o[0].sum() + o[2].sum() + o[3].sum(), contrib=True)
    assert len(only) == 5
    R, _, _, geom, binning, img = seen[-1]
    want = rz._C.render_contrib(P, W, H, R, geom, binning, img)
    both, g2 = run(lambda o: o[0].sum() + o[5].sum(), depth=True, contrib=True)
    assert len(both) == 8
    want_depth = rz._C.render_depth(P, W, H, *[seen[-1][k] for k in (0, 3, 4, 5)])
    for got in (only[2:], both[5:]):
        for t, w, dt in zip(got, want, (torch.float32, torch.float32, torch.int32)):
            assert t.shape == (P,) and t.dtype == dt and not t.requires_grad
            assert torch.equal(t.view(torch.int32), w.view(torch.int32))
    for t, w in zip(both[2:5], want_depth):
        assert t.shape == (H, W) and torch.equal(t.view(torch.int32), w.view(torch.int32))
    assert int((only[4] > 0).sum()) > 100 and float(only[3].max()) <= depth_ref.A_MAX
    for out in (only, both):
        assert torch.equal(out[0].view(torch.int32), plain[0].view(torch.int32)) and torch.equal(out[1], plain[1])
    # no gradient through the extras: the parameter gradients are those of image.sum() alone
    for gx in (g1, g2):
        for k in g0:
            assert torch.equal(g0[k].view(torch.int32), gx[k].view(torch.int32)) or \
                (indexed and torch.allclose(g0[k], gx[k], rtol=1e-5, atol=1e-6 * float(g0[k].abs().max()))), k


class _Cam:
    def __init__(self, intrinsic, ev):
        self.intrinsic, self.extrinsic_vector = intrinsic.cuda(), ev.cuda()
        self.original_image = None


def _model(hip, path, P=2000, W=90, H=60, focal=80.0, quantization=True, behind_fraction=0.0):
    from c3dgs_amd.model import GaussianModel
    sc = synth.scene(P, W=W, H=H, focal=focal, seed=23, scale_median=0.06, behind_fraction=behind_fraction)
    m = GaussianModel(3, quantization=quantization, device="cuda")
    if path == "fused_indexed":
        m.set_tensors(**synth.raw_params(synth.index_scene(sc, seed=24, shs_extra=32, gs_extra=32)))
    else:
        op = sc["opacities"].clamp(1e-6, 1 - 1e-6)
        m.set_tensors(xyz=sc["means3D"], features_dc=sc["shs"][:, :1], features_rest=sc["shs"][:, 1:],
                      scaling=sc["scales"] / sc["scales"].norm(dim=1, keepdim=True), rotation=sc["rotations"],
                      opacity=torch.log(op / (1 - op)), scaling_factor=torch.log(sc["scales"].norm(dim=1, keepdim=True)))
    return m


_EVS = [(0, 0, 0, 1, 0, 0, 0), (0.02, -0.03, 0.0, 1.0, 0.4, 0.1, 0.3), (-0.03, 0.02, 0.01, 1.0, -0.5, -0.2, -0.2)]


@pytest.mark.parametrize("path,gather", [("fused_indexed", True), ("composed", True), ("composed", False)])
def test_model_render_return_contrib(hip, path, gather):
    from c3dgs_amd.model import PipelineParams
    W, H, focal = 90, 60, 80.0
    m = _model(hip, path, behind_fraction=0.2)
    P = m._xyz.shape[0]
    intr, ev = synth.camera(W, H, focal)
    cam, bg = _Cam(intr, ev), torch.zeros(3, device="cuda")
    before = m.render(cam, PipelineParams(), bg, gather_visible=gather)
    assert set(before) == {"render", "viewspace_points", "visibility_filter", "radii", "visible"}        # today's keys, exactly
    out = m.render(cam, PipelineParams(), bg, gather_visible=gather, return_contrib=True)
    keys = {"contrib_sum", "contrib_max", "contrib_hits"}
    assert set(out) == set(before) | keys | {"contrib_rank"}
    if gather:                                                  # model row -> row of the statistics, for the visible ones
        vis = out["visible"]
        assert out["contrib_rank"].dtype == torch.int32 and torch.equal(out["contrib_rank"][vis].long(), torch.arange(int(vis.sum()), device="cuda"))
    else:
        assert out["contrib_rank"] is None
    rows = out["radii"].shape[0]
    assert rows == (int(out["visible"].sum()) if gather else P)
    assert not gather or rows < P                               # a fifth of the scene lies behind the camera
    for k in keys:
        assert out[k].shape == (rows,) and not out[k].requires_grad
    assert bool((out["contrib_hits"][out["radii"] == 0] == 0).all()) and int((out["contrib_hits"] > 0).sum()) > 100
    assert bool((out["contrib_max"] <= out["contrib_sum"]).all())
    total = float(out["contrib_sum"].double().sum())
    both = m.render(cam, PipelineParams(), bg, gather_visible=gather, return_contrib=True, return_depth=True)
    assert set(both) == set(out) | {"depth", "alpha", "median_depth"}
    assert torch.equal(both["contrib_hits"], out["contrib_hits"]) and both["alpha"].shape == (H, W)
    blended = float(both["alpha"].double().sum())               # conservation once more, through the model
    assert abs(total - blended) <= 1e-5 * blended
    out["render"].sum().backward()
    assert all(p.grad is not None and torch.isfinite(p.grad).all() for p in m.parameters())


def _fold_by_hand(m, cams, bg):
    from c3dgs_amd.model import PipelineParams
    P = m._xyz.shape[0]
    ws, wm = np.zeros(P, np.float32), np.zeros(P, np.float32)
    hits, views = np.zeros(P, np.int64), np.zeros(P, np.int64)
    with torch.no_grad():
        for cam in cams:
            out = m.render(cam, PipelineParams(), bg, return_contrib=True)
            vis = out["visible"].cpu().numpy().astype(bool)
            s, x, h = (out[k].cpu().numpy() for k in ("contrib_sum", "contrib_max", "contrib_hits"))
            ws[vis] = ws[vis] + s
            wm[vis] = np.maximum(wm[vis], x)
            hits[vis] += h.view(np.uint32).astype(np.int64)
            views[vis] += h != 0
    return ws, wm, hits, views


@pytest.mark.parametrize("path", ["fused_indexed", "composed"])
def test_contribution_stats_equal_the_views_folded_by_hand(hip, path):
    from c3dgs_amd.model import PipelineParams
    W, H, focal = 90, 60, 80.0
    m = _model(hip, path, quantization=False, behind_fraction=0.2)
    cams = [_Cam(*synth.camera(W, H, focal, extrinsic_vector=ev)) for ev in _EVS]
    bg = torch.zeros(3, device="cuda")
    st = m.contribution_stats(cams, PipelineParams(), bg)
    assert set(st) == {"weight_sum", "weight_max", "hits", "views"}
    ws, wm, hits, views = _fold_by_hand(m, cams, bg)
    np.testing.assert_array_equal(_bits(st["weight_sum"].cpu().numpy()), _bits(ws))
    np.testing.assert_array_equal(_bits(st["weight_max"].cpu().numpy()), _bits(wm))
    np.testing.assert_array_equal(st["hits"].cpu().numpy(), hits)
    np.testing.assert_array_equal(st["views"].cpu().numpy().astype(np.int64), views)
    assert views.max() == 3 and views.min() == 0 and not any(t.requires_grad for t in st.values())


@pytest.mark.parametrize("path", ["fused_indexed", "composed"])
def test_contribution_stats_leave_the_observers_alone(hip, path):
    """On a quantisation-aware model every render moves the observers; the statistics pass puts their state back."""
    from c3dgs_amd.model import PipelineParams
    W, H, focal = 90, 60, 80.0
    m = _model(hip, path, quantization=True)
    cams = [_Cam(*synth.camera(W, H, focal, extrinsic_vector=ev)) for ev in _EVS]
    bg = torch.zeros(3, device="cuda")
    with torch.no_grad():
        m.render(cams[0], PipelineParams(), bg)                 # the observers have seen something
        m._opacity += 1.0                                       # ... and the next getter call would move the opacity observer
        state = m._fq_state.clone()
    st = m.contribution_stats(cams, PipelineParams(), bg)
    assert int(st["views"].max()) == 3
    assert torch.equal(m._fq_state.view(torch.int32), state.view(torch.int32))
    with torch.no_grad():
        m.render(cams[0], PipelineParams(), bg)
    assert not torch.equal(m._fq_state.view(torch.int32), state.view(torch.int32)), "a render moved no observer: nothing was protected"


# ---------------------------------------------------------------------------------------------------------------- pruning
def test_prune_by_contribution_removes_what_no_view_blends(hip, monkeypatch):
    from c3dgs_amd import _lib, rasterizer as rz
    from c3dgs_amd.model import PipelineParams
    W, H, focal = 90, 60, 80.0
    m = _model(hip, "composed", quantization=False, behind_fraction=0.2)
    cams = [_Cam(*synth.camera(W, H, focal, extrinsic_vector=ev)) for ev in _EVS]
    bg = torch.zeros(3, device="cuda")
    pipe = PipelineParams()
    attrs = ("_xyz", "_features_dc", "_features_rest", "_scaling", "_rotation", "_opacity", "_scaling_factor")
    orig = {a: getattr(m, a).detach().clone() for a in attrs}
    P = m._xyz.shape[0]
    seen = []
    real = rz._C.rasterize_gaussians

    def spy(*a):
        out = real(*a)
        seen.append(out)
        return out
    monkeypatch.setattr(rz._C, "rasterize_gaussians", spy)
    il = _lib.ImageLayout()
    _lib.lib().c3dgs_get_image_layout(W, H, C.byref(il))
    before = []
    with torch.no_grad():
        for cam in cams:
            out = m.render(cam, pipe, bg)
            _, color, radii, geom, _, img = seen[-1]            # the buffers of that very forward
            assert torch.equal(color.view(torch.int32), out["render"].view(torch.int32))
            V = int(radii.numel())
            gl = _lib.GeomLayout()
            _lib.lib().c3dgs_get_geom_layout(V, C.byref(gl))
            splat = gpu_util._view(geom, gl.splat, 12 * V, torch.float32).view(V, 12)
            cmax = float(splat[radii > 0][:, 6:9].max())         # the largest colour component the forward stored
            final_T = gpu_util._view(img, il.final_T, W * H, torch.float32).view(H, W).clone()
            before.append((out["render"].clone(), final_T, cmax))
    stats = m.contribution_stats(cams, pipe, bg)
    unseen = stats["views"] == 0
    n_unseen = int(unseen.sum())
    assert 0 < n_unseen < P
    assert m.prune_by_contribution(stats) == n_unseen
    keep = (~unseen).nonzero().squeeze(1)
    assert m._xyz.shape[0] == P - n_unseen
    for a in attrs:
        assert torch.equal(getattr(m, a).detach().view(torch.int32), orig[a][keep].view(torch.int32)), a
    with torch.no_grad():
        for cam, (img0, final_T, cmax) in zip(cams, before):
            img1 = m.render(cam, pipe, bg)["render"]
            bound = final_T * max(1.0, cmax) + 1e-6
            worst = float(((img1 - img0).abs() - bound[None]).max())
            print("re-render after pruning: largest |difference| %.3g, largest excess over the bound %.3g" % (float((img1 - img0).abs().max()), worst))
            assert worst <= 0
    # a threshold on the largest weight takes more; nothing to remove -> 0
    stats2 = m.contribution_stats(cams, pipe, bg)
    assert int((stats2["views"] == 0).sum()) == 0 and m.prune_by_contribution(stats2) == 0
    assert m.prune_by_contribution(stats2, min_weight_max=0.05) == int((stats2["weight_max"] < 0.05).sum()) > 0


def _mean_loss(student, cams, bg):
    from c3dgs_amd import loss as _loss
    from c3dgs_amd.model import PipelineParams
    with torch.no_grad():
        return float(torch.stack([_loss.l1_ssim_loss(student.render(c, PipelineParams(), bg)["render"], c.original_image, 0.2)
                                  for c in cams]).mean())


def test_finetune_prunes_by_contribution(hip, tmp_path):
    from c3dgs_amd import pipeline
    from c3dgs_amd.model import PipelineParams
    from tests import train_scene
    student, cams, _ = train_scene.make(tmp_path, "cuda")
    P0 = student._xyz.shape[0]
    bg = torch.zeros(3, device="cuda")
    # As the scene comes, every one of its 500 Gaussians is blended by some of the 8 views (measured: 500 -> 500, nothing to
    # remove). So, like the `forced` opacities of tests/test_index_prune_gpu.py's driver test, a few are put where no training
    # view can blend them: behind every camera.
    forced = torch.arange(P0)[::max(1, P0 // 7)][:7].to("cuda")
    with torch.no_grad():
        student._xyz[forced, 2] = -5.0
    st0 = student.contribution_stats(cams, PipelineParams(), bg)
    n_unseen = int((st0["views"] == 0).sum())
    assert bool((st0["views"][forced] == 0).all()) and forced.numel() <= n_unseen < P0 // 2
    loss0 = _mean_loss(student, cams, bg)
    events = []

    class Scene:
        gaussians = student

        def getTrainCameras(self):
            return cams

    random.seed(3)
    torch.manual_seed(0)
    ema = pipeline.finetune(Scene(), pipeline._Dataset(), pipeline.OptimizationParams(), pipeline.CompressionParams(finetune_iterations=30),
                            PipelineParams(), log=lambda it, e: events.append((it, e, student._xyz.shape[0])), prune_interval=5,
                            prune_min_views=1)
    loss1 = _mean_loss(student, cams, bg)
    print("finetune(prune_interval=5, prune_min_views=1): Gaussians", P0, "->", student._xyz.shape[0], "; mean loss %.5f -> %.5f" % (loss0, loss1), events)
    assert np.isfinite(ema) and student._xyz.shape[0] < P0
    assert [e[0] for e in events] == [5, 10, 10, 15, 20, 20, 25, 30]                # a log call after every prune
    assert events[0][2] <= P0 - forced.numel() and all(b[2] <= a[2] for a, b in zip(events, events[1:]))
    assert loss1 < loss0
    # what is left is blended by some training view
    st = student.contribution_stats(cams, PipelineParams(), bg)
    assert st["views"].shape[0] == student._xyz.shape[0] and bool((student._xyz[:, 2] > 0).all())


# ---------------------------------------------------------------------------------------------------------------- sort time-out
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
ws, wm, hits = rz._C.render_contrib(int(fw["radii"].numel()), 640, 360, fw["num_rendered"], fw["geom"], fw["binning"], fw["img"])
torch.cuda.synchronize()
assert ws.shape == (400_000,) and torch.isnan(ws).all() and torch.isnan(wm).all(), "statistics of a forward whose sort timed out must be NaN"
assert int((hits != 0).sum()) == 0
print("NAN_ROWS")
"""


def test_sort_timeout_gives_nan_rows():
    """With the `spin1` variant of the library, started the way tests/test_render_depth_gpu.py::test_sort_timeout_gives_nan_maps
    starts its child: the forward's image is NaN, weight_sum and weight_max are NaN, hits are 0."""
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    lib = os.path.join(root, "c3dgs_amd", "libc3dgs_hip_spin1.so")
    if not os.path.exists(lib):
        from c3dgs_amd import build
        build.build_variant("spin1")
    r = subprocess.run([sys.executable, "-c", _TIMEOUT_CHILD], cwd=root, env=dict(os.environ, C3DGS_LIB_PATH=lib),
                       capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    assert "NAN_ROWS" in r.stdout, r.stdout
