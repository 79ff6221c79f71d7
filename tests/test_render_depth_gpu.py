"""-m gpu: depth, accumulated opacity and median depth of a finished forward (csrc/render_depth.hip, c3dgs_render_depth).

The kernel replays the forward's blend over the tile's compact list; it decides nothing again. So two of its three maps have an
exact yardstick in the product forward itself, and are held to it BIT FOR BIT, with no exemption:
  1. depth: the same scene rendered a second time by the product forward with colors_precomp[i] = (z_i, z_i, z_i) and a black
     background, z_i = the depth the first forward stored; `depth` must equal channel 0 of that image as uint32 patterns on
     every pixel. That image in turn is held to oracle.rasterize_forward of the depth-coloured scene at the repository's image
     bar scaled by the largest visible depth: |a - b| <= zmax 2e-5 + 1e-4 |b|, at most max(2, 2e-5 x pixels) pixels excepted.
  2. alpha: == float32(1) - final_T as uint32 patterns, final_T from the forward's image buffer.
  3. median: against the float64 walk of tests/depth_ref.py. With u = 2^-24 and n = n_contrib[pix] the kernel's T differs from
     the float64 one by at most band = 4 (n + 1) u relative (two roundings per blended entry in T, alpha within 3 u). The value
     must be bit-equal to the depth of a blended entry between the first with T64 < 0.5 (1 + band) and the first with
     T64 < 0.5 (1 - band), inclusive; 0 exactly when the second does not exist and no entry lies in between; where only the first
     exists, 0 or any entry from it on. Pixels where the HIP forward and the oracle disagree on n_contrib are skipped, and their
     number is asserted to be within max(2, 2e-5 x pixels) (tests/test_depth_ref_cpu.py: the reference side alone meets that).
  4. bitwise reproducible, and the same bits after hip_backward has run on the same buffers.
  5. a NULL output leaves the other two unchanged; a guard row behind every [H, W] buffer stays intact.
  6. P = 0 and R = 0: exact zeros.
Then the Python layer (settings.depth, GaussianModel.render(return_depth=True)) and the sort time-out (NaN maps)."""
import ctypes as C
import functools
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from tests import cases, depth_ref, gpu_util, synth

pytestmark = pytest.mark.gpu

GUARD = float(np.float32(-7.25))           # what the buffers and their guard rows hold before a call


def _render_depth(fw, want=(True, True, True)):
    """c3dgs_render_depth on the buffers of forward `fw`, into three [(H + 1), W] buffers pre-filled with GUARD (row H: the guard).
    -> list of numpy [(H + 1), W] (None where the output was passed as NULL)."""
    from c3dgs_amd import _lib
    W, H = fw["W"], fw["H"]
    bufs = [torch.full((H + 1, W), GUARD, dtype=torch.float32, device="cuda") if w else None for w in want]
    ptr = lambda t: t.data_ptr() if t is not None and t.numel() else None      # noqa: E731
    rc = _lib.lib().c3dgs_render_depth(int(fw["radii"].numel()), W, H, fw["num_rendered"], ptr(fw["geom"]), ptr(fw["binning"]),
                                       ptr(fw["img"]), *[ptr(b) for b in bufs], C.c_void_p(torch.cuda.current_stream().cuda_stream))
    _lib.check(rc)
    torch.cuda.synchronize()
    return [None if b is None else b.cpu().numpy() for b in bufs]


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def _maps(fw):
    out = _render_depth(fw)
    H = fw["H"]
    for b in out:
        assert (b[H] == np.float32(GUARD)).all(), "the guard row behind an output was written"
    return [b[:H] for b in out]


def _depth_coloured(inp, z):
    d = dict(inp)
    d.update(shs=None, sh_indices=None, colors_precomp=torch.from_numpy(np.repeat(z[:, None], 3, 1).copy()), bg=torch.zeros(3))
    return d


@functools.lru_cache(maxsize=None)
def _median_reference(name):
    st = depth_ref.oracle_state(name)
    return depth_ref.walk(st, st.W, st.H)


def check_maps(name, inp, cam, indexed, st, u, depth, alpha, median, walk=None):
    """points 1 to 3 of the module's list for the three maps of scene `name` (its forward unpacked: `u`, its oracle state: `st`;
    `walk`: depth_ref.walk of `st` where the scene is not one of depth_ref.SCENES); shared with tests/test_scratch_poison_gpu.py
    and tests/test_call_sequence_gpu.py"""
    W, H = cam["W"], cam["H"]
    # 1. depth == the product forward's image of the depth-coloured scene, bit for bit
    z = u["depths"].copy()
    z[~np.isfinite(z)] = 0.0                                # culled rows hold 0xFFFFFFFF
    inp_z = _depth_coloured(inp, z)
    fz = gpu_util.hip_forward(inp_z, cam, indexed)
    uz = gpu_util.unpack(fz)
    np.testing.assert_array_equal(uz["n_contrib"], u["n_contrib"])          # the colours change no decision
    np.testing.assert_array_equal(_bits(depth), _bits(uz["out_color"][0]))
    vis = u["radii"] > 0
    zmax = float(z[vis].max())
    assert 0.2 < zmax < 1e4
    stz = cases.oracle_forward(inp_z, cam)
    a, b = uz["out_color"], stz.out_color
    bad = (np.abs(a - b) > zmax * 2e-5 + 1e-4 * np.abs(b)).any(0)
    print(name, "depth image vs oracle: pixels over the bar", int(bad.sum()), "largest difference", float(np.abs(a - b).max()), "zmax", zmax)
    assert bad.sum() <= depth_ref.exemption_cap(W * H)
    assert depth.max() > 0

    # 2. alpha == 1 - final_T, bit for bit
    np.testing.assert_array_equal(_bits(alpha).reshape(-1), _bits(np.float32(1.0) - u["final_T"]))

    # 3. median against the float64 walk
    ref = _median_reference(name) if walk is None else walk
    n_hip = u["n_contrib"].astype(np.int64)
    skip = n_hip != st.n_contrib.astype(np.int64)
    print(name, "pixels skipped (HIP forward and oracle disagree on n_contrib):", int(skip.sum()))
    assert skip.sum() <= depth_ref.exemption_cap(W * H)
    med = median.reshape(-1)
    med_bits = _bits(med)
    wrong, nonzero, banded = [], 0, 0
    for p in np.nonzero(~skip)[0]:
        T64, zs = ref.pixel(p)
        cand, zero_ok = depth_ref.median_candidates(T64, zs, int(n_hip[p]))
        banded += int(cand.size > 1 or (cand.size == 1 and zero_ok))
        ok = (zero_ok and med_bits[p] == 0) or bool((_bits(cand) == med_bits[p]).any())
        nonzero += int(med_bits[p] != 0)
        if not ok:
            wrong.append((int(p), float(med[p]), cand.tolist(), zero_ok))
    print(name, "median: pixels with a crossing", nonzero, "of", int((~skip).sum()), "; with more than one admissible answer", banded)
    assert not wrong, (len(wrong), wrong[:5])
    assert nonzero > 0                                      # T crosses 0.5 somewhere


@pytest.mark.parametrize("name", depth_ref.SCENES)
def test_maps_replay_the_forward(hip, orc, name):
    inp, cam, indexed = depth_ref.scene(name)
    W, H = cam["W"], cam["H"]
    st = depth_ref.oracle_state(name)
    fw = gpu_util.hip_forward(inp, cam, indexed)
    u = gpu_util.unpack(fw)
    assert fw["num_rendered"] > 0
    depth, alpha, median = _maps(fw)
    assert np.isfinite(depth).all() and np.isfinite(alpha).all() and np.isfinite(median).all()

    if name == "deep":                                      # more than two staged batches of compact entries, per tile and per pixel
        from tests.test_compact_lists_gpu import _compact
        c = _compact(fw, u)
        assert c["tile_used_c"].max() > 2 * 256 + 1 and c["n_contrib_c"].max() > 512, (c["tile_used_c"].max(), c["n_contrib_c"].max())
    if name == "huge_faint":                                # compact index != list position: whole batches of dead entries
        from tests.test_compact_lists_gpu import _compact
        c = _compact(fw, u)
        assert (u["n_contrib"].astype(np.int64) - c["n_contrib_c"]).max() >= 512

    check_maps(name, inp, cam, indexed, st, u, depth, alpha, median)

    # 4. reproducible, and independent of the backward
    again = _maps(fw)
    for x, y in zip((depth, alpha, median), again):
        np.testing.assert_array_equal(_bits(x), _bits(y))
    gpu_util.hip_backward(fw, synth.grad_image(W, H).numpy())
    after = _maps(fw)
    for x, y in zip((depth, alpha, median), after):
        np.testing.assert_array_equal(_bits(x), _bits(y))

    # 5. NULL outputs: the other two unchanged, guard rows intact
    for k in range(3):
        want = [j != k for j in range(3)]
        out = _render_depth(fw, want)
        assert out[k] is None
        for j in range(3):
            if j != k:
                assert (out[j][H] == np.float32(GUARD)).all()
                np.testing.assert_array_equal(_bits(out[j][:H]), _bits((depth, alpha, median)[j]))


@pytest.mark.parametrize("name", ["empty", "all_behind"])
def test_nothing_to_blend_gives_exact_zeros(hip, name):
    inp, cam, indexed = cases.make_case(name)
    fw = gpu_util.hip_forward(inp, cam, indexed)
    assert fw["num_rendered"] == 0 and (int(fw["radii"].numel()) == 0) == (name == "empty")
    for m in _maps(fw):
        assert m.shape == (cam["H"], cam["W"]) and (_bits(m) == 0).all()
    for k in range(3):
        out = _render_depth(fw, [j == k for j in range(3)])
        assert (_bits(out[k][:cam["H"]]) == 0).all() and (out[k][cam["H"]] == np.float32(GUARD)).all()


# ---------------------------------------------------------------------------------------------------------------- Python layer
def _settings(hip, intr, ev, depth):
    kw = dict(intrinsic=intr.cuda(), extrinsic_vector=ev.cuda(), bg=torch.tensor((0.2, 0.4, 0.1), device="cuda"), scale_modifier=1.0,
              sh_degree=3, prefiltered=False, debug=False, clamp_color=True)
    return hip.GaussianRasterizationSettings(**kw, depth=True) if depth else hip.GaussianRasterizationSettings(**kw)


@pytest.mark.parametrize("indexed", [False, True])
def test_settings_depth_through_the_autograd_functions(hip, indexed, monkeypatch):
    from c3dgs_amd import rasterizer as rz
    P, W, H, focal = 1500, 75, 50, 60.0
    ev_t = (0.05, -0.03, 0.02, 0.99, 0.1, -0.05, 0.2)
    intr, ev = synth.camera(W, H, focal, extrinsic_vector=ev_t)
    sc = synth.scene(P, W, H, focal, seed=17, scale_median=0.08)
    names = ("means3D", "opacities", "shs", "scales", "rotations") + (("scale_factors",) if indexed else ())
    if indexed:
        sc = synth.index_scene(sc, shs_extra=32, gs_extra=32)
    assert hip.GaussianRasterizationSettings._fields[-1] == "depth" and _settings(hip, intr, ev, False).depth is False

    seen = []
    entry = "rasterize_gaussians_indexed" if indexed else "rasterize_gaussians"
    real = getattr(rz._C, entry)

    def spy(*a):
        out = real(*a)
        seen.append(out)
        return out
    monkeypatch.setattr(rz._C, entry, spy)

    def run(depth, loss):
        leaves = {k: sc[k].cuda().requires_grad_() for k in names}
        means2D = torch.zeros_like(leaves["means3D"], requires_grad=True)
        rs = _settings(hip, intr, ev, depth)
        if indexed:
            rast = hip.GaussianRasterizerIndexed(rs)
            out = rast(means3D=leaves["means3D"], means2D=means2D, opacities=leaves["opacities"], sh_indices=sc["sh_indices"].cuda(),
                       g_indices=sc["g_indices"].cuda(), shs=leaves["shs"], scales=leaves["scales"],
                       scale_factors=leaves["scale_factors"], rotations=leaves["rotations"], extrinsic_vector=ev.cuda())
        else:
            rast = hip.GaussianRasterizer(rs)
            out = rast(means3D=leaves["means3D"], means2D=means2D, opacities=leaves["opacities"], shs=leaves["shs"],
                       scales=leaves["scales"], rotations=leaves["rotations"], extrinsic_vector=ev.cuda())
        loss(out).backward()
        torch.cuda.synchronize()
        return out, {k: v.grad.clone() for k, v in leaves.items()}, means2D.grad.clone()

    plain, g0, s0 = run(False, lambda o: o[0].sum())
    assert len(plain) == 2
    full, g1, s1 = run(True, lambda o: o[0].sum() + o[2].sum() + o[3].sum() + o[4].sum())
    assert len(full) == 5
    image, radii, depth, alpha, median = full
    assert torch.equal(image.view(torch.int32), plain[0].view(torch.int32)) and torch.equal(radii, plain[1])
    for t in (depth, alpha, median):
        assert t.shape == (H, W) and t.dtype == torch.float32 and not t.requires_grad
    assert float(alpha.max()) > 0.5 and float(depth.max()) > 0 and float(median.max()) > 0
    # the extras are what _C.render_depth gives on the buffers of that very forward
    R, _, radii_c, geom, binning, img = seen[-1]
    want = rz._C.render_depth(P, W, H, R, geom, binning, img)
    for got, w in zip((depth, alpha, median), want):
        assert torch.equal(got.view(torch.int32), w.view(torch.int32))
    # no gradient through the extras: the parameter gradients are those of image.sum() alone
    for k in g0:
        assert torch.equal(g0[k].view(torch.int32), g1[k].view(torch.int32)) or (indexed and torch.allclose(g0[k], g1[k], rtol=1e-5, atol=1e-6 * float(g0[k].abs().max()))), k
    assert torch.equal(s0, s1)


class _Cam:
    def __init__(self, intrinsic, ev):
        self.intrinsic, self.extrinsic_vector = intrinsic.cuda(), ev.cuda()


@pytest.mark.parametrize("path", ["fused_indexed", "composed"])
def test_model_render_return_depth(hip, path):
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
    before = m.render(cam, PipelineParams(), bg)
    assert set(before) == {"render", "viewspace_points", "visibility_filter", "radii", "visible"}        # today's keys, exactly
    out = m.render(cam, PipelineParams(), bg, return_depth=True)
    assert set(out) == set(before) | {"depth", "alpha", "median_depth"}
    for k in ("depth", "alpha", "median_depth"):
        assert out[k].shape == (H, W) and out[k].dtype == torch.float32 and not out[k].requires_grad and torch.isfinite(out[k]).all()
    assert float(out["alpha"].max()) > 0.5 and float(out["alpha"].min()) >= 0 and float(out["alpha"].max()) <= 1
    hit = out["alpha"] > 0.5
    assert (out["median_depth"][hit] > 0).all() and float(out["depth"].max()) > 0
    (out["render"].sum() + out["depth"].sum()).backward()
    assert all(p.grad is not None and torch.isfinite(p.grad).all() for p in m.parameters())


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
maps = rz._C.render_depth(int(fw["radii"].numel()), 640, 360, fw["num_rendered"], fw["geom"], fw["binning"], fw["img"])
torch.cuda.synchronize()
for m in maps:
    assert m.shape == (360, 640) and torch.isnan(m).all(), "a map of a forward whose sort timed out must be NaN"
print("NAN_MAPS")
"""


def test_sort_timeout_gives_nan_maps():
    """With the `spin1` variant of the library (every look-back of the sorts gives up after one poll), started the way
    tests/test_sort_gpu.py::test_sort_timeout_is_not_silent starts its child: the forward's image is NaN, and so are the maps."""
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    lib = os.path.join(root, "c3dgs_amd", "libc3dgs_hip_spin1.so")
    if not os.path.exists(lib):
        from c3dgs_amd import build
        build.build_variant("spin1")
    r = subprocess.run([sys.executable, "-c", _TIMEOUT_CHILD], cwd=root, env=dict(os.environ, C3DGS_LIB_PATH=lib),
                       capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    assert "NAN_MAPS" in r.stdout, r.stdout
