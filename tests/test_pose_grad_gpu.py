"""-m gpu: the exact camera-pose gradient (csrc/pose_grad.hip) -- the kernels alone against tests/pose_ref.py's float64
restatement on the same fp32 arrays, pose.grad end to end against float64 autograd of a render with the pose as a leaf, what
must not move, reproducibility, and pipeline.refine_poses.

Measured on an MI355X (recorded from this file's prints):
  kernels alone, max over the seven components of |diff| / sum_i |contribution_i| (bar 1e-5): see KERNEL_MEASURED below;
  end to end, rel-inf against the float64 truth (bar 1e-4): see E2E_MEASURED below;
  refine_poses, 200 passes, two cameras moved by 0.02 N(0, 1): see DRIVER_MEASURED below."""
import numpy as np
import pytest
import torch

from tests import gpu_util, pose_ref, synth

pytestmark = pytest.mark.gpu

KERNEL_MEASURED = ("p1 4.0e-7, p63 2.1e-8, p64 2.8e-8, p65 3.8e-8, p257 1.5e-8, p10753 3.1e-9, indexed 7.6e-9, cov_precomp 8.3e-9, "
                   "colors_precomp 7.1e-9, deg0 7.2e-9, deg1 1.2e-8, deg2 6.5e-9, deg3 9.7e-9, nonunit_quat 5.3e-8")
E2E_MEASURED = "tiny 1.3e-6, indexed 1.5e-6, frustum_edge 1.3e-6"
DRIVER_MEASURED = ("exact: loss last / first 0.0043, 0.0021, pose distance last / first 0.0022, 0.0045; "
                   "reference formula, same start and learning rate: loss x 3.25, x 3.27, pose distance x 9.3, x 13.8 (it diverges)")

# Stage B sweeps the workspace 42 rows at a time (1024 // 24 threads per column): 42 x 256 + 1 Gaussians are one workgroup, and
# so one row, past a single sweep -- the smallest P at which a thread of the fold adds a second row.
P_PAST_ONE_SWEEP = 42 * 256 + 1

#            name               case             overrides
KERNEL_CASES = [("p1", "base", dict(P=1)), ("p63", "base", dict(P=63)), ("p64", "base", dict(P=64)), ("p65", "base", dict(P=65)),
                ("p257", "p257", dict(P=257)), ("p10753", "base", dict(P=P_PAST_ONE_SWEEP, scale_median=0.03)),
                ("indexed", "indexed", {}), ("cov_precomp", "cov_precomp", {}), ("colors_precomp", "colors_precomp", {}),
                ("deg0", "deg0", {}), ("deg1", "deg1", {}), ("deg2", "deg2", {}), ("deg3", "base", {}),
                ("nonunit_quat", "nonunit_quat", {})]


def _dev(t, dtype=None):
    if t is None:
        return None
    t = torch.from_numpy(np.ascontiguousarray(t)) if isinstance(t, np.ndarray) else t
    return t.cuda() if dtype is None else t.to(dtype).cuda()


def _kernel_inputs(case, kw):
    """-> (inp, cam, indexed, pose, fw, bw): one HIP forward + backward of the case (nothing skipped, as _C.* does)."""
    inp, cam, indexed, pose, _ = pose_ref.make_pose_case(case, **kw)
    P = inp["means3D"].shape[0]
    if P == 1:
        inp["means3D"][0] = torch.tensor([0.1, -0.1, 4.0])          # the lone Gaussian in front of the camera
    fw = gpu_util.hip_forward(inp, cam, indexed)
    dL = synth.grad_image(cam["W"], cam["H"]).numpy()
    if P == 0:
        bw = {k: np.zeros((0, n), np.float32) for k, n in (("dL_dmeans3D", 3), ("dL_dcov3D", 6), ("dL_dcolors", 3))}
    else:
        bw = gpu_util.hip_backward(fw, dL)
    return inp, cam, indexed, pose, fw, bw


def _pose_grad(hip, inp, fw, bw, pose):
    rz = hip.rasterizer
    sh_used = inp.get("shs") is not None
    return rz._C.pose_grad(_dev(inp["means3D"]), _dev(bw["dL_dmeans3D"]), _dev(bw["dL_dcov3D"]),
                           _dev(bw["dL_dcolors"]) if sh_used else None, _dev(inp.get("shs")), int(inp["degree"]),
                           _dev(inp.get("sh_indices")), _dev(inp.get("cov3D_precomp")), _dev(inp.get("scales")),
                           _dev(inp.get("rotations")), _dev(inp.get("scale_factors")), _dev(inp.get("g_indices")),
                           float(inp["scale_modifier"]), fw["geom"], fw["radii"], _dev(pose))


@pytest.mark.parametrize("name,case,kw", KERNEL_CASES, ids=[c[0] for c in KERNEL_CASES])
def test_kernels_alone_against_float64_on_the_same_arrays(hip, name, case, kw):
    """Bar per component: |diff| <= 1e-5 x sum_i |contribution_i|. Derived: an fp32 butterfly over 256 values plus a double fold
    has an error of order log2(256) x 2^-24 = 4.8e-7 of the sum of magnitudes; 1e-5 leaves a decade (Sigma and gdir in fp32
    against float64 add a few 2^-24 of their own terms)."""
    inp, cam, indexed, pose, fw, bw = _kernel_inputs(case, kw)
    got = _pose_grad(hip, inp, fw, bw, pose).cpu().numpy().astype(np.float64)
    check_kernels_alone(name, inp, cam, pose, fw, bw, got)


def check_kernels_alone(name, inp, cam, pose, fw, bw, got):
    """the seven components `got` (float64) of the kernels on forward `fw` and backward `bw` against float64 on the same arrays, at
    the bar of test_kernels_alone_against_float64_on_the_same_arrays; shared with tests/test_scratch_poison_gpu.py"""
    u = gpu_util.unpack(fw)
    radii = u["radii"]
    assert int((radii > 0).sum()) >= 1 and np.abs(bw["dL_dmeans3D"]).max() > 0          # something was blended
    gdir = pose_ref.direction_part(inp, cam["campos"], bw["dL_dcolors"], u["clamped"], radii)
    if inp.get("shs") is not None and int(inp["degree"]) > 0:
        assert np.abs(gdir).max() > 0
    else:
        assert not gdir.any()                                                            # colors_precomp, deg0: gdir == 0
    want, contrib = pose_ref.pose_grad_ref(pose, inp["means3D"].numpy(), pose_ref.sigma_of(inp), radii, bw["dL_dmeans3D"],
                                           bw["dL_dcov3D"], gdir)
    scale = np.abs(contrib).sum(0)
    ratio = np.abs(got - want) / scale
    print(f"pose_grad kernels {name}: P {radii.size} visible {int((radii > 0).sum())} max |diff| / sum |contribution| {ratio.max():.3e}")
    assert (scale > 0).all()
    assert (ratio <= 1e-5).all(), (name, ratio, got, want)


@pytest.mark.parametrize("case", ["all_behind", "empty"])
def test_nothing_visible_gives_seven_exact_zeros(hip, case):
    inp, cam, indexed, pose, fw, bw = _kernel_inputs(case, {})
    assert int((fw["radii"] > 0).sum()) == 0
    got = _pose_grad(hip, inp, fw, bw, pose)
    assert got.shape == (7,) and got.dtype == torch.float32
    assert (got.cpu().numpy().view(np.uint32) == 0).all()                                # +0.0, all seven


def test_two_runs_give_equal_bits(hip):
    inp, cam, indexed, pose, fw, bw = _kernel_inputs("base", dict(P=P_PAST_ONE_SWEEP, scale_median=0.03))
    a = _pose_grad(hip, inp, fw, bw, pose).cpu().numpy().view(np.uint32)
    for _ in range(3):
        b = _pose_grad(hip, inp, fw, bw, pose).cpu().numpy().view(np.uint32)
        np.testing.assert_array_equal(a, b)


def test_binding_refuses_mismatched_rows(hip):
    inp, cam, indexed, pose, fw, bw = _kernel_inputs("base", dict(P=65))
    bw = dict(bw, dL_dcov3D=bw["dL_dcov3D"][:-1])
    with pytest.raises(RuntimeError, match="dL_dcov3D must have 65 x 6 elements"):
        _pose_grad(hip, inp, fw, bw, pose)


# ----------------------------------------------------------------------------- end to end through autograd
LEAF_KEYS = ("means3D", "opacities", "shs", "colors_precomp", "scales", "scale_factors", "rotations", "cov3D_precomp")


def _settings(hip, r):
    inp = r["inp"]
    return hip.GaussianRasterizationSettings(intrinsic=r["intrinsic"].cuda(), extrinsic_vector=_dev(r["pose"]), bg=inp["bg"].cuda(),
                                             scale_modifier=float(inp["scale_modifier"]), sh_degree=int(inp["degree"]),
                                             prefiltered=False, debug=False, clamp_color=bool(inp["clamp_color"]))


def _run(hip, r, optimize_camera, pose_requires_grad, model_requires_grad=True):
    """One forward + backward of sum(image * dL) through the module of the case's kind. -> (image, {name: grad}, pose grad | None)"""
    inp = r["inp"]
    rs = _settings(hip, r)
    leaves = {k: inp[k].cuda().requires_grad_(model_requires_grad) for k in LEAF_KEYS if inp.get(k) is not None}
    means2D = torch.zeros_like(leaves["means3D"], requires_grad=True)
    pose = _dev(r["pose"]).requires_grad_(pose_requires_grad)
    kw = dict(means3D=leaves["means3D"], means2D=means2D, opacities=leaves["opacities"], shs=leaves.get("shs"),
              colors_precomp=leaves.get("colors_precomp"), scales=leaves.get("scales"), rotations=leaves.get("rotations"),
              cov3D_precomp=leaves.get("cov3D_precomp"), extrinsic_vector=pose)
    if r["indexed"]:
        rast = hip.GaussianRasterizerIndexed(rs, optimize_camera=optimize_camera)
        kw.update(sh_indices=inp["sh_indices"].cuda(), g_indices=inp["g_indices"].cuda(), scale_factors=leaves.get("scale_factors"))
    else:
        rast = hip.GaussianRasterizer(rs, optimize_camera=optimize_camera) if optimize_camera else hip.GaussianRasterizer(rs)
    color, radii = rast(**kw)
    (color * _dev(r["dL"])).sum().backward()
    grads = {k: v.grad for k, v in leaves.items()}
    grads["means2D"] = means2D.grad
    return color.detach(), grads, pose.grad


@pytest.mark.parametrize("name", ["tiny", "indexed", "frustum_edge"])
def test_pose_grad_end_to_end_against_float64_autograd(hip, name):
    """`tiny` and `frustum_edge` go through GaussianRasterizer(optimize_camera="exact"), `indexed` through
    GaussianRasterizerIndexed(optimize_camera="exact"). Bar: rel-inf <= 1e-4 over the seven components. Precondition, asserted:
    the oracle (whose discrete structure the truth borrows) and the HIP forward agree on n_contrib at every pixel."""
    r = pose_ref.reference(name)
    fw = gpu_util.hip_forward(r["inp"], r["cam"], r["indexed"])
    np.testing.assert_array_equal(gpu_util.unpack(fw)["n_contrib"], r["st"].n_contrib)
    color, grads, gpose = _run(hip, r, "exact", True)
    assert gpose is not None and gpose.shape == (7,) and gpose.dtype == torch.float32
    err = gpu_util.rel_inf(gpose.cpu().numpy(), r["truth"])
    print(f"pose_grad end to end {name}: rel-inf {err:.3e} got {gpose.cpu().numpy()} truth {r['truth']}")
    assert err <= 1e-4, (name, err)


def test_indexed_module_with_precomputed_covariance_and_colours(hip):
    """The indexed entry carries sh_indices / g_indices even where colours and covariances are precomputed and nothing is
    looked up through them. Both precomputed inputs are leaves here, so autograd hands out the very dL_dcov3D and dL_dcolors the
    pass read: pose.grad against pose_grad_ref on them (gdir == 0), at the kernel test's bar."""
    base = pose_ref.reference("indexed")
    inp = dict(base["inp"])
    sg = pose_ref.sigma_of(inp)
    inp["cov3D_precomp"] = torch.from_numpy(np.stack([sg[:, 0, 0], sg[:, 0, 1], sg[:, 0, 2], sg[:, 1, 1], sg[:, 1, 2], sg[:, 2, 2]], 1)).float()
    inp["colors_precomp"] = torch.rand(sg.shape[0], 3, generator=torch.Generator().manual_seed(3))
    inp.update(shs=None, scales=None, rotations=None)
    r = dict(base, inp=inp)
    color, grads, gpose = _run(hip, r, "exact", True)
    radii = gpu_util.hip_forward(inp, r["cam"], True)["radii"].cpu().numpy()
    want, contrib = pose_ref.pose_grad_ref(r["pose"], inp["means3D"].numpy(), pose_ref.sigma_of(inp), radii,
                                           grads["means3D"].cpu().numpy(), grads["cov3D_precomp"].cpu().numpy(), np.zeros((sg.shape[0], 3)))
    ratio = np.abs(gpose.cpu().numpy() - want) / np.abs(contrib).sum(0)
    assert (ratio <= 1e-5).all(), ratio


# ----------------------------------------------------------------------------- nothing else moves
# The codebook-sized gradients of the indexed backward (shs, scales, rotations) are scatter-ADDED with fp32 atomics
# (csrc/backward_preprocess.hip): two runs of the SAME code differ in their last bits, so equality of bits between two backwards
# cannot hold for them in any mode. They are held to what tests/test_render_contrib_gpu.py holds them to between two runs;
# everything written with plain stores is compared bit for bit.
ATOMIC = ("shs", "scales", "rotations")


def _same(a, b, indexed, where):
    assert set(a) == set(b), where
    for k in a:
        if a[k] is None or b[k] is None:
            assert a[k] is None and b[k] is None, (where, k)
            continue
        if indexed and k in ATOMIC:
            assert torch.allclose(a[k], b[k], rtol=1e-5, atol=1e-6 * float(a[k].abs().max())), (where, k)
        else:
            assert torch.equal(a[k].view(torch.int32), b[k].view(torch.int32)), (where, k)


def _stage_counts(hip, fn):
    from c3dgs_amd import _lib
    torch.cuda.synchronize()
    _lib.profile_enable(True)
    _lib.profile_read()
    try:
        out = fn()
        torch.cuda.synchronize()
        st = _lib.profile_read()
    finally:
        _lib.profile_enable(False)
    return out, {k: v[1] for k, v in st.items() if v[1]}


def test_exact_mode_moves_nothing_but_the_pose_gradient(hip):
    r = pose_ref.reference("indexed")
    (img_t, g_t, p_t), n_t = _stage_counts(hip, lambda: _run(hip, r, True, True))
    (img_e, g_e, p_e), n_e = _stage_counts(hip, lambda: _run(hip, r, "exact", True))
    assert torch.equal(img_t.view(torch.int32), img_e.view(torch.int32))
    _same(g_t, g_e, True, "exact vs True")
    assert p_t is not None and p_e is not None and not torch.equal(p_t, p_e)
    # the launches: the same stages, plus pose_grad's two kernels once
    extra = {"pose_grad": 1, "pose_grad_sums": 1, "pose_grad_fold": 1}
    assert n_e == dict(n_t, **extra), (n_t, n_e)
    # `True` is still the reference's formula on the backward's dL_dmeans2D
    want = hip.rasterizer.camera_pose_jacobian_sum(r["inp"]["means3D"].cuda(), r["intrinsic"].cuda(), _dev(r["pose"]),
                                                   g_t["means2D"][:, 0], g_t["means2D"][:, 1])
    assert torch.equal(p_t.view(torch.int32), want.view(torch.int32))


@pytest.mark.parametrize("name", ["indexed", "tiny"])
def test_a_pose_that_needs_no_grad_costs_nothing(hip, name):
    r = pose_ref.reference(name)
    (img_f, g_f, p_f), n_f = _stage_counts(hip, lambda: _run(hip, r, False, False))
    (img_e, g_e, p_e), n_e = _stage_counts(hip, lambda: _run(hip, r, "exact", False))
    assert p_f is None and p_e is None
    assert torch.equal(img_f.view(torch.int32), img_e.view(torch.int32))
    _same(g_f, g_e, r["indexed"], "exact without a pose gradient vs False")
    assert n_e == n_f and "pose_grad" not in n_e, (n_f, n_e)


def test_non_indexed_default_gives_no_pose_gradient_and_true_is_refused(hip):
    r = pose_ref.reference("tiny")
    _, _, p = _run(hip, r, False, True)
    assert p is None
    with pytest.raises(ValueError, match="optimize_camera"):
        hip.GaussianRasterizer(_settings(hip, r), optimize_camera=True)
    with pytest.raises(ValueError, match="optimize_camera"):
        hip.GaussianRasterizer(_settings(hip, r), optimize_camera="exakt")


def test_frozen_model_still_gets_the_pose_gradient(hip):
    """what refine_poses does: no model tensor requires grad, only the pose"""
    r = pose_ref.reference("indexed")
    _, _, p_all = _run(hip, r, "exact", True)
    _, grads, p_frozen = _run(hip, r, "exact", True, model_requires_grad=False)
    assert all(grads[k] is None for k in grads if k != "means2D")
    assert torch.equal(p_all.view(torch.int32), p_frozen.view(torch.int32))


def test_end_to_end_two_runs_give_equal_bits(hip):
    r = pose_ref.reference("indexed")
    a = _run(hip, r, "exact", True)[2]
    b = _run(hip, r, "exact", True)[2]
    assert torch.equal(a.view(torch.int32), b.view(torch.int32))


# ----------------------------------------------------------------------------- model and driver
def test_model_render_pose_grad_modes(hip):
    from c3dgs_amd.model import PipelineParams
    model, cams, _ = pose_ref.refine_problem(noisy=())
    cam, bg = cams[2], torch.zeros(3, device="cuda")
    dL = synth.grad_image(160, 112).cuda()
    got = {}
    for mode in ("reference", "exact"):
        cam.extrinsic_vector = cam.extrinsic_vector.detach().requires_grad_(True)
        img = model.render(cam, PipelineParams(), bg, pose_grad=mode)["render"]
        (img * dL).sum().backward()
        got[mode] = (img.detach(), cam.extrinsic_vector.grad.clone())
        for t in model.parameters():
            t.grad = None
    assert torch.equal(got["reference"][0], got["exact"][0])
    assert torch.isfinite(got["exact"][1]).all() and not torch.equal(got["reference"][1], got["exact"][1])
    with pytest.raises(ValueError, match="pose_grad"):
        model.render(cam, PipelineParams(), bg, pose_grad="both")


def test_refine_poses_moves_noisy_cameras_towards_the_true_pose(hip):
    """Two of the toy scene's eight cameras start 0.02 N(0, 1) per element away from the pose their ground truth was rendered
    from; 200 passes of refine_poses (exact gradient, lr 1e-3). Each camera's last loss is below its first and its pose ends
    closer to the true one than it started. No ratio is fixed: DRIVER_MEASURED records what an MI355X gave."""
    from c3dgs_amd import pipeline
    from c3dgs_amd.model import PipelineParams
    model, cams, true = pose_ref.refine_problem()
    idx = sorted(true)
    start = {k: pose_ref.pose_distance(cams[k].extrinsic_vector, true[k]) for k in idx}
    flags = [t.requires_grad for t in model.parameters()]
    fq = model._fq_state.clone()
    logged = []
    res = pipeline.refine_poses(cams, model, PipelineParams(), torch.zeros(3, device="cuda"), 200, cameras=idx,
                                log=lambda it, losses: logged.append(it))
    assert len(res) == 2 and logged == list(range(10, 201, 10))
    assert [t.requires_grad for t in model.parameters()] == flags and all(flags)
    assert all(t.grad is None for t in model.parameters())
    assert torch.equal(model._fq_state.view(torch.int32), fq.view(torch.int32))
    for (first, last), k in zip(res, idx):
        end = pose_ref.pose_distance(cams[k].extrinsic_vector, true[k])
        print(f"refine_poses camera {k}: loss {first:.5f} -> {last:.5f} ({last / first:.3f}), pose distance {start[k]:.5f} -> {end:.5f} "
              f"({end / start[k]:.3f})")
        assert last < first, (k, first, last)
        assert end < start[k], (k, start[k], end)
    for k in range(len(cams)):                           # the other cameras were not touched
        if k not in true:
            assert not cams[k].extrinsic_vector.requires_grad
