"""-m gpu: no result may depend on what scratch and outputs hold on entry (include/c3dgs_hip.h: "the callee writes EVERY element of
every non-NULL output ... the caller may pass uninitialised memory"; DESIGN.md "Scratch contracts" lists who writes each field
first). Every family runs three times through tests/poison.py, its uninitialised allocations filled with 0x00, 0xFF (NaN, -1,
UINT_MAX, the culled depth key) and 0x7F (a large finite float, a large positive integer) between guard bands:

  * outputs the project declares run-to-run reproducible are bit-equal across the three runs (`exact`);
  * outputs that pass through float atomics (the indexed backward's codebook gradients and their like) are held to the bar their
    own test holds them to (`barred`), on every run;
  * every run that is checked against a reference uses the family's EXISTING check, imported from its test: the 0xFF run always,
    so that being equal to a wrong baseline is not enough;
  * no guard band changes.

One exemption, by contract: the geometry buffer's splat record and `clamped` byte of a CULLED Gaussian (radii == 0) are never written
and never read (every reader goes through radii > 0 or a tile list); their rows are zeroed before the comparison.
The sizes are the smallest that reach a family's branches: 63 (one ragged block), 257 (two blocks), 12,289 (one depth-sort tile
plus one item), 3 x 12,288 + 137 (three tiles with a ragged tail)."""
import functools
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from tests import cases, gpu_util, poison, synth

pytestmark = pytest.mark.gpu

TILE = 12288
SIZES = (63, 257, TILE + 1, 3 * TILE + 137)
VARIANTS = ("base", "indexed", "cov_precomp", "colors_precomp")
IMAGES = {"64x64": dict(W=64, H=64, focal=60.0), "33x17": dict(W=33, H=17, focal=30.0)}
SCALE_MEDIAN = 0.05
SCATTERED = ("dL_dsh", "dL_dscales", "dL_drotations")      # indexed backward: float atomics into the codebook gradients
CULLED_UNWRITTEN = ("means2D", "conic_opacity", "rgb", "clamped")


# ---------------------------------------------------------------------------------------------------------------- forward + backward
@functools.lru_cache(maxsize=None)
def _raster_reference(variant, P, image, route="plain"):
    """case, oracle state and oracle gradients: computed once per process, shared, not to be modified"""
    from oracle import oracle as orc
    inp, cam, indexed = cases.make_case(variant, P=P, scale_median=SCALE_MEDIAN, **IMAGES.get(image, {}))
    if route == "far":                                      # one Gaussian past the three-pass range (tests/test_depth_sort3_gpu.py)
        view = torch.from_numpy(np.asarray(cam["viewmatrix"], np.float64).reshape(4, 4))      # stored transposed: p_view = [p, 1] @ view
        p_view = torch.tensor([0.5, -0.25, 600.0], dtype=torch.float64)
        inp["means3D"][7] = ((p_view - view[3, :3]) @ torch.linalg.inv(view[:3, :3])).float()
        inp["scales"][7] = torch.tensor([2.0, 2.0, 2.0])
    if route == "prefiltered":
        inp["prefiltered"] = True
    if route == "wide":                                     # 257 tile columns: the rectangles no longer fit bytes
        # (an identity pose: make_case's would move the scene off a strip 16 pixels high)
        W, H, focal = 4112, 16, 2000.0
        intr, ev = synth.camera(W, H, focal)
        cam = orc.camera(intr.numpy(), ev.numpy())
        sc = synth.scene(P, W, H, focal, seed=7, scale_median=0.01)
        inp = dict(inp, **{k: sc[k] for k in ("means3D", "opacities", "shs", "scales", "rotations")})
    st = cases.oracle_forward(inp, cam)
    dL = synth.grad_image(cam["W"], cam["H"]).numpy()
    ref = orc.rasterize_backward(st, dL)
    return inp, cam, indexed, st, dL, ref


def _forward_outputs(fw):
    """gpu_util.unpack of a forward, the never-written rows of culled Gaussians zeroed (module docstring)"""
    u = gpu_util.unpack(fw)
    if "means2D" in u:
        culled = u["radii"] == 0
        for k in CULLED_UNWRITTEN:
            u[k][culled] = 0
    return u


def _raster_run(inp, cam, indexed, dL):
    def run():
        fw = gpu_util.hip_forward(inp, cam, indexed)
        got = gpu_util.hip_backward(fw, dL)
        return dict(_forward_outputs(fw), **got)
    return run


def _raster_check(st, ref, label):
    from tests import fullsize
    from tests.test_raster_gpu import GRAD_TOL, _check_forward

    def check(o):
        u = {k: v for k, v in o.items() if not k.startswith("dL_")}
        got = {k: v for k, v in o.items() if k.startswith("dL_")}
        u["num_rendered"] = int(u["num_rendered"])
        _check_forward(u, st)
        fullsize.check_grads(st, u, got, ref, GRAD_TOL, label)
    return check


def _raster_independent(inp, cam, indexed, st, dL, ref, label):
    probe = _raster_run(inp, cam, indexed, dL)()            # the output names (a plain run; also warms the library up)
    barred = {k: None for k in probe if indexed and k in SCATTERED}
    exact = tuple(k for k in probe if k not in barred)
    # with float atomics among the outputs every run is held to the oracle; otherwise the three are one set of bits
    return poison.assert_independent(_raster_run(inp, cam, indexed, dL), exact=exact, barred=barred, check=_raster_check(st, ref, label),
                                     check_bytes=poison.POISON_BYTES if barred else (0xFF,))


@pytest.mark.parametrize("image", list(IMAGES))
@pytest.mark.parametrize("P", SIZES)
@pytest.mark.parametrize("variant", VARIANTS)
def test_forward_and_backward(hip, orc, variant, P, image):
    inp, cam, indexed, st, dL, ref = _raster_reference(variant, P, image)
    assert st.P == P and (st.radii > 0).any()
    if P == SIZES[-1] and image == "64x64":
        assert st.num_rendered > 8192, "the tile sort has one tile only"
    base = _raster_independent(inp, cam, indexed, st, dL, ref, f"{variant} P={P} {image}")
    assert np.abs(base["dL_dmeans3D"]).max() > 0


@pytest.mark.parametrize("name", ["all_behind", "empty"])
def test_nothing_to_render(hip, orc, name):
    inp, cam, indexed, st, dL, ref = _raster_reference(name, 257, "64x64")
    assert st.num_rendered == 0 and (st.P == 0) == (name == "empty")
    base = _raster_independent(inp, cam, indexed, st, dL, ref, name)
    for k, v in base.items():
        if k.startswith("dL_"):
            assert not v.any(), k


# ---------------------------------------------------------------------------------------------------------------- depth-sort routes
BIAS = 0x3C000000
LIMIT3 = BIAS + (1 << 27) - 1                               # tests/test_depth_sort3_gpu.py: the smallest key that needs the fourth pass
ROUTES = ("below_512", "far", "prefiltered", "wide")


def _route_case(route):
    inp, cam, indexed, st, dL, ref = _raster_reference("base", SIZES[-1], "64x64", "plain" if route == "below_512" else route)
    keys = st.depths.view(np.uint32)[st.radii > 0]
    assert keys.size > TILE and int(keys.min()) >= BIAS
    if route == "far":
        assert st.radii[7] > 0 and int(st.depths.view(np.uint32)[7]) >= LIMIT3, "the far Gaussian must be visible: the fallback runs"
    else:
        assert int(keys.max()) < LIMIT3                     # all depths below 512
    assert (((cam["W"] + 15) // 16) > 255) == (route == "wide")
    return inp, cam, indexed, st, dL, ref


@pytest.mark.parametrize("route", ROUTES)
def test_depth_sort_routes_through_the_forward(hip, orc, route):
    """the three-pass sort, its four-pass fallback, the four raw passes of `prefiltered` and the gather variant above 255 tile
    columns, each through the whole forward at three depth-sort tiles with a ragged tail"""
    inp, cam, indexed, st, dL, ref = _route_case(route)
    _raster_independent(inp, cam, indexed, st, dL, ref, f"route {route}")


def test_depth_sort_routes_with_the_copy_based_host_read(hip):
    """C3DGS_HOST_READ_COPY=1: no mapped pad, so no largest-key read and no three-pass plan; the switch is read once per thread,
    hence the child process (as tests/test_raster_gpu.py does it)"""
    env = dict(os.environ, C3DGS_HOST_READ_COPY="1")
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    r = subprocess.run([sys.executable, "-m", "pytest", "tests/test_scratch_poison_gpu.py", "-q", "-m", "gpu", "-x", "-k",
                        "through_the_forward and (below_512 or far)"], cwd=root, env=env, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    assert "2 passed" in r.stdout


# ---------------------------------------------------------------------------------------------------------------- the extras
@pytest.mark.parametrize("name", ["odd_size", "indexed"])
def test_render_depth(hip, orc, name):
    from c3dgs_amd import rasterizer as rz
    from tests import depth_ref
    from tests.test_render_depth_gpu import check_maps
    inp, cam, indexed = depth_ref.scene(name)
    st = depth_ref.oracle_state(name)
    fwd_names = ("radii", "depths", "n_contrib", "final_T")

    def run():
        fw = gpu_util.hip_forward(inp, cam, indexed)
        depth, alpha, median = rz._C.render_depth(st.P, cam["W"], cam["H"], fw["num_rendered"], fw["geom"], fw["binning"], fw["img"])
        u = _forward_outputs(fw)
        return dict(depth=depth, alpha=alpha, median=median, **{k: u[k] for k in fwd_names})

    poison.assert_independent(run, exact=("depth", "alpha", "median") + fwd_names, check_bytes=(0xFF,),
                              check=lambda o: check_maps(name, inp, cam, indexed, st, o, o["depth"], o["alpha"], o["median"]))


@pytest.mark.parametrize("image_gradient", ["none", "zeros"])
@pytest.mark.parametrize("name,as_indexed", [("odd_size", False), ("odd_size", True), ("indexed", True)])
def test_depth_and_alpha_backward(hip, name, as_indexed, image_gradient):
    """both maps; without an image gradient (no colour blend launch: the depth pass is the first to write the partial sums and their
    flags) and with one of zeros (the colour blend has flagged the slots before it)"""
    from tests import depth_ref
    from tests.test_depth_grad_gpu import GRADS, _backward, _colour_coded, _lift, _maps, _reference, _worst
    inp, cam, indexed = depth_ref.scene(name)
    if as_indexed and not indexed:
        inp = _lift(inp)
    W, H = cam["W"], cam["H"]
    gD, gA = _maps(W, H)
    inp_z, z_term = _colour_coded(inp, cam)
    ref = _reference(gpu_util.hip_forward(inp_z, cam, as_indexed), z_term, gD, gA, H, W)
    names = GRADS if as_indexed else tuple(g for g in GRADS if g != "dL_dscale_factors")
    dL = None if image_gradient == "none" else np.zeros((3, H, W), np.float32)

    def run():
        return _backward(gpu_util.hip_forward(inp, cam, as_indexed), dL, gD, gA)

    probe = run()
    barred = {k: None for k in probe if as_indexed and k in SCATTERED}
    base = poison.assert_independent(run, exact=tuple(k for k in probe if k not in barred), barred=barred,
                                     check=lambda o: _worst(o, ref, names, 1e-4, f"poisoned {name} {image_gradient}:"))
    assert np.abs(base["dL_dopacity"]).max() > 0 and not base["dL_dcolors"].any() and not base["dL_dsh"].any()


@pytest.mark.parametrize("name", ["odd_size", "indexed", "long_run"])
def test_render_contrib(hip, orc, name):
    from c3dgs_amd import rasterizer as rz
    from tests.test_render_contrib_gpu import _scene, check_against_walk
    inp, cam, indexed = _scene(name)
    P = inp["means3D"].shape[0]

    def run():
        fw = gpu_util.hip_forward(inp, cam, indexed)
        wsum, wmax, hits = rz._C.render_contrib(P, cam["W"], cam["H"], fw["num_rendered"], fw["geom"], fw["binning"], fw["img"])
        return dict(weight_sum=wsum, weight_max=wmax, hits=hits, radii=fw["radii"])

    poison.assert_independent(run, exact=("weight_sum", "weight_max", "hits", "radii"), check_bytes=(0xFF,),
                              check=lambda o: check_against_walk(name, o, o["weight_sum"], o["weight_max"], o["hits"].view(np.uint32)))


@pytest.mark.parametrize("name", ["odd_size", "indexed", "long_run"])
def test_render_error(hip, orc, name):
    from c3dgs_amd import rasterizer as rz
    from tests import error_ref
    from tests.test_render_error_gpu import _scene, check_scores
    inp, cam, indexed = _scene(name)
    P, W, H = inp["means3D"].shape[0], cam["W"], cam["H"]
    emap = torch.from_numpy(error_ref.standard_map(H, W)).cuda()

    def run():
        fw = gpu_util.hip_forward(inp, cam, indexed)
        bufs = (fw["geom"], fw["binning"], fw["img"])
        err = rz._C.render_error(P, W, H, fw["num_rendered"], *bufs, emap)
        hits = rz._C.render_contrib(P, W, H, fw["num_rendered"], *bufs)[2]
        return dict(err_sum=err, hits=hits, radii=fw["radii"])

    poison.assert_independent(run, exact=("err_sum", "hits", "radii"), check_bytes=(0xFF,),
                              check=lambda o: check_scores(name, o, o["err_sum"], o["hits"].view(np.uint32)))


@pytest.mark.parametrize("name", ["floor", "indexed"])
def test_aa_opacity_and_its_backward(hip, orc, name):
    """the antialiased module (aa_opacity in front of a poisoned forward, aa_opacity_backward behind a poisoned backward) against
    the plain module fed the reference's rho: the composition bar of tests/test_aa_gpu.py"""
    from tests import aa_ref
    from tests import test_aa_gpu as t
    c = aa_ref.aa_case(name)
    inp = c["inp"]
    _, want = t._compose(hip, c)
    dL = synth.grad_image(t.W, t.H).cuda()

    def run():
        lv = t._leaves(c)
        m2 = lv.pop("means2D")
        rs, ev = t._settings(hip, inp, antialiasing=True)
        out = t._module_call(hip, c, rs, ev, lv, means2D=m2)
        (out[0] * dL).sum().backward()
        o_k, rho_k = t._kernel_rho(hip, c)
        lv["means2D"] = m2
        got = {k: (torch.zeros_like(v) if v.grad is None else v.grad) for k, v in lv.items()}
        return dict(got, image=out[0].detach(), radii=out[1], aa_opacity=o_k, rho=rho_k)

    probe = run()
    # the codebook gradients of the indexed form are scatter-added, and aa_opacity_backward adds into them
    barred = {k: None for k in ("shs", "scales", "rotations") if c["indexed"]}
    poison.assert_independent(run, exact=tuple(k for k in probe if k not in barred), barred=barred,
                              check=lambda o: t._check_composition(f"poisoned {name}", o, want))


@pytest.mark.parametrize("name,case,kw", [("p257", "p257", dict(P=257)), ("indexed", "indexed", {})])
def test_pose_grad(hip, name, case, kw):
    from tests import test_pose_grad_gpu as t
    inp, cam, indexed, pose, _ = t.pose_ref.make_pose_case(case, **kw)
    dL = synth.grad_image(cam["W"], cam["H"]).numpy()
    last = {}

    def run():
        fw = gpu_util.hip_forward(inp, cam, indexed)
        bw = gpu_util.hip_backward(fw, dL)
        last.update(fw=fw, bw=bw)
        return dict(pose_grad=t._pose_grad(hip, inp, fw, bw, pose))

    poison.assert_independent(run, exact=("pose_grad",), check=lambda o: t.check_kernels_alone(
        f"poisoned {name}", inp, cam, pose, last["fw"], last["bw"], o["pose_grad"].astype(np.float64)))


@pytest.mark.parametrize("P,C", [(257, 2), (5000, 7)])
def test_filter3d_compute(hip, P, C):
    from tests import filter3d_ref as ref
    from tests.test_filter3d_gpu import _compute
    xyz, table = ref.ring_scene(P, C, seed=P + C)
    want, seen_w, _ = ref.filter_np(xyz, table)

    def run():
        f, seen = _compute(xyz, table)
        return dict(filter_3D=f, seen=seen)

    def check(o):                                           # the float32 restatement, bit for bit (test_filter_is_the_float32_restatement)
        np.testing.assert_array_equal(o["seen"], seen_w)
        np.testing.assert_array_equal(o["filter_3D"].view(np.uint32), want.view(np.uint32))

    poison.assert_independent(run, exact=("filter_3D", "seen"), check=check, check_bytes=(0xFF,))


@pytest.mark.parametrize("name", ["floor", "indexed"])
def test_filter3d_apply_and_backward(hip, name):
    """filter3d.apply and its autograd backward under the hashed cotangents tests/filter3d_ref.py measures its float32 deviation
    with, at the bars of tests/test_filter3d_gpu.py"""
    from c3dgs_amd import filter3d
    from tests import aa_ref
    from tests import filter3d_ref as ref
    from tests.test_filter3d_gpu import KEY_OF, _bar, _cuda
    a = ref.apply_inputs(name)
    indexed = a["g_indices"] is not None
    n = a["opacities"].shape[0]
    d_cov = torch.as_tensor(aa_ref.hashed(6 * n, 11)).reshape(n, 6).float()
    gp = torch.as_tensor(aa_ref.hashed(n, 13)).float()
    want = ref.autograd_backward(a["opacities"], a["scales"], a["rotations"], a["f"], d_cov, gp, a["scale_modifier"], a["scale_factors"],
                                 a["g_indices"])
    d = lambda t: None if t is None else t.double()          # noqa: E731
    with torch.no_grad():
        cov64, o64 = ref.apply(d(a["opacities"]), d(a["scales"]), d(a["rotations"]), d(a["f"]), a["scale_modifier"], d(a["scale_factors"]),
                               a["g_indices"])
    dev = ref.f32_deviation(name)
    g = _cuda(a)
    leaf_names = [k for k in ("opacities", "scales", "rotations", "scale_factors") if g[k] is not None]

    def run():
        lv = {k: g[k].clone().requires_grad_() for k in leaf_names}
        cov, o = filter3d.apply(lv["opacities"], lv["scales"], lv["rotations"], g["f"], g["scale_modifier"],
                                scale_factors=lv.get("scale_factors"), g_indices=g["g_indices"])
        ((cov * d_cov.cuda()).sum() + (o * gp.cuda()).sum()).backward()
        return dict({"d_" + k: v.grad for k, v in lv.items()}, cov3D=cov.detach(), opacity=o.detach())

    def check(o):
        assert ref.relinf(o["cov3D"], cov64) <= _bar(dev["cov3D"], 1e-6) and ref.relinf(o["opacity"], o64) <= _bar(dev["opacity"], 1e-6)
        for out, key in KEY_OF.items():
            if key in leaf_names:
                atomic = indexed and out in ("dL_dscales", "dL_drotations")
                e = ref.relinf(o["d_" + key], want[key].reshape(o["d_" + key].shape))
                print(f"poisoned filter3d {name} {out}: rel-inf {e:.3e}")
                assert e <= _bar(dev["d_" + key], 1e-5 if atomic else 1e-6), (name, out, e)

    barred = {"d_" + k: None for k in ("scales", "rotations") if indexed}       # scatter-added codebook rows
    exact = tuple(["cov3D", "opacity"] + ["d_" + k for k in leaf_names if "d_" + k not in barred])
    poison.assert_independent(run, exact=exact, barred=barred, check=check)


# ---------------------------------------------------------------------------------------------------------------- the other families
# Every other family that works in a workspace or writes into uninitialised outputs, through its Python wrapper, at the smallest
# case of its own GPU test: that test function IS the check against the family's reference, and is called under each poison byte.
def _metrics_golden(hip, orc):
    from tests import test_metrics_gpu as t
    t.test_metrics_match_reference_golden(hip, np.load(os.path.join(t.G, "metrics.npz"), allow_pickle=False), "batch")


def _knn_neighbours(hip, orc):
    from tests import test_knn_neighbours_gpu as t
    t._cache.clear()                                        # its cases are computed once per process: again, under this byte
    try:
        t.test_knn3_equals_the_brute_force("P257")
        t.test_distCUDA2_is_the_mean_of_knn3_and_unchanged("P257")
    finally:
        t._cache.clear()


def _call(module, test, *args, fixtures="h"):
    """-> fn(hip, orc) that calls tests.<module>.<test>(<the fixtures named by `fixtures`: h = hip, o = orc>, *args)"""
    def fn(hip, orc):
        import importlib
        f = getattr(importlib.import_module("tests." + module), test)
        f(*[{"h": hip, "o": orc}[c] for c in fixtures], *args)
    return fn


#        id                          the family's own test, at its smallest case                                     allocates uninitialised
FAMILIES = [
    ("sparse_adam_select", _call("test_sparse_adam_gpu", "test_select_lists_the_rows_of_every_mask_kind_in_order", 257), False),
    ("sparse_adam_step", _call("test_sparse_adam_gpu", "test_step_every_alignment_step_count_and_lerp_form_at_every_row_length", 0, 1, 0.9), False),
    ("multi_tensor_adam", _call("test_optim_gpu", "test_adam_more_than_sixteen_tensors_take_several_launches", 17), False),
    ("mcmc_sample", _call("test_mcmc_gpu", "test_sample_is_bit_equal_to_the_host_sampler_on_the_kernels_weights", 257), True),
    ("mcmc_apply", _call("test_mcmc_gpu", "test_relocation_values_against_float64", True), True),
    ("bilagrid_slice_backward_tv", _call("test_bilagrid_gpu", "test_autograd_through_the_module", (3, 2, 5), (64, 64)), True),
    ("fused_loss", _call("test_loss_gpu", "test_loss_shapes_around_window_and_tile", (3, 23, 33), "loss", fixtures="ho"), True),
    ("image_metrics", _metrics_golden, True),
    ("knn_mean_distance", _call("test_knn_gpu", "test_exact_small", "gaussian", 1000), True),
    ("knn_neighbours", _knn_neighbours, True),
    ("morton_order", _call("test_encode_gpu", "test_morton_order_matches_oracle", 777, fixtures="ho"), True),
    ("rows_plan_and_densify", _call("test_densify_gpu", "test_against_the_reference_fixture", "factor_qat", True, fixtures=""), True),
    ("ray_fill", _call("test_densify_initial_gpu", "test_against_the_reference_fixture", "qat_factor_outliers", True, fixtures=""), True),
    ("qat_observe_and_visible_scan", _call("test_model_gpu", "test_fused_render_equals_reference_glue_with_device_torch_modules", fixtures=""), True),
    ("weighted_distance_ws", _call("test_vq_gpu", "test_weighted_distance_bit_exact", 513, 33, 5, fixtures="ho"), True),
    ("fused_lloyd_step", _call("test_vq_gpu", "test_fused_lloyd_step_is_bit_identical_to_the_plain_pair", 12, 256, 1000, False), True),
]


@pytest.mark.parametrize("fn,allocates", [t[1:] for t in FAMILIES], ids=[t[0] for t in FAMILIES])
def test_family_through_its_python_wrapper(hip, orc, fn, allocates):
    poison.under_every_byte(lambda: fn(hip, orc), expect_allocations=allocates)
