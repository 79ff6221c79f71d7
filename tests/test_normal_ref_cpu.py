"""CPU: the float64 references of the normal maps (tests/normal_ref.py) against themselves and against independent
restatements, and the fp32 restatements of the kernels' arithmetic that set the GPU bars of tests/test_normal_gpu.py.

  per-Gaussian      the closed-form chain dL/dn -> dL/dq against float64 autograd of the definition restated in torch; the tie rule
                    on `huge_faint` (many rows with two equal smallest scales); the raw-row rule on a row whose scale x scale
                    factor rounds to a tie while the raw row does not
  sign condition    every scene of depth_ref.SCENES has at most ONE Gaussian with |v . p| / |p| < 1e-5 (a condition of the GPU
                    tests, which adopt the GPU's sign for such a Gaussian; not a tolerance)
  normal map        the float64 sum over the walk's pairs against a per-pixel loop, on `one_pixel` and `odd_size`
  depth_to_normal   planes a . X = d through synth.camera at focal 50 and 125: the plane's unit normal facing the camera at every
                    interior pixel; the float64 backward against autograd and a central difference on a 7 x 5 map
  gradients         restated() (the closed form the GPU is held to) against autograd_truth() on `tiny`
  fp32              the restatements' worst errors, recorded in FP32_MEASURED: they set the GPU bars"""
import numpy as np
import pytest
import torch

from tests import depth_grad_ref as dgr, depth_ref, normal_ref as nr, synth

FP32_MEASURED = ("fp32 restatement against float64: gaussian_normals worst component error 1.79e-7 = 3.0 x 2^-24 over the seven scenes (bar "
                 "16 x 2^-24); depth_to_normal worst 0.409 x 2^-24 max(fx, fy), so k = 1.635; depth_to_normal_backward worst rel-inf "
                 "1.46e-6, so the GPU bar is 5.8e-6; the chain dL/dn -> dL/dq worst rel-inf 2.5e-7")


def _tan_fov(W, H, focal):
    from c3dgs_amd.rasterizer import _intrinsic_scalars
    intr, _ = synth.camera(W, H, focal)
    return _intrinsic_scalars(intr)[0][:2]


# ---------------------------------------------------------------------------------------------------------------- per Gaussian
def _definition_torch(q, m, sigma, view):
    """n from the definition, restated independently: the rotation matrix of the NORMALISED quaternion times |q|^2 is not what
    the kernels use, so build R entry by entry from the products q_a q_b, pick the column by a one-hot product, normalise, rotate"""
    r, x, y, z = q.unbind(1)
    R = torch.stack([torch.stack([1 - 2 * (y * y + z * z), 2 * (x * y - r * z), 2 * (x * z + r * y)], 1),
                     torch.stack([2 * (x * y + r * z), 1 - 2 * (x * x + z * z), 2 * (y * z - r * x)], 1),
                     torch.stack([2 * (x * z - r * y), 2 * (y * z + r * x), 1 - 2 * (x * x + y * y)], 1)], 1)
    onehot = torch.nn.functional.one_hot(torch.as_tensor(m), 3).to(q.dtype)
    c = (R * onehot[:, None, :]).sum(2)
    ch = c / c.norm(dim=1, keepdim=True)
    Rv = torch.as_tensor(view.reshape(4, 4)[:3, :3].T.copy())     # R_view[i][k] = view[4 k + i]
    return torch.as_tensor(sigma)[:, None] * (ch @ Rv.T)


@pytest.mark.parametrize("name", ["indexed", "odd_size", "huge_faint"])
def test_chain_against_autograd_of_the_definition(name):
    inp, cam, _ = depth_ref.scene(name)
    view = np.asarray(cam["viewmatrix"], np.float64)
    ref = nr.gaussian_normals(inp, view)
    q, s, _ = nr._rows(inp)
    qt = torch.tensor(q.astype(np.float64), requires_grad=True)
    n = _definition_torch(qt, ref["m"], ref["sigma"], view)
    assert np.abs(n.detach().numpy() - ref["n"]).max() <= 1e-14
    # unit length up to the view matrix's own rotation (the test poses' quaternions are not normalised: |R_view x| = |x| (1 + 1e-4))
    Rv = view.reshape(4, 4)[:3, :3]
    stretch = np.linalg.svd(Rv, compute_uv=False)
    assert (np.sqrt((ref["n"] ** 2).sum(1)) <= stretch.max() + 1e-14).all() and (np.sqrt((ref["n"] ** 2).sum(1)) >= stretch.min() - 1e-14).all()
    p = np.concatenate([np.asarray(inp["means3D"], np.float64), np.ones((q.shape[0], 1))], 1) @ view.reshape(4, 4)
    assert ((ref["n"] * p[:, :3]).sum(1) <= 0).all()             # faces the camera
    g = np.random.default_rng(3).standard_normal(ref["n"].shape)
    (n * torch.as_tensor(g)).sum().backward()
    got = nr.normal_chain(q, ref["m"], ref["sigma"], view, g)
    e = dgr.rel_inf(got, qt.grad.numpy())
    f32 = dgr.rel_inf(nr.normal_chain(q, ref["m"], ref["sigma"], view, g, np.float32), got)
    print(f"{name}: chain against autograd rel-inf {e:.3e}; fp32 restatement of the chain against float64 {f32:.3e}")
    assert e <= 1e-12 and f32 <= 1e-5
    # through the codebook of an indexed scene: normals_torch scatters to the rows
    if inp.get("g_indices") is not None:
        rt = torch.tensor(np.asarray(inp["rotations"], np.float64), requires_grad=True)
        (nr.normals_torch(inp, rt, view, ref["m"], ref["sigma"]) * torch.as_tensor(g)).sum().backward()
        want = np.zeros_like(rt.grad.numpy())
        np.add.at(want, np.asarray(inp["g_indices"]).astype(np.int64), got)
        assert dgr.rel_inf(rt.grad.numpy(), want) <= 1e-12


def test_tie_goes_to_the_lowest_index():
    inp, cam, _ = depth_ref.scene("huge_faint")
    q, s, _ = nr._rows(inp)
    srt = np.sort(s, axis=1)
    ties = srt[:, 0] == srt[:, 1]
    print("huge_faint: rows whose two smallest scales are equal:", int(ties.sum()), "of", s.shape[0])
    assert ties.sum() >= 100
    m = nr.smallest_axis(s)
    for row, mm in zip(s[ties], m[ties]):
        assert mm == min(j for j in range(3) if row[j] == row.min())
    assert (s[np.arange(s.shape[0]), m] == s.min(1)).all()


def test_argmin_is_taken_on_the_raw_row():
    """scale x scale factor can round two different scales into a tie; the raw row decides"""
    f = np.float32
    # two neighbours just below 2 and a factor that lifts both over 2, where fp32 is half as fine
    s0, s1 = f(2.0) - f(2.0 ** -23), f(2.0) - f(2.0 ** -22)
    assert s1 < s0
    sf = next(v for v in (f(1.0) + f(k) * f(2.0 ** -20) for k in range(1, 4096)) if f(s0 * v) == f(s1 * v))
    raw = np.array([[s0, s1, f(2.0)]], f)
    assert nr.smallest_axis(raw)[0] == 1 and np.argmin(raw * sf, axis=1)[0] == 0
    inp = dict(scales=torch.from_numpy(raw), rotations=torch.tensor([[0.9, 0.1, -0.3, 0.2]]), g_indices=torch.tensor([0, 0]),
               scale_factors=torch.tensor([[float(sf)], [1.0]]), means3D=torch.tensor([[0.1, 0.2, 4.0], [0.3, -0.2, 5.0]]))
    view = np.eye(4).reshape(-1)
    ref = nr.gaussian_normals(inp, view)
    assert (ref["m"] == 1).all()


@pytest.mark.parametrize("name", depth_ref.SCENES)
def test_at_most_one_sign_ambiguous_gaussian_per_scene(name):
    ref = nr.scene_normals(name)
    c = np.abs(ref["cos"])
    print(f"{name}: Gaussians with |cos| < 1e-5: {int((c < 1e-5).sum())}, < 1e-4: {int((c < 1e-4).sum())}, < 1e-3: {int((c < 1e-3).sum())}")
    assert (c < nr.AMBIGUOUS_COS).sum() <= 1


def test_fp32_restatement_of_gaussian_normals():
    worst, bar = nr.gaussian_normals_bar()
    print(f"gaussian_normals: fp32 restatement worst component error {worst:.3e} = {worst / nr.U:.2f} x 2^-24; GPU bar {bar:.3e}")
    assert bar == 16 * nr.U, "the restatement needs more than 16 x 2^-24: the GPU bar is 4 x its worst (say so in DESIGN.md)"


# ---------------------------------------------------------------------------------------------------------------- the map
@pytest.mark.parametrize("name,stride", [("one_pixel", 1), ("odd_size", 53)])
def test_normal_map_against_a_per_pixel_loop(name, stride):
    inp, cam, _ = depth_ref.scene(name)
    st = depth_ref.oracle_state(name)
    n = nr.scene_normals(name)["n"]
    W, H = cam["W"], cam["H"]
    ref = nr.normal_map(st, W, H, n)
    brute = nr.normal_map_brute(st, W, H, n, stride)
    seen = np.isfinite(brute[0])
    e = float(np.abs(ref["normal"] - brute)[:, seen].max())
    print(f"{name}: {int(seen.sum())} pixels, largest difference {e:.3e}, largest value {float(np.abs(ref['normal']).max()):.3e}")
    assert e <= 1e-12 and np.abs(ref["normal"]).max() > 0.05
    assert (np.sqrt((ref["normal"] ** 2).sum(0)) <= np.sqrt((n ** 2).sum(1)).max() + 1e-12).all()       # weights sum to A <= 1


# ---------------------------------------------------------------------------------------------------------------- the stencil
PLANES = ((0.0, 0.0, 1.0),) + tuple(tuple(a) for a in nr.TILTED)


@pytest.mark.parametrize("focal", [50.0, 125.0])
@pytest.mark.parametrize("a", PLANES, ids=["fronto", "tilted0", "tilted1"])
def test_planes_give_their_normal_facing_the_camera(a, focal):
    W, H = 70, 45
    tfx, tfy = _tan_fov(W, H, focal)
    assert abs(W / (2 * tfx) - focal) < 1e-3 * focal
    a = np.asarray(a, np.float64)
    z = nr.plane_depth(W, H, tfx, tfy, a, 4.0)
    assert (z > 0).all()
    n = nr.depth_to_normal(z, tfx, tfy)
    want = -a / np.sqrt((a * a).sum())                          # a . X = d > 0 with a_z > 0: -a looks back at the camera
    e = float(np.abs(n[:, 1:-1, 1:-1] - want[:, None, None]).max())
    print(f"plane {tuple(a)} focal {focal}: largest error {e:.3e}")
    assert e <= 1e-9
    assert not n[:, 0].any() and not n[:, -1].any() and not n[:, :, 0].any() and not n[:, :, -1].any()
    nt = nr.depth_to_normal_torch(torch.as_tensor(z), tfx, tfy).numpy()
    assert np.abs(nt - n).max() <= 1e-14
    for shape in ((2, 2), (2, 9), (9, 2), (1, 1)):
        assert not nr.depth_to_normal(np.full(shape, 3.0), tfx, tfy).any()


def test_stencil_backward_against_autograd_and_a_central_difference():
    W, H = 7, 5
    tfx, tfy = 7 / 20.0, 5 / 20.0
    rng = np.random.default_rng(11)
    z = 3.0 + rng.random((H, W))
    g = rng.standard_normal((3, H, W))
    got = nr.depth_to_normal_backward(z, g, tfx, tfy)
    zt = torch.tensor(z, requires_grad=True)
    (nr.depth_to_normal_torch(zt, tfx, tfy) * torch.as_tensor(g)).sum().backward()
    e = dgr.rel_inf(got, zt.grad.numpy())
    fd = np.zeros_like(z)
    h = 1e-6
    for i in range(H):
        for j in range(W):
            zp, zm = z.copy(), z.copy()
            zp[i, j] += h; zm[i, j] -= h
            fd[i, j] = ((nr.depth_to_normal(zp, tfx, tfy) - nr.depth_to_normal(zm, tfx, tfy)) * g).sum() / (2 * h)
    e_fd = dgr.rel_inf(got, fd)
    print(f"stencil backward: against autograd {e:.3e}, against a central difference {e_fd:.3e}")
    assert e <= 1e-12 and e_fd <= 1e-6
    assert got[0, 0] == 0 and got[H - 1, W - 1] == 0 and np.abs(got[1, 0]) > 0        # corners feed no stencil; edges do


def test_fp32_restatement_of_the_stencil():
    bars = nr.stencil_bars()
    for label, z, tfx, tfy in nr.stencil_inputs():
        assert z.min() > 1.0 and z.max() < 10.0
        n = nr.depth_to_normal(z, tfx, tfy)
        assert np.abs(np.sqrt((n[:, 1:-1, 1:-1] ** 2).sum(0)) - 1.0).max() <= 1e-12, label
    wf, k = bars["forward"]
    wb, bb = bars["backward"]
    print(f"depth_to_normal fp32 restatement: worst {wf:.3f} x 2^-24 max(fx, fy), k = {k:.3f}; backward worst rel-inf {wb:.3e}, GPU bar "
          f"{bb:.3e}")
    assert 0 < wf < 64 and 0 < wb < 1e-3          # sanity of the restatement itself: a wrong stencil is off by O(1)


# ---------------------------------------------------------------------------------------------------------------- gradients
@pytest.mark.parametrize("combo", ["gN", "gD+gA+gN"])
def test_closed_form_matches_float64_autograd(combo):
    st, inp, _, _ = dgr.black_state("tiny")
    W, H = st.W, st.H
    gN = nr.gn_map(W, H)
    gD, gA = (dgr.hashed_map(W, H, 1), dgr.hashed_map(W, H, 2)) if "gD" in combo else (None, None)
    got = nr.restated(st, inp, gN, gD, gA)
    want = nr.autograd_truth(st, inp, gN, gD, gA)
    assert got["pairs"] > 0 and np.abs(got["rotations"]).max() > 0
    for k in dgr.LEAF_ORDER:
        if k in want:
            e = dgr.rel_inf(got[k], want[k]) if np.abs(want[k]).max() > 0 else float(np.abs(got[k]).max())
            print(f"closed form tiny {combo}: {k} rel-inf {e:.3e}, reference max {float(np.abs(want[k]).max()):.3e}")
            assert e <= 1e-9, (k, e)
    if combo == "gN":
        # the rotations receive the weights' share (through the covariance) plus the chain of dL/dn; nothing else sees n
        ng = nr.gaussian_normals(inp, st.inputs["viewmatrix"])
        chain = nr.normal_chain(nr._rows(inp)[0], ng["m"], ng["sigma"], st.inputs["viewmatrix"], got["n"])
        assert np.abs(chain).max() > 0.01 * np.abs(got["rotations"]).max()
