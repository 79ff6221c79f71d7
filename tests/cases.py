"""Raster parity cases shared by the CPU (oracle vs float64 autograd) and GPU (HIP vs oracle) tests.
Edge cases follow SURVEY.md section 7's list: P=0, R=0, Gaussians behind the camera, image size not a multiple
of 16, SH degree 0-3, clamp_color on/off, precomputed covariance / colour variants, indexed codebooks,
t-clamp at the frustum edge, scale_modifier != 1, non-zero background.

EDGE_GAUSSIAN_CASES are what a TRAINED scene holds and synth-v1 does not: splats whose opacity saturated (the min(0.99, o G)
clamp, the stop test right behind clamped layers), needles and flat discs (a conic with cancelling terms), quaternions whose
norm drifted, floaters centimetres from the camera (1/z^2 Jacobians, the z <= 0.01 cull). Each has a guard (edge_guard) read
off the oracle state in float64, so that a changed seed cannot hollow it out. Anisotropy of 40 and more, with radii of
thousands of pixels, is left out on purpose: there the reference's own fp32 formula is ill-conditioned (two legitimate fp32
evaluations of one view differ by 0.2 in the image), so there is nothing to hold a kernel to."""
import functools

import numpy as np
import torch

from oracle import oracle as orc
from tests import synth


def _cam(W, H, focal, ev=(0.05, -0.03, 0.02, 0.99, 0.1, -0.05, 0.2)):
    intr, e = synth.camera(W, H, focal, extrinsic_vector=ev)
    return orc.camera(intr.numpy(), e.numpy()), intr, e


def make_case(name, P=4000, W=200, H=136, focal=125.0, seed=7, scale_median=0.03):
    """-> (inputs dict of CPU tensors/None + flags, cam dict, indexed bool)."""
    deg = 3
    kw = {}
    if name == "tiny":
        P, W, H, focal, scale_median = 48, 48, 32, 40.0, 0.25
        kw = dict(zmin=2, zmax=6)
    if name == "odd_size":
        W, H = 203, 131
    if name == "behind":
        kw["behind_fraction"] = 0.3
    if name.startswith("deg"):
        deg = int(name[3])
    if name == "deep_tile":      # thousands of faint splats stacked over four tiles: many staging rounds per tile
        P, W, H, focal, scale_median = 5000, 32, 32, 30.0, 0.2
        kw = dict(zmin=3, zmax=9)
    if name == "huge_splats":    # every splat's rectangle is clipped by the screen: R = P x (all tiles)
        P, W, H, focal, scale_median = 300, 150, 100, 90.0, 6.0
    if name == "one_tile":       # a 1 x 1 tile grid, narrower than one wave's pixel block
        P, W, H, focal, scale_median = 200, 9, 5, 8.0, 0.3
        kw = dict(zmin=2, zmax=6)
    if name == "p257":           # one Gaussian past a 256-block of the two-level scans
        P = 257
    if name == "p8193":          # one key past an 8192-item tile of the sorts
        P = 8193
    if name == "p12289":         # one key past a 12288-item tile of the depth sort (keys + ids + packed rectangles: two tiles)
        P = 12289
    if name == "p24577":         # three depth-sort tiles, the last holding one item
        P = 24577
    if name == "p1024":          # exactly one full list of the backward's blended Gaussians (csrc/common.hpp: BWD_LIST)
        P = 1024
    if name in ("p1025", "indexed_p1025"):   # one Gaussian past it: a second list that holds one entry
        P = 1025
    if name == "p2049":          # three lists, the last holding one entry
        P = 2049
    if name in EDGE_GAUSSIAN_CASES:   # 6 x 4 tiles: the smallest grid on which a needle still crosses several tiles
        P, W, H, focal, scale_median = 300, 96, 64, 60.0, EDGE_SCALE_MEDIAN[name]
    ev = (0.05, -0.03, 0.02, 0.99, 0.1, -0.05, 0.2)
    if name == "equal_depth":    # identity camera + one z: all depth keys tie -> the stable sort must keep id order
        ev = (0, 0, 0, 1, 0, 0, 0)
    cam, intr, ev = _cam(W, H, focal, ev)
    sc = synth.scene(P, W, H, focal, seed=seed, sh_degree=3, scale_median=scale_median, **kw)
    if name == "deep_tile":
        sc["opacities"] = sc["opacities"] * 0.02
    if name == "equal_depth":
        sc["means3D"][:, :2] *= (5.0 / sc["means3D"][:, 2])[:, None]
        sc["means3D"][:, 2] = 5.0
        sc["means3D"][::3, 2] = 5.5
    if name == "all_behind":
        sc["means3D"][:, 2] = -sc["means3D"][:, 2].abs() - 1.0
    if name == "wide_depth":     # depths over five decades (0.05 .. 6000): every digit of the depth sort keys is exercised
        g = torch.Generator().manual_seed(11)
        z = torch.exp(torch.rand(P, generator=g) * (np.log(6000.0) - np.log(0.05)) + np.log(0.05)).float()
        sc["means3D"] = sc["means3D"] * (z / sc["means3D"][:, 2])[:, None]
        sc["scales"] = sc["scales"] * (z / 7.0)[:, None]
    if name == "frustum_edge":   # exercise the 1.3*tan_fov clamp of computeCov2D
        sc["means3D"][:, 0] *= 1.6
        sc["scales"] *= 3.0
    if name in EDGE_GAUSSIAN_CASES:
        _edge_scene(name, sc, cam, seed)
    inp = dict(bg=torch.tensor([0.2, 0.4, 0.1]), means3D=sc["means3D"], opacities=sc["opacities"], shs=sc["shs"],
               colors_precomp=None, scales=sc["scales"], rotations=sc["rotations"], cov3D_precomp=None, scale_factors=None,
               sh_indices=None, g_indices=None, degree=deg, scale_modifier=1.0, prefiltered=False, clamp_color=True)
    indexed = False
    if name == "empty":
        for k in ("means3D", "opacities", "shs", "scales", "rotations"):
            inp[k] = inp[k][:0].contiguous()
    if name == "no_clamp":
        inp["clamp_color"] = False
        inp["shs"] = inp["shs"] * 3.0          # make some colours negative
    if name == "clamp_hits":
        inp["shs"] = inp["shs"] * 3.0
    if name == "black_bg":
        inp["bg"] = torch.zeros(3)
    if name == "scale_mod":
        inp["scale_modifier"] = 1.7
    if name == "colors_precomp":
        g = torch.Generator().manual_seed(3)
        inp["shs"] = None
        inp["colors_precomp"] = torch.rand(P, 3, generator=g)
    if name == "cov_precomp":
        # unit-scale covariance from the reference's own helper semantics: Sigma = R S^2 R^T, upper triangle
        from tests.dense_ref import _rot
        Rm = _rot(sc["rotations"].double())
        Lm = Rm * sc["scales"].double()[:, None, :]
        Sg = Lm @ Lm.transpose(1, 2)
        inp["cov3D_precomp"] = torch.stack([Sg[:, 0, 0], Sg[:, 0, 1], Sg[:, 0, 2], Sg[:, 1, 1], Sg[:, 1, 2], Sg[:, 2, 2]], 1).float().contiguous()
        inp["scales"] = None
        inp["rotations"] = None
    if name.startswith("indexed"):
        extra = 16 if name == "indexed_needles" else 64
        ix = synth.index_scene(sc, shs_extra=extra, gs_extra=extra)
        inp.update(shs=ix["shs"], scales=ix["scales"], rotations=ix["rotations"], scale_factors=ix["scale_factors"],
                   sh_indices=ix["sh_indices"], g_indices=ix["g_indices"])
        indexed = True
        if name == "indexed_deg1":
            inp["degree"] = 1
        if name == "indexed_scale_mod":
            inp["scale_modifier"] = 1.3
    return inp, cam, indexed


# Sizes chosen on the CPU so that the reference's own fp32 formula (the oracle) stays a usable yardstick: its deviation from
# float64 grows with cov2D's eigenvalue ratio (det = a c - b^2 cancels), i.e. with a needle's LENGTH IN PIXELS over the 0.3
# low-pass. At these medians it is <= 2e-5 on opaque_big / discs / unnorm_quat and <= 3e-3 on the needle cases; one step up
# (needles_long at 0.1) the oracle and float64 already take different blend decisions.
EDGE_SCALE_MEDIAN = {"opaque_big": 0.25, "needles": 0.1, "needles_long": 0.05, "indexed_needles": 0.1, "discs": 0.06,
                     "unnorm_quat": 0.1, "near_camera": 0.25}
OPAQUE_VALUES = (1.0, 0.9999, 0.999, 0.995, 1.5, 3.0)   # the raw op admits opacity > 1: the reference's min() defines the result
NEAR_STRADDLE, NEAR_CLOSE = 20, 40                      # near_camera: rows [0, 20) straddle the z <= 0.01 cull, [20, 60) lie behind it


def _edge_scene(name, sc, cam, seed):
    """Turns the synth-v1 Gaussians `sc` into the named edge case, in place."""
    P = sc["means3D"].shape[0]
    g = torch.Generator().manual_seed(1000 + seed)
    if name == "opaque_big":
        pick = torch.randint(0, len(OPAQUE_VALUES), (P // 2,), generator=g)
        sc["opacities"][P - P // 2:, 0] = torch.tensor(OPAQUE_VALUES)[pick]
        sc["opacities"][:5] = 0.0
    if name in ("needles", "needles_long", "indexed_needles"):
        a = 10.0 if name == "needles_long" else 5.0
        rows = torch.randperm(P, generator=g)[:P // 2]
        axis = torch.randint(0, 3, (P // 2,), generator=g)
        f = torch.full((P // 2, 3), 1.0 / 30.0)
        f[torch.arange(P // 2), axis] = a
        sc["scales"][rows] *= f
    if name == "discs":
        rows = torch.randperm(P, generator=g)[:P // 2]
        sc["scales"][rows] *= torch.tensor([3.0, 3.0, 1e-3])
        sc["scales"][rows[:20], 2] = 0.0
    if name == "unnorm_quat":
        sc["rotations"] *= torch.exp(0.3 * torch.randn(P, 1, generator=g))
    if name == "near_camera":
        n0, n1 = NEAR_STRADDLE, NEAR_CLOSE
        z = torch.cat([torch.linspace(0.0099, 0.0101, n0, dtype=torch.float64),
                       torch.exp(torch.rand(n1, generator=g, dtype=torch.float64) * np.log(0.3 / 0.011) + np.log(0.011))])
        xy = (torch.rand(n0 + n1, 2, generator=g, dtype=torch.float64) - 0.5) * z[:, None]
        view = torch.from_numpy(cam["viewmatrix"]).double().reshape(4, 4)       # stored transposed: p_view = [p, 1] @ view
        p_view = torch.cat([xy, z[:, None]], 1)
        sc["means3D"][:n0 + n1] = ((p_view - view[3, :3]) @ torch.linalg.inv(view[:3, :3])).float()
        sc["scales"][:n0 + n1] *= 0.05
        sc["opacities"][:n0 + n1] = 0.05


def blend_census(st):
    """Float64 walk of every tile list from the oracle's own per-Gaussian values (means2D, conic_opacity), with the reference's
    fp32 thresholds. -> dict(blends, clamped = blended pairs with o G >= 0.99, stopped = pixels that end on the T(1-alpha) test)."""
    A_MAX, A_THR, T_THR = float(np.float32(0.99)), float(np.float32(1.0) / np.float32(255.0)), float(np.float32(0.0001))
    gx = (st.W + 15) // 16
    m, co = st.means2D.astype(np.float64), st.conic_opacity.astype(np.float64)
    out = dict(blends=0, clamped=0, stopped=0)
    for t in range(st.T):
        ys, xs = np.meshgrid(np.arange((t // gx) * 16, min((t // gx) * 16 + 16, st.H)),
                             np.arange((t % gx) * 16, min((t % gx) * 16 + 16, st.W)), indexing="ij")
        xs, ys = xs.ravel().astype(np.float64), ys.ravel().astype(np.float64)
        T = np.ones(xs.size)
        done = np.zeros(xs.size, bool)
        for gid in st.point_list[st.ranges[t, 0]:st.ranges[t, 1]]:
            dx, dy = m[gid, 0] - xs, m[gid, 1] - ys
            power = -0.5 * (co[gid, 0] * dx * dx + co[gid, 2] * dy * dy) - co[gid, 1] * dx * dy
            raw = co[gid, 3] * np.exp(np.minimum(power, 0.0))
            alpha = np.minimum(A_MAX, raw)
            hit = (power <= 0) & (alpha >= A_THR) & ~done
            stop = hit & (T * (1 - alpha) < T_THR)
            blend = hit & ~stop
            out["blends"] += int(blend.sum())
            out["clamped"] += int((blend & (raw >= A_MAX)).sum())
            out["stopped"] += int(stop.sum())
            T = np.where(blend, T * (1 - alpha), T)
            done |= stop
    return out


# visible Gaussians with a cov2D eigenvalue ratio >= 100 and a radius >= 32 px (two tiles). Measured: 15, 15, 8.
NEEDLE_FLOOR = {"needles": 8, "needles_long": 8, "indexed_needles": 4}


def edge_guard(name, st):
    """What makes `name` the edge case it claims to be, asserted on the oracle state `st`. -> the measured figures."""
    if name == "opaque_big":
        c = blend_census(st)
        assert c["clamped"] >= 0.02 * c["blends"], c        # measured 3.2 %: the clamp needs a pixel within ~0.14 sigma of an opaque mean
        assert c["stopped"] >= 100, c                       # measured 1153 of 6144 pixels
        assert int((st.inputs["opacities"] == 0).sum()) == 5 and float(st.inputs["opacities"].max()) == 3.0
        return c
    if name in NEEDLE_FLOOR:
        a, b, c = (st.conic_opacity[:, k].astype(np.float64) for k in range(3))
        mid, det = 0.5 * (a + c), a * c - b * b
        with np.errstate(invalid="ignore", divide="ignore"):
            root = np.sqrt(np.maximum(mid * mid - det, 0.0))
            ratio = (mid + root) / (mid - root)               # of the conic's eigenvalues = of cov2D's
        n = int(((st.radii > 0) & (ratio >= 100.0) & (st.radii >= 32)).sum())
        assert n >= NEEDLE_FLOOR[name], n
        return dict(needles=n, visible=int((st.radii > 0).sum()), max_radius=int(st.radii.max()))
    if name == "discs":
        s = st.inputs["scales"]
        assert int((s[:, 2] == 0).sum()) == 20 and int((st.radii[s[:, 2] == 0] > 0).sum()) >= 10
        return dict(flat=20)
    if name == "unnorm_quat":
        nrm = np.linalg.norm(st.inputs["rotations"].astype(np.float64), axis=1)
        assert nrm.min() < 0.6 and nrm.max() > 1.6
        return dict(norm_min=float(nrm.min()), norm_max=float(nrm.max()))
    if name == "near_camera":
        r = st.radii[:NEAR_STRADDLE]
        assert (r == 0).any() and (r > 0).any(), r
        full = int((st.tiles_touched[NEAR_STRADDLE:NEAR_STRADDLE + NEAR_CLOSE] == st.T).sum())
        assert full >= 10, full
        return dict(culled=int((r == 0).sum()), kept=int((r > 0).sum()), full_grid=full)
    raise KeyError(name)


def oracle_forward(inp, cam):
    n = {k: (v.numpy() if isinstance(v, torch.Tensor) else v) for k, v in inp.items()}
    return orc.rasterize_forward(bg=n["bg"], means3D=n["means3D"], opacities=n["opacities"], shs=n["shs"],
                                 colors_precomp=n["colors_precomp"], scales=n["scales"], rotations=n["rotations"],
                                 cov3D_precomp=n["cov3D_precomp"], scale_factors=n["scale_factors"],
                                 sh_indices=n["sh_indices"], g_indices=n["g_indices"], degree=n["degree"],
                                 scale_modifier=n["scale_modifier"], prefiltered=n["prefiltered"],
                                 clamp_color=n["clamp_color"], **cam)


FORWARD_CASES = ["tiny", "base", "odd_size", "behind", "all_behind", "empty", "deg0", "deg1", "deg2", "no_clamp",
                 "clamp_hits", "black_bg", "scale_mod", "colors_precomp", "cov_precomp", "frustum_edge", "indexed",
                 "indexed_deg1", "indexed_scale_mod", "wide_depth", "deep_tile", "huge_splats", "one_tile", "p257", "p8193",
                 "p12289", "p24577", "equal_depth", "p1024", "p1025", "p2049", "indexed_p1025"]

# held to the bars of tests/test_edge_gaussians_gpu.py, NOT appended to FORWARD_CASES (a fixed 1e-4 on every gradient)
EDGE_GAUSSIAN_CASES = ["opaque_big", "needles", "needles_long", "indexed_needles", "discs", "unnorm_quat", "near_camera"]
EDGE_WITHIN_TOL = ["opaque_big", "discs", "unnorm_quat"]     # the oracle is within 2e-5 of float64 on these (test_edge_gaussians_cpu.py)


@functools.lru_cache(maxsize=None)
def edge_reference(name):
    """Everything the tests of one edge case compare against, computed ONCE per process and not to be modified: the case, its
    oracle state (guard asserted) and gradients for synth.grad_image, and the float64 truth of tests/dense_ref.py on the same
    discrete structure. d_ref[k] = ||oracle - truth||_inf / ||truth||_inf is the reference's own fp32 deviation."""
    from oracle import oracle as orc
    from tests import dense_ref
    inp, cam, indexed = make_case(name)
    st = oracle_forward(inp, cam)
    guard = edge_guard(name, st)
    dL = synth.grad_image(cam["W"], cam["H"]).numpy()
    ref = orc.rasterize_backward(st, dL)
    img64, truth = dense_ref.truth(st, inp, dL)
    d_ref = {k: float(np.abs(ref[k] - t).max() / max(np.abs(t).max(), 1e-30)) for k, t in truth.items() if t.size}
    return dict(inp=inp, cam=cam, indexed=indexed, st=st, guard=guard, dL=dL, ref=ref, img64=img64, truth=truth, d_ref=d_ref)
