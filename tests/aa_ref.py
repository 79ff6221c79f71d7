"""Torch restatement of the antialiased mode's opacity factor rho (TEST INFRASTRUCTURE; csrc/aa_opacity.hip).

    D0 = a0 c0 - b b,  D1 = (a0 + h)(c0 + h) - b b,  r = D0 / D1,  rho = sqrt(max(0.000025, r)),  o' = o rho

with (a0, b, c0) the 2D covariance of csrc/gsmath.hpp: cov2d() before its 0.3 low-pass. Differentiable and dtype-generic: in
float64 it is the reference the kernels are held to, in float32 -- the same expressions in the same order as
cov3d_from_scale_rot() and cov2d(), matrices element by element with glm's products -- it is a second fp32 evaluation whose
distance from the float64 one is what 40-odd fp32 operations cost on a given scene (f32_deviation), the yardstick of the GPU
bars. The clamp of t.x, t.y at 1.3 tan_fov passes no gradient through the clamped coordinate (tests/dense_ref.py's .detach()).
rho = 1, without a gradient, on a row that fails the forward's near-plane test, has D1 == 0 or a non-finite D0, D1 or r; at the
floor (r <= 0.000025) rho is constant, so its gradient is zero too.

The near-plane test is the one csrc/preprocess.hip applies, view z <= 0.01 (the reference fork's value); upstream 3DGS culls
at 0.2. The `behind` rows of aa_case lie behind both.

aa_case(name) -> the scenes of the antialiasing tests: tests/cases.py scenes with rows rewritten, each with a guard
(aa_guard) asserted from the float64 rho and the oracle's radii, so that a changed seed cannot hollow a case out."""
import functools

import numpy as np
import torch

H_LOWPASS = float(np.float32(0.3))            # the kernels' fp32 constants, as tests/dense_ref.py takes the blend's
R_FLOOR = float(np.float32(0.000025))
RHO_FLOOR32 = np.sqrt(np.float32(0.000025))   # float32: what the kernel writes on a floor row
LIM = float(np.float32(1.3))
NEAR = float(np.float32(0.01))

LEAVES = ("means3D", "opacities", "scales", "rotations", "scale_factors", "cov3D_precomp")


def _mul(a, b):
    """glm operator* on m[col][row] lists: r[c][q] = a[0][q] b[c][0] + a[1][q] b[c][1] + a[2][q] b[c][2]"""
    return [[a[0][q] * b[c][0] + a[1][q] * b[c][1] + a[2][q] * b[c][2] for q in range(3)] for c in range(3)]


def _t(a):
    return [[a[q][c] for q in range(3)] for c in range(3)]


def cov3d(lv, inp):
    """the six entries of Sigma as cov3d_from_scale_rot forms them (or cov3D_precomp), each [P]"""
    if "cov3D_precomp" in lv:
        return [lv["cov3D_precomp"][:, k] for k in range(6)]
    sc, rt = lv["scales"], lv["rotations"]
    mod = float(inp["scale_modifier"])
    if inp.get("g_indices") is not None:
        gi = torch.as_tensor(inp["g_indices"]).to(sc.device)
        sc, rt = sc[gi], rt[gi]
        mod = lv["scale_factors"].reshape(-1) * mod
    zero, one = torch.zeros_like(sc[:, 0]), torch.ones_like(sc[:, 0])
    S = [[mod * sc[:, 0], zero, zero], [zero, mod * sc[:, 1], zero], [zero, zero, mod * sc[:, 2]]]
    r, x, y, z = rt[:, 0], rt[:, 1], rt[:, 2], rt[:, 3]
    R = [[one - 2 * (y * y + z * z), 2 * (x * y - r * z), 2 * (x * z + r * y)],
         [2 * (x * y + r * z), one - 2 * (x * x + z * z), 2 * (y * z - r * x)],
         [2 * (x * z - r * y), 2 * (y * z + r * x), one - 2 * (x * x + y * y)]]
    M = _mul(S, R)
    Sg = _mul(_t(M), M)
    return [Sg[0][0], Sg[0][1], Sg[0][2], Sg[1][1], Sg[1][2], Sg[2][2]]


def terms(lv, inp, cam, keep=None):
    """keep: a dict that receives "cov3D" [P,6], the covariance as an intermediate with retain_grad() set (what dL_dcov3D is the
    gradient of when the covariance is built from scales and rotations).
    -> dict of [P] tensors in the dtype of lv["means3D"]: rho, r, a0, b, c0, z (view-space depth) and the masks valid (rho is
    sqrt(max(floor, r))), floor (valid and r <= floor), clamped (t.x or t.y clamped), behind (fails the near-plane test)"""
    mean = lv["means3D"]
    dt, dev = mean.dtype, mean.device
    v = torch.as_tensor(np.asarray(cam["viewmatrix"], np.float32).reshape(-1), dtype=dt, device=dev)
    scal = lambda s: torch.tensor(s, dtype=dt, device=dev)          # noqa: E731
    tfx, tfy = scal(np.float32(cam["tan_fovx"])), scal(np.float32(cam["tan_fovy"]))
    fx, fy = scal(float(cam["W"])) / (2 * tfx), scal(float(cam["H"])) / (2 * tfy)
    px, py, pz = mean[:, 0], mean[:, 1], mean[:, 2]
    t0 = v[0] * px + v[4] * py + v[8] * pz + v[12]
    t1 = v[1] * px + v[5] * py + v[9] * pz + v[13]
    t2 = v[2] * px + v[6] * py + v[10] * pz + v[14]
    behind = t2 <= NEAR
    tz = torch.where(behind, torch.ones_like(t2), t2)
    limx, limy = scal(LIM) * tfx, scal(LIM) * tfy
    txtz, tytz = t0 / tz, t1 / tz
    cx, cy = (txtz < -limx) | (txtz > limx), (tytz < -limy) | (tytz > limy)
    vx = torch.minimum(limx, torch.maximum(-limx, txtz)) * tz       # the value cov2d() continues with, clamped or not
    vy = torch.minimum(limy, torch.maximum(-limy, tytz)) * tz
    tx = torch.where(cx, vx.detach(), t0 + (vx - t0).detach())      # its gradient: none where clamped, t.x's own otherwise
    ty = torch.where(cy, vy.detach(), t1 + (vy - t1).detach())
    zero = torch.zeros_like(tz)
    J = [[fx / tz, zero, -(fx * tx) / (tz * tz)], [zero, fy / tz, -(fy * ty) / (tz * tz)], [zero, zero, zero]]
    Wm = [[v[0], v[4], v[8]], [v[1], v[5], v[9]], [v[2], v[6], v[10]]]
    T = _mul(Wm, J)
    c6 = cov3d(lv, inp)
    if keep is not None:
        kept = torch.stack(c6, 1)
        kept.retain_grad()
        keep["cov3D"] = kept
        c6 = [kept[:, k] for k in range(6)]
    Vrk = [[c6[0], c6[1], c6[2]], [c6[1], c6[3], c6[4]], [c6[2], c6[4], c6[5]]]
    cov = _mul(_mul(_t(T), _t(Vrk)), T)
    a0, b, c0 = cov[0][0], cov[0][1], cov[1][1]
    h = scal(H_LOWPASS)
    D0 = a0 * c0 - b * b
    D1 = (a0 + h) * (c0 + h) - b * b
    ok = ~behind & torch.isfinite(D0) & torch.isfinite(D1) & (D1 != 0)
    r = torch.where(ok, D0, torch.ones_like(D0)) / torch.where(ok, D1, torch.ones_like(D1))
    valid = ok & torch.isfinite(r)
    r = torch.where(valid, r, torch.ones_like(r))
    floor = scal(R_FLOOR)
    rho = torch.where(valid, torch.sqrt(torch.where(r > floor, r, floor)), torch.ones_like(r))
    return dict(rho=rho, r=r, a0=a0, b=b, c0=c0, z=t2, valid=valid, floor=valid & ~(r > floor), clamped=(cx | cy) & ~behind,
                behind=behind)


def rho(lv, inp, cam):
    return terms(lv, inp, cam)["rho"]


def leaves_of(inp, dtype=torch.float64, device="cpu"):
    """the leaves of tests/dense_ref.py: leaves_of that rho depends on, in `dtype`"""
    return {k: inp[k].detach().to(device=device, dtype=dtype, copy=True).requires_grad_() for k in LEAVES if inp.get(k) is not None}


def hashed(n, salt, signed=True):
    """n reproducible values in [-1, 1) (or [0, 1)), none of them zero: a cotangent or a preset no run can match by accident"""
    i = np.arange(n, dtype=np.uint64)
    u = ((i * np.uint64(2654435761) + np.uint64(salt) * np.uint64(40503) + np.uint64(12345)) % np.uint64(1 << 24)).astype(np.float64)
    u = (u + 0.5) / float(1 << 24)
    return 2.0 * u - 1.0 if signed else u


def vjp(inp, cam, g, dtype=torch.float64, rows=None):
    """(rho, gradients of sum_rows(o rho g) with respect to every leaf and, without cov3D_precomp, to the covariance as "cov3D") in
    `dtype`, as float64 numpy; rows: bool [P] or None"""
    lv = leaves_of(inp, dtype)
    keep = {}
    rh = terms(lv, inp, cam, keep)["rho"]
    w = torch.as_tensor(np.asarray(g, np.float64)).to(dtype)
    if rows is not None:
        w = w * torch.as_tensor(rows).to(dtype)
    (lv["opacities"].reshape(-1) * rh * w).sum().backward()
    if "cov3D_precomp" not in lv:
        lv = dict(lv, cov3D=keep["cov3D"])
    return rh.detach().double().numpy(), {k: (torch.zeros_like(t) if t.grad is None else t.grad).double().numpy() for k, t in lv.items()}


# ---------------------------------------------------------------------------------------------------------------- cases
AA_CASES = ("floor", "needles", "clamped", "behind", "indexed", "indexed_scale_mod", "cov_precomp")
BASE_OF = {"floor": "base", "needles": "base", "clamped": "frustum_edge", "behind": "behind", "indexed": "indexed",
           "indexed_scale_mod": "indexed_scale_mod", "cov_precomp": "cov_precomp"}
N_FLOOR, N_NEEDLES, N_SMALL = 200, 400, 800


@functools.lru_cache(maxsize=None)
def aa_case(name):
    """-> dict(inp, cam, indexed, radii (the oracle's), t (terms in float64, numpy), guard): computed once per process, not to be
    modified. inp / cam are those of cases.make_case, at most 4000 Gaussians at 200 x 136."""
    from tests import cases
    inp, cam, indexed = cases.make_case(BASE_OF[name])
    inp = {k: (v.clone() if isinstance(v, torch.Tensor) else v) for k, v in inp.items()}
    P = inp["means3D"].shape[0]
    g = torch.Generator().manual_seed(2024)
    if name == "floor":          # sub-pixel specks: sigma / z <= 3e-4, far below the low-pass, which still gives them radius 2
        inp["scales"][:N_FLOOR] *= (torch.rand(N_FLOOR, 1, generator=g) * 0.02 + 0.01)
    if name == "needles":        # one axis x 5, the others / 30: large b, D0 = a0 c0 - b b cancels
        axis = torch.randint(0, 3, (N_NEEDLES,), generator=g)
        f = torch.full((N_NEEDLES, 3), 1.0 / 30.0)
        f[torch.arange(N_NEEDLES), axis] = 5.0
        inp["scales"][:N_NEEDLES] *= f
    if name == "clamped":        # frustum_edge triples every scale: shrink rows the clamp does not touch, for small rho as well
        with torch.no_grad():
            free = ~terms(leaves_of(inp), inp, cam)["clamped"]
        rows = torch.nonzero(free).squeeze(1)[:N_SMALL]
        inp["scales"][rows] *= 0.1
    if name.startswith("indexed"):   # several Gaussians per codebook row: every fifth Gaussian shares one of 16 rows
        inp["g_indices"][::5] = inp["g_indices"][::5] % 16
    st = cases.oracle_forward(inp, cam)
    radii = np.asarray(st.radii).copy()
    with torch.no_grad():
        t = {k: v.numpy() for k, v in terms(leaves_of(inp), inp, cam).items()}
    return dict(inp=inp, cam=cam, indexed=indexed, radii=radii, t=t, guard=aa_guard(name, inp, radii, t))


def aa_guard(name, inp, radii, t):
    """what makes `name` the case it claims to be, from the float64 rho and the oracle's radii -> the measured figures"""
    vis = radii > 0
    assert np.isfinite(t["rho"]).all()
    fig = dict(visible=int(vis.sum()), floor=int((vis & t["floor"]).sum()), clamped=int((vis & t["clamped"]).sum()),
               behind=int(t["behind"].sum()))
    rest = vis & t["valid"] & ~t["floor"]
    fig["rho_min"], fig["rho_max"] = float(t["rho"][rest].min()), float(t["rho"][rest].max())
    assert fig["rho_min"] < 0.2 and fig["rho_max"] > 0.9, fig
    assert not (vis & t["behind"]).any()
    if name == "floor":
        assert fig["floor"] >= 10, fig
    if name == "clamped":
        assert fig["clamped"] >= 10, fig
    if name == "behind":
        assert fig["behind"] >= 10 and float(t["z"][t["behind"]].max()) <= 0.2, fig
    if name == "needles":
        # cancelling: b b within 10 % of a0 c0 on visible rows that are not at the floor
        canc = rest & (t["b"] ** 2 > 0.9 * t["a0"] * t["c0"])
        fig["cancelling"] = int(canc.sum())
        assert fig["cancelling"] >= 10, fig
    if name.startswith("indexed"):
        gi = np.asarray(inp["g_indices"])
        fig["max_shared"] = int(np.bincount(gi[vis]).max())
        assert fig["max_shared"] >= 8, fig
        if name == "indexed_scale_mod":
            assert float(inp["scale_modifier"]) != 1.0
    return fig


def interior_rows(name, n=16):
    """n visible rows of the case away from the floor and from the clamp edge: where rho is smooth (gradcheck)"""
    c = aa_case(name)
    t, cam = c["t"], c["cam"]
    mean = c["inp"]["means3D"].double().numpy()
    v = np.asarray(cam["viewmatrix"], np.float64).reshape(-1)
    z = v[2] * mean[:, 0] + v[6] * mean[:, 1] + v[10] * mean[:, 2] + v[14]
    x = v[0] * mean[:, 0] + v[4] * mean[:, 1] + v[8] * mean[:, 2] + v[12]
    y = v[1] * mean[:, 0] + v[5] * mean[:, 1] + v[9] * mean[:, 2] + v[13]
    with np.errstate(divide="ignore", invalid="ignore"):
        ex = np.abs(np.abs(x / z) / (LIM * cam["tan_fovx"]) - 1.0)
        ey = np.abs(np.abs(y / z) / (LIM * cam["tan_fovy"]) - 1.0)
    ok = (c["radii"] > 0) & t["valid"] & (t["r"] > 4 * R_FLOOR) & (ex > 0.02) & (ey > 0.02)
    rows = np.nonzero(ok)[0]
    assert len(rows) >= n, (name, len(rows))
    return rows[np.linspace(0, len(rows) - 1, n).astype(np.int64)]


def sub_case(name, rows):
    """the case restricted to `rows` (and, indexed, to the codebook rows they use): small enough for torch.autograd.gradcheck"""
    c = aa_case(name)
    rows_t = torch.as_tensor(rows)
    per_row = ("means3D", "opacities", "scale_factors", "cov3D_precomp", "g_indices")
    if c["inp"].get("g_indices") is None:
        per_row = per_row + ("scales", "rotations")
    inp = {k: (v[rows_t].clone() if (k in per_row and isinstance(v, torch.Tensor)) else v) for k, v in c["inp"].items()}
    if inp.get("g_indices") is not None:
        used, inp["g_indices"] = torch.unique(inp["g_indices"], return_inverse=True)
        inp["scales"], inp["rotations"] = inp["scales"][used].clone(), inp["rotations"][used].clone()
    return inp, c["cam"]


@functools.lru_cache(maxsize=None)
def f32_deviation(name):
    """How far a second fp32 evaluation of the same formulas lands from float64 on this case, reference against reference:
    -> dict(rho = max_i |rho32_i - rho64_i| over all rows, and per leaf the rel-inf (max abs difference over the float64 max abs)
    of the VJP of sum_{visible} o rho g under the hashed cotangent g = hashed(P, 7))"""
    c = aa_case(name)
    P = c["inp"]["means3D"].shape[0]
    g, rows = hashed(P, 7), c["radii"] > 0
    r64, v64 = vjp(c["inp"], c["cam"], g, torch.float64, rows)
    r32, v32 = vjp(c["inp"], c["cam"], g, torch.float32, rows)
    out = dict(rho=float(np.abs(r32 - r64).max()))
    for k in v64:
        out[k] = float(np.abs(v32[k] - v64[k]).max() / max(np.abs(v64[k]).max(), 1e-30))
    return out
