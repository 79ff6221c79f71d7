"""Float64 references for the exact camera-pose gradient (csrc/pose_grad.hip) -- TEST INFRASTRUCTURE.

(a) pose_render: tests/dense_ref.py's dense render restated with the 7-element pose (qx, qy, qz, qw, tx, ty, tz) as an autograd
    leaf: view, proj and campos = -R^-1 t are built in float64 torch from the pose by camera_from_pose_kernel's formulas (the
    quaternion is NOT normalised), everything downstream is dense_ref's math with its semantics (straight-through 0.99 clamp,
    no gradient through a t-clamped coordinate, the discrete structure borrowed from an oracle forward). pose_truth
    differentiates sum(image * dL) with respect to the pose.
(b) pose_grad_ref: numpy float64 restatement of what the kernels compute from given per-Gaussian gradient arrays: the 24 sums
        S_g = sum g, S_d = sum gdir, M1 = sum (g - gdir) mu^T, M2 = sum (G + G^T) Sigma
    and the epilogue  dL/dt = R^-T S_g,  dL/dR = R^-T [M1 + M2 + S_d c^T],  chained through the entries of the quaternion matrix.
    The map from the 24 numbers to the seven is linear, so every Gaussian has a contribution [7]: they are returned too (the
    kernel test's bar is relative to the sum of their magnitudes).
"""
import functools

import numpy as np
import torch

from tests import dense_ref

DD = torch.float64
NONUNIT_POSE = (0.3, -0.2, 0.1, 1.2, 0.1, -0.05, 0.4)      # |q|^2 = 1.58: R is far from orthonormal


# ----------------------------------------------------------------------------- (a) the render with the pose as a leaf
def _rot_of_pose(x, y, z, w):
    d2 = y * y + z * z + x * x
    return [[1.0 + 2.0 * (x * x - d2), 2.0 * (x * y - w * z), 2.0 * (x * z + w * y)],
            [2.0 * (x * y + w * z), 1.0 + 2.0 * (y * y - d2), 2.0 * (y * z - w * x)],
            [2.0 * (x * z - w * y), 2.0 * (y * z + w * x), 1.0 + 2.0 * (z * z - d2)]]


def camera_from_pose(pose, tan_fovx, tan_fovy):
    """pose: float64 tensor [7] -> (R [3,3] world->camera, t [3], proj [4,4] (row-vector convention, like the library's
    transposed matrices), campos [3]); differentiable."""
    R = torch.stack([torch.stack(r) for r in _rot_of_pose(pose[0], pose[1], pose[2], pose[3])])
    t = pose[4:7]
    view = torch.cat([torch.cat([R.T, torch.zeros(3, 1, dtype=DD)], 1),
                      torch.cat([t.reshape(1, 3), torch.ones(1, 1, dtype=DD)], 1)], 0)      # = W2C^T
    znear, zfar = 0.01, 100.0
    Pm = torch.tensor([[1.0 / tan_fovx, 0, 0, 0], [0, 1.0 / tan_fovy, 0, 0],
                       [0, 0, zfar / (zfar - znear), -(zfar * znear) / (zfar - znear)], [0, 0, 1.0, 0]], dtype=DD)
    campos = -torch.linalg.solve(R, t)
    return R, t, view @ Pm.T, campos


def pose_render(st, leaves, pose):
    """dense_ref.dense_render with the camera taken from `pose` (float64 leaf) instead of st.inputs' matrices."""
    i = st.inputs
    W, H = st.W, st.H
    tfx, tfy = float(i["tan_fovx"]), float(i["tan_fovy"])
    fx, fy = W / (2.0 * tfx), H / (2.0 * tfy)
    Rw, tw, proj, campos = camera_from_pose(pose, tfx, tfy)
    mean = leaves["means3D"]
    P = mean.shape[0]
    ones = torch.ones(P, 1, dtype=DD)
    hom = torch.cat([mean, ones], 1) @ proj
    p_w = 1.0 / (hom[:, 3] + 0.0000001)
    ndc = hom[:, :2] * p_w[:, None]
    t = mean @ Rw.T + tw

    if "cov3D_precomp" in leaves:
        c6 = leaves["cov3D_precomp"]
        Sigma = torch.stack([c6[:, 0], c6[:, 1], c6[:, 2], c6[:, 1], c6[:, 3], c6[:, 4], c6[:, 2], c6[:, 4], c6[:, 5]],
                            -1).reshape(-1, 3, 3)
    else:
        sc, rt = leaves["scales"], leaves["rotations"]
        mod = float(i["scale_modifier"])
        if i["g_indices"] is not None:
            gi = torch.as_tensor(i["g_indices"])
            s = sc[gi] * (leaves["scale_factors"].reshape(-1, 1) * mod)
            Rm = dense_ref._rot(rt[gi])
        else:
            s = sc * mod
            Rm = dense_ref._rot(rt)
        Lm = Rm * s[:, None, :]
        Sigma = Lm @ Lm.transpose(1, 2)

    limx, limy = 1.3 * tfx, 1.3 * tfy
    txtz, tytz = t[:, 0] / t[:, 2], t[:, 1] / t[:, 2]
    cx = (txtz < -limx) | (txtz > limx)
    cy = (tytz < -limy) | (tytz > limy)
    tx = torch.where(cx, (txtz.clamp(-limx, limx) * t[:, 2]).detach(), t[:, 0])
    ty = torch.where(cy, (tytz.clamp(-limy, limy) * t[:, 2]).detach(), t[:, 1])
    tz = t[:, 2]
    zero = torch.zeros_like(tz)
    J = torch.stack([fx / tz, zero, -(fx * tx) / (tz * tz), zero, fy / tz, -(fy * ty) / (tz * tz)], -1).reshape(-1, 2, 3)
    A = J @ Rw
    cov = A @ Sigma @ A.transpose(1, 2)
    a, b, c = cov[:, 0, 0] + 0.3, cov[:, 0, 1], cov[:, 1, 1] + 0.3
    det = a * c - b * b
    con = torch.stack([c / det, -b / det, a / det], -1)

    pixx = ((ndc[:, 0] + 1.0) * W - 1.0) * 0.5
    pixy = ((ndc[:, 1] + 1.0) * H - 1.0) * 0.5

    if "colors_precomp" in leaves:
        col = leaves["colors_precomp"]
    else:
        sh = leaves["shs"]
        if i["sh_indices"] is not None:
            sh = sh[torch.as_tensor(i["sh_indices"])]
        d = mean - campos
        d = d / d.norm(dim=1, keepdim=True)
        col = dense_ref._sh_color(int(i["degree"]), sh, d) + 0.5
        if i["clamp_color"]:
            col = torch.clamp_min(col, 0.0)

    opac = leaves["opacities"].reshape(-1)
    bg = torch.tensor(i["bg"], dtype=DD)
    img = torch.zeros(3, H, W, dtype=DD)
    gx = (W + 15) // 16
    A_MAX, A_THR, T_THR = dense_ref.A_MAX, dense_ref.A_THR, dense_ref.T_THR
    for tile in range(st.T):
        r0, r1 = int(st.ranges[tile, 0]), int(st.ranges[tile, 1])
        tx0, ty0 = (tile % gx) * 16, (tile // gx) * 16
        xs = torch.arange(tx0, min(tx0 + 16, W), dtype=DD)
        ys = torch.arange(ty0, min(ty0 + 16, H), dtype=DD)
        if len(xs) == 0 or len(ys) == 0:
            continue
        py, px = torch.meshgrid(ys, xs, indexing="ij")
        T = torch.ones_like(px)
        Cc = torch.zeros(3, *px.shape, dtype=DD)
        done = torch.zeros_like(px, dtype=torch.bool)
        for k in range(r0, r1):
            g = int(st.point_list[k])
            dx, dy = pixx[g] - px, pixy[g] - py
            power = -0.5 * (con[g, 0] * dx * dx + con[g, 2] * dy * dy) - con[g, 1] * dx * dy
            G = torch.exp(power)
            raw = opac[g] * G
            alpha = torch.clamp_max(raw, A_MAX)
            alpha = raw + (alpha - raw).detach()
            ok = (power <= 0) & (alpha >= A_THR) & ~done
            test_T = T * (1 - alpha)
            newly = ok & (test_T < T_THR)
            done = done | newly
            contrib = ok & ~newly
            Cc = Cc + torch.where(contrib, alpha * T, torch.zeros_like(T))[None] * col[g][:, None, None]
            T = torch.where(contrib, test_T, T)
        y0, x0 = int(ys[0]), int(xs[0])
        img[:, y0:y0 + len(ys), x0:x0 + len(xs)] = Cc + T[None] * bg[:, None, None]
    return img


def pose_truth(st, inp, pose, dL):
    """-> (image [3,H,W] float64 numpy, d sum(image * dL) / d pose [7] float64 numpy). The model's leaves carry no gradient."""
    lv = {}
    for k in ("means3D", "opacities", "shs", "colors_precomp", "scales", "rotations", "cov3D_precomp", "scale_factors"):
        if inp.get(k) is not None:
            lv[k] = inp[k].to(DD)
    p = torch.as_tensor(np.asarray(pose, dtype=np.float32)).to(DD).requires_grad_()
    img = pose_render(st, lv, p)
    (img * torch.as_tensor(dL, dtype=DD)).sum().backward()
    return img.detach().numpy(), p.grad.numpy()


# ----------------------------------------------------------------------------- (b) the kernels' arithmetic in float64
def sigma_of(inp):
    """Sigma_i [P,3,3] float64 from a tests/cases.py input dict: cov3D_precomp, or R diag(s)^2 R^T with s = scale x modifier
    (x scale factor, codebook rows through g_indices, on the indexed path)."""
    f = lambda k: None if inp.get(k) is None else np.asarray(inp[k], dtype=np.float64)
    if inp.get("cov3D_precomp") is not None:
        c = f("cov3D_precomp")
        return np.stack([c[:, 0], c[:, 1], c[:, 2], c[:, 1], c[:, 3], c[:, 4], c[:, 2], c[:, 4], c[:, 5]], -1).reshape(-1, 3, 3)
    sc, rt, mod = f("scales"), f("rotations"), float(inp.get("scale_modifier", 1.0))
    if inp.get("g_indices") is not None:
        gi = np.asarray(inp["g_indices"])
        s = sc[gi] * (f("scale_factors").reshape(-1, 1) * mod)
        rt = rt[gi]
    else:
        s = sc * mod
    Rm = dense_ref._rot(torch.from_numpy(rt)).numpy()
    Lm = Rm * s[:, None, :]
    return Lm @ Lm.transpose(0, 2, 1)


def direction_part(inp, campos, dL_dcolors, clamped, radii):
    """gdir [P,3]: the share of dL/dmean that arrives through the SH view direction (oracle.sh_backward; zero with precomputed
    colours, at degree 0 and for culled rows). clamped: [P,3] channel flags of the forward."""
    from oracle import oracle as orc
    P = int(np.asarray(inp["means3D"]).shape[0])
    out = np.zeros((P, 3), np.float64)
    deg = int(inp.get("degree", 0))
    if inp.get("shs") is None or deg == 0 or P == 0:
        return out
    sh = np.asarray(inp["shs"], dtype=np.float32)
    if inp.get("sh_indices") is not None:
        sh = sh[np.asarray(inp["sh_indices"])]
    vis = np.asarray(radii) > 0
    if vis.any():
        _, dmean = orc.sh_backward(deg, np.asarray(inp["means3D"], dtype=np.float32)[vis], np.asarray(campos, dtype=np.float32),
                                   np.ascontiguousarray(sh[vis]), np.asarray(dL_dcolors, dtype=np.float32)[vis],
                                   np.asarray(clamped)[vis])
        out[vis] = dmean
    return out


def pose_camera(pose):
    """float64 (R, R^-1, t, c = -R^-1 t) of a pose, the matrix entries from the pose's fp32 values."""
    x, y, z, w, tx, ty, tz = [float(v) for v in np.asarray(pose, dtype=np.float32)]
    R = np.array(_rot_of_pose(x, y, z, w), dtype=np.float64)
    inv = np.linalg.inv(R)
    t = np.array([tx, ty, tz])
    return R, inv, t, -(inv @ t)


def pose_distance(a, b):
    """Distance of two poses in what the image depends on. The render is exactly invariant under (R, t) -> (s R, s t): p scales
    by s, the projection divides by depth, R Sigma R^T scales by s^2 and the Jacobian by 1/s, c = -R^-1 t stays. The 7-vector
    therefore has a direction no loss can see (the unnormalised quaternion's R is not orthonormal, so s is free), and noise
    along it cannot be refined away. Measured here: |c_a - c_b| + ||R_a / det(R_a)^(1/3) - R_b / det(R_b)^(1/3)||_F."""
    out = []
    for p in (a, b):
        p = p.detach().cpu().numpy() if isinstance(p, torch.Tensor) else p
        R, _, _, c = pose_camera(p)
        out.append((R / np.cbrt(np.linalg.det(R)), c))
    return float(np.linalg.norm(out[0][1] - out[1][1]) + np.linalg.norm(out[0][0] - out[1][0]))


def pose_epilogue(pose, v):
    """v [..., 24] = (S_g, S_d, M1 row major, M2 row major) -> dL/dpose [..., 7]; linear in v."""
    v = np.asarray(v, dtype=np.float64)
    x, y, z, w = [float(q) for q in np.asarray(pose, dtype=np.float32)[:4]]
    _, inv, _, c = pose_camera(pose)
    Sg, Sd = v[..., 0:3], v[..., 3:6]
    S = v[..., 6:15].reshape(v.shape[:-1] + (3, 3)) + v[..., 15:24].reshape(v.shape[:-1] + (3, 3)) + Sd[..., :, None] * c
    D = np.einsum("ka,...kb->...ab", inv, S)                  # R^-T S
    dt = np.einsum("ka,...k->...a", inv, Sg)
    d = lambda r, q: D[..., r, q]
    dqx = 2 * (y * (d(0, 1) + d(1, 0)) + z * (d(0, 2) + d(2, 0)) + w * (d(2, 1) - d(1, 2))) - 4 * x * (d(1, 1) + d(2, 2))
    dqy = 2 * (x * (d(0, 1) + d(1, 0)) + z * (d(1, 2) + d(2, 1)) + w * (d(0, 2) - d(2, 0))) - 4 * y * (d(0, 0) + d(2, 2))
    dqz = 2 * (x * (d(0, 2) + d(2, 0)) + y * (d(1, 2) + d(2, 1)) + w * (d(1, 0) - d(0, 1))) - 4 * z * (d(0, 0) + d(1, 1))
    dqw = 2 * (z * (d(1, 0) - d(0, 1)) + y * (d(0, 2) - d(2, 0)) + x * (d(2, 1) - d(1, 2)))
    return np.concatenate([np.stack([dqx, dqy, dqz, dqw], -1), dt], -1)


def pose_grad_ref(pose, means3D, sigma, radii, dL_dmeans3D, dL_dcov3D, gdir):
    """-> (dL/dpose [7], contributions [P,7]) in float64 from fp32 / float64 per-Gaussian arrays; rows with radii <= 0 are skipped."""
    mu = np.asarray(means3D, dtype=np.float64).reshape(-1, 3)
    P = mu.shape[0]
    g = np.asarray(dL_dmeans3D, dtype=np.float64).reshape(P, 3)
    dc = np.asarray(dL_dcov3D, dtype=np.float64).reshape(P, 6)
    gd = np.asarray(gdir, dtype=np.float64).reshape(P, 3)
    # G + G^T: an off-diagonal entry of the six is already the derivative with respect to BOTH symmetric positions
    G2 = np.stack([2 * dc[:, 0], dc[:, 1], dc[:, 2], dc[:, 1], 2 * dc[:, 3], dc[:, 4], dc[:, 2], dc[:, 4], 2 * dc[:, 5]], -1).reshape(P, 3, 3)
    M1 = (g - gd)[:, :, None] * mu[:, None, :]
    M2 = G2 @ np.asarray(sigma, dtype=np.float64).reshape(P, 3, 3)
    v = np.concatenate([g, gd, M1.reshape(P, 9), M2.reshape(P, 9)], 1)
    v[np.asarray(radii).reshape(P) <= 0] = 0.0
    contrib = pose_epilogue(pose, v) if P else np.zeros((0, 7))
    return contrib.sum(0), contrib


# ----------------------------------------------------------------------------- shared references
CASE_POSE = (0.05, -0.03, 0.02, 0.99, 0.1, -0.05, 0.2)     # the pose tests/cases.py renders every case from
SMALL = dict(W=64, H=64, focal=40.0, scale_median=0.09)    # 4 x 4 tiles, the splats' pixel footprint of the 200 x 136 original


def make_pose_case(name, **kw):
    """A tests/cases.py case on a small image, and its pose. "nonunit_quat" is `tiny` seen from NONUNIT_POSE; every case but
    `tiny` (48 x 32) is made with SMALL and P = 800 unless `kw` says otherwise: the float64 walk of `reference` is a Python
    loop over every list entry. -> (inp, cam, indexed, pose fp32 [7], intrinsic tensor [3,3])"""
    from oracle import oracle as orc
    from tests import cases, synth
    pose, case = CASE_POSE, name
    if name == "nonunit_quat":
        pose, case = NONUNIT_POSE, "tiny"
    args = {} if case == "tiny" else dict(dict(P=800, **SMALL), **kw)
    inp, cam, indexed = cases.make_case(case, **args)
    intr, ev = synth.camera(cam["W"], cam["H"], 40.0, extrinsic_vector=pose)
    if pose is not CASE_POSE:
        cam = orc.camera(intr.numpy(), ev.numpy())
    return inp, cam, indexed, ev.numpy(), intr


@functools.lru_cache(maxsize=None)
def reference(name):
    """Everything the tests of one case compare against, computed ONCE per process and not to be modified: the case, its oracle
    forward and backward for synth.grad_image, pose_grad_ref on the oracle's gradients, and the float64 autograd truth."""
    from oracle import oracle as orc
    from tests import cases, synth
    inp, cam, indexed, pose, intr = make_pose_case(name)
    st = cases.oracle_forward(inp, cam)
    dL = synth.grad_image(cam["W"], cam["H"]).numpy()
    ref = orc.rasterize_backward(st, dL)
    gdir = direction_part(inp, cam["campos"], ref["dL_dcolors"], st.clamped, st.radii)
    grad, contrib = pose_grad_ref(pose, inp["means3D"].numpy(), sigma_of(inp), st.radii, ref["dL_dmeans3D"], ref["dL_dcov3D"], gdir)
    img64, truth = pose_truth(st, inp, pose, dL)
    return dict(inp=inp, cam=cam, indexed=indexed, pose=pose, intrinsic=intr, st=st, dL=dL, ref=ref, gdir=gdir, grad=grad, contrib=contrib,
                img64=img64, truth=truth)


# ----------------------------------------------------------------------------- the pose-refinement problem (GPU)
def refine_problem(device="cuda", noisy=(1, 5), noise=0.02, seed=5):
    """tests/train_scene.py's toy scene as a pose-refinement problem: its 4000-Gaussian teacher as an INDEXED model (both pose
    gradients exist there), its 8 views 160 x 112 rendered from the true poses as ground truth, and the poses of the cameras
    `noisy` moved by noise * N(0, 1) per element. -> (model, cameras, {camera index: true pose [7] on the device})"""
    from c3dgs_amd.model import GaussianModel, PipelineParams
    from tests import synth, train_scene
    W, H, focal = 160, 112, 150.0
    sc = synth.scene(4000, W=W, H=H, focal=focal, seed=31, scale_median=0.06, zmin=3.0, zmax=8.0)
    sc["opacities"] = sc["opacities"].clamp(0.3, 1 - 1e-6)
    model = GaussianModel(3, quantization=False, device=device)
    model.set_tensors(**synth.raw_params(synth.index_scene(sc, seed=24, shs_extra=64, gs_extra=64)))
    cams, bg = [], torch.zeros(3, device=device)
    for k in range(8):
        a = 2 * np.pi * k / 8
        ev = (0.015 * np.sin(a), 0.015 * np.cos(a), 0.0, 1.0, 0.25 * np.cos(a), 0.25 * np.sin(a), 0.0)
        intr, e = synth.camera(W, H, focal, extrinsic_vector=ev)
        cam = train_scene.Cam(intr, e, device)
        with torch.no_grad():
            cam.original_image = model.render(cam, PipelineParams(), bg)["render"].clamp(0, 1).clone()
        cams.append(cam)
    g = torch.Generator().manual_seed(seed)
    true = {}
    for k in noisy:
        true[k] = cams[k].extrinsic_vector.clone()
        cams[k].extrinsic_vector = (true[k] + noise * torch.randn(7, generator=g).to(device)).contiguous()
    return model, cams, true
