"""-m gpu: GaussianModel PLY IO (load_ply / save_ply / load, c3dgs_amd/model.py) against restatements of the
reference's formulas (scene/gaussian_model.py:324-503) on PLY files this test assembles byte by byte, and the
npz2ply converter end to end."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from tests import knn_ref, synth

pytestmark = pytest.mark.gpu
DEV = "cuda"
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
C0 = 0.28209479177387814


class _Cam:
    def __init__(self, intrinsic, ev):
        self.intrinsic, self.extrinsic_vector = intrinsic.to(DEV), ev.to(DEV)


def _write_ply(path, cols, types=None, fmt="binary_little_endian"):
    """Header and records assembled here, not through c3dgs_amd.ply.write_ply."""
    types = types or {}
    n = len(next(iter(cols.values())))
    lines = ["ply", f"format {fmt} 1.0", "comment hand-made", f"element vertex {n}"]
    lines += [f"property {types.get(k, 'float')} {k}" for k in cols]
    lines.append("end_header")
    code = {"float": "<f4", "uchar": "u1", "double": "<f8"}
    rec = np.empty(n, dtype=[(k, code[types.get(k, "float")]) for k in cols])
    for k, v in cols.items():
        rec[k] = v
    with open(path, "wb") as f:
        f.write(("\n".join(lines) + "\n").encode())
        f.write(rec.tobytes())
    return str(path)


def _trained_cols(P, degree, seed):
    g = np.random.default_rng(seed)
    K = (degree + 1) ** 2 - 1
    c = {"x": g.normal(size=P), "y": g.normal(size=P), "z": g.uniform(3, 9, size=P)}
    c.update({"nx": np.zeros(P), "ny": np.zeros(P), "nz": np.zeros(P)})
    c.update({f"f_dc_{i}": g.normal(size=P) * 0.5 for i in range(3)})
    rest = {f"f_rest_{i}": g.normal(size=P) * 0.05 for i in range(3 * K)}
    for k in g.permutation(list(rest)):                       # property order scrambled: load sorts by the number
        c[str(k)] = rest[k]
    c["opacity"] = g.normal(size=P)
    c.update({f"scale_{i}": np.log(0.01) + 0.5 * g.normal(size=P) for i in range(3)})
    c.update({f"rot_{i}": g.normal(size=P) for i in range(4)})
    return {k: v.astype(np.float32) for k, v in c.items()}, K


def _expected(cols, K, factor):
    P = len(cols["x"])
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a, np.float32)).to(DEV)  # noqa: E731
    rest = np.stack([cols[f"f_rest_{i}"] for i in range(3 * K)], 1).reshape(P, 3, K).transpose(0, 2, 1)
    s = t(np.stack([cols[f"scale_{i}"] for i in range(3)], 1))
    e = {"xyz": t(np.stack([cols["x"], cols["y"], cols["z"]], 1)),
         "features_dc": t(np.stack([cols[f"f_dc_{i}"] for i in range(3)], 1)[:, None, :]),
         "features_rest": t(rest), "opacity": t(cols["opacity"][:, None]),
         "rotation": t(np.stack([cols[f"rot_{i}"] for i in range(4)], 1))}
    if factor:
        ex = torch.exp(s)
        nrm = ex.norm(2, -1, keepdim=True)
        e["scaling"], e["scaling_factor"] = ex / nrm, torch.log(nrm)
    else:
        e["scaling"], e["scaling_factor"] = s, None
    return e


def _assert_model(m, e):
    for k, want in e.items():
        got = getattr(m, "_" + k)
        if want is None:
            assert got is None, k
            continue
        assert got.shape == want.shape and got.dtype == torch.float32 and got.is_contiguous(), k
        assert torch.equal(got.detach().view(torch.int32), want.view(torch.int32)), k
        assert got.requires_grad, k


@pytest.mark.parametrize("factor", [True, False])
@pytest.mark.parametrize("degree", [3, 1])
def test_load_trained_layout(hip, tmp_path, degree, factor):
    from c3dgs_amd.model import GaussianModel
    cols, K = _trained_cols(3000, degree, seed=degree * 2 + factor)
    path = _write_ply(tmp_path / "trained.ply", cols)
    m = GaussianModel(3, quantization=False, use_factor_scaling=factor).load(path)
    assert m.active_sh_degree == degree and m.max_sh_degree == 3
    _assert_model(m, _expected(cols, K, factor))
    assert not m.is_color_indexed and not m.is_gaussian_indexed
    assert m.max_radii2D.shape == (3000,) and float(m.max_radii2D.abs().sum()) == 0.0


def test_degree1_render_equals_direct_rasterizer(hip, tmp_path):
    from c3dgs_amd.model import GaussianModel, PipelineParams
    from c3dgs_amd.rasterizer import GaussianRasterizationSettings, GaussianRasterizer
    W, H = 640, 360
    sc = synth.scene(20000, W=W, H=H, focal=400.0, seed=5, scale_median=0.02, sh_degree=1)
    P = 20000
    cols = {"x": sc["means3D"][:, 0], "y": sc["means3D"][:, 1], "z": sc["means3D"][:, 2]}
    cols.update({f"f_dc_{i}": sc["shs"][:, 0, i] for i in range(3)})
    rest = sc["shs"][:, 1:].transpose(1, 2).reshape(P, 9)
    cols.update({f"f_rest_{i}": rest[:, i] for i in range(9)})
    op = sc["opacities"].clamp(1e-4, 1 - 1e-4)
    cols["opacity"] = torch.log(op / (1 - op))[:, 0]
    cols.update({f"scale_{i}": torch.log(sc["scales"][:, i]) for i in range(3)})
    cols.update({f"rot_{i}": sc["rotations"][:, i] * 1.7 for i in range(4)})
    path = _write_ply(tmp_path / "d1.ply", {k: v.numpy() for k, v in cols.items()})
    m = GaussianModel(3, quantization=False, use_factor_scaling=False).load_ply(path)
    m.opacity_qa.disable_fake_quant()                         # the reference keeps this one on even without quantization
    m.opacity_qa.disable_observer()
    intr, ev = synth.camera(W, H, 400.0)
    cam, bg = _Cam(intr, ev), torch.tensor([0.1, 0.2, 0.3], device=DEV)
    img = m.render(cam, PipelineParams(), bg)["render"].detach()
    settings = GaussianRasterizationSettings(intrinsic=cam.intrinsic, extrinsic_vector=cam.extrinsic_vector, bg=bg,
                                             scale_modifier=1.0, sh_degree=1, prefiltered=False, debug=False, clamp_color=True)
    rast = GaussianRasterizer(raster_settings=settings)
    # the activated tensors: the model's device getters, which are the reference's activations up to an ulp
    opac, scales, rots = m.get_opacity.detach(), m.get_scaling.detach(), m.get_rotation.detach()
    shs = m.get_features.detach()
    torch.testing.assert_close(opac, torch.sigmoid(m._opacity.detach()), rtol=1e-6, atol=1e-7)
    torch.testing.assert_close(scales, torch.exp(m._scaling.detach()), rtol=1e-6, atol=0)
    torch.testing.assert_close(rots, torch.nn.functional.normalize(m._rotation.detach()), rtol=1e-6, atol=1e-7)
    assert torch.equal(shs, torch.cat((m._features_dc, m._features_rest), 1).detach()) and shs.shape == (P, 4, 3)
    xyz = m._xyz.detach()
    vis = rast.markVisible(xyz, extrinsic_vector=cam.extrinsic_vector)
    direct, _ = rast(means3D=xyz[vis], means2D=torch.zeros_like(xyz)[vis], shs=shs[vis], colors_precomp=None,
                     opacities=opac[vis], scales=scales[vis], rotations=rots[vis], cov3D_precomp=None,
                     extrinsic_vector=cam.extrinsic_vector)
    assert float(img.sum()) > 0
    assert torch.equal(img, direct), float((img - direct).abs().max())


@pytest.mark.parametrize("factor", [False, True])
def test_load_point_cloud(hip, tmp_path, factor):
    from c3dgs_amd.model import GaussianModel
    g = np.random.default_rng(8)
    P = 5000
    xyz = (g.normal(size=(P, 3)) * [2, 1, 0.5]).astype(np.float32)
    xyz[10] = xyz[11]
    rgb = g.integers(0, 256, size=(P, 3)).astype(np.uint8)
    cols = {"x": xyz[:, 0], "y": xyz[:, 1], "z": xyz[:, 2], "nx": np.zeros(P), "ny": np.zeros(P), "nz": np.zeros(P),
            "red": rgb[:, 0], "green": rgb[:, 1], "blue": rgb[:, 2]}
    types = {"red": "uchar", "green": "uchar", "blue": "uchar"}
    path = _write_ply(tmp_path / "points3D.ply", cols, types)
    m = GaussianModel(3, quantization=False, use_factor_scaling=factor).load_ply(path)
    assert m.active_sh_degree == 0
    dc = ((rgb.astype(np.float64) / 255.0 - 0.5) / C0).astype(np.float32)[:, None, :]
    assert torch.equal(m._features_dc.detach().cpu(), torch.from_numpy(dc))
    assert m._features_rest.shape == (P, 15, 3) and float(m._features_rest.detach().abs().sum()) == 0.0
    assert torch.equal(m._opacity.detach().cpu(), torch.full((P, 1), float(np.float32(np.log(0.1 / 0.9)))))
    rot = torch.zeros(P, 4)
    rot[:, 0] = 1
    assert torch.equal(m._rotation.detach().cpu(), rot)
    d2 = torch.from_numpy(knn_ref.mean_dist2(xyz)).to(DEV)
    s = torch.log(torch.sqrt(torch.clamp_min(d2, 0.0000001)))[..., None].repeat(1, 3)
    if factor:
        ex = torch.exp(s)
        nrm = ex.norm(2, -1, keepdim=True)
        assert torch.equal(m._scaling.detach(), ex / nrm) and torch.equal(m._scaling_factor.detach(), torch.log(nrm))
    else:
        assert torch.equal(m._scaling.detach(), s) and m._scaling_factor is None


def test_rest_count_matching_no_degree_raises(hip, tmp_path):
    from c3dgs_amd.model import GaussianModel
    cols, _ = _trained_cols(100, 1, seed=1)
    cols["f_rest_9"] = cols["f_rest_0"]                       # 10 coefficients: no degree has that many
    path = _write_ply(tmp_path / "bad.ply", cols)
    with pytest.raises(ValueError, match="f_rest"):
        GaussianModel(3, quantization=False).load_ply(path)
    cols, _ = _trained_cols(100, 3, seed=1)
    with pytest.raises(ValueError, match="f_rest"):           # degree 3 in the file, degree 1 model
        GaussianModel(1, quantization=False).load_ply(_write_ply(tmp_path / "deg3.ply", cols))
    with pytest.raises(NotImplementedError):
        GaussianModel(3).load(str(tmp_path / "scene.obj"))


def _indexed_model(P=6000, seed=3, quantization=True):
    from c3dgs_amd.model import GaussianModel
    sc = synth.scene(P, W=640, H=360, focal=400.0, seed=seed, scale_median=0.02)
    raw = synth.raw_params(synth.index_scene(sc, seed=seed + 1, shs_extra=64, gs_extra=64))
    return GaussianModel(3, quantization=quantization, device=DEV).set_tensors(**raw)


def test_save_ply_columns_follow_reference_formulas(hip, tmp_path):
    from c3dgs_amd import ply
    from c3dgs_amd.model import PipelineParams
    a, b = _indexed_model(), _indexed_model()
    intr, ev = synth.camera(640, 360, 400.0)
    for m in (a, b):                                          # observers hold ranges before the save
        m.render(_Cam(intr, ev), PipelineParams(), torch.zeros(3, device=DEV))
    path = str(tmp_path / "out" / "dense.ply")
    a.save_ply(path)
    got = ply.read_ply(path)
    # reference save_ply on the twin model: same getter order, so the observers step identically
    feat = b.get_features.detach()
    scale = torch.log(b.get_scaling.detach())
    rot = b.get_rotation.detach()
    assert torch.equal(a._fq_state.view(torch.int32), b._fq_state.view(torch.int32))
    P = b._xyz.shape[0]
    assert feat.shape == (P, 16, 3) and rot.shape == (P, 4)       # indexed colours and shapes written dense
    want = {"x": b._xyz[:, 0], "y": b._xyz[:, 1], "z": b._xyz[:, 2]}
    want.update({f"f_dc_{i}": feat[:, 0, i] for i in range(3)})
    fr = feat[:, 1:].transpose(1, 2).flatten(start_dim=1)
    want.update({f"f_rest_{i}": fr[:, i] for i in range(45)})
    want["opacity"] = b._opacity[:, 0]
    want.update({f"scale_{i}": scale[:, i] for i in range(3)})
    want.update({f"rot_{i}": rot[:, i] for i in range(4)})
    names = ["x", "y", "z", "nx", "ny", "nz"] + [f"f_dc_{i}" for i in range(3)] + [f"f_rest_{i}" for i in range(45)] + \
        ["opacity"] + [f"scale_{i}" for i in range(3)] + [f"rot_{i}" for i in range(4)]
    assert list(got) == names
    for k in ("nx", "ny", "nz"):
        assert not got[k].any()
    for k, v in want.items():
        np.testing.assert_array_equal(got[k].view(np.uint32), v.detach().cpu().numpy().view(np.uint32), err_msg=k)


@pytest.mark.parametrize("factor", [True, False])
def test_save_load_round_trip(hip, tmp_path, factor):
    from c3dgs_amd.model import GaussianModel
    sc = synth.scene(4000, seed=9, scale_median=0.02)
    op = sc["opacities"].clamp(1e-4, 1 - 1e-4)
    nrm = sc["scales"].norm(dim=1, keepdim=True)
    a = GaussianModel(3, quantization=False, use_factor_scaling=factor).set_tensors(
        xyz=sc["means3D"], features_dc=sc["shs"][:, :1], features_rest=sc["shs"][:, 1:],
        scaling=sc["scales"] / nrm if factor else torch.log(sc["scales"]), rotation=sc["rotations"] * 2.5,
        opacity=torch.log(op / (1 - op)), scaling_factor=torch.log(nrm) if factor else None)
    path = str(tmp_path / "rt.ply")
    a.save_ply(path)
    b = GaussianModel(3, quantization=False, use_factor_scaling=factor).load(path)
    for k in ("_xyz", "_features_dc", "_features_rest", "_opacity"):
        assert torch.equal(getattr(a, k).detach(), getattr(b, k).detach()), k
    assert b.active_sh_degree == 3
    # exp/log once; with factor scaling also the split into norm and direction and its exp(log(norm)): a few ulps more
    torch.testing.assert_close(b.get_scaling.detach(), a.get_scaling.detach(), rtol=3e-6 if factor else 1e-6, atol=0)
    torch.testing.assert_close(b.get_rotation.detach(), a.get_rotation.detach(), rtol=1e-6, atol=1e-7)


def _psnr(a, b):
    mse = float(((a - b) ** 2).mean())
    return float("inf") if mse == 0 else 10 * np.log10(1.0 / mse)


def test_npz2ply_cli_matches_npz_render(hip, tmp_path):
    from c3dgs_amd.model import GaussianModel, PipelineParams
    P = 100_000
    sc = synth.scene(P, seed=13, scale_median=0.006)
    raw = synth.raw_params(synth.index_scene(sc, seed=14))
    m = GaussianModel(3, quantization=True, device=DEV).set_tensors(**raw)
    intr, ev = synth.camera()
    cam, bg = _Cam(intr, ev), torch.zeros(3, device=DEV)
    m.render(cam, PipelineParams(), bg)                       # observers hold ranges
    npz = str(tmp_path / "scene.npz")
    m.save_npz(npz)
    env = dict(os.environ, PYTHONPATH=ROOT + os.pathsep + os.environ.get("PYTHONPATH", ""))
    r = subprocess.run([sys.executable, "-m", "c3dgs_amd.npz2ply", npz], cwd=ROOT, env=env, capture_output=True,
                       text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    ply_path = str(tmp_path / "scene.ply")
    assert os.path.exists(ply_path)
    from_npz = GaussianModel(3, quantization=False, device=DEV).load(npz)
    from_ply = GaussianModel(3, quantization=False, device=DEV).load(ply_path)
    assert from_ply._xyz.shape == (P, 3) and not from_ply.is_color_indexed and from_ply.active_sh_degree == 3
    a = from_npz.render(cam, PipelineParams(), bg)["render"].detach()
    b = from_ply.render(cam, PipelineParams(), bg)["render"].detach()
    assert float(a.mean()) > 0.01
    assert _psnr(a, b) >= 60.0, _psnr(a, b)
