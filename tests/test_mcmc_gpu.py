"""-m gpu: MCMC density control (csrc/mcmc.hip; c3dgs_amd.mcmc, GaussianModel.relocate_gs / add_new_gs / add_position_noise,
pipeline.train(strategy="mcmc")) against tests/mcmc_ref.py.

sample:  q within 1 of the float64 floor(sigmoid 2^20) and exactly 0 on excluded rows; sources, counts and T BIT-EQUAL to the host
         sampler run on the kernel's own q (integer weights: the prefix is exact), at the wave, block and scan-sweep edges, with
         T > 2^32, for every kind of mask; two calls give identical bits.
values:  new raw opacity and raw scale (factor) against float64. The bar is 4 x the distance of the float32 restatement of the
         write-back step from float64, at least 1e-6 relative (the convention of tests/test_aa_ref_cpu.py).
apply:   bit-level bookkeeping of relocate_gs (in place) and add_new_gs (appended rows) on a model with Adam moments.
noise:   the xyz delta against the float64 formula, rel-inf, bar 4 x the float32 restatement's distance, at least 1e-6.
train:   the toy scene of tests/train_scene.py with a budget of 700 rows."""
import math

import numpy as np
import pytest
import torch

from tests import mcmc_ref as ref
from tests.gpu_util import rel_inf

pytestmark = pytest.mark.gpu

DEV = "cuda"
# 1_048_833: blocks of 256 rows, 4096 blocks per sweep of the 64-bit block scan -> 4098 blocks: a second sweep with two blocks,
# the last of them ragged (one row). Every level of the scan (row in block, block in sweep, sweep) then has at least two units.
P_TWO_SWEEPS = 4096 * 256 + 257
PS = [1, 2, 63, 64, 65, 255, 256, 257, 1023, 1025, 5000, P_TWO_SWEEPS]
MASKS = ["none_dead", "all_dead", "one_alive", "alternating", "run_over_block_edge", "derived"]
MIN_OPACITY = 0.005


def _logit(o):
    o = np.asarray(o, dtype=np.float64)
    return np.log(o / (1 - o))


def _draws(n, seed):
    u = np.random.default_rng(seed).random(n)
    return np.concatenate((u, [0.0, np.nextafter(1.0, 0.0)]))


def _opacities(P, seed):
    """Raw opacities whose sigmoid stays 1e-3 away from MIN_OPACITY: about a quarter below it."""
    rng = np.random.default_rng(seed)
    o = np.where(rng.random(P) < 0.25, rng.uniform(0.0005, MIN_OPACITY - 1e-3, P), rng.uniform(MIN_OPACITY + 1e-3, 0.995, P))
    if P == 5000:
        o[:] = 0.99                                    # T = 5000 x 1038090 > 2^32
    return _logit(o).astype(np.float32)


def _mask(name, P):
    m = np.zeros(P, dtype=bool)
    if name == "all_dead":
        m[:] = True
    elif name == "one_alive":
        m[:] = True
        m[(2 * P) // 3] = False
    elif name == "alternating":
        m[::2] = True
    elif name == "run_over_block_edge":
        lo = max(0, min(P - 300, 201))
        m[lo:lo + 300] = True
    return m


@pytest.mark.parametrize("P", PS)
def test_sample_is_bit_equal_to_the_host_sampler_on_the_kernels_weights(hip, P):
    from c3dgs_amd import mcmc
    raw = _opacities(P, P)
    raw_d = torch.from_numpy(raw).to(DEV)
    draws = _draws(1500, P + 1)
    draws_d = torch.from_numpy(draws).to(DEV)
    for name in MASKS if P != P_TWO_SWEEPS else ["none_dead", "alternating", "derived"]:
        if name == "derived":
            q, sources, counts, T, dead = mcmc.sample(raw_d, draws_d, None, MIN_OPACITY)
            q64, dead_ref = ref.weights(raw, None, MIN_OPACITY)
            assert np.array_equal(dead.cpu().numpy().astype(bool), dead_ref), name
            again = mcmc.sample(raw_d, draws_d, None, MIN_OPACITY)
        else:
            mask = _mask(name, P)
            mask_d = None if name == "none_dead" else torch.from_numpy(mask).to(DEV)
            q, sources, counts, T, dead = mcmc.sample(raw_d, draws_d, mask_d)
            q64, dead_ref = ref.weights(raw, mask)
            again = mcmc.sample(raw_d, draws_d, mask_d)
        qn = q.cpu().numpy().view(np.uint32).astype(np.int64)
        assert np.abs(qn - q64).max() <= 1, (name, int(np.abs(qn - q64).max()))
        assert not qn[dead_ref].any(), name
        s_ref, c_ref, T_ref = ref.sample(qn, draws)
        assert int(T.item()) == T_ref, name
        if P == 5000 and name == "none_dead":
            assert T_ref > 2 ** 32
        assert np.array_equal(sources.cpu().numpy(), s_ref), name
        assert np.array_equal(counts.cpu().numpy(), c_ref), name
        if T_ref:
            assert (qn[s_ref] > 0).all() and c_ref.sum() == draws.shape[0]
        else:                                          # every row excluded (all_dead, or a small P the mask covers)
            assert (s_ref == -1).all() and not c_ref.any()
        for a, b in zip((q, sources, counts, T), again):
            assert torch.equal(a, b), name


def test_the_two_stage_form_draws_what_the_single_call_draws(hip):
    from c3dgs_amd import mcmc
    P = 1025
    raw_d = torch.from_numpy(_opacities(P, 3)).to(DEV)
    draws_d = torch.from_numpy(_draws(700, 4)).to(DEV)
    q, sources, counts, T, dead = mcmc.sample(raw_d, draws_d, None, MIN_OPACITY)
    w = mcmc.weights(raw_d, None, MIN_OPACITY)
    assert torch.equal(w.q, q) and torch.equal(w.T, T) and torch.equal(w.dead, dead) and not bool(w.counts.any())
    assert torch.equal(mcmc.draw(w, draws_d), sources) and torch.equal(w.counts, counts)
    assert torch.equal(mcmc.draw(w, draws_d, 100), sources[:100]) and int(w.counts.sum()) == 100      # counts start from zero again


# ------------------------------------------------------------------------------------------------ models
def _model(P, factor, seed, opacity, quantization=False, moments=True):
    from c3dgs_amd.model import GaussianModel
    from c3dgs_amd.pipeline import OptimizationParams
    g = torch.Generator().manual_seed(seed)
    r = lambda *s: torch.randn(*s, generator=g)      # noqa: E731
    m = GaussianModel(1, quantization=quantization, use_factor_scaling=factor, device=DEV)
    scaling = r(P, 3).abs() + 0.1 if factor else r(P, 3) * 0.5 - 3.0
    m.set_tensors(xyz=r(P, 3), features_dc=r(P, 1, 3), features_rest=r(P, 3, 3), scaling=scaling, rotation=r(P, 4) * 3,
                  opacity=torch.from_numpy(np.asarray(opacity, dtype=np.float32)).reshape(P, 1),
                  scaling_factor=(r(P, 1) * 0.5 - 3.0) if factor else None)
    m.spatial_lr_scale = 1.0
    if moments:
        m.training_setup(OptimizationParams())
        for g_ in m.optimizer.param_groups:
            g_["lr"] = 1e-3
        for _ in range(3):                           # a few Adam steps: non-trivial moments in every group
            for p in m.parameters():
                p.grad = torch.randn(p.shape, generator=g).to(DEV)
            m.optimizer.step()
        m.optimizer.zero_grad(set_to_none=True)
    return m


def _snapshot(m):
    out = {}
    for name, attr, _ in m._GROUPS:
        p = getattr(m, attr)
        if p is None:
            continue
        st = m.optimizer.state[p]
        out[attr] = (p.detach().clone(), st["exp_avg"].clone(), st["exp_avg_sq"].clone(), float(st["step"]), p)
    return out


def _scale_attr(m):
    return "_scaling_factor" if m.use_factor_scaling else "_scaling"


def _bar(f32, f64):
    return max(1e-6, 4 * float(np.abs(f32.astype(np.float64) - f64).max() / np.abs(f64).max()))


def _check_values(m, before, rows, counts, label):
    """Raw opacity and raw scale of `rows` (sources with count > 0) against float64 -> the measured worst relative distances."""
    raw_op = before["_opacity"][0].cpu().numpy().reshape(-1)
    sc = before[_scale_attr(m)][0].cpu().numpy().reshape(raw_op.shape[0], -1)
    r, on, c = ref.values(raw_op, counts, MIN_OPACITY)
    assert np.array_equal(r, rows), label
    worst = [0.0, 0.0]
    for a, i in enumerate(rows):
        op64, sc64 = ref.write_back(on[a:a + 1], c[a:a + 1], sc[i:i + 1])
        op32, sc32 = ref.write_back(on[a:a + 1], c[a:a + 1], sc[i:i + 1], np.float32)
        got_op = m._opacity.detach().cpu().numpy().reshape(-1)[i:i + 1].astype(np.float64)
        got_sc = getattr(m, _scale_attr(m)).detach().cpu().numpy().reshape(m._xyz.shape[0], -1)[i:i + 1].astype(np.float64)
        d_op = float(np.abs(got_op - op64).max() / np.abs(op64).max())
        d_sc = float(np.abs(got_sc - sc64).max() / np.abs(sc64).max())
        assert d_op <= _bar(op32, op64), (label, int(i), int(counts[i]), d_op, _bar(op32, op64))
        assert d_sc <= _bar(sc32, sc64), (label, int(i), int(counts[i]), d_sc, _bar(sc32, sc64))
        worst = [max(worst[0], d_op), max(worst[1], d_sc)]
    return worst


def _draws_for_counts(q, wanted):
    """Draws that give row i exactly wanted[i] hits: the middle of its interval of the prefix."""
    C = ref.prefix(q)
    T = C[-1]
    u = []
    for i, k in enumerate(wanted):
        u += [(C[i] - int(q[i]) / 2) / T] * int(k)
    return np.array(u, dtype=np.float64)


def _relocation_case(factor):
    """-> (model, snapshot before, dead mask on the device, draws, wanted counts, counts, number of dead rows): the case of
    test_relocation_values_against_float64, shared with tests/test_scratch_poison_gpu.py"""
    from c3dgs_amd import mcmc
    os_, ks = (0.006, 0.3, 0.9, 0.99, 1 - 1e-6), (1, 2, 4, 19, 50)         # N = count + 1 in {2, 3, 5, 20, 51}
    live = [(o, k) for o in os_ for k in ks]
    n_dead = sum(k for _, k in live)
    P = len(live) + n_dead
    opacity = np.concatenate((_logit([o for o, _ in live]), np.full(n_dead, _logit(0.001))))
    order = np.random.default_rng(11).permutation(P)                       # live and dead rows interleaved
    opacity = opacity[order]
    wanted = np.concatenate(([k for _, k in live], np.zeros(n_dead, dtype=int)))[order]
    dead = np.concatenate((np.zeros(len(live), dtype=bool), np.ones(n_dead, dtype=bool)))[order]
    m = _model(P, factor, 21, opacity)
    before = _snapshot(m)
    dead_d = torch.from_numpy(dead).to(DEV)
    q = mcmc.weights(m._opacity, dead_d).q.cpu().numpy().view(np.uint32).astype(np.int64)
    draws = _draws_for_counts(q, wanted)
    assert draws.shape[0] == n_dead
    _, counts, _ = ref.sample(q, draws)
    assert np.array_equal(counts, wanted)
    return m, before, dead_d, draws, wanted, counts, n_dead


@pytest.mark.parametrize("factor", [True, False])
def test_relocation_values_against_float64(hip, factor):
    m, before, dead_d, draws, wanted, counts, n_dead = _relocation_case(factor)
    assert m.relocate_gs(dead_d, MIN_OPACITY, torch.from_numpy(draws).to(DEV)) == n_dead
    worst = _check_values(m, before, np.nonzero(wanted)[0], counts, f"factor={factor}")
    print(f"relocation values, factor={factor}: worst relative distance from float64: raw opacity {worst[0]:.3g}, raw scale {worst[1]:.3g}")


def test_relocation_clamps_the_number_of_copies_at_51(hip):
    P = 61
    opacity = np.full(P, _logit(0.001))
    opacity[40] = _logit(0.8)
    m = _model(P, True, 22, opacity)
    before = _snapshot(m)
    dead = torch.ones(P, dtype=torch.bool, device=DEV)
    dead[40] = False
    assert m.relocate_gs(dead, MIN_OPACITY, torch.from_numpy(_draws(58, 1)).to(DEV)) == 60
    counts = np.zeros(P, dtype=np.int64)
    counts[40] = 60
    _check_values(m, before, np.array([40]), counts, "clamp")
    on51, _ = ref.relocation(float(ref.sigmoid(np.float32(before["_opacity"][0][40].item()))), 51)
    assert abs(float(torch.sigmoid(m._opacity.detach()[40].double())) - on51) <= 1e-6 * on51   # N = 51, not 61
    assert bool((m._opacity == m._opacity[40]).all()) and bool((m._scaling_factor == m._scaling_factor[40]).all())


# ------------------------------------------------------------------------------------------------ apply
def _check_bookkeeping(m, before, dst, sources, copy_rows, P_before):
    """The bit-level contract of c3dgs_mcmc_apply on rows `dst` <- `sources`; every other row of the first P_before untouched."""
    P = m._xyz.shape[0]
    touched = np.zeros(P, dtype=bool)
    touched[dst] = True
    touched[sources] = True
    dst_d, src_d = torch.from_numpy(dst).to(DEV), torch.from_numpy(sources).to(DEV)
    rest = torch.from_numpy(np.nonzero(~touched[:P_before])[0]).to(DEV)
    for attr, (old, m1, m2, step, obj) in before.items():
        p = getattr(m, attr)
        st = m.optimizer.state[p]
        assert float(st["step"]) == step, attr
        if copy_rows:
            assert p is obj, f"{attr}: the relocation is in place"
        new = p.detach()
        if attr not in ("_opacity", _scale_attr(m)):
            assert torch.equal(new[dst_d], old[src_d]), f"{attr}: a destination is its source's pre-call row"
            assert torch.equal(new[src_d], old[src_d]), f"{attr}: a source keeps everything but opacity and scale"
        else:
            assert torch.equal(new[dst_d], new[src_d]), f"{attr}: source and destination carry the same bits"
            assert not torch.equal(new[src_d], old[src_d]), attr
        for mom, old_mom in ((st["exp_avg"], m1), (st["exp_avg_sq"], m2)):
            assert not bool(mom[dst_d].any()) and not bool(mom[src_d].any()), f"{attr}: moments of sources and destinations are zero"
            assert torch.equal(mom[rest], old_mom[rest]), f"{attr}: moments of untouched rows"
            assert rest.numel() == 0 or bool(old_mom[rest].any())
        assert torch.equal(new[rest], old[rest]), f"{attr}: untouched rows"


@pytest.mark.parametrize("factor", [True, False])
def test_relocate_gs_bookkeeping(hip, factor):
    from c3dgs_amd import mcmc
    P = 300
    raw = _opacities(P, 31)
    m = _model(P, factor, 32, raw)
    before = _snapshot(m)
    dead = ref.weights(raw, None, MIN_OPACITY)[1]
    n = int(dead.sum())
    assert 30 < n < 150
    draws = torch.from_numpy(_draws(n, 33)).to(DEV)                # two more than needed: only the first n are used
    _, sources, counts, _, dead_k = mcmc.sample(m._opacity, draws[:n], None, MIN_OPACITY)
    assert np.array_equal(dead_k.cpu().numpy().astype(bool), dead)
    assert m.relocate_gs(None, MIN_OPACITY, draws) == n
    sources = sources.cpu().numpy().astype(np.int64)
    _check_bookkeeping(m, before, np.nonzero(dead)[0], sources, True, P)
    _check_values(m, before, np.nonzero(counts.cpu().numpy())[0], counts.cpu().numpy(), f"relocate factor={factor}")
    # nothing dead, everything dead: nothing changes
    snap = _snapshot(m)
    assert m.relocate_gs(torch.zeros(P, dtype=torch.bool, device=DEV)) == 0
    assert m.relocate_gs(torch.ones(P, dtype=torch.bool, device=DEV)) == 0
    for attr, (old, m1, m2, step, obj) in snap.items():
        st = m.optimizer.state[getattr(m, attr)]
        assert getattr(m, attr) is obj and torch.equal(obj.detach(), old) and torch.equal(st["exp_avg"], m1) and torch.equal(st["exp_avg_sq"], m2)


def test_one_wave_of_destinations_drawing_a_source_in_the_same_wave(hip):
    """64 dead rows and one live row among them: every destination reads the opacity and scale of a row the same step rewrites."""
    P = 65
    opacity = np.full(P, _logit(0.002))
    opacity[5] = _logit(0.7)
    m = _model(P, False, 41, opacity)
    before = _snapshot(m)
    assert m.relocate_gs(None, MIN_OPACITY, torch.from_numpy(_draws(62, 2)).to(DEV)) == 64
    dst = np.array([i for i in range(P) if i != 5])
    _check_bookkeeping(m, before, dst, np.full(64, 5), True, P)
    counts = np.zeros(P, dtype=np.int64)
    counts[5] = 64
    _check_values(m, before, np.array([5]), counts, "hazard")


@pytest.mark.parametrize("factor", [True, False])
def test_add_new_gs_bookkeeping(hip, factor):
    from c3dgs_amd import mcmc
    P = 300
    m = _model(P, factor, 51, _opacities(P, 52))
    before = _snapshot(m)
    draws = torch.from_numpy(_draws(20, 53)).to(DEV)
    n_new = min(310, int(1.05 * P)) - P
    assert n_new == 10
    _, sources, counts, _, _ = mcmc.sample(m._opacity, draws[:n_new])
    assert m.add_new_gs(310, draws) == n_new and m._xyz.shape[0] == 310
    _check_bookkeeping(m, before, np.arange(P, P + n_new), sources.cpu().numpy().astype(np.int64), False, P)
    _check_values(m, {k: v for k, v in before.items()}, np.nonzero(counts.cpu().numpy())[0], counts.cpu().numpy(), f"grow factor={factor}")
    objs = [getattr(m, attr) for attr in before]
    assert m.add_new_gs(310) == 0 and m.add_new_gs(100) == 0 and m._xyz.shape[0] == 310
    assert all(getattr(m, attr) is o for attr, o in zip(before, objs))
    assert m.add_new_gs(1000) == int(1.05 * 310) - 310                  # the 5 % step, not the cap


def test_indexed_models_are_refused(hip):
    m = _model(64, True, 61, _opacities(64, 62), moments=False)
    m._gaussian_indices = torch.zeros(64, dtype=torch.int64, device=DEV)
    for call in (lambda: m.relocate_gs(), lambda: m.add_new_gs(100), lambda: m.add_position_noise(5e5, 1e-4)):
        with pytest.raises(NotImplementedError, match="non-indexed"):
            call()


# ------------------------------------------------------------------------------------------------ noise
@pytest.mark.parametrize("factor", [True, False])
@pytest.mark.parametrize("P", [1, 65, 1025])
def test_position_noise_against_float64(hip, P, factor):
    opacity = _logit(np.array([0.001, 0.005, 0.05, 0.9])[np.arange(P) % 4])
    m = _model(P, factor, 70 + P, opacity, quantization=True)
    with torch.no_grad():
        if factor:
            m._scaling[P // 2] = torch.tensor([1.0, 1e-3, 1e-3])             # a needle: scale ratio 1e3
            m._scaling[P // 3, 0] = -0.5                                    # relu
        else:
            m._scaling[P // 2] = torch.tensor([0.0, math.log(1e-3), math.log(1e-3)])
    xi = torch.randn(P, 3, generator=torch.Generator().manual_seed(P)).to(DEV)
    noise_lr, xyz_lr = 5e5, 1.6e-4
    xyz0 = m._xyz.detach().clone()
    others = {a: getattr(m, a).detach().clone() for a in ("_rotation", "_scaling", "_opacity", "_features_dc", "_features_rest")}
    fac = m._scaling_factor.detach().clone() if factor else None
    moments = {a: (m.optimizer.state[getattr(m, a)]["exp_avg"].clone(), m.optimizer.state[getattr(m, a)]["exp_avg_sq"].clone())
               for a in ("_xyz", "_rotation", "_scaling", "_opacity")}
    fq = m._fq_state.clone()
    xyz_obj = m._xyz

    m.add_position_noise(noise_lr, xyz_lr, torch.zeros(P, 3, device=DEV))
    assert torch.equal(m._xyz.detach(), xyz0), "zero draws leave xyz bit-identical"

    with torch.no_grad():
        m._xyz.zero_()
    m.add_position_noise(noise_lr, xyz_lr, xi)
    delta = m._xyz.detach().clone()
    args = (None, others["_rotation"].cpu().numpy(), others["_scaling"].cpu().numpy(), None if fac is None else fac.cpu().numpy(),
            others["_opacity"].cpu().numpy(), xi.cpu().numpy(), noise_lr, xyz_lr)
    d64, d32 = ref.noise(*args), ref.noise(*args, dtype=np.float32)
    got, bar = rel_inf(delta.cpu().numpy(), d64), max(1e-6, 4 * rel_inf(d32, d64))
    print(f"position noise P={P} factor={factor}: rel-inf {got:.3g} (float32 restatement {rel_inf(d32, d64):.3g}, bar {bar:.3g})")
    assert np.abs(d64).max() > 1e-4 and got <= bar, (got, bar)

    with torch.no_grad():
        m._xyz.copy_(xyz0)
    m.add_position_noise(noise_lr, xyz_lr, xi)
    assert m._xyz is xyz_obj and torch.equal(m._xyz.detach(), xyz0 + delta), "in place: one fp32 add of the same delta"
    for a, old in others.items():
        assert torch.equal(getattr(m, a).detach(), old), a
    assert fac is None or torch.equal(m._scaling_factor.detach(), fac)
    for a, (m1, m2) in moments.items():
        st = m.optimizer.state[getattr(m, a)]
        assert torch.equal(st["exp_avg"], m1) and torch.equal(st["exp_avg_sq"], m2), a
    assert torch.equal(m._fq_state.view(torch.int32), fq.view(torch.int32)), "the FakeQuantize observers are not touched"
    lr = next(g["lr"] for g in m.optimizer.param_groups if g["name"] == "xyz")
    with torch.no_grad():
        m._xyz.zero_()
    m.add_position_noise(noise_lr, None, xi)                                 # xyz_lr=None: the xyz group's
    m2 = m._xyz.detach().clone()
    with torch.no_grad():
        m._xyz.zero_()
    m.add_position_noise(noise_lr, lr, xi)
    assert torch.equal(m._xyz.detach(), m2)


# ------------------------------------------------------------------------------------------------ train
CAP = 700


class _Run:
    pass


@pytest.fixture(scope="module")
def mcmc_run(hip, tmp_path_factory):
    """ONE toy training with strategy="mcmc", cap_max=700, shared by the tests below."""
    from c3dgs_amd import loss, pipeline
    from c3dgs_amd.model import PipelineParams
    from tests import train_scene
    student, cams, extent = train_scene.make(tmp_path_factory.mktemp("mcmc"), DEV)

    def mean_loss():
        bg = torch.zeros(3, device=DEV)
        with torch.no_grad():
            return sum(float(loss.l1_ssim_loss(student.render(c, PipelineParams(), bg)["render"], c.original_image, 0.2)) for c in cams) / len(cams)

    class Scene:
        gaussians = student
        cameras_extent = extent

        def getTrainCameras(self):
            return cams

    run = _Run()
    run.student, run.scene, run.events = student, Scene(), []
    run.rows0, run.start = student._xyz.shape[0], mean_loss()
    torch.manual_seed(0)
    run.n = pipeline.train(run.scene, None, train_scene.schedule(400), PipelineParams(), camera_stride=1, degree_up_iter=80,
                           log=lambda e, i: run.events.append(dict(i)), strategy="mcmc", cap_max=CAP)
    run.end = mean_loss()
    return run


def test_mcmc_training_follows_the_budget_and_lowers_the_loss(mcmc_run):
    run = mcmc_run
    assert run.n == 400 and len(run.events) == 50
    rows, refinements = run.rows0, 0
    for info in run.events:
        assert info["densified"] is None and info["reset_opacity"] is False
        if info["mcmc"] is not None:
            refinements += 1
            relocated, added = info["mcmc"]
            assert info["N"] == min(CAP, int(1.05 * rows)) and added == info["N"] - rows and 0 <= relocated < rows
        else:
            assert info["N"] == rows
        rows = info["N"]
        assert rows <= CAP
    assert refinements == 7                                      # schedule(400): epochs 5, 10, ... 35, densify_from_epoch included
    for p in run.student.parameters():
        assert bool(torch.isfinite(p).all())
    print(f"mcmc toy training: mean loss {run.start:.4f} -> {run.end:.4f}, rows {run.rows0} -> {run.student._xyz.shape[0]}, "
          f"(relocated, added) per refinement {[i['mcmc'] for i in run.events if i['mcmc'] is not None]}")
    assert run.end < run.start


def test_mcmc_training_reaches_the_cap(mcmc_run):
    """500 -> 525 -> 551 -> 578 -> 606 -> 636 -> 667 -> 700: the seventh refinement is the one the cap binds."""
    counts = [i["N"] for i in mcmc_run.events if i["mcmc"] is not None]
    assert counts == [525, 551, 578, 606, 636, 667, CAP]
    assert max(i["N"] for i in mcmc_run.events) == CAP and mcmc_run.student._xyz.shape[0] == CAP


def test_the_default_strategy_is_reproducible(hip, tmp_path):
    """Runs none of the new code: it guards the plumbing of train(strategy=...) around the default loop."""
    from c3dgs_amd import pipeline
    from c3dgs_amd.model import PipelineParams
    from tests import train_scene
    results = []
    for k in range(2):
        student, cams, extent = train_scene.make(tmp_path, DEV)

        class Scene:
            gaussians = student
            cameras_extent = extent

            def getTrainCameras(self):
                return cams

        torch.manual_seed(0)
        events = []
        pipeline.train(Scene(), None, train_scene.schedule(80), PipelineParams(), camera_stride=1, degree_up_iter=16,
                       log=lambda e, i: events.append(i), strategy="default")
        assert all("mcmc" not in i for i in events)
        results.append([p.detach().clone() for p in student.parameters()])
    assert len(results[0]) == len(results[1])
    for a, b in zip(*results):
        assert a.shape == b.shape and torch.equal(a, b)


def test_train_refuses_contradictory_strategies(hip, tmp_path):
    from c3dgs_amd import pipeline
    from c3dgs_amd.model import PipelineParams
    from tests import train_scene
    student, cams, extent = train_scene.make(tmp_path, DEV, P_teacher=400)

    class Scene:
        gaussians = student
        cameras_extent = extent

        def getTrainCameras(self):
            return cams

    opt = train_scene.schedule(16)
    with pytest.raises(ValueError, match="strategy"):
        pipeline.train(Scene(), None, opt, PipelineParams(), strategy="MCMC", cap_max=100)
    with pytest.raises(ValueError, match="densify_by"):
        pipeline.train(Scene(), None, opt, PipelineParams(), strategy="mcmc", cap_max=100, densify_by="error", error_threshold=1.0)
    with pytest.raises(ValueError, match="cap_max"):
        pipeline.train(Scene(), None, opt, PipelineParams(), strategy="mcmc")
    student._gaussian_indices = torch.zeros(student._xyz.shape[0], dtype=torch.int64, device=DEV)
    with pytest.raises(NotImplementedError, match="non-indexed"):
        pipeline.train(Scene(), None, opt, PipelineParams(), strategy="mcmc", cap_max=100)
