"""CPU: tests/densify_ref.py (the staged torch restatement, and the fused decision GaussianModel.densify_and_prune takes)
reproduces every case of tests/golden/densify.npz, which tests/golden/make_golden_densify.py recorded from the reference
itself: provenance and observer states exactly, child rows and reset_opacity bit for bit (same torch CPU ops, same order)."""
import numpy as np
import pytest
import torch

from tests import densify_ref as dr

CASES = dr.load_fixture()
END_TO_END = [n for n in CASES if n not in ("clone", "split", "prune")]


def _qa_equal(scene, case, tag):
    for k, mod in scene.qa.items():
        if tag + k not in case:
            continue
        lo, hi, scale, zp = dr.qa_state(mod)
        np.testing.assert_array_equal(np.array([lo, hi, scale], np.float32), case[tag + k], err_msg=k)
        assert zp == int(case[tag + k + "_zp"][0]), k


def test_fixture_holds_the_cases_the_issue_lists():
    assert set(END_TO_END) == {"factor_fp", "factor_fp_screen", "factor_qat", "factor_qat_screen", "plain_fp_screen"}
    assert {"clone", "split", "prune"} <= set(CASES)
    for name in END_TO_END:
        c = CASES[name]
        kinds = c["kind"]
        assert (kinds == 0).any() and (kinds == 1).any() and (kinds == 2).any() and (kinds == 3).any(), name
        S = len(c["z"]) // int(c["N"][0])
        assert 0 < (kinds == 2).sum() < S, name                 # some children pruned, some kept
        assert c["margin"][0] >= 1e-3 and c["margin"][1] >= 1e-4, name


@pytest.mark.parametrize("name", list(CASES))
def test_staged_restatement_reproduces_the_reference(name):
    case = CASES[name]
    scene = dr.staged_from_case(case, "cpu")
    before = {k: v.clone() for k, v in scene.p.items()}
    mom = {k: (v[0].clone(), v[1].clone()) for k, v in scene.m.items()}
    stats = (scene.accum.clone(), scene.denom.clone(), scene.max_radii2D.clone())
    with torch.no_grad():
        dr.run_case_method(scene, case, name, torch.from_numpy(case["z"].copy()))
    src, kind = scene.src, scene.kind
    np.testing.assert_array_equal(src.numpy(), case["src"])
    np.testing.assert_array_equal(kind.numpy(), case["kind"])
    _qa_equal(scene, case, "qa_after_")
    child = kind >= 2
    np.testing.assert_array_equal(scene.p["xyz"][child].numpy().view(np.uint32), case["child_xyz"].view(np.uint32))
    np.testing.assert_array_equal(scene.p["scaling"][child].numpy().view(np.uint32), case["child_scaling"].view(np.uint32))
    for k, v in scene.p.items():
        rows = ~child if k in ("xyz", "scaling") else torch.ones_like(child)
        assert torch.equal(v[rows], before[k][src[rows]]), k
        orig = kind == 0
        assert torch.equal(scene.m[k][0][orig], mom[k][0][src[orig]]) and torch.equal(scene.m[k][1][orig], mom[k][1][src[orig]]), k
        assert float(scene.m[k][0][~orig].abs().sum()) == 0 and float(scene.m[k][1][~orig].abs().sum()) == 0, k
    if name == "prune":
        assert torch.equal(scene.accum, stats[0][src]) and torch.equal(scene.denom, stats[1][src])
        assert torch.equal(scene.max_radii2D, stats[2][src])
    else:
        n = len(src)
        assert tuple(scene.accum.shape) == (n, 1) and tuple(scene.denom.shape) == (n, 1) and tuple(scene.max_radii2D.shape) == (n,)
        assert float(scene.accum.abs().sum() + scene.denom.abs().sum() + scene.max_radii2D.abs().sum()) == 0
    if "reset_opacity" in case:
        with torch.no_grad():
            scene.reset_opacity()
        np.testing.assert_array_equal(scene.p["opacity"].numpy().view(np.uint32), case["reset_opacity"].view(np.uint32))
        _qa_equal(scene, case, "qa_after_reset_")
        assert float(scene.m["opacity"][0].abs().sum()) == 0


@pytest.mark.parametrize("name", END_TO_END)
def test_fused_decision_reproduces_the_reference(name):
    """classify on the P-row batches + plan gives the staged result's rows, and leaves the observers where it leaves them."""
    case = CASES[name]
    scene = dr.staged_from_case(case, "cpu")
    N = int(case["N"][0])
    with torch.no_grad():
        code, std = dr.fused_codes(scene, float(case["max_grad"][0]), float(case["min_opacity"][0]), float(case["extent"][0]),
                                   int(case["max_screen_size"][0]) or None, N)
        src, kind, draw_row, totals = dr.plan_ref(code, N)
    np.testing.assert_array_equal(src.numpy(), case["src"])
    np.testing.assert_array_equal(kind.numpy(), case["kind"])
    np.testing.assert_array_equal(draw_row[kind >= 2].numpy(), case["draw_row"])
    assert totals[2] * N == len(case["z"])
    _qa_equal(scene, case, "qa_after_")
    # the children the apply kernel computes: std / (0.8 N) of the split-stage scales
    child = kind >= 2
    want = std[src[child]] / (0.8 * N)
    if not bool(case["use_factor_scaling"][0]):
        want = torch.log(want)
    np.testing.assert_array_equal(want.numpy().view(np.uint32), case["child_scaling"].view(np.uint32))


def test_classify_ref_boundaries():
    """Rows exactly at each threshold, 0/0 and x/0, on the predicates as the reference writes them."""
    f = torch.tensor
    one = torch.ones(6, 3)
    accum = f([0.0002, 0.0, 1.0, 0.0004, 0.0002, -0.0004])
    denom = f([1.0, 0.0, 0.0, 2.0, 1.0, 2.0])
    thr = float(torch.tensor(0.0002))                            # the fp32 value, so rows 0, 3, 4 sit exactly on it
    sc = one * f([0.5, 0.5, 0.5, 0.5, 0.25, 0.5])[:, None]
    op = f([0.5, 0.5, 0.5, 0.005, 0.5, 0.5])
    code = dr.classify_ref(accum, denom, sc, sc, None, None, op, thr, 0.5, float(torch.tensor(0.005)), 1.0)
    # row 0: |g| == thr, scale == dense -> clone (<=), not split (>);  row 1: 0/0 -> 0 -> neither;  row 2: inf -> clone
    # row 3: opacity == min_opacity is not < -> kept + clone;  row 4: clone;  row 5: g = -thr: |g| clones, g >= thr does not split
    assert code.tolist() == [3, 1, 3, 3, 3, 3]
    code = dr.classify_ref(accum, denom, sc, sc * 1.5, None, None, op, thr, 0.5, 0.5, 1.0)
    # split scales above dense: rows 0, 2, 3 split (4 has 0.375 <= 0.5, 5 has negative g); opacity 0.005 < 0.5 prunes row 3
    assert code.tolist() == [2 | 4 | 8, 1, 2 | 4 | 8, 4, 3, 3]
