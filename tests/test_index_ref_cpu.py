"""CPU: the vectorised restatement of the indexed prune (tests/index_ref.py) against the fixture recorded from the reference
itself (tests/golden/index_prune.npz) and against the reference's loop over ids on random small inputs."""
import numpy as np
import pytest
import torch

from tests import index_ref as ir

CASES = ir.load_fixture()


def _t(a):
    return torch.from_numpy(np.ascontiguousarray(a))


def test_fixture_has_the_cases_and_their_premises():
    assert {"both", "color", "geometry", "unindexed"} <= set(CASES)
    assert "idx0" in CASES["both"] and "idx1" in CASES["both"]
    assert "idx0" in CASES["color"] and "idx1" not in CASES["color"]
    assert "idx1" in CASES["geometry"] and "idx0" not in CASES["geometry"]
    for name in ("both", "color", "geometry"):
        case = CASES[name]
        mask = case["mask"]
        assert mask.shape == (200,) and 0 < mask.sum() < 200
        for tag, K in (("0", 64), ("1", 48)):
            if "idx" + tag not in case:
                continue
            idx = case["idx" + tag]
            before = np.unique(idx)
            after = np.unique(idx[~mask])
            assert len(before) < K, "rows unreferenced before the prune"
            assert len(after) < len(before), "rows that become unreferenced by the prune"


@pytest.mark.parametrize("name", ["both", "color", "geometry"])
def test_restatement_equals_the_reference_fixture(name):
    case = CASES[name]
    keep = ~_t(case["mask"])
    idx0 = _t(case["idx0"]) if "idx0" in case else None
    idx1 = _t(case["idx1"]) if "idx1" in case else None
    src, new0, new1, cb0, cb1 = ir.plan_ref(keep, idx0, 64, idx1, 48)
    assert torch.equal(src, _t(case["src"]).long())
    for tag, new, cb in (("0", new0, cb0), ("1", new1, cb1)):
        if "idx" + tag not in case:
            assert new is None and cb is None
            continue
        assert new.dtype == torch.int64
        assert torch.equal(new, _t(case["new_idx" + tag])) and torch.equal(cb, _t(case["cb_src" + tag]).long())
    for k in ("accum", "denom", "max_radii2D"):
        assert torch.equal(_t(case[k + "_in"])[src], _t(case[k]))


def test_unindexed_provenance_is_the_index_arrays():
    case = CASES["unindexed"]
    assert np.array_equal(case["rows_features_dc"], case["idx0"]) and np.array_equal(case["rows_features_rest"], case["idx0"])
    assert np.array_equal(case["rows_scaling"], case["idx1"]) and np.array_equal(case["rows_rotation"], case["idx1"])


@pytest.mark.parametrize("seed", range(12))
def test_restatement_equals_the_loop_form(seed):
    g = torch.Generator().manual_seed(seed)
    P = int(torch.randint(1, 60, (1,), generator=g))
    K = int(torch.randint(1, 40, (1,), generator=g))
    idx = torch.randint(0, K, (P,), generator=g)
    keep = torch.rand(P, generator=g) < 0.6
    keep[int(torch.randint(0, P, (1,), generator=g))] = True       # the loop form needs a survivor (unique_ids[-1])
    feat_valid, new_loop = ir.loop_ref(K, idx, keep)
    cb, new = ir.remap_ref(keep, idx, K)
    assert torch.equal(new, new_loop) and torch.equal(cb, torch.nonzero(feat_valid).squeeze(1))
    assert torch.equal(cb[new], idx[keep])
