"""Vectorised torch restatement of the index remapping of the reference's prune_points on an indexed model
(scene/gaussian_model.py:1104-1114): flags -> cumsum -> gather, no Python loop over ids. Runs on any device; it is what
c3dgs_index_plan (csrc/index_plan.hip) is tested against and what tools/time_index_prune.py times it against.

tests/test_index_ref_cpu.py pins it to tests/golden/index_prune.npz (recorded from the reference itself) and to the
reference's loop form (`loop_ref`)."""
import os

import numpy as np
import torch

FIXTURE = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "index_prune.npz")


def remap_ref(keep, idx, K):
    """One index space. keep: bool [P]; idx: int64 [P] with every kept entry in [0, K).
    -> (cb_src int64 [K_new]: the referenced old ids, ascending; new_idx int64 [P_new]: rank of idx[kept] among them)."""
    sel = idx[keep]
    flags = torch.zeros(K, dtype=torch.bool, device=idx.device)
    flags[sel] = True
    rank = torch.cumsum(flags, 0) - 1
    return torch.nonzero(flags).squeeze(1), rank[sel]


def plan_ref(keep, idx0, K0, idx1, K1):
    """-> (src int64 [P_new], new_idx0, new_idx1, cb_src0, cb_src1); None for an index space that is None."""
    src = torch.nonzero(keep).squeeze(1)
    cb0, new0 = remap_ref(keep, idx0, K0) if idx0 is not None else (None, None)
    cb1, new1 = remap_ref(keep, idx1, K1) if idx1 is not None else (None, None)
    return src, new0, new1, cb0, cb1


def loop_ref(K, idx, keep):
    """The remap built the slow way, one table write per referenced id in ascending order, as the reference does it
    (:1110-1113). Works on any device (tools/time_index_prune.py times it on the GPU). -> (referenced bool [K], new index)."""
    kept_ids = idx[keep]
    referenced = torch.zeros(K, dtype=torch.bool, device=idx.device)
    referenced[kept_ids] = True
    table = torch.full((K,), -1, dtype=idx.dtype, device=idx.device)
    position = 0
    for old_id in torch.nonzero(referenced).squeeze(1).tolist():
        table[old_id] = position
        position += 1
    return referenced, table[kept_ids]


def load_fixture():
    """-> {case: {key: numpy array}} of tests/golden/index_prune.npz."""
    data = np.load(FIXTURE)
    cases = {}
    for key in data.files:
        if "/" in key:
            case, k = key.split("/", 1)
            cases.setdefault(case, {})[k] = data[key]
    return cases
