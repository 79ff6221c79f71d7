"""-m gpu: the depth sort on biased keys (csrc/radix_sort.hip, csrc/common.hpp: depth_sort_plan) against numpy's stable sort on
(key, id), element for element, through c3dgs_debug_depth_sort, which drives the sort as the forward does: the histogram launch
that also reduces the largest visible key, two 9-bit passes, then one more pass (every visible key below the three-pass limit) or
two (the fallback). Item counts around one 12,288-item sort tile and three tiles with a ragged tail; key patterns that put
everything into one digit, on the edges of the three-pass range, past it, and -- `prefiltered` -- below the bias, where the four
8-bit passes on the raw keys run. Every rectangle is distinct, so a second payload that loses its item shows.
One full forward with a Gaussian at depth 600 must leave the binning arrays the rocPRIM path leaves."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

TILE = 12288
RAGGED = 3 * TILE + 137
CULLED, BIAS = 0xFFFFFFFF, 0x3C000000
LIMIT3 = BIAS + (1 << 27) - 1                       # the smallest visible key that needs the fourth pass


def _bits(depths):
    return np.asarray(depths, dtype=np.float32).view(np.uint32).copy()


def _cull_every_third(k):
    k = k.copy()
    k[::3] = CULLED
    return k


def _keys(pattern, n, rng):
    """-> (uint32 keys, prefiltered, digit passes the sort must report)"""
    uniform = _bits(rng.uniform(2.0, 12.0, n))
    if pattern == "all_culled":
        return np.full(n, CULLED, np.uint32), 0, 3
    if pattern == "all_equal":
        return np.full(n, _bits([5.0])[0], np.uint32), 0, 3
    if pattern == "one_ulp_apart":
        a = int(_bits([3.25])[0])
        return np.where(rng.integers(0, 2, n) == 1, a + 1, a).astype(np.uint32), 0, 3
    if pattern == "uniform":
        return uniform, 0, 3
    if pattern == "uniform_third_culled":
        return _cull_every_third(uniform), 0, 3
    if pattern == "range_edges":                    # the bias itself and the last key three passes order
        k = uniform
        k[rng.integers(0, n, max(1, n // 8))] = BIAS
        k[rng.integers(0, n, max(1, n // 8))] = LIMIT3 - 1
        k[0], k[n - 1] = LIMIT3 - 1, BIAS
        return _cull_every_third(k) if n > 3 else k, 0, 3
    if pattern == "at_the_limit":                   # one key exactly at the limit: the fallback
        k = uniform
        k[rng.integers(0, n, max(1, n // 8))] = LIMIT3 - 1
        k[n // 2] = LIMIT3
        return k, 0, 4
    if pattern == "far_mix":                        # depths up to 1e6, culled ones between them
        k = _bits(np.exp(rng.uniform(np.log(0.02), np.log(1e6), n)))
        k[n - 1] = _bits([1e6])[0]
        k = _cull_every_third(k)
        k[n - 1] = _bits([1e6])[0]
        return k, 0, 4
    if pattern == "prefiltered":                    # no near-plane test: keys below the bias, a negative float's pattern
        k = _bits(rng.uniform(-3.0, 12.0, n))
        k[rng.integers(0, n, max(1, n // 8))] = _bits([1e-5])[0]
        k[0] = _bits([-0.5])[0]
        k[n - 1] = 0
        return k, 1, 4
    raise AssertionError(pattern)


CASES = [(p, n) for p, sizes in [
    ("uniform", [1, 63, TILE - 1, TILE, TILE + 1, RAGGED]),
    ("all_culled", [63, TILE + 1]),
    ("all_equal", [1, TILE]),
    ("one_ulp_apart", [TILE - 1, RAGGED]),
    ("uniform_third_culled", [TILE + 1, RAGGED]),
    ("range_edges", [63, RAGGED]),
    ("at_the_limit", [63, RAGGED]),
    ("far_mix", [TILE + 1, RAGGED]),
    ("prefiltered", [63, RAGGED]),
] for n in sizes]


def _depth_sort(keys, rects, prefiltered):
    from c3dgs_amd import _lib
    L = _lib.lib()
    n = keys.size
    k = torch.from_numpy(keys.view(np.int32)).cuda()
    r = torch.from_numpy(rects.view(np.int32)).cuda()
    tb = int(L.c3dgs_debug_depth_sort_temp_bytes(n))
    temp = torch.full((tb,), 0xff, dtype=torch.uint8, device="cuda")      # the entry clears what has to be clear
    order, ks, rs = torch.empty_like(k), torch.empty_like(k), torch.empty_like(r)
    passes = C.c_int32(-1)
    _lib.check(L.c3dgs_debug_depth_sort(n, prefiltered, k.data_ptr(), r.data_ptr(), order.data_ptr(), ks.data_ptr(), rs.data_ptr(),
                                        temp.data_ptr(), tb, C.byref(passes), C.c_void_p(torch.cuda.current_stream().cuda_stream)))
    torch.cuda.synchronize()
    return (order.cpu().numpy().view(np.uint32), ks.cpu().numpy().view(np.uint32), rs.cpu().numpy().view(np.uint32).reshape(n, 2),
            passes.value)


@pytest.mark.parametrize("pattern,n", CASES)
def test_depth_sort_matches_numpy_stable_sort(hip, pattern, n):
    rng = np.random.default_rng(7919 * n + len(pattern))
    keys, prefiltered, want_passes = _keys(pattern, n, rng)
    assert keys.dtype == np.uint32 and keys.size == n
    if not prefiltered:
        vis = keys[keys != CULLED]
        assert vis.size == 0 or int(vis.min()) >= BIAS                     # what preprocess's near-plane test guarantees
    # rectangles: four coordinates below 256, in the two halves of two words (as preprocess writes them)
    c = rng.integers(0, 256, (n, 4)).astype(np.uint32)
    rects = np.stack([c[:, 0] | (c[:, 1] << 16), c[:, 2] | (c[:, 3] << 16)], 1).astype(np.uint32)
    want = np.argsort(keys, kind="stable").astype(np.uint32)              # (key, id): ids ascend on input
    order, ks, rs, passes = _depth_sort(keys, rects, prefiltered)
    what = (pattern, n)
    assert passes == want_passes, what
    np.testing.assert_array_equal(order, want, err_msg=str(what))
    np.testing.assert_array_equal(ks, keys[want], err_msg=str(what))
    np.testing.assert_array_equal(rs, rects[want], err_msg=str(what))


def _forward_arrays():
    """the binning arrays of a 2,000-Gaussian 64 x 64 forward with one Gaussian at depth 600 (past the three-pass range)"""
    from c3dgs_amd import _lib
    from oracle import oracle as o
    from tests import gpu_util, synth
    W = H = 64
    focal = 60.0
    intr, ev = synth.camera(W, H, focal)
    cam = o.camera(intr.numpy(), ev.numpy())
    sc = synth.scene(2000, W, H, focal, seed=31, scale_median=0.05)
    sc["means3D"][7] = torch.tensor([0.5, -0.25, 600.0])
    sc["scales"][7] = torch.tensor([2.0, 2.0, 2.0])
    inp = dict(bg=torch.zeros(3), means3D=sc["means3D"], opacities=sc["opacities"], shs=sc["shs"], scales=sc["scales"],
               rotations=sc["rotations"], degree=3, clamp_color=True)
    fw = gpu_util.hip_forward(inp, cam, False)
    u = gpu_util.unpack(fw)
    P = 2000
    gl = _lib.GeomLayout()
    _lib.lib().c3dgs_get_geom_layout(P, C.byref(gl))
    geom = fw["geom"]
    out = {k: u[k] for k in ("depth_order", "point_list", "keys_sorted", "ranges", "radii")}
    out["num_rendered"] = np.array([u["num_rendered"]])
    out["depth_keys"] = u["depths"].view(np.uint32)
    out["depth_keys_sorted"] = gpu_util._view(geom, gl.depth_keys_sorted, P, torch.int32).cpu().numpy().view(np.uint32)
    out["sorted_offsets"] = gpu_util._view(geom, gl.sorted_offsets, 2 * P, torch.int32).cpu().numpy().view(np.uint32)
    return out


def test_forward_with_a_far_gaussian_bins_as_the_rocprim_path(hip, tmp_path):
    got = _forward_arrays()
    keys = got["depth_keys"]
    assert keys[7] == _bits([600.0])[0] >= LIMIT3 and got["radii"][7] > 0, "the far Gaussian must be visible: the fallback runs"
    assert int((keys == CULLED).sum()) > 0 and got["num_rendered"][0] > 2000
    # (depth_order, sorted keys and rectangles of the culled tail included: the sort is over all P)
    ref_path = str(tmp_path / "rocprim.npz")
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    r = subprocess.run([sys.executable, "-m", "tests.test_depth_sort3_gpu", ref_path], cwd=root,
                       env=dict(os.environ, C3DGS_SORT_ROCPRIM="1"), capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    ref = np.load(ref_path)
    assert set(ref.files) == set(got)
    for k in sorted(got):
        np.testing.assert_array_equal(got[k], ref[k], err_msg=k)


if __name__ == "__main__":
    assert os.environ.get("C3DGS_SORT_ROCPRIM") == "1"
    np.savez(sys.argv[1], **_forward_arrays())
