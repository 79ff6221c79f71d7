"""-m gpu: the hand-written stable onesweep radix sort of the binning stage (csrc/radix_sort.hip) against torch's stable
sort: ragged sizes around the 8192-item tile, every digit split the tile sort can take, heavy ties, both key widths."""
import ctypes as C

import pytest
import torch

pytestmark = pytest.mark.gpu


def _sort(keys, values, end_bit):
    from c3dgs_amd import _lib
    L = _lib.lib()
    kb = keys.element_size()
    n = keys.numel()
    tb = int(L.c3dgs_debug_sort_temp_bytes(kb, n, end_bit))
    temp = torch.empty(max(tb, 256), dtype=torch.uint8, device="cuda")
    ko, vo = torch.empty_like(keys), torch.empty_like(values)
    _lib.check(L.c3dgs_debug_sort_pairs(kb, n, end_bit, keys.data_ptr(), ko.data_ptr(), values.data_ptr(), vo.data_ptr(),
                                        temp.data_ptr(), tb, C.c_void_p(torch.cuda.current_stream().cuda_stream)))
    return ko, vo


@pytest.mark.parametrize("n", [1, 2, 63, 64, 65, 8191, 8192, 8193, 16384, 100_003, 1_000_000, 3_000_001])
def test_tile_key_sort_is_stable_for_ragged_sizes(n):
    g = torch.Generator(device="cuda").manual_seed(n)
    for end_bit, hi in ((13, 8160), (7, 100), (16, 65536), (9, 300), (1, 2)):
        keys = torch.randint(0, min(hi, 1 << end_bit), (n,), device="cuda", generator=g, dtype=torch.int32).to(torch.int16)
        vals = torch.arange(n, device="cuda", dtype=torch.int32)
        ko, vo = _sort(keys, vals, end_bit)
        k32 = keys.to(torch.int32) & 0xffff
        want = torch.sort(k32, stable=True)
        assert torch.equal(vo.long(), want.indices), (n, end_bit)
        assert torch.equal(ko.to(torch.int32) & 0xffff, want.values), (n, end_bit)


@pytest.mark.parametrize("n", [1, 511, 8192, 8193, 300_000, 3_000_000])
def test_depth_key_sort_matches_stable_sort(n):
    g = torch.Generator(device="cuda").manual_seed(n + 7)
    depth = torch.rand(n, device="cuda", generator=g) * 10 + 2
    depth[torch.rand(n, device="cuda", generator=g) < 0.06] = float("nan")          # culled: key 0xFFFFFFFF
    keys = depth.view(torch.int32).clone()
    keys[torch.isnan(depth)] = -1
    keys[::7] = int(keys[0])                                                       # heavy ties
    vals = torch.arange(n, device="cuda", dtype=torch.int32)
    ko, vo = _sort(keys, vals, 32)
    ku = keys.to(torch.int64) & 0xffffffff
    want = torch.sort(ku, stable=True)
    assert torch.equal(vo.long(), want.indices)
    assert torch.equal(ko.to(torch.int64) & 0xffffffff, want.values)


def test_sort_of_already_sorted_and_constant_keys():
    n = 50_000
    vals = torch.arange(n, device="cuda", dtype=torch.int32)
    const = torch.full((n,), 4321, device="cuda", dtype=torch.int16)
    ko, vo = _sort(const, vals, 13)
    assert torch.equal(vo, vals) and torch.equal(ko, const)
    asc = (torch.arange(n, device="cuda") * 8160 // n).to(torch.int16)
    ko, vo = _sort(asc, vals, 13)
    assert torch.equal(vo, vals) and torch.equal(ko, asc)


def test_rocprim_fallback_gives_the_same_sorted_lists():
    """C3DGS_SORT_ROCPRIM=1 (also taken automatically from 2^30 items on) routes both sorts through rocPRIM: the raster
    parity cases that compare the sorted keys / point list bit-exactly must pass unchanged. Run in a child process
    because the switch is read once per process."""
    import os
    import subprocess
    import sys
    env = dict(os.environ, C3DGS_SORT_ROCPRIM="1")
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    r = subprocess.run([sys.executable, "-m", "pytest", "tests/test_raster_gpu.py", "tests/test_sort_gpu.py", "-q", "-m", "gpu", "-x",
                        "-k", "(forward_parity and (base or wide_depth or p8193 or equal_depth or indexed)) or ragged or stable_sort or grid_limit"],
                       cwd=root, env=env, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    assert " passed" in r.stdout


def test_depth_sort_gather_path_gives_the_same_sorted_lists():
    """By default the depth sort carries every Gaussian's tile rectangle through its passes as a packed second payload (grids up
    to 255 x 255 tiles); C3DGS_DEPTH_SORT_GATHER=1 makes it gather the rectangles behind the last pass instead (what larger
    grids get). The parity cases that compare keys / point lists / ranges bit-exactly must pass on that path too. Child process:
    the switch is read once per process."""
    import os
    import subprocess
    import sys
    env = dict(os.environ, C3DGS_DEPTH_SORT_GATHER="1")
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    r = subprocess.run([sys.executable, "-m", "pytest", "tests/test_raster_gpu.py", "-q", "-m", "gpu", "-x",
                        "-k", "forward_parity and (base or wide_depth or p8193 or p12289 or equal_depth or indexed or huge_splats)"],
                       cwd=root, env=env, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    assert " passed" in r.stdout


_TIMEOUT_CHILD = r"""
import numpy as np, torch, sys
from tests import cases, gpu_util, synth
from oracle import oracle as orc
from c3dgs_amd import _lib
assert _lib.LIB_PATH.endswith("libc3dgs_hip_spin1.so"), _lib.LIB_PATH
intr, ev = synth.camera(640, 360, 400.0)
cam = orc.camera(intr.numpy(), ev.numpy())
sc = synth.scene(400_000, 640, 360, 400.0, seed=3, scale_median=0.02)
inp = dict(bg=torch.zeros(3), means3D=sc["means3D"], opacities=sc["opacities"], shs=sc["shs"], scales=sc["scales"],
           rotations=sc["rotations"], degree=3, clamp_color=True)
fw = gpu_util.hip_forward(inp, cam, False)           # 49 depth-sort tiles, hundreds of tile-sort tiles: look-backs give up
torch.cuda.synchronize()
assert torch.isnan(fw["color"]).all(), "a forward whose sort timed out must return a NaN image"
try:
    gpu_util.hip_forward(inp, cam, False)
except RuntimeError as e:
    assert "look-back timed out in an earlier rasterizer call" in str(e), str(e)
    print("RAISED")
else:
    sys.exit("the call after a timed-out sort did not fail")
# debug mode reports it in the same call
a = list(fw["args"]); a[-2] = True
from c3dgs_amd import rasterizer as rz
try:
    rz._C.rasterize_gaussians(*a)
except RuntimeError as e:
    assert "look-back timed out" in str(e), str(e)
    print("DEBUG_RAISED")
"""


def test_sort_timeout_is_not_silent():
    """A look-back that gives up (pre-empted / dead predecessor) must not yield a plausible wrong image outside debug mode:
    with the `spin1` variant of the library (C3DGS_OS_SPIN_LIMIT=1: every look-back gives up after one poll) the forward
    returns a NaN image, the next forward fails with C3DGS_E_HIP, and debug mode fails in the same call."""
    import os
    import subprocess
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    lib = os.path.join(root, "c3dgs_amd", "libc3dgs_hip_spin1.so")
    if not os.path.exists(lib):
        from c3dgs_amd import build
        build.build_variant("spin1")
    r = subprocess.run([sys.executable, "-c", _TIMEOUT_CHILD], cwd=root, env=dict(os.environ, C3DGS_LIB_PATH=lib),
                       capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    assert "RAISED" in r.stdout and "DEBUG_RAISED" in r.stdout, r.stdout


# ------------------------------------------------------------------ the forward's tile sort at tile-grid limits
# c3dgs_debug_tile_sort_pairs takes the forward's own route: 16-bit keys up to 65,536 tiles and 32-bit above, sorted on
# min(higher_msb(T), key bits) bits. The grids: the smallest, the packed-rectangle limit (255 / 256 tiles a side), the 1080p
# headline (8160), both sides of the key-width switch (65,535 .. 65,537: 16 bits on 16-bit keys at exactly 65,536), the 32-bit
# key sort at 17 .. 24 bits (three passes of 6 .. 8 bits), and the largest grid the ABI admits (256 x 65,535 tiles).
GRID_TILES = [2, 255, 256, 8160, 65535, 65536, 65537, 1 << 17, (1 << 18) - 1, 1 << 18, 1 << 20, 1 << 22, 256 * 65535]
GRID_N = [1, 8191, 8192, 8193, 12287, 12288, 12289, 1_000_003]


def _tile_sort(T, keys, values):
    from c3dgs_amd import _lib
    L = _lib.lib()
    n = keys.numel()
    assert keys.element_size() == (2 if T <= 65536 else 4)
    tb = int(L.c3dgs_debug_tile_sort_temp_bytes(T, n))
    assert tb > 0, L.c3dgs_last_error()
    temp = torch.empty(tb, dtype=torch.uint8, device="cuda")
    ko, vo = torch.empty_like(keys), torch.empty_like(values)
    _lib.check(L.c3dgs_debug_tile_sort_pairs(T, n, keys.data_ptr(), ko.data_ptr(), values.data_ptr(), vo.data_ptr(),
                                             temp.data_ptr(), tb, C.c_void_p(torch.cuda.current_stream().cuda_stream)))
    return ko, vo


def _grid_shape(T):
    """a tiles_x x tiles_y factorisation of T, as square as its divisors allow"""
    tx = 1
    d = 1
    while d * d <= T:
        if T % d == 0:
            tx = d
        d += 1
    return T // tx, tx


def _emission_keys(T, n, g):
    """the pair emission's shape: per Gaussian, the tile ids of a rectangle (y outer, x inner), Gaussians one after the other
    (depth-major); a few rectangles span whole rows / the whole grid, like screen-filling splats"""
    tx, ty = _grid_shape(T)
    parts, total = [], 0
    while total < n:
        m = 4096
        x0 = torch.randint(0, tx, (m,), device="cuda", generator=g)
        y0 = torch.randint(0, ty, (m,), device="cuda", generator=g)
        w = torch.minimum(tx - x0, torch.randint(1, 24, (m,), device="cuda", generator=g))
        h = torch.minimum(ty - y0, torch.randint(1, 24, (m,), device="cuda", generator=g))
        if not parts:                                   # the first Gaussians cover a full row and, if small enough, the grid
            x0[:2], w[:2], h[0] = 0, tx, 1
            y0[1], h[1] = 0, min(ty, max(1, 200_000 // tx))
        cnt = w * h
        start = torch.cumsum(cnt, 0) - cnt
        own = torch.repeat_interleave(torch.arange(m, device="cuda"), cnt)
        local = torch.arange(int(cnt.sum()), device="cuda") - start[own]
        ry, rx = local // w[own], local % w[own]
        parts.append((y0[own] + ry) * tx + x0[own] + rx)
        total += parts[-1].numel()
    return torch.cat(parts)[:n]


def _grid_keys(T, n, pattern, g):
    if pattern == "uniform":
        k = torch.randint(0, T, (n,), device="cuda", generator=g)
    elif pattern == "top":                              # every key in the top digit of every pass
        k = torch.full((n,), T - 1, device="cuda", dtype=torch.int64)
    elif pattern == "ties":                             # four ids, one of them the largest
        pick = torch.tensor([0, T - 1, T // 2, (T * 2) // 3], device="cuda")
        k = pick[torch.randint(0, 4, (n,), device="cuda", generator=g)]
    else:
        k = _emission_keys(T, n, g)
    assert int(k.min()) >= 0 and int(k.max()) < T
    return k


def _check_tile_sort(T, k64, g, what):
    n = k64.numel()
    keys = (k64.to(torch.int32).to(torch.int16) if T <= 65536 else k64.to(torch.int32))   # 16-bit keys: same bits, wrapped
    vals = torch.randperm(n, device="cuda", generator=g).to(torch.int32)                # distinct payloads pin stability
    ko, vo = _tile_sort(T, keys, vals)
    want = torch.sort(k64, stable=True)
    mask = 0xffff if T <= 65536 else 0xffffffff
    assert torch.equal(ko.to(torch.int64) & mask, want.values), what
    assert torch.equal(vo, vals[want.indices]), what


@pytest.mark.parametrize("T", GRID_TILES)
def test_tile_sort_at_grid_limit_matches_stable_sort(T):
    g = torch.Generator(device="cuda").manual_seed(T)
    for n in GRID_N:
        for pattern in ("uniform", "top", "ties", "emission"):
            _check_tile_sort(T, _grid_keys(T, n, pattern, g), g, (T, n, pattern))


@pytest.mark.parametrize("T", [65536, 1 << 20])
def test_tile_sort_at_grid_limit_of_16m_pairs(T):
    """~16.4 M pairs (the bench view's instance count): thousands of sort tiles per pass, with the emission's shape."""
    g = torch.Generator(device="cuda").manual_seed(T + 1)
    n = 16_400_001
    for pattern in ("uniform", "emission"):
        _check_tile_sort(T, _grid_keys(T, n, pattern, g), g, (T, n, pattern))
