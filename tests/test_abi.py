"""CPU: the C-ABI shared library loads without a GPU, exports every symbol include/c3dgs_hip.h declares and the test hooks of
include/c3dgs_hip_debug.h, keeps the measurement entries to the diag variants, and its argument validation (no device work)
returns the documented codes."""
import ctypes as C
import os
import re

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def L():
    from c3dgs_amd import build, _lib
    build.build()
    return _lib.lib()


TEST_HOOKS = {"c3dgs_debug_sort_temp_bytes", "c3dgs_debug_sort_pairs", "c3dgs_debug_tile_sort_temp_bytes",
              "c3dgs_debug_tile_sort_pairs", "c3dgs_debug_wd_scores"}
MEASUREMENT = {"c3dgs_debug_lane_counters", "c3dgs_debug_sort_times", "c3dgs_debug_gather_probe"}


def _declared_symbols(header="c3dgs_hip.h"):
    h = open(os.path.join(ROOT, "include", header)).read()
    h = re.sub(r"/\*.*?\*/", "", h, flags=re.S)
    return sorted(set(re.findall(r"\b(c3dgs_[a-z0-9_]+)\s*\(", h)))


def test_every_declared_symbol_is_exported_and_bound(L):
    from c3dgs_amd import _lib
    syms = _declared_symbols()
    assert len(syms) >= 15
    assert not [s for s in syms if s.startswith("c3dgs_debug_")], "the public header declares no debug entry"
    assert set(_declared_symbols("c3dgs_hip_debug.h")) == TEST_HOOKS | MEASUREMENT
    for s in syms + sorted(TEST_HOOKS):
        assert hasattr(L, s), f"{s} declared in include/c3dgs_hip.h or as a test hook in c3dgs_hip_debug.h but not exported"
        assert s in _lib.PROTOTYPES, f"{s} has no ctypes prototype"
    assert L.c3dgs_abi_version() == 4


def test_product_library_exports_no_measurement_entry(L):
    from c3dgs_amd import _lib
    assert set(_lib.DIAG_PROTOTYPES) == MEASUREMENT and not MEASUREMENT & set(_lib.PROTOTYPES)
    for s in sorted(MEASUREMENT):
        assert not hasattr(L, s), f"{s} is a measurement entry: only the diag variants may export it"


def test_every_diag_variant_links_and_exports_the_measurement_entries(L):
    from c3dgs_amd import build
    assert set(build.VARIANTS) == {"spin1"} and set(build.DIAG_VARIANTS) == {"lanes", "bwdtime", "ostime"}
    for name in build.DIAG_VARIANTS:
        lib = C.CDLL(build.build_variant(name))             # loads: no undefined symbol
        for s in sorted(MEASUREMENT | TEST_HOOKS) + _declared_symbols():
            assert hasattr(lib, s), f"{s} missing from the {name} variant"
        assert lib.c3dgs_debug_lane_counters(None, None) == 1 and lib.c3dgs_debug_sort_times(None) == 1   # NULL buffer: refused


def test_layouts_are_consistent(L):
    from c3dgs_amd import _lib
    g = _lib.GeomLayout()
    assert L.c3dgs_get_geom_layout(1000, C.byref(g)) == 0
    offs = [g.splat, g.depth_keys, g.depth_keys_sorted, g.depth_order, g.sorted_offsets,
            g.inst_offset, g.rects, g.clamped, g.scan_temp]
    assert offs == sorted(offs) and all(o % 256 == 0 for o in offs) and g.total_bytes > g.scan_temp
    assert g.depth_keys - g.splat >= 1000 * 48
    b = _lib.BinningLayout()
    assert L.c3dgs_get_binning_layout(5000, 1920, 1080, C.byref(b)) == 0
    assert b.values_unsorted - b.keys_unsorted >= 5000 * 2 and b.total_bytes > b.sort_temp
    im = _lib.ImageLayout()
    assert L.c3dgs_get_image_layout(1920, 1080, C.byref(im)) == 0
    assert im.n_contrib - im.final_T >= 1920 * 1080 * 4 and im.tile_used - im.ranges >= 8160 * 8
    assert L.c3dgs_backward_workspace_bytes(10, 1000) >= 1000 * 36
    assert L.c3dgs_get_geom_layout(-1, C.byref(g)) == 1


def _up256(v):
    return (v + 255) // 256 * 256


def test_backward_layout_is_the_workspace_the_backward_asks_for(L):
    """One layout (csrc/common.hpp: backward_layout) gives the size the library asks its workspace callback for and every pointer
    it carves from it. Regions are 256-byte aligned, in order, and large enough for R instances and ceil(P / list_len) lists."""
    from c3dgs_amd import _lib
    for P in (0, 1, 1023, 1024, 1025, 2048, 2049, 3_000_000):
        for R in (0, 1, 255, 256, 257, 16_400_000):
            b = _lib.BackwardLayout()
            assert L.c3dgs_get_backward_layout(P, R, C.byref(b)) == 0, (P, R)
            assert b.list_len == 1024
            r, n_lists = max(R, 1), (max(P, 1) + b.list_len - 1) // b.list_len
            offs = [b.partials, b.touched, b.live_ids, b.live_slots, b.live_count, b.total_bytes]
            assert all(x < y for x, y in zip(offs, offs[1:])) and all(o % 256 == 0 for o in offs), (P, R, offs)
            assert b.touched - b.partials >= 36 * r
            assert b.live_ids - b.touched >= r
            assert b.live_slots - b.live_ids >= 4 * n_lists * b.list_len
            assert b.live_count - b.live_slots >= 4 * n_lists * b.list_len
            assert b.total_bytes - b.live_count >= 4 * n_lists
            assert b.total_bytes == L.c3dgs_backward_workspace_bytes(P, R), (P, R)
    b = _lib.BackwardLayout()
    assert L.c3dgs_get_backward_layout(-1, 10, C.byref(b)) == 1
    assert L.c3dgs_get_backward_layout(10, -1, C.byref(b)) == 1


def test_image_and_compact_layouts_agree(L):
    """The image buffer's private tail (tile_used_c | n_contrib_c) sits right behind its public fields and ends the buffer; the
    binning half of the compact layout depends on R alone."""
    from c3dgs_amd import _lib
    for W, H in ((9, 5), (203, 131), (1920, 1080), (4096, 4096), (7680, 4320)):
        T = ((W + 15) // 16) * ((H + 15) // 16)
        il = _lib.ImageLayout()
        assert L.c3dgs_get_image_layout(W, H, C.byref(il)) == 0
        for R in (0, 1, 255, 256, 257, 5000, 16_400_000):
            cl, bl = _lib.CompactLayout(), _lib.BinningLayout()
            assert L.c3dgs_get_compact_layout(R, W, H, C.byref(cl)) == 0
            assert L.c3dgs_get_binning_layout(R, W, H, C.byref(bl)) == 0
            assert il.total_bytes == cl.n_contrib_c + _up256(4 * W * H), (W, H)
            assert cl.tile_used_c == il.tile_order + _up256(4 * T), (W, H)
            assert cl.n_contrib_c == cl.tile_used_c + _up256(4 * T), (W, H)
            assert cl.cqm == bl.sort_temp and cl.cid - cl.cqm == _up256(max(R, 1)), (W, H, R)
            assert cl.cid + 4 * max(R, 1) <= bl.sort_temp + bl.sort_temp_bytes, (W, H, R)


STAGE_NAMES = ("mark_visible", "preprocess", "depth_sort", "scan", "duplicate_with_keys", "sort", "identify_ranges",
               "render_forward", "zero_partials", "render_backward", "backward_preprocess", "weighted_distance", "vq_accumulate",
               "vq_apply", "l1_ssim_forward", "l1_ssim_backward", "qat_observe", "qat_codebooks", "qat_visible", "qat_points",
               "qat_points_backward", "qat_codebooks_backward", "adam_step", "knn_sort", "knn_bounds", "knn_query")


def test_profile_only_knows_every_stage_name(L):
    """The 26 names bench.py and tools/ select stages by, spelled out: they are the contract, not the library's table."""
    assert len(set(STAGE_NAMES)) == 26
    try:
        for name in STAGE_NAMES:
            assert L.c3dgs_profile_only(name.encode()) == 0, name
        assert L.c3dgs_profile_only(b"render_backwards") == 1 and b"unknown stage" in L.c3dgs_last_error()
        assert L.c3dgs_profile_only(b"camera_from_pose") == 1            # launch-checked, never timed
    finally:
        assert L.c3dgs_profile_only(None) == 0


def test_validation_without_gpu(L):
    from c3dgs_amd import _lib
    # N == 0 is legal and touches nothing
    assert L.c3dgs_weighted_distance(0, 4, 6, None, None, None, None, None, None) == 0
    assert L.c3dgs_weighted_distance(10, 4, 6, None, None, None, None, None, None) == 1
    assert b"dimension 2" in L.c3dgs_last_error()
    assert L.c3dgs_mark_visible(0, None, None, None, None, None) == 0
    assert L.c3dgs_mark_visible(5, None, None, None, None, None) == 1
    assert L.c3dgs_mark_visible_pose(0, None, None, None, None) == 0
    assert L.c3dgs_mark_visible_pose(5, None, None, None, None) == 1
    p = _lib.RasterParams()
    p.P, p.W, p.H = 4, 64, 64
    n = C.c_int32(0)
    cb = _lib.RESIZE_FN(lambda u, b: 0)
    rc = L.c3dgs_rasterize_gaussians(C.byref(p), cb, None, cb, None, cb, None, None, None, C.byref(n), None)
    assert rc == 1 and b"means3D must have dimensions" in L.c3dgs_last_error()
    assert L.c3dgs_vq_apply(0, 4, None, None, None, 0.8, 0.2, 1e-5, 0, None) == 1
    st = (_lib.StageTime * 4)()
    assert L.c3dgs_profile_read(st, 4) == 0


def test_missing_library_fails_loudly(monkeypatch, tmp_path):
    from c3dgs_amd import _lib
    monkeypatch.setattr(_lib, "_lib", None)
    monkeypatch.setattr(_lib, "LIB_PATH", str(tmp_path / "nope.so"))
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        _lib.lib()


def test_image_size_limits(L):
    """More than 65,536 tiles is no longer a limit (32-bit tile keys take over, tests/test_raster_gpu.py::test_8k_image_...); what is
    rejected up front: tile coordinates beyond 16 bits and (tiles per row)^2 x (tile rows) >= 2^32 (the pair emission's exact
    multiply-high division). Checked without a GPU: validation runs before any launch, the callbacks refuse to allocate."""
    from c3dgs_amd import _lib
    one = (C.c_float * 16)()

    def call(W, H):
        p = _lib.RasterParams()
        p.P, p.W, p.H = 4, W, H
        for name in ("background", "means3D", "sh", "opacities", "scales", "rotations", "viewmatrix", "projmatrix", "campos"):
            setattr(p, name, C.addressof(one))
        p.M, p.D = 16, 3
        n = C.c_int32(0)
        cb = _lib.RESIZE_FN(lambda u, b: 0)
        rc = L.c3dgs_rasterize_gaussians(C.byref(p), cb, None, cb, None, cb, None, C.addressof(one), C.addressof(one), C.byref(n), None)
        return rc, L.c3dgs_last_error()

    rc, msg = call(7680, 4320)                           # 480 x 270 = 129,600 tiles: accepted (fails later, at the refused allocation)
    assert rc != 0 and b"allocation failed" in msg, msg
    rc, msg = call(40_000, 30_000)                       # 2500^2 x 1875 tiles^3 > 2^32
    assert rc == 1 and b"image too large" in msg, msg
    rc, msg = call(16 * 65536, 16)
    assert rc == 1 and b"16-bit tile coordinates" in msg, msg
    il = _lib.ImageLayout()
    assert L.c3dgs_get_image_layout(7680, 4320, C.byref(il)) == 0 and il.tile_order >= il.tile_used + 4 * 129_600
    b2, b4 = _lib.BinningLayout(), _lib.BinningLayout()
    L.c3dgs_get_binning_layout(1000, 4096, 4096, C.byref(b2))        # 65,536 tiles: 16-bit keys
    L.c3dgs_get_binning_layout(1000, 4112, 4096, C.byref(b4))        # 65,792 tiles: 32-bit keys
    assert b2.values_unsorted - b2.keys_unsorted < b4.values_unsorted - b4.keys_unsorted


def test_tile_sort_at_65536_tiles_is_sized_as_a_two_pass_16_bit_sort(L):
    """Exactly 65,536 tiles (4096 x 4096 pixels): higher_msb(65536) = 17, but the keys are 16-bit and every tile id fits them.
    The forward's tile sort (and its scratch) must use 16 bits -- two digit passes -- not the three-pass 17-bit plan the 16-bit
    sort cannot carry out (its look-back-free first pass holds global histograms for two passes only)."""
    from c3dgs_amd import _lib
    for n in (1, 8191, 8192, 8193, 1_000_000, 16_000_000):
        t = L.c3dgs_debug_tile_sort_temp_bytes(65536, n)
        assert t == L.c3dgs_debug_sort_temp_bytes(2, n, 16), n
        assert t < L.c3dgs_debug_sort_temp_bytes(2, n, 17), n
        assert t == L.c3dgs_debug_tile_sort_temp_bytes(65535, n), n       # same key width, same 16 bits
        assert L.c3dgs_debug_tile_sort_temp_bytes(65537, n) > t, n        # 32-bit keys from 65,537 tiles on
        b = _lib.BinningLayout()
        assert L.c3dgs_get_binning_layout(n, 4096, 4096, C.byref(b)) == 0
        assert b.sort_temp_bytes == t, n                                   # the forward sizes what the sort entry sorts with
        b17 = _lib.BinningLayout()
        assert L.c3dgs_get_binning_layout(n, 4112, 4096, C.byref(b17)) == 0
        assert b17.sort_temp_bytes == L.c3dgs_debug_tile_sort_temp_bytes(257 * 256, n), n


def test_tile_sort_debug_entries_validate_their_arguments(L):
    """Grids of 1 .. 256 x 65,535 tiles (the largest validate() accepts); n in [0, 2^30); NULL buffers and a short temp are
    refused before any device work (so this runs without a GPU)."""
    fake = C.c_void_p(16)
    big = 256 * 65535
    assert L.c3dgs_debug_tile_sort_temp_bytes(big, 1000) > 0
    for tiles, n in ((0, 10), (-1, 10), (big + 1, 10), (2, -1), (2, 1 << 30)):
        assert L.c3dgs_debug_tile_sort_temp_bytes(tiles, n) == 0, (tiles, n)
        assert b"bad arguments" in L.c3dgs_last_error()
        assert L.c3dgs_debug_tile_sort_pairs(tiles, n, fake, fake, fake, fake, fake, 1 << 40, None) == 1, (tiles, n)
        assert b"bad arguments" in L.c3dgs_last_error()
    assert L.c3dgs_debug_tile_sort_pairs(65536, 0, None, None, None, None, None, 0, None) == 0      # nothing to sort
    for i in range(5):
        ptrs = [fake] * 5
        ptrs[i] = None
        assert L.c3dgs_debug_tile_sort_pairs(65536, 100, *ptrs, 1 << 40, None) == 1, i
        assert b"NULL buffer" in L.c3dgs_last_error()
    for tiles in (2, 65536, 65537, big):
        need = L.c3dgs_debug_tile_sort_temp_bytes(tiles, 100_000)
        assert L.c3dgs_debug_tile_sort_pairs(tiles, 100_000, fake, fake, fake, fake, fake, need - 1, None) == 1, tiles
        assert b"temp smaller" in L.c3dgs_last_error()
