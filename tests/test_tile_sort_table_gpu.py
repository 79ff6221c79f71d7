"""-m gpu: the table-driven tile-key sort (csrc/radix_sort.hip: every pass of the u16 sort takes its offsets from a per-tile digit
table, no look-back) against torch's stable sort on the CPU, element for element: item counts one short of, at and one past one
and two 8192-item sort tiles, key widths that take one pass (1, 5, 8 bits) and two (9 bits, the headline's 13 bits), and key
patterns that leave one of the two digits (or both) constant. Payloads are distinct in every case, so a pass that is not stable
or reads another tile's table row shows as a wrong payload. Every case runs twice: the two results must be bit-identical."""
import ctypes as C

import pytest
import torch

pytestmark = pytest.mark.gpu

TILE = 8192
COUNTS = [1, TILE - 1, TILE, TILE + 1, 2 * TILE + 1, 5 * TILE - 1]
WIDTHS = [1, 5, 8, 9, 13]
PATTERNS = ["equal", "second_digit_only", "first_digit_only", "uniform"]


def _sort(keys, values, end_bit):
    """c3dgs_debug_sort_pairs with 2-byte keys: the product's tile-key sort on `end_bit` bits (as tests/test_sort_gpu.py)"""
    from c3dgs_amd import _lib
    L = _lib.lib()
    n = keys.numel()
    tb = int(L.c3dgs_debug_sort_temp_bytes(2, n, end_bit))
    # scratch filled with ones: the sort must not depend on cleared or left-over control words
    temp = torch.full((max(tb, 256),), 0xff, dtype=torch.uint8, device="cuda")
    ko, vo = torch.empty_like(keys), torch.empty_like(values)
    _lib.check(L.c3dgs_debug_sort_pairs(2, n, end_bit, keys.data_ptr(), ko.data_ptr(), values.data_ptr(), vo.data_ptr(),
                                        temp.data_ptr(), tb, C.c_void_p(torch.cuda.current_stream().cuda_stream)))
    return ko, vo


def _keys(n, bits, pattern, g):
    """int64 keys below 2^bits. The digits are os_plan's (csrc/radix_sort.hip): ceil(bits / 8) passes, the bits spread evenly, the
    wider digit first (13 -> 7 + 6, 9 -> 5 + 4); a width of one pass has no second digit, so its "second digit only" keys are all
    equal."""
    passes = (bits + 7) // 8
    lo_bits = (bits + passes - 1) // passes
    hi_bits = bits - lo_bits
    lo = torch.randint(0, 1 << lo_bits, (n,), generator=g)
    hi = torch.randint(0, 1 << hi_bits, (n,), generator=g) if hi_bits else torch.zeros(n, dtype=torch.int64)
    lo_c, hi_c = (1 << lo_bits) - 1, ((1 << hi_bits) - 1) if hi_bits else 0
    if pattern == "equal":
        return torch.full((n,), (hi_c << lo_bits) | (lo_c >> 1), dtype=torch.int64)
    if pattern == "second_digit_only":
        return (hi << lo_bits) | lo_c
    if pattern == "first_digit_only":
        return (hi_c << lo_bits) | lo
    return (hi << lo_bits) | lo


@pytest.mark.parametrize("bits", WIDTHS)
@pytest.mark.parametrize("n", COUNTS)
def test_table_driven_tile_sort_matches_cpu_stable_sort(n, bits):
    g = torch.Generator().manual_seed(1000 * bits + n)
    for pattern in PATTERNS:
        k64 = _keys(n, bits, pattern, g)
        assert int(k64.min()) >= 0 and int(k64.max()) < (1 << bits)
        pay = torch.randperm(n, generator=g).to(torch.int32)            # every payload distinct: stability is visible
        want = torch.sort(k64, stable=True)                              # on the CPU
        keys = k64.to(torch.int32).to(torch.int16).cuda()                # 16-bit keys: same bits, wrapped
        vals = pay.cuda()
        ko1, vo1 = _sort(keys, vals, bits)
        ko2, vo2 = _sort(keys, vals, bits)
        torch.cuda.synchronize()
        what = (n, bits, pattern)
        assert torch.equal(ko1.cpu().to(torch.int64) & 0xffff, want.values), what
        assert torch.equal(vo1.cpu(), pay[want.indices]), what
        assert torch.equal(ko1, ko2) and torch.equal(vo1, vo2), what
