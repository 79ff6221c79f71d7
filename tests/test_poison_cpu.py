"""The poison harness itself (tests/poison.py), proven on CPU tensors with three torch-only stand-ins for a kernel: one that reads
its workspace before writing it, one that writes one element past its buffer, and a well-behaved one. The stand-ins allocate from
THIS module, so the harness is told to treat it as the owner. The only mutation-style check of the scratch tests: no kernel is
broken on purpose to watch a GPU test fail."""
import numpy as np
import pytest
import torch

from tests import poison

ME = (__name__,)


def _reads_before_write(x):
    ws = torch.empty(64, dtype=torch.float32)
    s = ws.sum()                                    # the bug: nothing has written ws yet
    ws.copy_(x[:64])
    return {"out": x * 2 + s}


def _writes_past_the_end(x):
    ws = torch.empty(16, dtype=torch.float32)
    torch.as_strided(ws, (17,), (1,)).fill_(1.0)    # the bug: element 16 of a 16-element buffer
    return {"out": x + ws.sum()}


def _well_behaved(x):
    ws = torch.empty((4, 16), dtype=torch.float32)
    tmp = torch.empty_like(x)
    idx = x.new_empty(3, dtype=torch.int64)
    ws.copy_(x[:64].view(4, 16))
    tmp.copy_(x)
    idx.copy_(torch.arange(3))
    return {"out": tmp + ws.sum(), "idx": idx, "loose": tmp * (1 + 1e-7)}


X = torch.linspace(-1, 1, 100)


def test_a_read_before_write_is_reported():
    with pytest.raises(AssertionError, match="out"):
        poison.assert_independent(lambda: _reads_before_write(X), exact=("out",), device="cpu", owners=ME)
    # not bit-exact either way: the 0xFF run turns NaN where the 0x00 run is finite
    with pytest.raises(AssertionError, match="NaN/Inf"):
        poison.assert_independent(lambda: _reads_before_write(X), barred={"out": lambda v: None}, device="cpu", owners=ME)


def test_a_write_past_the_buffer_is_reported_with_its_record():
    with pytest.raises(AssertionError) as e:
        with poison.poisoned(0xFF, device="cpu", owners=ME) as p:
            _writes_past_the_end(X)
    msg = str(e.value)
    assert "64 bytes, float32 [16]" in msg and "_writes_past_the_end" in msg and __name__ in msg
    assert "back guard: 4 byte(s) changed, the first at payload offset 64" in msg
    assert len(p.records) == 1 and p.records[0].damage() is not None
    # one element in front of it: the front guard
    g = poison.buffer(64, 0x7F, device="cpu")
    torch.as_strided(g.raw, (1,), (1,), g.off - 1).fill_(0)
    with pytest.raises(AssertionError, match="front guard: 1 byte"):
        g.check()


def test_a_well_behaved_stand_in_passes():
    seen = []
    base = poison.assert_independent(lambda: _well_behaved(X), exact=("out", "idx"),
                                     barred={"loose": lambda v: np.testing.assert_allclose(v, X.numpy(), rtol=1e-6, atol=1e-6)},
                                     check=lambda o: seen.append(sorted(o)), device="cpu", owners=ME)
    assert seen == [["idx", "loose", "out"]] * 3
    np.testing.assert_array_equal(base["idx"], [0, 1, 2])


def test_the_carve_out():
    """payload 256-byte aligned and filled with the byte, guards with the canary, records complete; torch.zeros, other devices'
    and other modules' allocations untouched; the allocators are put back on exit"""
    before = (torch.empty, torch.empty_like, torch.Tensor.new_empty)
    with poison.poisoned(0x7F, guard=512, device="cpu", owners=ME) as p:
        a = torch.empty((3, 5), dtype=torch.int32)
        z = torch.zeros(7)
        b = torch.empty_like(a)
        e = torch.empty(0)
        np.testing.assert_array_equal(np.empty(3).shape, (3,))
        buf = poison.buffer(100, 0xFF, device="cpu", guard=512)
    assert (torch.empty, torch.empty_like, torch.Tensor.new_empty) == before
    assert [(r.nbytes, r.dtype, r.shape) for r in p.records] == [(60, torch.int32, (3, 5)), (60, torch.int32, (3, 5)),
                                                                  (0, torch.float32, (0,)), (100, torch.uint8, (100,))]
    assert all("test_the_carve_out" in r.frame for r in p.records)
    assert a.data_ptr() % 256 == 0 and b.data_ptr() % 256 == 0 and buf.ptr % 256 == 0
    assert bool((a == 0x7F7F7F7F).all()) and bool((z == 0).all()) and e.numel() == 0
    assert bool((buf.payload == 0xFF).all())
    for r in p.records:
        assert bool((r.raw[r.off - 512:r.off] == poison.CANARY).all())
        assert bool((r.raw[r.off + r.nbytes:r.off + r.nbytes + 512] == poison.CANARY).all())
    assert poison.CANARY not in poison.POISON_BYTES


def test_the_cached_workspaces_are_set_aside_and_put_back():
    from c3dgs_amd import _lib, rasterizer
    marker = torch.zeros(1)
    _lib._workspaces["poison-test", "cpu"] = marker
    rasterizer._pose_workspace.bufs["cpu"] = marker
    before = set(_lib._workspaces)
    try:
        with poison.poisoned(0xFF, device="cpu"):
            assert not _lib._workspaces and not rasterizer._pose_workspace.bufs
            ws = _lib.workspace("poison-test", "cpu", 300)                       # requested again, under poison
            assert bool((ws == 0xFF).all()) and ws.numel() == 300
            assert bool((rasterizer._pose_workspace.get("cpu", 10) == 0xFF).all())
        assert _lib._workspaces["poison-test", "cpu"] is marker and _lib._workspaces.keys() == before
        assert rasterizer._pose_workspace.bufs["cpu"] is marker
    finally:
        _lib._workspaces.pop(("poison-test", "cpu"), None)
        rasterizer._pose_workspace.bufs.pop("cpu", None)
