"""Poisoned scratch for the tests: every buffer the package allocates UNINITIALISED is handed out filled with a chosen byte and
fenced by guard bands, so that a kernel that reads a word before anything wrote it, or writes past its buffer, shows in a test
instead of depending on what the caching allocator happens to recycle (include/c3dgs_hip.h promises that the content of scratch
and of outputs on entry does not matter; DESIGN.md "Scratch contracts" says who writes what first).

    with poisoned(0xFF): ...            torch.empty / torch.empty_like / Tensor.new_empty called FROM c3dgs_amd on the target device
                                        come out of one uint8 allocation [guard | payload | guard]; torch.zeros is left alone (its
                                        zero is part of a contract); the cached workspaces are set aside, so they are requested again
    buffer(nbytes, byte, device)        the same carve-out for a test that calls the C ABI through ctypes
    assert_independent(run, ...)        run() under 0x00, 0xFF and 0x7F: no result may change
    under_every_byte(fn)                an existing test function, which is its own reference check, under each of the three bytes

Plain torch, works on CPU tensors (tests/test_poison_cpu.py proves the harness itself there). Not a conftest: nothing here changes
how the suite is collected or run."""
import contextlib
import sys

import numpy as np
import torch

CANARY = 0xC5                       # the guards' byte: none of the poison bytes below, nor the 0xA5 of the older guard tests
POISON_BYTES = (0x00, 0xFF, 0x7F)   # zero (what fresh memory reads as) | NaN, -1, UINT_MAX, the culled depth key | large finite
ALIGN = 256                         # the library's alignment demand on every workspace
OWNERS = ("c3dgs_amd",)             # module-name prefixes whose allocations are poisoned

_active = []                        # the open `poisoned` contexts, innermost last


class Guarded:
    """One carve-out: `raw` = [front guard | payload | back guard] (plus the slack that aligns the payload); `payload` is the
    uint8 view a caller works in, `tensor` the typed view handed to the package."""

    def __init__(self, nbytes, byte, device, guard, alloc, dtype=torch.uint8, shape=None, frame="<test>"):
        self.nbytes, self.byte, self.guard, self.dtype, self.frame = int(nbytes), int(byte), int(guard), dtype, frame
        self.shape = (self.nbytes,) if shape is None else tuple(shape)
        self.raw = alloc(self.nbytes + 2 * self.guard + ALIGN, dtype=torch.uint8, device=device)
        self.off = self.guard + (-(self.raw.data_ptr() + self.guard)) % ALIGN
        self.raw.fill_(CANARY)
        self.payload = self.raw[self.off:self.off + self.nbytes]
        self.payload.fill_(self.byte)
        assert self.nbytes == 0 or self.payload.data_ptr() % ALIGN == 0
        self.tensor = self.payload.view(dtype).view(self.shape) if shape is not None else self.payload

    @property
    def ptr(self):
        return self.payload.data_ptr()

    def describe(self):
        return (f"{self.nbytes} bytes, {str(self.dtype).split('.')[-1]} {list(self.shape)}, poison 0x{self.byte:02X}, "
                f"allocated at {self.frame}")

    def damage(self):
        """-> None, or which guard changed and where (offsets relative to the payload)"""
        front = self.raw[self.off - self.guard:self.off]
        back = self.raw[self.off + self.nbytes:self.off + self.nbytes + self.guard]
        out = []
        for name, band, base in (("front", front, -self.guard), ("back", back, self.nbytes)):
            bad = torch.nonzero(band != CANARY).reshape(-1)
            if bad.numel():
                out.append(f"{name} guard: {bad.numel()} byte(s) changed, the first at payload offset {base + int(bad[0])}")
        return "; ".join(out) or None

    def check(self):
        d = self.damage()
        assert d is None, f"write outside a buffer ({self.describe()}): {d}"


def _device_of(device):
    if device is None:
        device = torch.get_default_device() if hasattr(torch, "get_default_device") else "cpu"
    return torch.device(device)


def _same_device(a, b):
    return a.type == b.type and (a.index is None or b.index is None or a.index == b.index)


def _owner_frame(owners, depth=3):
    """-> "module:function:line" of the caller of a patched allocator (wrapper -> method -> here) if its module belongs to
    `owners` (None: whoever it is), else None"""
    f = sys._getframe(depth)
    name = f.f_globals.get("__name__", "")
    if owners is None or any(name == o or name.startswith(o + ".") for o in owners):
        return f"{name}:{f.f_code.co_name}:{f.f_lineno}"
    return None


class _Poisoned:
    def __init__(self, byte, guard, device, owners):
        assert 0 <= byte <= 0xFF and byte != CANARY
        self.byte, self.guard, self.device, self.owners = byte, guard, _device_of(device), tuple(owners)
        self.records = []

    # ---- the three allocators, patched
    def _carve(self, shape, dtype, frame):
        numel = 1
        for v in shape:
            numel *= int(v)
        nbytes = numel * torch.empty((), dtype=dtype).element_size()
        rec = Guarded(nbytes, self.byte, self.device, self.guard, self._empty, dtype, shape, frame)
        self.records.append(rec)
        return rec.tensor

    def _wants(self, device, kwargs, frame):
        plain = not any(kwargs.get(k) for k in ("out", "pin_memory", "requires_grad", "names")) \
            and kwargs.get("layout", torch.strided) == torch.strided \
            and kwargs.get("memory_format", torch.contiguous_format) in (torch.contiguous_format, torch.preserve_format)
        return frame is not None and plain and _same_device(_device_of(device), self.device)

    def empty(self, *size, **kwargs):
        frame = _owner_frame(self.owners)
        if not self._wants(kwargs.get("device"), kwargs, frame):
            return self._empty(*size, **kwargs)
        shape = tuple(size[0]) if len(size) == 1 and isinstance(size[0], (tuple, list, torch.Size)) else tuple(size)
        dtype = kwargs.get("dtype") or torch.get_default_dtype()
        return self._carve(shape, dtype, frame)

    def empty_like(self, t, **kwargs):
        frame = _owner_frame(self.owners)
        if not self._wants(kwargs.get("device", t.device), kwargs, frame) or not t.is_contiguous():
            return self._empty_like(t, **kwargs)
        return self._carve(tuple(t.shape), kwargs.get("dtype") or t.dtype, frame)

    def new_empty(self, t, *size, **kwargs):
        frame = _owner_frame(self.owners)
        if not self._wants(kwargs.get("device", t.device), kwargs, frame):
            return self._new_empty(t, *size, **kwargs)
        shape = tuple(size[0]) if len(size) == 1 and isinstance(size[0], (tuple, list, torch.Size)) else tuple(size)
        return self._carve(shape, kwargs.get("dtype") or t.dtype, frame)

    # ---- the package's caches: set aside on entry so that they are requested again under poison, put back on exit
    @staticmethod
    def _caches():
        from c3dgs_amd import _lib, model, rasterizer
        return [_lib._workspaces, model._WS] + [v.bufs for v in vars(rasterizer).values() if isinstance(v, rasterizer._GrowOnly)]

    def __enter__(self):
        self._saved = [(c, dict(c)) for c in self._caches()]
        for c, _ in self._saved:
            c.clear()
        self._empty, self._empty_like, self._new_empty = torch.empty, torch.empty_like, torch.Tensor.new_empty
        me = self
        torch.empty = lambda *a, **k: me.empty(*a, **k)
        torch.empty_like = lambda t, **k: me.empty_like(t, **k)
        torch.Tensor.new_empty = lambda t, *a, **k: me.new_empty(t, *a, **k)
        _active.append(self)
        return self

    def __exit__(self, et, ev, tb):
        _active.remove(self)
        torch.empty, torch.empty_like, torch.Tensor.new_empty = self._empty, self._empty_like, self._new_empty
        for c, old in self._saved:
            c.clear()
            c.update(old)
        if self.device.type == "cuda":
            torch.cuda.synchronize(self.device)
        if et is None:
            self.check()
        return False

    def check(self):
        bad = [(r, r.damage()) for r in self.records]
        bad = [f"({r.describe()}): {d}" for r, d in bad if d is not None]
        assert not bad, "write outside a buffer " + " | ".join(bad)


@contextlib.contextmanager
def poisoned(byte, guard=4096, device="cuda", owners=OWNERS):
    """Inside: uninitialised allocations made from `owners`' modules on `device` are filled with `byte` between two guard bands of
    `guard` canary bytes, their payload 256-byte aligned. Yields the manager (`.records`: one Guarded per allocation). On exit it
    synchronises, checks every guard and raises an AssertionError naming the record of each buffer whose guard changed."""
    with _Poisoned(byte, guard, device, owners) as p:
        yield p


def buffer(nbytes, byte, device="cuda", guard=4096):
    """A caller-owned workspace for a ctypes call: -> Guarded (`.ptr`, `.payload`, `.check()`). Inside a `poisoned` context it is
    checked on that context's exit as well."""
    alloc = _active[-1]._empty if _active else torch.empty
    rec = Guarded(nbytes, byte, _device_of(device), guard, alloc, frame=_owner_frame(None, 2))
    if _active:
        _active[-1].records.append(rec)
    return rec


def _np(v):
    if isinstance(v, torch.Tensor):
        v = v.detach().cpu().numpy()
    return np.asarray(v)


def _bits(a):
    a = np.ascontiguousarray(a)
    return a.reshape(-1).view(np.uint8) if a.size else np.zeros(0, np.uint8)


def assert_independent(run, exact=(), barred=None, check=None, check_bytes=POISON_BYTES, device="cuda", owners=OWNERS, guard=4096):
    """Calls `run()` under the three poison bytes; `run` returns {name: array, tensor or scalar}. Every name is in `exact` (bit-equal
    across the three runs) or in `barred` ({name: callable(value) or None}: the family's existing bar against its reference, applied to
    every run's value; None: the name is held by `check`). `check(outputs)`, if given, is the family's existing whole-result check
    against its reference; it is applied to the runs of `check_bytes`, 0xFF always among them, so being equal to a wrong baseline is
    not enough (where every output is exact one run says it for all three). Floating-point outputs must be finite wherever the
    0x00 run's are. -> the outputs of the 0x00 run."""
    barred = barred or {}
    assert 0xFF in check_bytes and set(check_bytes) <= set(POISON_BYTES)
    assert check is not None or all(v is not None for v in barred.values()), "a barred output without a bar"
    assert set(check_bytes) == set(POISON_BYTES) or not barred or check is None, "barred outputs are checked on every run"
    outs = {}
    for byte in POISON_BYTES:
        with poisoned(byte, guard=guard, device=device, owners=owners) as p:
            got = run()
            outs[byte] = {k: _np(v) for k, v in got.items()}
        assert any(r.nbytes for r in p.records), "run() allocated nothing under poison: the family is not covered"
        if check is not None and byte in check_bytes:      # behind the context: its guards are checked, the allocators are torch's again
            check(outs[byte])
    base = outs[POISON_BYTES[0]]
    assert set(base) == set(exact) | set(barred), f"unclassified outputs: {sorted(set(base) ^ (set(exact) | set(barred)))}"
    for byte, got in outs.items():
        what = f"poison 0x{byte:02X}"
        assert got.keys() == base.keys(), what
        for k, v in got.items():
            assert v.shape == base[k].shape and v.dtype == base[k].dtype, (what, k)
            if v.dtype.kind == "f":
                lost = np.isfinite(base[k]) & ~np.isfinite(v)
                assert not lost.any(), f"{what}: {k} has {int(lost.sum())} NaN/Inf where the 0x00 run is finite"
            if k in exact:
                diff = np.nonzero(_bits(v) != _bits(base[k]))[0]
                assert diff.size == 0, (f"{what}: {k} differs from the 0x00 run in {diff.size} byte(s), the first in element "
                                        f"{int(diff[0]) // max(v.dtype.itemsize, 1)}")
            elif barred[k] is not None:
                barred[k](v)
    return base


def under_every_byte(fn, expect_allocations=True):
    """Calls `fn()` once under each poison byte: for a family whose existing test is its own check against its reference (the
    test function is `fn`). `expect_allocations`: the family allocates something uninitialised through the package; False for the
    families whose only workspace is zeroed by contract (their cached workspaces are still set aside and requested again)."""
    for byte in POISON_BYTES:
        with poisoned(byte) as p:
            fn()
        assert not expect_allocations or any(r.nbytes for r in p.records), \
            f"poison 0x{byte:02X}: nothing was allocated under poison, the family is not covered"
