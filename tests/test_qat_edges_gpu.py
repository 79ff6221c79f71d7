"""-m gpu: csrc/qat.hip driven through its C ABI at the sizes, alignments and value ranges the model-level tests
(tests/test_model_gpu.py: one indexed scene, P = 20,000, SH degree 3, well-spread values) never reach:

  * above every block cap (observer 512 blocks, codebooks / stand-alone fake-quant 8192, quantize 4096), with the decisive
    element (minimum, maximum) in the scalar tail or in the first elements, aligned and misaligned bases;
  * SH degree 0 .. 3 (M = 1, 4, 9, 16: float4 and scalar concat paths, features_rest == NULL), every combination of empty
    jobs of the codebook launch, sentinel-filled outputs;
  * degenerate quantiser ranges (constant, one-signed, all-zero, exact rounding ties, values far outside a frozen range,
    non-positive _scaling rows, rotation rows that quantise to zero);
  * visibility patterns (none / all / first / last) around the 256-row block edge, and positions beyond fp16 range;
  * the int8 payload at exact ties of its double division.

Reference: oracle/qat.py (fp32 op order, pinned to torch.ao on the CPU by tests/test_oracle_qat.py). Bars are those of
tests/test_model_gpu.py and no looser: observer state exact for the identity-activation modules and rtol 3e-7 behind sigmoid /
normalize, fake-quantised identity tensors and gradient masks bit-exact, at most 2e-3 of the elements one quantisation step
off only behind a transcendental (opacity) or a division (scales_n)."""
import ctypes as C
import itertools

import numpy as np
import pytest
import torch

from oracle import qat

pytestmark = pytest.mark.gpu
DEV = "cuda"
F32 = np.float32
SENTINEL = 0x4B5A5A5A
SENT_F = float(np.array([SENTINEL], np.int32).view(np.float32)[0])
OP, SC, SF, ROT, DC, REST = range(6)
IDENTITY_SLOTS = (SF, ROT, DC, REST)
SIZES = [1, 2, 3, 4, 5, 1023, 1025, (1 << 21) + 3, 3_000_001, 6_000_001]     # 2^21 + 3: one n % 4 tail past the 512-block cap


# ----------------------------------------------------------------------------------------------------------- plumbing
@pytest.fixture(scope="module")
def L(hip):
    from c3dgs_amd import _lib
    return _lib.lib()


def _stream():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def _ws(L):
    return torch.empty(int(L.c3dgs_qat_workspace_bytes()), dtype=torch.uint8, device=DEV)


def _check(rc):
    from c3dgs_amd import _lib
    _lib.check(rc)


def _new_state(n=6):
    from c3dgs_amd.model import new_fq_state
    return new_fq_state(DEV, n)


def _put_state(state, slot, st):
    state[slot] = torch.from_numpy(st.as_row()).to(DEV)


def _get_state(state, slot):
    row = state[slot].cpu().numpy()
    return F32(row[0]), F32(row[1]), F32(row[2]), int(row[3:4].view(np.int32)[0])


def _assert_state(state, slot, st, exact, what=""):
    lo, hi, scale, zp = _get_state(state, slot)
    if exact:
        assert (lo, hi, scale) == (st.min_val, st.max_val, st.scale), (what, slot, (lo, hi, scale), (st.min_val, st.max_val, st.scale))
    else:
        np.testing.assert_allclose([lo, hi, scale], [st.min_val, st.max_val, st.scale], rtol=3e-7, err_msg=f"{what} slot {slot}")
    assert zp == st.zero_point, (what, slot, zp, st.zero_point)


def _dev(a, off=0):
    """numpy array -> contiguous GPU tensor; off = 1: the `[1:]` view of an aligned buffer (4-byte aligned, not 16)."""
    a = np.ascontiguousarray(a)
    if off == 0:
        return torch.from_numpy(a).to(DEV)
    buf = torch.empty(a.size + 4, dtype=torch.from_numpy(a).dtype, device=DEV)
    view = buf[off:off + a.size]
    view.copy_(torch.from_numpy(a.reshape(-1)))
    assert view.data_ptr() % 16 != 0
    return view.view(a.shape)


def _sentinel(shape, dtype=torch.float32):
    n = int(np.prod(shape))
    if dtype == torch.float32:
        return torch.full((n,), SENTINEL, dtype=torch.int32, device=DEV).view(torch.float32).view(shape)
    return torch.full(shape, 0x5A, dtype=dtype, device=DEV)


def _untouched(t):
    return bool((t.view(torch.int32) == SENTINEL).all())


def _no_sentinel_left(t):
    return not bool((t.view(torch.int32) == SENTINEL).any())


def _ptr(t):
    return None if t is None else t.data_ptr()


def _params(state, *, P=0, GS=0, SHS=0, M=1, xyz=None, opacity=None, scaling_factor=None, scaling=None, rotation=None,
            fdc=None, frest=None, observer=(1,) * 6, fq=(1,) * 6, half_xyz=1):
    from c3dgs_amd import _lib
    q = _lib.QatParams()
    q.P, q.GS, q.SHS, q.M = P, GS, SHS, M
    q.xyz, q.opacity, q.scaling_factor = _ptr(xyz), _ptr(opacity), _ptr(scaling_factor)
    q.scaling, q.rotation, q.features_dc, q.features_rest = _ptr(scaling), _ptr(rotation), _ptr(fdc), _ptr(frest)
    q.state = state.data_ptr()
    for i in range(6):
        q.observer_enabled[i], q.fake_quant_enabled[i] = int(observer[i]), int(fq[i])
    q.half_xyz, q.averaging_constant = int(half_xyz), 0.01
    return q


def _flip_close(a, b, step, what, frac=2e-3):
    """tests/test_model_gpu.py's rule: at most `frac` of the elements differ, and those by one quantisation step."""
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    d = np.abs(a - b)
    tol = 1e-6 * max(1.0, np.abs(b).max())
    flips = d > tol
    assert flips.mean() <= frac, f"{what}: {flips.mean():.2e} differ"
    if flips.any():
        assert d[flips].max() <= float(step) * 1.001 + tol, f"{what}: {d[flips].max()} > step {step}"


def _bits_equal(got, want):
    return np.array_equal(np.asarray(got, np.float32).view(np.int32), np.asarray(want, np.float32).view(np.int32))


def _planted(n, rng, lo, hi, mirror, band=(0.2, 0.3)):
    """n values in a narrow band; the minimum in the LAST element and the maximum in element n - 2 (mirror: first / second)."""
    x = rng.uniform(band[0], band[1], n).astype(np.float32)
    i_lo, i_hi = (0, 1) if mirror else (n - 1, n - 2)
    if n >= 2:
        x[i_hi] = hi
    x[i_lo] = lo
    return x


# ------------------------------------------------------------------------------------- observer: sizes and placement
@pytest.mark.parametrize("off", [0, 1], ids=["aligned", "misaligned"])
@pytest.mark.parametrize("n", SIZES)
def test_observer_finds_extrema_in_tail_and_head(L, n, off):
    """opacity (sigmoid) and scaling_factor (n floats), features_dc and features_rest (3n floats, M = 2; one all-positive, one
    all-negative) and rotation (n rows, always aligned: the ABI asks for it) in ONE observe launch; three observer steps
    (first batch, then two moving-average updates) with the extremum moving between the tail and the head."""
    rng = np.random.default_rng(n)
    state, ws = _new_state(), _ws(L)
    st = {k: qat.FqState() for k in (OP, SF, ROT, DC, REST)}
    for step in range(3):
        mirror = step == 1
        grow = F32(1 + 0.25 * step)
        op = _planted(n, rng, -1.5 * grow, 2.0 * grow, mirror)
        sf = _planted(n, rng, -3.0 * grow, 0.7 * grow, mirror)
        rot = _planted(4 * n, rng, -0.9 * grow, 1.1 * grow, mirror).reshape(n, 4)
        dc = _planted(3 * n, rng, 0.05 * grow, 4.0 * grow, mirror).reshape(n, 1, 3)          # all-positive tensor
        rest = _planted(3 * n, rng, -2.0 * grow, -0.1 * grow, mirror, band=(-0.3, -0.2)).reshape(n, 1, 3)   # all-negative
        t = dict(opacity=_dev(op, off), scaling_factor=_dev(sf, off), rotation=_dev(rot), fdc=_dev(dc, off), frest=_dev(rest, off))
        q = _params(state, P=n, GS=n, SHS=n, M=2, **t)
        _check(L.c3dgs_qat_observe(C.byref(q), ws.data_ptr(), _stream()))
        torch.cuda.synchronize()
        for slot, x in ((OP, qat.sigmoid(op)), (SF, sf), (ROT, rot), (DC, dc), (REST, rest)):
            qat.observe(st[slot], x)
            _assert_state(state, slot, st[slot], exact=slot in IDENTITY_SLOTS, what=f"n={n} step {step}")
    lo, hi, _, _ = _get_state(state, SC)
    assert lo == np.inf and hi == -np.inf, "a module without input must keep its state"


@pytest.mark.parametrize("off", [0, 1], ids=["aligned", "misaligned"])
@pytest.mark.parametrize("rows", SIZES + [(1 << 19) + 1])
def test_observer_scaling_rows(L, rows, off):
    """_scaling is observed through normalize(relu(.)) row by row: 2^19 + 1 rows is one row past the 512-block cap."""
    rng = np.random.default_rng(rows)
    state, ws = _new_state(), _ws(L)
    st = qat.FqState()
    for step in range(3):
        x = rng.uniform(0.5, 0.65, (rows, 3)).astype(np.float32)
        i_lo, i_hi = (0, 1) if step == 1 else (rows - 1, rows - 2)
        if rows >= 2:
            x[i_hi] = (5.0 + step, 0.6, 0.6)                        # the largest normalised component
        x[i_lo] = (1.0, 1.0, 0.01 * (1 + step))                     # the smallest
        t = _dev(x, off)
        q = _params(state, GS=rows, scaling=t)
        _check(L.c3dgs_qat_observe(C.byref(q), ws.data_ptr(), _stream()))
        torch.cuda.synchronize()
        v, _, _ = qat.normalize_rows(np.maximum(x, F32(0)))
        qat.observe(st, v)
        _assert_state(state, SC, st, exact=False, what=f"rows={rows} step {step}")


# ------------------------------------------------------------------------------------- stand-alone fake-quant module
@pytest.mark.parametrize("off", [0, 1], ids=["aligned", "misaligned"])
@pytest.mark.parametrize("n", SIZES + [(1 << 23) + 5])
def test_standalone_fake_quantize_sizes_and_alignment(L, n, off):
    """c3dgs_fake_quantize + backward: state, outputs and masks bit-exact. 2^23 + 5 is past the 8192-block cap of the
    elementwise kernel. From the second step on the moving average lags behind the growing extremes: clamped values, mask 0."""
    rng = np.random.default_rng(n + off)
    state, ws = _new_state(1), _ws(L)
    st = qat.FqState()
    for step in range(3):
        grow = F32(1 + 0.5 * step)
        x = _planted(n, rng, -1.5 * grow, 2.0 * grow, mirror=step == 1, band=(-0.4, 0.9))
        g = rng.standard_normal(n).astype(np.float32)
        xd, gd = _dev(x, off), _dev(g, off)
        out, dx = _sentinel((n + 8,)), _sentinel((n + 8,))
        _check(L.c3dgs_fake_quantize(n, xd.data_ptr(), state.data_ptr(), 1, 1, 0.01, out.data_ptr(), ws.data_ptr(), _stream()))
        _check(L.c3dgs_fake_quantize_backward(n, xd.data_ptr(), state.data_ptr(), 1, gd.data_ptr(), dx.data_ptr(), _stream()))
        torch.cuda.synchronize()
        qat.observe(st, x)
        _assert_state(state, 0, st, exact=True, what=f"n={n} step {step}")
        want, mask = qat.fake_quant(st, x)
        assert _bits_equal(out[:n].cpu().numpy(), want), (n, step)
        assert _bits_equal(dx[:n].cpu().numpy(), np.where(mask, g, F32(0))), (n, step)
        assert _untouched(out[n:]) and _untouched(dx[n:])
        if step > 0 and n >= 2:
            assert not mask.all(), "the lagging range should clamp the planted extremes"


# --------------------------------------------------------------------------------------------------- degenerate ranges
def _fq_roundtrip(L, x, st0=None, observe=True):
    """One module call on x (observer on or frozen at st0) -> (state row, out, dx) with g = 1 + index / 8."""
    n = x.size
    state, ws = _new_state(1), _ws(L)
    if st0 is not None:
        _put_state(state, 0, st0)
    g = (1 + np.arange(n) / 8).astype(np.float32)
    xd, gd = _dev(x), _dev(g)
    out, dx = _sentinel((n,)), _sentinel((n,))
    _check(L.c3dgs_fake_quantize(n, xd.data_ptr(), state.data_ptr(), int(observe), 1, 0.01, out.data_ptr(), ws.data_ptr(), _stream()))
    _check(L.c3dgs_fake_quantize_backward(n, xd.data_ptr(), state.data_ptr(), 1, gd.data_ptr(), dx.data_ptr(), _stream()))
    torch.cuda.synchronize()
    return state, out.cpu().numpy(), dx.cpu().numpy(), g


DEGENERATE = {
    "constant": lambda rng: np.full(1001, 0.37, np.float32),
    "constant_negative": lambda rng: np.full(1001, -2.5, np.float32),
    "all_positive": lambda rng: rng.uniform(3.0, 5.0, 1001).astype(np.float32),
    "all_negative": lambda rng: rng.uniform(-5.0, -3.0, 1001).astype(np.float32),
    "all_zero": lambda rng: np.zeros(1001, np.float32),
    "tiny": lambda rng: rng.uniform(-1e-9, 1e-9, 1001).astype(np.float32),          # range / 255 below FLT_EPSILON
}


@pytest.mark.parametrize("name", list(DEGENERATE))
def test_degenerate_ranges_observer_on_then_frozen(L, name):
    rng = np.random.default_rng(3)
    x = DEGENERATE[name](rng)
    st = qat.FqState()
    qat.observe(st, x)
    state, out, dx, g = _fq_roundtrip(L, x)
    _assert_state(state, 0, st, exact=True, what=name)
    want, mask = qat.fake_quant(st, x)
    assert np.isfinite(out).all() and _bits_equal(out, want) and _bits_equal(dx, np.where(mask, g, F32(0))), name
    if name in ("all_zero", "tiny"):
        assert st.scale == qat.EPS and _get_state(state, 0)[2] == np.finfo(np.float32).eps
    if name == "all_zero":
        assert st.zero_point == -128 and not out.any() and mask.all()
    if name in ("all_positive", "constant"):
        assert st.zero_point == -128 and st.scale == F32(st.max_val / F32(255))              # range widened down to 0
    if name in ("all_negative", "constant_negative"):
        assert st.zero_point == 127 and st.scale == F32(F32(0 - st.min_val) / F32(255))      # ... and up to 0
    # frozen: another tensor through the same state, observer off: state untouched, same arithmetic
    y = (x * F32(1.7) + F32(0.01)).astype(np.float32)
    state2, out2, dx2, g2 = _fq_roundtrip(L, y, st0=st, observe=False)
    _assert_state(state2, 0, st, exact=True, what=name + " frozen")
    want2, mask2 = qat.fake_quant(st, y)
    assert _bits_equal(out2, want2) and _bits_equal(dx2, np.where(mask2, g2, F32(0))), name


@pytest.mark.parametrize("scale_exp,zp", [(-7, 0), (-3, -128), (0, 13), (-10, 127)])
def test_exact_rounding_ties_round_half_to_even(L, scale_exp, zp):
    """scale = 2^e: x * (1 / scale) is exact, so x = (k + 1/2) * scale sits exactly on a tie. nearbyint rounds to even;
    bit-exact, no flip allowance."""
    st = qat.FqState()
    st.scale, st.zero_point = F32(2.0 ** scale_exp), zp
    st.min_val, st.max_val = F32((-128 - zp) * st.scale), F32((127 - zp) * st.scale)
    k = np.arange(-140, 140)
    x = ((k + 0.5) * float(st.scale)).astype(np.float32)
    assert np.array_equal(x.astype(np.float64) / float(st.scale), k + 0.5)
    state, out, dx, g = _fq_roundtrip(L, x, st0=st, observe=False)
    want, mask = qat.fake_quant(st, x)
    even = np.where(k % 2 == 0, k, k + 1)                                                   # round half to even, by hand
    by_hand = ((np.clip(even + zp, -128, 127) - zp) * float(st.scale)).astype(np.float32)
    assert _bits_equal(want, by_hand)
    assert _bits_equal(out, want) and _bits_equal(dx, np.where(mask, g, F32(0)))
    assert (~mask).any() and mask.any()


def test_values_far_outside_a_frozen_range_are_clamped_with_zero_gradient(L):
    rng = np.random.default_rng(5)
    st = qat.FqState()
    qat.observe(st, np.array([-1.0, 2.0], np.float32))
    x = np.concatenate([rng.uniform(-1, 2, 500), rng.uniform(20, 30, 250), rng.uniform(-30, -10, 250), [3e38, -3e38]]).astype(np.float32)
    state, out, dx, g = _fq_roundtrip(L, x, st0=st, observe=False)
    with np.errstate(all="ignore"):
        want, mask = qat.fake_quant(st, x)
    assert _bits_equal(out, want) and _bits_equal(dx, np.where(mask, g, F32(0)))
    hi, lo = F32((127 - st.zero_point) * st.scale), F32((-128 - st.zero_point) * st.scale)
    assert (out[500:750] == hi).all() and (out[750:1000] == lo).all() and out[1000] == hi and out[1001] == lo
    assert not dx[500:].any() and mask[:500].all()


# ------------------------------------------------------------------------------------------------------ codebooks
def _raw_codebooks(rng, GS, SHS, M):
    scaling = rng.standard_normal((GS, 3)).astype(np.float32)
    rotation = rng.standard_normal((GS, 4)).astype(np.float32)
    fdc = (rng.standard_normal((SHS, 1, 3)) * 1.5).astype(np.float32)
    frest = (rng.standard_normal((SHS, M - 1, 3)) * 0.3).astype(np.float32) if M > 1 else None
    return scaling, rotation, fdc, frest


def _oracle_codebooks(scaling, rotation, fdc, frest, present, narrow=0.5):
    """Getters with an observer step on `narrow` x the tensors (so that the second, frozen pass clamps some values)."""
    g = qat.Getters(True)
    for i, k in enumerate(qat.SLOTS):
        g.observer[k] = (i in present)
    z1, z3, z4 = np.zeros((1, 1), F32), np.zeros((1, 3), F32), np.zeros((1, 4), F32)
    args = lambda s: (z3, z1, z1, scaling * s if scaling is not None else z3, rotation * s if rotation is not None else z4,
                      fdc * s if fdc is not None else np.zeros((1, 1, 3), F32),
                      (frest * s if frest is not None else None))
    g.forward(*args(F32(narrow)))
    for k in qat.SLOTS:
        g.observer[k] = False
    return g, g.forward(*args(F32(1.0)))


def _run_codebooks(L, state, GS, SHS, M, scaling, rotation, fdc, frest, jobs, ups):
    """Forward + backward of the jobs in `jobs` (subset of 'scaling', 'rotation', 'features'); the other jobs' INPUT pointers
    are NULL while their sentinel-filled outputs are still passed. -> dict of GPU tensors."""
    t = dict(scaling=_dev(scaling) if "scaling" in jobs else None, rotation=_dev(rotation) if "rotation" in jobs else None,
             fdc=_dev(fdc) if "features" in jobs else None,
             frest=_dev(frest) if ("features" in jobs and frest is not None) else None)
    q = _params(state, GS=GS, SHS=SHS, M=M, observer=(0,) * 6, **t)
    o = dict(scales_n=_sentinel((GS, 3)), rotations=_sentinel((GS, 4)), shs=_sentinel((SHS, M, 3)),
             d_scaling=_sentinel((GS, 3)), d_rotation=_sentinel((GS, 4)), d_dc=_sentinel((SHS, 1, 3)),
             d_rest=_sentinel((SHS, max(M - 1, 1), 3)))
    _check(L.c3dgs_qat_codebooks(C.byref(q), o["scales_n"].data_ptr(), o["rotations"].data_ptr(), o["shs"].data_ptr(), _stream()))
    gs, gr, gh = _dev(ups["scales_n"]), _dev(ups["rotations"]), _dev(ups["shs"])
    _check(L.c3dgs_qat_codebooks_backward(C.byref(q), gs.data_ptr(), gr.data_ptr(), gh.data_ptr(), o["d_scaling"].data_ptr(),
                                          o["d_rotation"].data_ptr(), o["d_dc"].data_ptr(),
                                          o["d_rest"].data_ptr() if M > 1 else None, _stream()))
    torch.cuda.synchronize()
    return o


def _check_codebooks(o, ora, g, ups, scaling, jobs, M, what):
    c = lambda t: t.cpu().numpy()
    r = qat.Getters.backward(ora, scaling, g_scales_n=ups["scales_n"], g_rot=ups["rotations"], g_shs=ups["shs"])
    if "scaling" in jobs:
        assert _no_sentinel_left(o["scales_n"]) and _no_sentinel_left(o["d_scaling"]), what
        _flip_close(c(o["scales_n"]), ora["scales_n"], g.st["scaling"].scale, what + " scales_n")
        got, want = c(o["d_scaling"]), r["scaling"]
        bad = np.abs(got - want) > 2e-5 * max(1.0, np.abs(want).max())
        assert bad.mean() <= 2e-3, (what, "d_scaling", bad.mean())
        assert np.abs(want).max() > 0
    else:
        assert _untouched(o["scales_n"]) and _untouched(o["d_scaling"]), what + ": absent scaling job wrote its output"
    if "rotation" in jobs:
        assert _no_sentinel_left(o["rotations"]) and _no_sentinel_left(o["d_rotation"]), what
        np.testing.assert_allclose(c(o["rotations"]), ora["rotations"], rtol=0, atol=3e-7, err_msg=what)
        got, want = c(o["d_rotation"]), r["rotation"]
        assert (np.abs(got - want) <= 2e-5 * max(1.0, np.abs(want).max())).all(), (what, "d_rotation", np.abs(got - want).max())
        assert not got[~ora["m_rot"]].any(), what + ": masked rotation gradient must be exactly 0"
    else:
        assert _untouched(o["rotations"]) and _untouched(o["d_rotation"]), what + ": absent rotation job wrote its output"
    if "features" in jobs:
        assert _bits_equal(c(o["shs"]), ora["shs"]), what + " shs"
        # identity modules: the gradient is the upstream one where the mask passes and +0 elsewhere, bit for bit
        assert _bits_equal(c(o["d_dc"]), np.where(ora["m_dc"], ups["shs"][:, :1], F32(0))), what + " d_dc"
        if M > 1:
            assert _bits_equal(c(o["d_rest"]), np.where(ora["m_rest"], ups["shs"][:, 1:], F32(0))), what + " d_rest"
            if ora["m_rest"].size >= 1000:
                assert (~ora["m_rest"]).any() and ora["m_rest"].any(), "the frozen range should clamp some values"
        else:
            assert _untouched(o["d_rest"])
    else:
        assert _untouched(o["shs"]) and _untouched(o["d_dc"]) and _untouched(o["d_rest"]), what + ": absent features job wrote"


def _codebook_case(L, GS, SHS, M, jobs, seed):
    rng = np.random.default_rng(seed)
    scaling, rotation, fdc, frest = _raw_codebooks(rng, GS, SHS, M)
    present = ({SC} if "scaling" in jobs else set()) | ({ROT} if "rotation" in jobs else set()) | \
              ({DC, REST} if "features" in jobs else set())
    g, ora = _oracle_codebooks(scaling, rotation, fdc, frest, present)
    state = _new_state()
    for i, k in enumerate(qat.SLOTS):
        _put_state(state, i, g.st[k])
    ups = dict(scales_n=rng.standard_normal((GS, 3)).astype(np.float32), rotations=rng.standard_normal((GS, 4)).astype(np.float32),
               shs=rng.standard_normal((SHS, M, 3)).astype(np.float32))
    o = _run_codebooks(L, state, GS, SHS, M, scaling, rotation, fdc, frest, jobs, ups)
    _check_codebooks(o, ora, g, ups, scaling, jobs, M, f"GS={GS} SHS={SHS} M={M} jobs={sorted(jobs)}")


ALL_JOBS = ("scaling", "rotation", "features")


@pytest.mark.parametrize("SHS", [1, 2, 5, 1025, 800_000])
@pytest.mark.parametrize("M", [1, 4, 9, 16])
def test_codebooks_every_sh_degree_forward_and_backward(L, M, SHS):
    """M = 16 and 4 take the float4 concat, M = 9 and 1 the scalar one (M = 1: features_rest == NULL, rrow == 0). SHS = 800,000
    puts the SH job past its 8192-block cap at M = 9 (scalar path, 21.6M floats > 2^23) and at M = 16 (float4 path, 38.4M
    floats > 2^25); at M = 1 and M = 4 it is many blocks but below the cap."""
    _codebook_case(L, GS=min(SHS + 3, 4099), SHS=SHS, M=M, jobs=set(ALL_JOBS), seed=M * 1000 + SHS % 997)


@pytest.mark.parametrize("jobs", [c for r in (1, 2, 3) for c in itertools.combinations(ALL_JOBS, r)], ids="+".join)
@pytest.mark.parametrize("M", [1, 4, 9, 16])
def test_codebooks_every_combination_of_empty_jobs(L, M, jobs):
    """Each job alone and every pair: an empty job's first_block is pushed past the grid; its sentinel-filled output must stay
    untouched while the present ones are written completely."""
    _codebook_case(L, GS=1027, SHS=1025, M=M, jobs=set(jobs), seed=M + len(jobs))


def test_codebooks_geometry_alone_past_the_block_cap(L):
    """scaling + rotation with 2^22 + 3 rows (8192 blocks x 256 threads x 2 rows = 2^22), no SH tensor."""
    _codebook_case(L, GS=(1 << 22) + 3, SHS=0, M=1, jobs={"scaling", "rotation"}, seed=22)


def test_codebooks_non_indexed_geometry_three_million_rows(L):
    """GS = SHS = 3,000,001, M = 16: the SH concat on its float4 path past the block cap (144M floats), forward and backward;
    the float64-free features comparison runs in row chunks so that the host never holds more than one chunk of references."""
    n, M = 3_000_001, 16
    rng = np.random.default_rng(16)
    g = qat.Getters(True)
    state = _new_state()
    fdc = (rng.standard_normal((n, 1, 3), dtype=np.float32) * F32(1.5))
    frest = (rng.standard_normal((n, M - 1, 3), dtype=np.float32) * F32(0.3))
    fdc[-1, 0, 2], frest[-1, -1, 2], frest[0, 0, 0] = 9.0, -4.0, 3.5                        # extremes in the last / first floats
    qat.observe(g.st["features_dc"], fdc * F32(0.5))
    qat.observe(g.st["features_rest"], frest * F32(0.5))
    scaling = rng.standard_normal((n, 3), dtype=np.float32)
    rotation = rng.standard_normal((n, 4), dtype=np.float32)
    v, _, _ = qat.normalize_rows(np.maximum(scaling, F32(0)))
    qat.observe(g.st["scaling"], v * F32(0.9))
    qat.observe(g.st["rotation"], rotation * F32(0.5))
    for i, k in enumerate(qat.SLOTS):
        _put_state(state, i, g.st[k])
    t = dict(scaling=_dev(scaling), rotation=_dev(rotation), fdc=_dev(fdc), frest=_dev(frest))
    q = _params(state, GS=n, SHS=n, M=M, observer=(0,) * 6, **t)
    scales_n, rotations, shs = _sentinel((n, 3)), _sentinel((n, 4)), _sentinel((n, M, 3))
    _check(L.c3dgs_qat_codebooks(C.byref(q), scales_n.data_ptr(), rotations.data_ptr(), shs.data_ptr(), _stream()))
    gen = torch.Generator(device=DEV).manual_seed(1)
    g_s, g_r = torch.randn(n, 3, device=DEV, generator=gen), torch.randn(n, 4, device=DEV, generator=gen)
    g_h = torch.randn(n, M, 3, device=DEV, generator=gen)
    d_s, d_r, d_dc, d_rest = _sentinel((n, 3)), _sentinel((n, 4)), _sentinel((n, 1, 3)), _sentinel((n, M - 1, 3))
    _check(L.c3dgs_qat_codebooks_backward(C.byref(q), g_s.data_ptr(), g_r.data_ptr(), g_h.data_ptr(), d_s.data_ptr(), d_r.data_ptr(),
                                          d_dc.data_ptr(), d_rest.data_ptr(), _stream()))
    torch.cuda.synchronize()
    for t_ in (scales_n, rotations, d_s, d_r):
        assert _no_sentinel_left(t_)
    chunk = 250_000
    for lo in range(0, n, chunk):
        sl = slice(lo, min(n, lo + chunk))
        dc_q, m_dc = qat.fake_quant(g.st["features_dc"], fdc[sl])
        rest_q, m_rest = qat.fake_quant(g.st["features_rest"], frest[sl])
        assert _bits_equal(shs[sl].cpu().numpy(), np.concatenate([dc_q, rest_q], 1)), lo
        gh = g_h[sl].cpu().numpy()
        assert _bits_equal(d_dc[sl].cpu().numpy(), np.where(m_dc, gh[:, :1], F32(0))), lo
        assert _bits_equal(d_rest[sl].cpu().numpy(), np.where(m_rest, gh[:, 1:], F32(0))), lo
    # geometry rows in full, chunked as well (observers off: Getters.forward is then pure)
    for k in qat.SLOTS:
        g.observer[k] = False
    for lo in range(0, n, 1_000_000):
        sl = slice(lo, min(n, lo + 1_000_000))
        o = g.forward(np.zeros((1, 3), F32), np.zeros((1, 1), F32), np.zeros((1, 1), F32), scaling[sl], rotation[sl], fdc[:1], frest[:1])
        _flip_close(scales_n[sl].cpu().numpy(), o["scales_n"], g.st["scaling"].scale, "3M scales_n")
        np.testing.assert_allclose(rotations[sl].cpu().numpy(), o["rotations"], rtol=0, atol=3e-7)
        r = qat.Getters.backward(o, scaling[sl], g_scales_n=g_s[sl].cpu().numpy(), g_rot=g_r[sl].cpu().numpy())
        got, want = d_r[sl].cpu().numpy(), r["rotation"]
        assert (np.abs(got - want) <= 2e-5 * max(1.0, np.abs(want).max())).all()
        got, want = d_s[sl].cpu().numpy(), r["scaling"]
        assert (np.abs(got - want) > 2e-5 * max(1.0, np.abs(want).max())).mean() <= 2e-3


def test_non_positive_scaling_rows_and_zero_quaternions(L):
    """_scaling rows with one, two and three non-positive components (the all-non-positive row: normalize of the zero vector,
    output fq(0), gradient exactly 0) and rotation rows that fake-quantise to (0, 0, 0, 0) (output 0; the norm is below eps, so
    the gradient is g / 1e-12 through the mask, as torch's clamp_min backward gives it)."""
    rng = np.random.default_rng(8)
    GS = 1024
    scaling = rng.uniform(0.1, 2.0, (GS, 3)).astype(np.float32)
    scaling[0::8, 0] = -1.0                                          # one non-positive component
    scaling[1::8, :2] = (-0.5, 0.0)                                  # two
    scaling[2::8] = (-1.0, 0.0, -3.0)                                # three: relu -> zero vector
    scaling[-1] = 0.0
    rotation = rng.standard_normal((GS, 4)).astype(np.float32)
    rotation[3::8] = rng.uniform(-1e-4, 1e-4, rotation[3::8].shape)  # far below half a quantisation step of a +-3 range
    rotation[-2] = 0.0
    g = qat.Getters(True)
    qat.observe(g.st["scaling"], qat.normalize_rows(np.maximum(scaling, F32(0)))[0])
    qat.observe(g.st["rotation"], rotation)
    for k in qat.SLOTS:
        g.observer[k] = False
    ora = g.forward(np.zeros((1, 3), F32), np.zeros((1, 1), F32), np.zeros((1, 1), F32), scaling, rotation, np.zeros((1, 1, 3), F32), None)
    t = dict(scaling=_dev(scaling), rotation=_dev(rotation))
    # observer on: c3dgs_qat_observe on these very rows (relu, the 1e-12 clamp, 0 / 1e-12, minimum exactly 0)
    state = _new_state()
    _check(L.c3dgs_qat_observe(C.byref(_params(state, GS=GS, M=1, **t)), _ws(L).data_ptr(), _stream()))
    torch.cuda.synchronize()
    _assert_state(state, SC, g.st["scaling"], exact=False, what="observer on non-positive rows")
    _assert_state(state, ROT, g.st["rotation"], exact=True, what="observer on zero quaternions")
    assert _get_state(state, SC)[0] == 0.0, "normalize(relu) of a row with a non-positive component has minimum exactly 0"
    # ... and then frozen, from the oracle's state so that the comparison below has no 1-ulp scale difference in it
    for i, k in enumerate(qat.SLOTS):
        _put_state(state, i, g.st[k])
    ups = dict(scales_n=rng.standard_normal((GS, 3)).astype(np.float32), rotations=rng.standard_normal((GS, 4)).astype(np.float32),
               shs=np.zeros((0, 1, 3), np.float32))
    q = _params(state, GS=GS, M=1, observer=(0,) * 6, **t)
    scales_n, rotations, d_s, d_r = (_sentinel((GS, 3)), _sentinel((GS, 4)), _sentinel((GS, 3)), _sentinel((GS, 4)))
    _check(L.c3dgs_qat_codebooks(C.byref(q), scales_n.data_ptr(), rotations.data_ptr(), None, _stream()))
    gs, gr = _dev(ups["scales_n"]), _dev(ups["rotations"])
    _check(L.c3dgs_qat_codebooks_backward(C.byref(q), gs.data_ptr(), gr.data_ptr(), None, d_s.data_ptr(), d_r.data_ptr(), None, None, _stream()))
    torch.cuda.synchronize()
    scales_n, rotations, d_s, d_r = (x.cpu().numpy() for x in (scales_n, rotations, d_s, d_r))
    assert np.isfinite(scales_n).all() and np.isfinite(rotations).all() and np.isfinite(d_s).all() and np.isfinite(d_r).all()
    r = qat.Getters.backward(ora, scaling, g_scales_n=ups["scales_n"], g_rot=ups["rotations"])
    _flip_close(scales_n, ora["scales_n"], g.st["scaling"].scale, "scales_n")
    zero_rows = (scaling <= 0).all(1)
    assert zero_rows.sum() >= GS // 8
    fq0 = qat.fake_quant(g.st["scaling"], np.zeros(1, F32))[0][0]
    assert (scales_n[zero_rows] == fq0).all() and not d_s[zero_rows].any(), "normalize(relu) of a zero vector: output fq(0), gradient 0"
    assert not d_s[scaling <= 0].any(), "relu passes no gradient at x <= 0"
    assert (np.abs(d_s - r["scaling"]) > 2e-5 * max(1.0, np.abs(r["scaling"]).max())).mean() <= 2e-3
    zq = (ora["w"] == 0).all(1)
    assert zq.sum() >= GS // 8 and zq[-2]
    assert not rotations[zq].any(), "a quaternion that quantises to zero normalises to zero"
    np.testing.assert_allclose(rotations, ora["rotations"], rtol=0, atol=3e-7)
    np.testing.assert_allclose(d_r[zq], r["rotation"][zq], rtol=1e-6)                          # g / 1e-12 where the mask passes
    assert (np.abs(d_r[~zq] - r["rotation"][~zq]) <= 2e-5 * max(1.0, np.abs(r["rotation"][~zq]).max())).all()


@pytest.mark.parametrize("off", [0, 1], ids=["aligned", "misaligned"])
@pytest.mark.parametrize("rows", [1, 3, 257, (1 << 19) + 1])
def test_scaling_tensor_with_no_positive_component_observer_on_then_frozen(L, rows, off):
    """Every row of _scaling is <= 0: normalize(relu(.)) is the zero tensor, the observed range is [0, 0], the scale is
    FLT_EPSILON and the zero point -128; three observer steps, then the frozen forward (fq(0) = 0) and backward (exactly 0)."""
    rng = np.random.default_rng(rows)
    state, st = _new_state(), qat.FqState()
    for step in range(3):
        x = -rng.uniform(0.0, 2.0, (rows, 3)).astype(np.float32)
        x[::3, step % 3] = 0.0
        x[-1] = 0.0
        t = _dev(x, off)
        _check(L.c3dgs_qat_observe(C.byref(_params(state, GS=rows, scaling=t)), _ws(L).data_ptr(), _stream()))
        torch.cuda.synchronize()
        qat.observe(st, qat.normalize_rows(np.maximum(x, F32(0)))[0])
        _assert_state(state, SC, st, exact=True, what=f"all <= 0, step {step}")
        assert (st.min_val, st.max_val, st.scale, st.zero_point) == (0.0, 0.0, qat.EPS, -128)
    q = _params(state, GS=rows, scaling=t, observer=(0,) * 6)
    scales_n, d_s = _sentinel((rows, 3)), _sentinel((rows, 3))
    gs = _dev(rng.standard_normal((rows, 3)).astype(np.float32))
    _check(L.c3dgs_qat_codebooks(C.byref(q), scales_n.data_ptr(), None, None, _stream()))
    _check(L.c3dgs_qat_codebooks_backward(C.byref(q), gs.data_ptr(), None, None, d_s.data_ptr(), None, None, None, _stream()))
    torch.cuda.synchronize()
    assert not scales_n.view(torch.int32).any().item() and not d_s.view(torch.int32).any().item(), "output and gradient must be +0"
    _assert_state(state, SC, st, exact=True, what="frozen")


@pytest.mark.parametrize("off", [0, 1], ids=["aligned", "misaligned"])
@pytest.mark.parametrize("rows", [5, 1025, (1 << 19) + 1])
def test_observer_scaling_rows_with_non_positive_components(L, rows, off):
    """The ACT_NORMRELU3 branch of the observer on rows with one, two and three non-positive components, the decisive rows
    (the only one with a zero component -> minimum 0; the only one-hot row -> maximum 1) at the end / at the start."""
    rng = np.random.default_rng(rows + off)
    state, st = _new_state(), qat.FqState()
    for step in range(3):
        x = rng.uniform(0.5, 0.65, (rows, 3)).astype(np.float32)
        i_lo, i_hi, i_zero = (0, 1, 2) if step == 1 else (rows - 1, rows - 2, rows - 3)
        x[i_zero] = (-1.0, 0.0, -2.0)                               # three: the zero vector, 0 / 1e-12 = 0
        x[i_hi] = (0.0, 3.0 + step, -0.5)                           # two: one-hot after relu -> 1.0
        x[i_lo] = (0.7, -0.1 * (1 + step), 0.7)                     # one
        t = _dev(x, off)
        _check(L.c3dgs_qat_observe(C.byref(_params(state, GS=rows, scaling=t)), _ws(L).data_ptr(), _stream()))
        torch.cuda.synchronize()
        qat.observe(st, qat.normalize_rows(np.maximum(x, F32(0)))[0])
        _assert_state(state, SC, st, exact=False, what=f"rows={rows} step {step}")
    assert st.min_val == 0.0 and st.max_val == 1.0 and _get_state(state, SC)[:2] == (0.0, 1.0)


# ---------------------------------------------------------------------------------------------- visibility and points
VIEW = np.eye(4, dtype=np.float32).reshape(-1)                     # view-space z = z: visible iff z > 0.01


def _visibility_case(P, pattern, rng):
    xyz = rng.uniform(-3, 3, (P, 3)).astype(np.float32)
    xyz[:, 2] = {"none": -1.0, "all": 2.0, "first": -1.0, "last": -1.0, "mixed": 0.0}[pattern]
    if pattern == "first":
        xyz[0, 2] = 2.0
    elif pattern == "last":
        xyz[-1, 2] = 2.0
    elif pattern == "mixed":
        xyz[:, 2] = rng.uniform(-1, 1, P)
    xyz[P // 2, 0] = 1e5                                            # beyond fp16 range: inf after x.half().float()
    xyz[0, 1] = -7e4
    return xyz


@pytest.mark.parametrize("half", [1, 0], ids=["half_xyz", "full_xyz"])
@pytest.mark.parametrize("pattern", ["none", "all", "last", "first", "mixed"])
@pytest.mark.parametrize("P", [1, 255, 256, 257, 3_000_001])
def test_visibility_and_point_gathers(L, P, pattern, half):
    rng = np.random.default_rng(P + len(pattern))
    xyz = _visibility_case(P, pattern, rng)
    opacity = rng.standard_normal((P, 1)).astype(np.float32) * 2
    sfac = rng.standard_normal((P, 1)).astype(np.float32)
    sh_idx, g_idx = rng.integers(0, 1 << 40, P), rng.integers(0, 1 << 40, P)
    g = qat.Getters(True)
    qat.observe(g.st["opacity"], qat.sigmoid(opacity * F32(0.5)))
    qat.observe(g.st["scaling_factor"], sfac * F32(0.5))
    state = _new_state()
    for i, k in enumerate(qat.SLOTS):
        _put_state(state, i, g.st[k])
    t = dict(xyz=_dev(xyz), opacity=_dev(opacity), scaling_factor=_dev(sfac))
    q = _params(state, P=P, observer=(0,) * 6, half_xyz=half, **t)
    visible, rank = _sentinel((P,), torch.uint8), torch.full((P,), -7, dtype=torch.int32, device=DEV)
    count = torch.full((1,), -7, dtype=torch.int32, device=DEV)
    scan = torch.empty(max(int(L.c3dgs_qat_scan_bytes(P)), 256), dtype=torch.uint8, device=DEV)
    view = _dev(VIEW)
    _check(L.c3dgs_qat_visible(C.byref(q), view.data_ptr(), visible.data_ptr(), rank.data_ptr(), count.data_ptr(), scan.data_ptr(), _stream()))
    torch.cuda.synchronize()
    with np.errstate(over="ignore"):
        xq = qat.half_round(xyz) if half else xyz
    if half:
        assert np.isinf(xq[P // 2, 0]) and np.isinf(xq[0, 1])
    with np.errstate(invalid="ignore"):
        vis = qat.visible_rows(xq, VIEW)
    want_rank = np.concatenate([[0], np.cumsum(vis)[:-1]]).astype(np.int32)
    V = int(vis.sum())
    assert np.array_equal(visible.cpu().numpy(), vis.astype(np.uint8)) and np.array_equal(rank.cpu().numpy(), want_rank)
    assert int(count.item()) == V
    if pattern in ("none", "all", "first", "last") and not (half and pattern in ("none", "first", "last")):
        assert V == {"none": 0, "all": P, "first": 1, "last": 1}[pattern]
    sig = qat.sigmoid(opacity)
    op_q, m_op = qat.fake_quant(g.st["opacity"], sig)
    sf_q, m_sf = qat.fake_quant(g.st["scaling_factor"], sfac)
    want = dict(means3D=xq, opac=op_q, sfac=np.exp(sf_q, dtype=np.float32), sh=sh_idx, gi=g_idx)
    up = dict(m3=rng.standard_normal((P, 3)).astype(np.float32), m2=rng.standard_normal((P, 3)).astype(np.float32),
              op=rng.standard_normal((P, 1)).astype(np.float32), sf=rng.standard_normal((P, 1)).astype(np.float32))
    for gathered in (True, False):
        rows = vis if gathered else np.ones(P, bool)
        n_out = V if gathered else P
        pad = 3                                                     # guard rows behind the V gathered ones
        o = dict(means3D=_sentinel((n_out + pad, 3)), opac=_sentinel((n_out + pad, 1)), sfac=_sentinel((n_out + pad, 1)),
                 sh=torch.full((n_out + pad,), -5, dtype=torch.int64, device=DEV), gi=torch.full((n_out + pad,), -5, dtype=torch.int64, device=DEV))
        vp, rp = (visible.data_ptr(), rank.data_ptr()) if gathered else (None, None)
        shd, gid = _dev(sh_idx), _dev(g_idx)
        _check(L.c3dgs_qat_points(C.byref(q), vp, rp, shd.data_ptr(), gid.data_ptr(), o["means3D"].data_ptr(), o["opac"].data_ptr(),
                                  o["sfac"].data_ptr(), o["sh"].data_ptr(), o["gi"].data_ptr(), _stream()))
        gup = {k: _dev(v[rows]) if n_out else torch.zeros((1,) + v.shape[1:], device=DEV) for k, v in up.items()}
        d = dict(xyz=_sentinel((P, 3)), screen=_sentinel((P, 3)), op=_sentinel((P, 1)), sf=_sentinel((P, 1)))
        _check(L.c3dgs_qat_points_backward(C.byref(q), vp, rp, gup["m3"].data_ptr(), gup["m2"].data_ptr(), gup["op"].data_ptr(),
                                           gup["sf"].data_ptr(), d["xyz"].data_ptr(), d["screen"].data_ptr(), d["op"].data_ptr(),
                                           d["sf"].data_ptr(), _stream()))
        torch.cuda.synchronize()
        what = f"P={P} {pattern} gathered={gathered}"
        c = lambda x: x.cpu().numpy()
        assert _bits_equal(c(o["means3D"][:n_out]), want["means3D"][rows]), what
        assert np.array_equal(c(o["sh"][:n_out]), sh_idx[rows]) and np.array_equal(c(o["gi"][:n_out]), g_idx[rows]), what
        for k in ("means3D", "opac", "sfac"):
            assert _untouched(o[k][n_out:]), what + ": wrote behind the gathered rows"
        assert (o["sh"][n_out:] == -5).all() and (o["gi"][n_out:] == -5).all()
        if n_out:
            _flip_close(c(o["opac"][:n_out]), want["opac"][rows], g.st["opacity"].scale, what + " opacity")
            np.testing.assert_allclose(c(o["sfac"][:n_out]), want["sfac"][rows], rtol=3e-6, err_msg=what)
        # backward: P-sized, fully written, zeros for invisible rows
        for k in d:
            assert _no_sentinel_left(d[k]), what + f": d_{k} not fully written"
        sel = lambda a: np.where(rows[:, None], a, F32(0))
        assert _bits_equal(c(d["xyz"]), sel(up["m3"])) and _bits_equal(c(d["screen"]), sel(up["m2"])), what
        want_op = sel((up["op"] * m_op * (1.0 - sig.astype(np.float64)) * sig).astype(np.float32))
        bad = np.abs(c(d["op"]) - want_op) > 2e-5 * max(1.0, np.abs(want_op).max())
        assert bad.mean() <= 2e-3, (what, bad.mean())
        want_sf = sel((up["sf"] * m_sf * want["sfac"].astype(np.float64)).astype(np.float32))
        np.testing.assert_allclose(c(d["sf"]), want_sf, rtol=3e-6, atol=0, err_msg=what)
        assert not c(d["op"])[~rows].any() and not c(d["sf"])[~rows].any()


# ------------------------------------------------------------------------------------------------------- int8 payload
@pytest.mark.parametrize("scaling_is_exp", [0, 1])
@pytest.mark.parametrize("M", [1, 9, 16])
def test_quantize_codes_above_the_block_cap_and_on_exact_ties(L, M, scaling_is_exp):
    """c3dgs_qat_quantize rounds nearbyint(double(x) / double(scale)): x = (k + 1/2) * scale with a power-of-two scale is an
    exact tie of that division. P = 2^22 + 5 units is past the 4096-block cap. Codes equal the oracle's exactly: everywhere for
    the identity tensors, for rotation and for normalize(relu(scaling)) (+ - * / sqrt in the oracle's order, all correctly
    rounded); behind sigmoid / exp (1 - 2 ulp between expf and numpy) everywhere except where the oracle's quotient x / scale
    lies within 2 ulp of x of a rounding boundary -- there, and only there, one code of difference is allowed. The last four
    units of every job (the tail past the block cap) are asserted to be away from a boundary, so they are always exact."""
    rng = np.random.default_rng(M + scaling_is_exp)
    P, GS, SHS = (1 << 22) + 5, 70_001, 1_400_003 // M
    g = qat.Getters(True)
    opacity = (rng.standard_normal((P, 1)) * 2).astype(np.float32)
    scaling = rng.standard_normal((GS, 3)).astype(np.float32) * F32(0.7)
    rotation = rng.standard_normal((GS, 4)).astype(np.float32)
    rotation[::5] = 0.0                                             # zero quaternion: normalises to 0, code = zero point
    # identity tensors on exact ties: scale 2^-5, zero_point 3 / -20 / 7
    def ties(n, lo=-140, hi=140):
        k = rng.integers(lo, hi, n)
        half = rng.integers(0, 2, n) * 0.5
        return ((k + half) * 2.0 ** -5).astype(np.float32)
    sfac, fdc = ties(P).reshape(P, 1), ties(SHS * 3).reshape(SHS, 1, 3)
    frest = ties(SHS * 3 * (M - 1)).reshape(SHS, M - 1, 3) if M > 1 else None
    sfac[-1], fdc[-1, 0, 2] = 2.0 ** -6, -(2.0 ** -6)               # +-half a step in the last element: ties to even 0
    for k, zp in (("scaling_factor", 3), ("features_dc", -20), ("features_rest", 7)):
        g.st[k].scale, g.st[k].zero_point = F32(2.0 ** -5), zp
    qat.observe(g.st["opacity"], qat.sigmoid(opacity))
    act_scaling = np.exp(scaling, dtype=np.float32) if scaling_is_exp else qat.normalize_rows(np.maximum(scaling, F32(0)))[0]
    qat.observe(g.st["scaling"], act_scaling)
    rot_n = qat.normalize_rows(rotation)[0]
    qat.observe(g.st["rotation"], rot_n)
    state = _new_state()
    for i, k in enumerate(qat.SLOTS):
        _put_state(state, i, g.st[k])
    t = dict(opacity=_dev(opacity), scaling_factor=_dev(sfac), scaling=_dev(scaling), rotation=_dev(rotation), fdc=_dev(fdc),
             frest=_dev(frest) if frest is not None else None)
    q = _params(state, P=P, GS=GS, SHS=SHS, M=M, observer=(0,) * 6, **t)
    pad = 16
    out = {k: torch.full((n + pad,), 0x5A, dtype=torch.int8, device=DEV) for k, n in
           dict(opacity=P, scaling=GS * 3, scaling_factor=P, rotation=GS * 4, features_dc=SHS * 3, features_rest=max(SHS * 3 * (M - 1), 1)).items()}
    _check(L.c3dgs_qat_quantize(C.byref(q), scaling_is_exp, out["opacity"].data_ptr(), out["scaling"].data_ptr(),
                                out["scaling_factor"].data_ptr(), out["rotation"].data_ptr(), out["features_dc"].data_ptr(),
                                out["features_rest"].data_ptr() if M > 1 else None, _stream()))
    torch.cuda.synchronize()
    acts = dict(opacity=qat.sigmoid(opacity), scaling=act_scaling, scaling_factor=sfac, rotation=rot_n, features_dc=fdc)
    if M > 1:
        acts["features_rest"] = frest
    transcendental = ("opacity",) + (("scaling",) if scaling_is_exp else ())
    for k, x in acts.items():
        x = x.reshape(-1)
        want = qat.quantize_codes(g.st[k], x, device_rounding=True)
        got = out[k][:x.size].cpu().numpy()
        diff = got.astype(np.int32) - want.astype(np.int32)
        print(f"quantize M={M} exp={scaling_is_exp} {k}: {int((diff != 0).sum())} of {x.size} codes differ")
        if k in transcendental:
            quot = x.astype(np.float64) / np.float64(g.st[k].scale)
            to_boundary = np.abs(quot - np.floor(quot) - 0.5)                    # distance of the quotient from the nearest k + 1/2
            borderline = to_boundary <= 2 * np.spacing(np.abs(x)).astype(np.float64) / np.float64(g.st[k].scale)
            assert borderline.mean() < 1e-4 and not borderline[-12:].any(), (k, borderline.mean())
            assert not diff[~borderline].any(), (k, int((diff[~borderline] != 0).sum()))
            assert np.abs(diff[borderline]).max(initial=0) <= 1, k
        else:
            assert np.array_equal(got, want), k
        assert (out[k][x.size:] == 0x5A).all(), k + ": wrote behind its output"
    if M == 1:
        assert (out["features_rest"] == 0x5A).all()
    z = g.st["rotation"].zero_point
    assert (out["rotation"][:GS * 4].view(GS, 4)[::5].cpu().numpy() == z).all()
    # the ties themselves: round half to even in the double division, e.g. +-1/64 / (1/32) = +-0.5 -> 0
    assert int(out["scaling_factor"][P - 1]) == 3 and int(out["features_dc"][SHS * 3 - 1]) == -20
