"""CPU: documented rejections of the training-step entry points (fused Adam, QAT getters, abs_accumulate, stand-alone
fake-quant). Validation runs before any device work, so this needs no GPU: the pointers are fakes that are never read."""
import ctypes as C

import pytest


@pytest.fixture(scope="module")
def L():
    from c3dgs_amd import build, _lib
    build.build()
    return _lib.lib()


# A 16-byte aligned address nobody dereferences. Every call below must be refused by the host-side validation, which runs before
# any device work: if an entry point ever validates later than it launches, these calls would hand this address to a kernel.
FAKE = 4096


def _q(**kw):
    from c3dgs_amd import _lib
    q = _lib.QatParams()
    q.P, q.GS, q.SHS, q.M = 8, 8, 8, 16
    q.state = FAKE
    for k, v in kw.items():
        setattr(q, k, v)
    return q


def _qat_entries(L):
    f = C.c_void_p(FAKE)
    return {
        "qat_observe": lambda q: L.c3dgs_qat_observe(C.byref(q), f, None),
        "qat_codebooks": lambda q: L.c3dgs_qat_codebooks(C.byref(q), f, f, f, None),
        "qat_codebooks_backward": lambda q: L.c3dgs_qat_codebooks_backward(C.byref(q), f, f, f, f, f, f, f, None),
        "qat_visible": lambda q: L.c3dgs_qat_visible(C.byref(q), f, f, f, f, f, None),
        "qat_points": lambda q: L.c3dgs_qat_points(C.byref(q), f, f, f, f, f, f, f, f, f, None),
        "qat_points_backward": lambda q: L.c3dgs_qat_points_backward(C.byref(q), f, f, f, f, f, f, f, f, f, f, None),
        "qat_quantize": lambda q: L.c3dgs_qat_quantize(C.byref(q), 0, f, f, f, f, f, f, None),
    }


@pytest.mark.parametrize("bad,message", [
    (dict(rotation=FAKE + 4), b"rotation must be 16-byte aligned"),
    (dict(rotation=FAKE + 8), b"rotation must be 16-byte aligned"),
    (dict(M=0), b"bad sizes"),
    (dict(M=-1), b"bad sizes"),
    (dict(P=-1), b"bad sizes"),
    (dict(GS=-1), b"bad sizes"),
    (dict(SHS=-1), b"bad sizes"),
    (dict(features_dc=FAKE, features_rest=None, M=2), b"features_rest is required"),
    (dict(features_dc=FAKE, features_rest=None, M=16), b"features_rest is required"),
    (dict(state=None), b"state is required"),
])
def test_every_qat_entry_rejects_bad_params(L, bad, message):
    for name, call in _qat_entries(L).items():
        assert call(_q(**bad)) == 1, name
        err = L.c3dgs_last_error()
        assert message in err and name.encode() in err, (name, err)


def test_qat_entries_reject_misaligned_outputs_and_missing_buffers(L):
    f, odd = C.c_void_p(FAKE), C.c_void_p(FAKE + 4)
    q = _q(rotation=FAKE, features_dc=FAKE, features_rest=FAKE)
    assert L.c3dgs_qat_codebooks(C.byref(q), f, odd, f, None) == 1 and b"16-byte aligned" in L.c3dgs_last_error()
    assert L.c3dgs_qat_codebooks(C.byref(q), f, f, odd, None) == 1 and b"16-byte aligned" in L.c3dgs_last_error()
    for args in ((f, odd, f, f, f, f, f), (f, f, odd, f, f, f, f), (f, f, f, f, odd, f, f)):
        assert L.c3dgs_qat_codebooks_backward(C.byref(q), *args, None) == 1 and b"16-byte aligned" in L.c3dgs_last_error()
    assert L.c3dgs_qat_codebooks_backward(C.byref(q), f, f, f, f, f, None, f, None) == 1
    assert b"dL_dfeatures_dc / dL_dfeatures_rest are required" in L.c3dgs_last_error()
    assert L.c3dgs_qat_codebooks_backward(C.byref(q), f, f, f, f, f, f, None, None) == 1
    assert L.c3dgs_qat_observe(C.byref(q), None, None) == 1 and b"workspace is required" in L.c3dgs_last_error()
    assert L.c3dgs_qat_visible(C.byref(q), f, f, f, None, f, None) == 1 and b"count is required" in L.c3dgs_last_error()
    assert L.c3dgs_qat_points(C.byref(q), f, None, f, f, f, f, f, f, f, None) == 1 and b"go together" in L.c3dgs_last_error()
    assert L.c3dgs_qat_points_backward(C.byref(q), None, f, f, f, f, f, f, f, f, f, None) == 1 and b"go together" in L.c3dgs_last_error()
    assert L.c3dgs_qat_quantize(C.byref(q), 0, f, f, f, C.c_void_p(FAKE + 2), f, f, None) == 1
    assert b"4-byte aligned" in L.c3dgs_last_error()
    assert L.c3dgs_qat_observe(None, f, None) == 1 and b"params is NULL" in L.c3dgs_last_error()


def test_adam_step_rejections(L):
    from c3dgs_amd import _lib
    rows = (_lib.AdamTensor * 17)()
    for r in rows:
        r.param = r.grad = r.exp_avg = r.exp_avg_sq = FAKE
        r.n = 4
    assert L.c3dgs_adam_step(17, rows, 0.9, 0.999, 1e-15, None) == 1
    assert b"between 0 and 16 tensors" in L.c3dgs_last_error()
    assert L.c3dgs_adam_step(-1, rows, 0.9, 0.999, 1e-15, None) == 1
    assert L.c3dgs_adam_step(0, None, 0.9, 0.999, 1e-15, None) == 0                  # nothing to do: legal, touches nothing
    assert L.c3dgs_adam_step(3, None, 0.9, 0.999, 1e-15, None) == 1 and b"tensors is NULL" in L.c3dgs_last_error()
    for field in ("param", "grad", "exp_avg", "exp_avg_sq"):
        one = (_lib.AdamTensor * 2)()
        for r in one:
            r.param = r.grad = r.exp_avg = r.exp_avg_sq = FAKE
            r.n = 4
        setattr(one[1], field, None)
        assert L.c3dgs_adam_step(2, one, 0.9, 0.999, 1e-15, None) == 1 and b"NULL tensor pointer" in L.c3dgs_last_error(), field


def test_abs_accumulate_and_fake_quantize_rejections(L):
    f = C.c_void_p(FAKE)
    assert L.c3dgs_abs_accumulate(-1, f, f, None) == 1 and b"abs_accumulate" in L.c3dgs_last_error()
    assert L.c3dgs_abs_accumulate(4, None, f, None) == 1 and L.c3dgs_abs_accumulate(4, f, None, None) == 1
    assert L.c3dgs_fake_quantize(-1, f, f, 1, 1, 0.01, f, f, None) == 1 and b"n must be >= 0" in L.c3dgs_last_error()
    assert L.c3dgs_fake_quantize(0, None, None, 1, 1, 0.01, None, None, None) == 0
    assert L.c3dgs_fake_quantize(4, f, f, 1, 1, 0.01, f, None, None) == 1                # observing needs the workspace
    assert L.c3dgs_fake_quantize(4, f, None, 0, 1, 0.01, f, None, None) == 1
    assert L.c3dgs_fake_quantize_backward(-1, f, f, 1, f, f, None) == 1
    assert L.c3dgs_fake_quantize_backward(4, f, f, 1, None, f, None) == 1
    assert L.c3dgs_fake_quantize_backward(0, None, None, 1, None, None, None) == 0
