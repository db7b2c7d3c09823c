"""CPU: the fused 16-bit softmax attention entry points (include/glfusion.h: glf_s16_attn_softmax_fwd / _bwd) are exported and
reject bad arguments with the documented codes and a message, before any HIP runtime call (no device is touched here)."""
import ctypes as C

import pytest

from glfusion_amd import _lib

GLF_ERR_BAD_SHAPE, GLF_ERR_UNSUPPORTED, GLF_ERR_NULL = -1, -2, -5


@pytest.fixture(scope="module")
def dll():
    d = C.CDLL(_lib.LIB_PATH)
    protos = _lib.parse_header()
    for name in ("glf_s16_attn_softmax_fwd", "glf_s16_attn_softmax_bwd", "glf_last_error"):
        assert name in protos, name
        assert hasattr(d, name), f"libglfusion_hip.so does not export {name}"
        restype, argtypes = protos[name]
        fn = getattr(d, name)
        fn.restype, fn.argtypes = restype, argtypes
    return d


def params(frames=2, L=100, ci=128, ld=None):
    p = _lib.AttnParams()
    p.frames, p.L, p.ci = frames, L, ci
    ld = 3 * ci if ld is None else ld
    p.ldq = p.ldk = p.ldv = p.ldd = ld
    p.ldy = p.lddy = ci
    return p


# fake, 16-byte-aligned addresses: validation must reject every case below before anything dereferences them
P = 1 << 20


def fwd(dll, p, theta=P, phi=P, g=P, y=P, lse=P):
    return dll.glf_s16_attn_softmax_fwd(theta, phi, g, y, lse, C.byref(p), None)


def bwd(dll, p, null_at=None):
    args = [P] * 10
    if null_at is not None:
        args[null_at] = None
    return dll.glf_s16_attn_softmax_bwd(*args, C.byref(p), None)


@pytest.mark.parametrize("which", range(5))
def test_fwd_null_pointer(dll, which):
    args = [P] * 5
    args[which] = None
    assert fwd(dll, params(), *args) == GLF_ERR_NULL
    assert b"null" in dll.glf_last_error()


@pytest.mark.parametrize("which", range(10))
def test_bwd_null_pointer(dll, which):
    assert bwd(dll, params(), null_at=which) == GLF_ERR_NULL
    assert b"null" in dll.glf_last_error()


def test_null_params(dll):
    assert dll.glf_s16_attn_softmax_fwd(P, P, P, P, P, None, None) == GLF_ERR_NULL
    assert dll.glf_s16_attn_softmax_bwd(*([P] * 10), None, None) == GLF_ERR_NULL


@pytest.mark.parametrize("frames,L", [(0, 100), (2, 0), (-1, 64), (2, -5)])
def test_bad_shape(dll, frames, L):
    p = params(frames=frames, L=L)
    assert fwd(dll, p) == GLF_ERR_BAD_SHAPE
    assert b"frames" in dll.glf_last_error()
    assert bwd(dll, p) == GLF_ERR_BAD_SHAPE


@pytest.mark.parametrize("ci", [32, 96, 1088, 2048, 0])
def test_unsupported_width(dll, ci):
    p = params(ci=ci, ld=max(3 * ci, 8))
    assert fwd(dll, p) == GLF_ERR_UNSUPPORTED
    assert b"Ci" in dll.glf_last_error()
    assert bwd(dll, p) == GLF_ERR_UNSUPPORTED


@pytest.mark.parametrize("field,value", [("ldq", 100), ("ldk", 3 * 128 + 4), ("ldv", 64), ("ldy", 130), ("lddy", 127), ("ldd", 120)])
def test_unsupported_stride(dll, field, value):
    p = params()
    setattr(p, field, value)
    if field not in ("lddy", "ldd"):                     # forward reads neither
        assert fwd(dll, p) == GLF_ERR_UNSUPPORTED
        assert b"stride" in dll.glf_last_error()
    assert bwd(dll, p) == GLF_ERR_UNSUPPORTED
    assert b"stride" in dll.glf_last_error()


def test_unaligned_operand(dll):
    assert fwd(dll, params(), theta=P + 2) == GLF_ERR_UNSUPPORTED
    assert b"aligned" in dll.glf_last_error()


def test_null_pointer_wins_over_other_errors(dll):
    """A null pointer is reported as GLF_ERR_NULL whatever else is wrong with the call."""
    bad = params(frames=0, L=0, ci=96, ld=100)
    for which in range(5):
        args = [P] * 5
        args[which] = None
        assert fwd(dll, bad, *args) == GLF_ERR_NULL, which
    for which in range(10):
        assert bwd(dll, bad, null_at=which) == GLF_ERR_NULL, which
