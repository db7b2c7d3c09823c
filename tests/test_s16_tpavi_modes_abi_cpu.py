"""CPU: the 16-bit-storage entry points of the `concatenate` and `gaussian` modes (include/glfusion.h: glf_s16_attn_pair_*,
glf_s16_softmax_rows_*, glf_s16_transpose2d_strided) are exported and reject bad arguments with the documented codes and a message,
in the documented order (NULL, extents, support, workspace), before any HIP runtime call (no device is touched here)."""
import ctypes as C

import pytest

from glfusion_amd import _lib

GLF_ERR_BAD_SHAPE, GLF_ERR_UNSUPPORTED, GLF_ERR_WORKSPACE, GLF_ERR_NULL = -1, -2, -3, -5

NAMES = ("glf_s16_attn_pair_relu_workspace_bytes", "glf_s16_attn_pair_relu_fwd", "glf_s16_attn_pair_relu_bwd",
         "glf_s16_attn_pair_proj_workspace_bytes", "glf_s16_attn_pair_proj_fwd", "glf_s16_attn_pair_proj_bwd",
         "glf_s16_softmax_rows_fwd", "glf_s16_softmax_rows_bwd", "glf_s16_transpose2d_strided", "glf_last_error", "glf_abi_version")


@pytest.fixture(scope="module")
def dll():
    d = C.CDLL(_lib.LIB_PATH)
    protos = _lib.parse_header()
    for name in NAMES:
        assert name in protos, name
        assert hasattr(d, name), f"libglfusion_hip.so does not export {name}"
        fn = getattr(d, name)
        fn.restype, fn.argtypes = protos[name]
    return d


def params(frames=2, L=100, ci=128, ld=None):
    p = _lib.AttnPairParams()
    p.frames, p.L, p.ci = frames, L, ci
    p.ldg = p.lddg = 3 * ci if ld is None else ld
    p.ldy = p.lddy = ci
    return p


# fake, 16-byte-aligned addresses: validation must reject every case below before anything dereferences them
P = 1 << 20


def fwd(dll, p, null_at=None):
    args = [P] * 5
    if null_at is not None:
        args[null_at] = None
    return dll.glf_s16_attn_pair_relu_fwd(*args, C.byref(p), None)


def bwd(dll, p, null_at=None, ws_bytes=1 << 40):
    args = [P] * 10
    if null_at is not None:
        args[null_at] = None
    return dll.glf_s16_attn_pair_relu_bwd(*args, ws_bytes, C.byref(p), None)


def test_abi_version_stays_7(dll):
    assert dll.glf_abi_version() == 7


def test_workspace_sizes(dll):
    p = params(frames=3, L=130)
    assert dll.glf_s16_attn_pair_relu_workspace_bytes(C.byref(p)) == 3 * 3 * 130 * 4
    assert dll.glf_s16_attn_pair_proj_workspace_bytes(1000, 128) == 4 * 2 * 128 * 4


@pytest.mark.parametrize("which", range(5))
def test_fwd_null_pointer(dll, which):
    assert fwd(dll, params(), null_at=which) == GLF_ERR_NULL
    assert b"null" in dll.glf_last_error()


@pytest.mark.parametrize("which", range(10))
def test_bwd_null_pointer(dll, which):
    assert bwd(dll, params(), null_at=which) == GLF_ERR_NULL
    assert b"null" in dll.glf_last_error()


def test_null_c_and_null_params(dll):
    assert fwd(dll, params(), null_at=2) == GLF_ERR_NULL                      # c: the device scalar
    assert dll.glf_s16_attn_pair_relu_fwd(P, P, P, P, P, None, None) == GLF_ERR_NULL


@pytest.mark.parametrize("frames,L", [(0, 100), (2, 0), (-1, 64)])
def test_bad_shape(dll, frames, L):
    p = params(frames=frames, L=L)
    assert fwd(dll, p) == GLF_ERR_BAD_SHAPE
    assert b"frames" in dll.glf_last_error()
    assert bwd(dll, p) == GLF_ERR_BAD_SHAPE


@pytest.mark.parametrize("ci", [96, 32, 1088, 2048, 0])
def test_unsupported_width(dll, ci):
    p = params(ci=ci, ld=max(3 * ci, 8))
    assert fwd(dll, p) == GLF_ERR_UNSUPPORTED
    assert b"Ci" in dll.glf_last_error()
    assert bwd(dll, p) == GLF_ERR_UNSUPPORTED


@pytest.mark.parametrize("field,value", [("ldg", 100), ("ldy", 130), ("lddy", 127), ("lddg", 3 * 128 + 4)])
def test_unsupported_stride(dll, field, value):
    p = params()
    setattr(p, field, value)
    if field in ("ldg", "ldy"):
        assert fwd(dll, p) == GLF_ERR_UNSUPPORTED
    if field != "ldy":
        assert bwd(dll, p) == GLF_ERR_UNSUPPORTED


def test_short_workspace(dll):
    p = params()
    need = dll.glf_s16_attn_pair_relu_workspace_bytes(C.byref(p))
    assert bwd(dll, p, ws_bytes=need - 4) == GLF_ERR_WORKSPACE
    assert b"workspace" in dll.glf_last_error()
    assert dll.glf_s16_attn_pair_proj_bwd(*([P] * 4), P, P, P, P, 128, P, P, 16, 1000, 128, None) == GLF_ERR_WORKSPACE


def test_order_null_then_extents_then_support_then_workspace(dll):
    bad = params(frames=0, L=0, ci=96, ld=100)
    assert bwd(dll, bad, null_at=4, ws_bytes=0) == GLF_ERR_NULL
    assert bwd(dll, bad, ws_bytes=0) == GLF_ERR_BAD_SHAPE
    assert bwd(dll, params(ci=96, ld=288), ws_bytes=0) == GLF_ERR_UNSUPPORTED
    assert bwd(dll, params(), ws_bytes=0) == GLF_ERR_WORKSPACE


def test_proj_checks(dll):
    assert dll.glf_s16_attn_pair_proj_fwd(P, None, 384, P, P, P, 100, 128, None) == GLF_ERR_NULL
    assert dll.glf_s16_attn_pair_proj_fwd(P, P, 64, P, P, P, 100, 128, None) == GLF_ERR_BAD_SHAPE        # ld < Ci
    assert dll.glf_s16_attn_pair_proj_fwd(P, P, 388, P, P, P, 100, 128, None) == GLF_ERR_UNSUPPORTED     # ld % 8


def test_softmax_rows_checks(dll):
    assert dll.glf_s16_softmax_rows_fwd(None, P, 10, 90, 128, 128, None) == GLF_ERR_NULL
    assert dll.glf_s16_softmax_rows_bwd(P, None, P, 10, 90, 128, 128, 128, None) == GLF_ERR_NULL
    assert dll.glf_s16_softmax_rows_fwd(P, P, 0, 90, 128, 128, None) == GLF_ERR_BAD_SHAPE
    assert dll.glf_s16_softmax_rows_fwd(P, P, 10, 90, 64, 128, None) == GLF_ERR_BAD_SHAPE               # ld_s < cols
    assert dll.glf_s16_softmax_rows_fwd(P, P, 10, 90, 128, 92, None) == GLF_ERR_UNSUPPORTED             # ld_p % 8
    assert dll.glf_s16_softmax_rows_bwd(P, P + 4, P, 10, 90, 128, 128, 128, None) == GLF_ERR_UNSUPPORTED
    assert b"aligned" in dll.glf_last_error()


def test_transpose_strided_checks(dll):
    assert dll.glf_s16_transpose2d_strided(None, 8, 64, P, 8, 64, 8, 8, 8, 1, None) == GLF_ERR_NULL
    assert dll.glf_s16_transpose2d_strided(P, 8, 64, P, 8, 64, 8, 8, 4, 1, None) == GLF_ERR_BAD_SHAPE   # rows_pad < rows
