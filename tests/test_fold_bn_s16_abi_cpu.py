"""CPU: the folded-BatchNorm inference entry points of 16-bit storage (include/glfusion.h: glf_s16_fold_bn, glf_s16_gemm_nt_epilogue) are
exported and reject bad arguments with the documented codes before any HIP runtime call (no device is touched here): NULL wins over
every other error, bad extents give GLF_ERR_BAD_SHAPE, and every configuration the fused epilogue cannot honour gives
GLF_ERR_UNSUPPORTED instead of being ignored."""
import ctypes as C

import pytest

from glfusion_amd import _lib

GLF_OK, GLF_ERR_BAD_SHAPE, GLF_ERR_UNSUPPORTED, GLF_ERR_NULL = 0, -1, -2, -5
GLF_DT_F32, GLF_DT_BF16 = 0, 1
NAMES = ("glf_s16_fold_bn", "glf_s16_gemm_nt_epilogue", "glf_last_error", "glf_abi_version")

# fake, 16-byte-aligned addresses: validation must reject every case below before anything dereferences them
P = 1 << 20


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


def test_abi_version_unchanged(dll):
    assert dll.glf_abi_version() == 7


def test_epilogue_struct_mirror():
    """glf_s16_gemm_epilogue: two pointers, an int64 and two int32 -- 32 bytes, ld_res at 16, relu at 24."""
    e = _lib.S16GemmEpilogue
    assert C.sizeof(e) == 32 and (e.shift.offset, e.residual.offset, e.ld_res.offset, e.relu.offset, e.reserved.offset) == (0, 8, 16, 24, 28)


# ------------------------------------------------------------------------------------------------ glf_s16_fold_bn
def fold(dll, null_at=None, eps=1e-5, taps=9, cout=8, cin=32, alias=False, w=P, out=P + 4096):
    args = [w, P + 64, P + 128, P + 192, P + 256, P + 320]                    # w_tap, bias, gamma, beta, mean, var
    outs = [w if alias else out, P + 8192]                                    # w_folded_bf16, shift
    if null_at is not None:
        (args if null_at < 6 else outs)[null_at if null_at < 6 else null_at - 6] = None
    return dll.glf_s16_fold_bn(*args, eps, *outs, taps, cout, cin, None)


@pytest.mark.parametrize("which", [0, 2, 3, 4, 5, 6, 7])                       # every pointer but the optional conv bias
def test_fold_bn_null_pointer(dll, which):
    assert fold(dll, null_at=which) == GLF_ERR_NULL
    assert b"null" in dll.glf_last_error()
    assert fold(dll, null_at=which, cout=0) == GLF_ERR_NULL                    # NULL wins over a bad extent
    assert fold(dll, null_at=which, cin=12) == GLF_ERR_NULL                    # ... and over an unsupported one


@pytest.mark.parametrize("kw", [dict(taps=0), dict(cout=0), dict(cin=-8), dict(eps=-1.0), dict(alias=True)])
def test_fold_bn_bad_shape(dll, kw):
    assert fold(dll, **kw) == GLF_ERR_BAD_SHAPE
    assert dll.glf_last_error()


@pytest.mark.parametrize("kw", [dict(cin=12), dict(cin=63), dict(w=P + 4), dict(out=P + 4098)])
def test_fold_bn_unsupported_is_refused_not_ignored(dll, kw):
    """cin % 8 != 0 (no 16-byte rows of bf16) and weight images off 16-byte alignment."""
    assert fold(dll, **kw) == GLF_ERR_UNSUPPORTED
    assert dll.glf_last_error()


def test_fold_bn_bad_extent_wins_over_unsupported(dll):
    assert fold(dll, cin=12, cout=0) == GLF_ERR_BAD_SHAPE


# ------------------------------------------------------------------------------------------------ glf_s16_gemm_nt_epilogue
CONV = dict(gather=1, taps=9, tap_mask=0x1ff, kh=3, kw=3, n_img=2, hs=14, ws=14, hd=14, wd=14, pad=1, tap_stride_b=256 * 64)


def gparams(M=392, N=256, K=64, **kw):
    p = _lib.GemmParams()
    p.M, p.N, p.K, p.lda, p.ldb, p.ldc = M, N, K, K, K, N
    p.taps, p.tap_mask, p.tap_stride_b, p.gather = 1, 1, 0, 0
    (p.n_img, p.hs, p.ws, p.hd, p.wd, p.kh, p.kw, p.stride, p.pad, p.dil) = (1, 1, 1, 1, 1, 1, 1, 1, 0, 1)
    p.batch, p.alpha, p.split, p.c_dtype = 1, 1.0, 1, GLF_DT_BF16
    for k, v in kw.items():
        setattr(p, k, v)
    return p


def epi(shift=P, residual=None, ld_res=0, relu=1):
    e = _lib.S16GemmEpilogue()
    e.shift, e.residual, e.ld_res, e.relu = shift, residual, ld_res, relu
    return e


def nt(dll, p, e, A=P, B=P, Cm=P):
    return dll.glf_s16_gemm_nt_epilogue(A, B, Cm, C.byref(p) if p is not None else None, C.byref(e) if e is not None else None, None)


@pytest.mark.parametrize("which", ["A", "B", "C", "p", "e", "shift"])
def test_gemm_epilogue_null_pointer(dll, which):
    bad = gparams(M=0, c_dtype=GLF_DT_F32, accumulate=1)                       # also a bad extent and unsupported settings: NULL wins
    kw = {"A": P, "B": P, "Cm": P}
    p, e = bad, epi(relu=3)
    if which in ("A", "B", "C"):
        kw["Cm" if which == "C" else which] = None
    elif which == "p":
        p = None
    elif which == "e":
        e = None
    else:
        e = epi(shift=None, relu=3)
    assert nt(dll, p, e, **kw) == GLF_ERR_NULL
    assert b"null" in dll.glf_last_error()


@pytest.mark.parametrize("p,e", [
    (gparams(M=0), epi()),
    (gparams(K=-64), epi()),
    (gparams(taps=0), epi()),
    (gparams(tap_mask=0), epi()),
    (gparams(ldc=128), epi()),                                                 # ldc < N
    (gparams(**dict(CONV, n_img=3)), epi()),                                   # M != n_img * hd * wd
    (gparams(), epi(relu=3)),
    (gparams(), epi(relu=-1)),
    (gparams(), epi(residual=P, ld_res=128)),                                  # ld_res < N
])
def test_gemm_epilogue_bad_shape(dll, p, e):
    assert nt(dll, p, e) == GLF_ERR_BAD_SHAPE
    assert dll.glf_last_error()


def test_gemm_epilogue_bad_shape_wins_over_unsupported(dll):
    assert nt(dll, gparams(c_dtype=GLF_DT_F32, accumulate=1), epi(relu=3)) == GLF_ERR_BAD_SHAPE
    assert nt(dll, gparams(split=2), epi(residual=P, ld_res=100)) == GLF_ERR_BAD_SHAPE


@pytest.mark.parametrize("kw,ekw", [
    (dict(c_dtype=GLF_DT_F32), {}),
    (dict(c_dtype=7), {}),
    (dict(accumulate=1), {}),
    (dict(colstats=P), {}),
    (dict(split=2), {}),
    (dict(batch=2), {}),
    (dict(CONV, gather=2), {}),                                                # the transposed (dgrad) gather
    ({}, dict(residual=P + 8, ld_res=256)),                                    # residual not 16-byte aligned
    ({}, dict(residual=P, ld_res=260)),                                        # ld_res % 8 != 0
    (dict(K=96), {}),                                                          # K % 64 != 0
    (dict(CONV, rect=1), {}),                                                  # per-tap rectangles: not a store-once mode
    (dict(CONV, rect=2, pad=2, dil=1), {}),                                    # region mode needs pad == dil
])
def test_gemm_epilogue_unsupported_is_refused_not_ignored(dll, kw, ekw):
    assert nt(dll, gparams(**kw), epi(**ekw)) == GLF_ERR_UNSUPPORTED
    assert dll.glf_last_error()
