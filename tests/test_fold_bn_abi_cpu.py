"""CPU: the folded-BatchNorm inference entry points (include/glfusion.h: glf_fold_bn, glf_gemm_nt_epilogue, glf_conv2d_fwd_folded and
pass 3 of glf_conv2d_plan) are exported and reject bad arguments with the documented codes before any HIP runtime call (no device is
touched here): NULL wins over every other error, bad extents give GLF_ERR_BAD_SHAPE, and every configuration the fused epilogue cannot
honour gives GLF_ERR_UNSUPPORTED instead of being ignored."""
import ctypes as C

import pytest

from glfusion_amd import _lib

GLF_OK, GLF_ERR_BAD_SHAPE, GLF_ERR_UNSUPPORTED, GLF_ERR_NULL = 0, -1, -2, -5
NAMES = ("glf_fold_bn", "glf_gemm_nt_epilogue", "glf_conv2d_fwd_folded", "glf_conv2d_plan", "glf_last_error", "glf_abi_version")

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


# ------------------------------------------------------------------------------------------------ glf_fold_bn
def fold(dll, null_at=None, eps=1e-5, taps=9, cout=8, cin=32, alias=False):
    args = [P, P + 64, P + 128, P + 192, P + 256, P + 320]                     # w_tap, conv_bias, gamma, beta, mean, var
    outs = [P if alias else P + 4096, P + 8192]                               # w_out, shift_out
    if null_at is not None:
        (args if null_at < 6 else outs)[null_at if null_at < 6 else null_at - 6] = None
    return dll.glf_fold_bn(*args, eps, *outs, taps, cout, cin, None)


@pytest.mark.parametrize("which", [0, 2, 3, 4, 5, 6, 7])
def test_fold_bn_null_pointer(dll, which):
    assert fold(dll, null_at=which) == GLF_ERR_NULL
    assert b"null" in dll.glf_last_error()
    assert fold(dll, null_at=which, cout=0) == GLF_ERR_NULL                    # NULL wins over a bad extent


@pytest.mark.parametrize("kw", [dict(taps=0), dict(cout=0), dict(cin=-1), dict(eps=-1.0), dict(alias=True)])
def test_fold_bn_bad_shape(dll, kw):
    assert fold(dll, **kw) == GLF_ERR_BAD_SHAPE


# ------------------------------------------------------------------------------------------------ glf_gemm_nt_epilogue
def gparams(M=392, N=256, K=64, precision=3, **kw):
    p = _lib.GemmParams()
    p.M, p.N, p.K, p.lda, p.ldb, p.ldc = M, N, K, K, K, N
    p.taps, p.tap_mask, p.tap_stride_b, p.gather = 1, 1, 0, 0
    (p.n_img, p.hs, p.ws, p.hd, p.wd, p.kh, p.kw, p.stride, p.pad, p.dil) = (1, 1, 1, 1, 1, 1, 1, 1, 0, 1)
    p.batch, p.alpha, p.split, p.precision = 1, 1.0, 1, precision
    for k, v in kw.items():
        setattr(p, k, v)
    return p


def epi(shift=P, residual=None, ld_res=0, relu=1):
    e = _lib.GemmEpilogue()
    e.shift, e.residual, e.ld_res, e.relu = shift, residual, ld_res, relu
    return e


def nt(dll, p, e, A=P, B=P, Cm=P):
    return dll.glf_gemm_nt_epilogue(A, B, Cm, C.byref(p) if p is not None else None, C.byref(e) if e is not None else None, None)


@pytest.mark.parametrize("which", ["A", "B", "C", "p", "e", "shift"])
def test_gemm_epilogue_null_pointer(dll, which):
    bad = gparams(M=0, precision=1, accumulate=1)                              # also a bad extent and unsupported settings: NULL wins
    kw = {"A": P, "B": P, "Cm": P}
    p, e = bad, epi()
    if which in ("A", "B", "C"):
        kw["Cm" if which == "C" else which] = None
    elif which == "p":
        p = None
    elif which == "e":
        e = None
    else:
        e = epi(shift=None)
    assert nt(dll, p, e, **kw) == GLF_ERR_NULL
    assert b"null" in dll.glf_last_error()


@pytest.mark.parametrize("p,e", [
    (gparams(M=0), epi()),
    (gparams(K=-32), epi()),
    (gparams(taps=0), epi()),
    (gparams(ldc=128), epi()),                                                 # ldc < N
    (gparams(), epi(relu=2)),
    (gparams(), epi(residual=P, ld_res=128)),                                  # ld_res < N
])
def test_gemm_epilogue_bad_shape(dll, p, e):
    assert nt(dll, p, e) == GLF_ERR_BAD_SHAPE


@pytest.mark.parametrize("kw", [
    dict(precision=1),                                                         # exact fp32
    dict(precision=2),                                                         # bf16x6
    dict(rect=1, gather=1, taps=9, tap_mask=0x1ff, kh=3, kw=3, n_img=2, hs=14, ws=14, hd=14, wd=14, pad=1),
    dict(accumulate=1),
    dict(split=2),
    dict(colstats=P),
    dict(colmax=P),
    dict(batch=2),
    dict(K=48),                                                                # off the aligned fast path
    dict(lda=66),
    dict(b_presplit=1),                                                        # pre-split operand without the amax it was split with
    dict(rect=2, gather=1, taps=9, tap_mask=0x1ff, kh=3, kw=3, n_img=2, hs=14, ws=14, hd=14, wd=14, pad=2, dil=1),   # region needs pad == dil
])
def test_gemm_epilogue_unsupported_is_refused_not_ignored(dll, kw):
    assert nt(dll, gparams(**kw), epi()) == GLF_ERR_UNSUPPORTED
    assert dll.glf_last_error()


def test_gemm_epilogue_unaligned_operand(dll):
    assert nt(dll, gparams(), epi(), A=P + 4) == GLF_ERR_UNSUPPORTED


# ------------------------------------------------------------------------------------------------ glf_conv2d_fwd_folded / plan pass 3
def cparams(n=2, h=14, w=14, cin=64, cout=256, k=1, stride=1, pad=0, dil=1, precision=3, colstats=None):
    p = _lib.ConvParams()
    p.n, p.h, p.w, p.cin, p.cout, p.kh, p.kw, p.stride, p.pad, p.dil, p.precision = n, h, w, cin, cout, k, k, stride, pad, dil, precision
    p.colstats = colstats
    return p


def folded(dll, p, x=P, w=P, shift=P, residual=None, ld_res=0, relu=1, y=P):
    return dll.glf_conv2d_fwd_folded(x, w, shift, residual, ld_res, relu, y, C.byref(p) if p is not None else None, None)


@pytest.mark.parametrize("which", ["x", "w", "shift", "y", "p"])
def test_conv_folded_null_pointer(dll, which):
    p = cparams(n=0, precision=1)                                              # bad extent + unsupported precision: NULL wins
    kw = {}
    if which == "p":
        p = None
    else:
        kw[which] = None
    assert folded(dll, p, **kw) == GLF_ERR_NULL
    assert b"null" in dll.glf_last_error()


def test_conv_folded_bad_shape(dll):
    assert folded(dll, cparams(n=0)) == GLF_ERR_BAD_SHAPE
    assert folded(dll, cparams(k=3, pad=0, h=2, w=2)) == GLF_ERR_BAD_SHAPE     # empty output
    assert folded(dll, cparams(), relu=3) == GLF_ERR_BAD_SHAPE
    assert folded(dll, cparams(), residual=P, ld_res=64) == GLF_ERR_BAD_SHAPE  # ld_res < cout


def test_conv_folded_unsupported(dll):
    assert folded(dll, cparams(precision=1)) == GLF_ERR_UNSUPPORTED
    assert folded(dll, cparams(precision=2)) == GLF_ERR_UNSUPPORTED
    assert folded(dll, cparams(colstats=P)) == GLF_ERR_UNSUPPORTED
    assert folded(dll, cparams(cin=48)) == GLF_ERR_UNSUPPORTED                 # K % 32 != 0
    # a 3x3 conv whose taps mostly fall into the padding, with pad != dil: per-tap rectangles with atomics, no region form
    assert folded(dll, cparams(h=28, w=28, cin=512, cout=256, k=3, pad=10, dil=12)) == GLF_ERR_UNSUPPORTED


def test_plan_pass3_is_pass0_except_regions(dll):
    """Pass 3 (the folded forward) plans like pass 0, except that the ASPP-style 3x3 'same' convs pass 0 runs as per-tap rectangles
    (rect 1, atomics into a zero-filled output) run as regions (rect 2, every element stored once, no zero fill)."""
    for kw in (dict(), dict(k=3, pad=1), dict(k=3, stride=2, pad=1, cin=128, cout=128), dict(h=14, w=14, cin=256, k=3, pad=2, dil=2)):
        p0, p3 = _lib.ConvPlan(), _lib.ConvPlan()
        assert dll.glf_conv2d_plan(C.byref(cparams(**kw)), 0, C.byref(p0)) == GLF_OK
        assert dll.glf_conv2d_plan(C.byref(cparams(**kw)), 3, C.byref(p3)) == GLF_OK
        assert p0.rect == 0 and p3.rect == 0 and p3.zero_fill == 0 and p3.colstats_ok == 0
        assert (p0.M, p0.N, p0.K, p0.tap_mask, p0.plain) == (p3.M, p3.N, p3.K, p3.tap_mask, p3.plain)
    aspp = cparams(n=1, h=28, w=28, cin=512, cout=256, k=3, pad=12, dil=12)
    p0, p3 = _lib.ConvPlan(), _lib.ConvPlan()
    assert dll.glf_conv2d_plan(C.byref(aspp), 0, C.byref(p0)) == GLF_OK and p0.rect == 1 and p0.zero_fill == 1
    assert dll.glf_conv2d_plan(C.byref(aspp), 3, C.byref(p3)) == GLF_OK and p3.rect == 2 and p3.zero_fill == 0
    assert dll.glf_conv2d_plan(C.byref(aspp), 4, C.byref(p3)) == GLF_ERR_NULL  # unknown pass: as before
