"""The second stage of glf_gemm_tn storing the parameter layout (glf_gemm_params.c_oihw) against the two-step route it replaces:
glf_gemm_tn into a tap-major [taps][Cout][Cin] image, then glf_tap_major_to_oihw.  The comparison is BIT FOR BIT -- the fused
store adds the same slabs in the same order -- and every destination starts as NaN, so an element never written shows up."""
import pytest
import torch

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
CENTRE = 1 << 4


def _bits(a, b):
    return torch.equal(a.contiguous().view(torch.int32), b.contiguous().view(torch.int32))


def _operands(n, h, w, cin, cout, seed=11):
    g = torch.Generator().manual_seed(seed)
    rows = n * h * w
    return torch.randn(rows, cout, generator=g).to(DEV), torch.randn(rows, cin, generator=g).to(DEV)


def _kw(n, h, w, cin, cout, dil, mask, split, rect):
    return dict(M=cout, N=cin, K=n * h * w, lda=cout, ldb=cin, ldc=cin, taps=9, mask=mask, tap_stride_b=cout * cin, gather=1,
                geo=(n, h, w, h, w, 3, 3, 1, dil, dil), split=split, rect=rect)


def _two_step(ops, dy, x, cin, cout, kw, foreign=None):
    """Today's route: tap-major (zero-filled where the mask is partial), the foreign tap copied in, then the re-layout."""
    from glfusion_amd._lib import check, lib
    full = kw["mask"] == (1 << 9) - 1
    dwt = torch.full((9, cout, cin), float("nan"), device=DEV) if full else torch.zeros(9, cout, cin, device=DEV)
    if kw["mask"]:
        ops.gemm("tn", dy, x, dwt, **kw)
    if foreign is not None:
        dwt[foreign[0]].copy_(foreign[1])
    dw = torch.full((cout, cin, 3, 3), float("nan"), device=DEV)
    check(lib.glf_tap_major_to_oihw(dwt.data_ptr(), dw.data_ptr(), cout, cin, 9, torch.cuda.current_stream().cuda_stream), "tap_major_to_oihw")
    return dw


def _fused(ops, dy, x, cin, cout, kw, foreign=None, into=None, **extra):
    dw = torch.full((cout, cin, 3, 3), float("nan"), device=DEV) if into is None else into
    f = None if foreign is None else (foreign[0], foreign[1], foreign[1].stride(0))
    ops.gemm("tn", dy, x, dw, oihw=True, foreign=f, **kw, **extra)
    return dw


# (n, h, w, Cin, Cout, split): the launcher takes slice lanes while 4 lanes <= split and Cout Cin / 4 x lanes < 65536.
#   2 x 12 x 10, 64 -> 32 (512 float4 groups): split 3 -> the plain walk, 5 -> lanes<4>, 16 -> lanes<16> (8 of the 16 slices run)
#   3 x 28 x 28, 64 -> 32, split 40: lanes<16> with 37 slices, the lanes' two-at-a-time loop and its tail
#   3 x 28 x 28, 1024 -> 256 (65536 groups), split 7: the plain walk past its four-at-a-time loop, 256 workgroups
#   2 x 12 x 10, 68 -> 30 (510 groups): a ragged last workgroup; Cout % 4 != 0 sends the contraction to the exact kernel
#   split 1: one slab, which the reference route never makes (it stores directly)
VARIANTS = [(2, 12, 10, 64, 32, 3), (2, 12, 10, 64, 32, 5), (2, 12, 10, 64, 32, 16), (3, 28, 28, 64, 32, 40), (3, 28, 28, 1024, 256, 7),
            (2, 12, 10, 68, 30, 3), (2, 12, 10, 68, 30, 6), (2, 12, 10, 64, 32, 1)]


@pytest.mark.parametrize("prec", ["f32", "f16x3"])
@pytest.mark.parametrize("case", VARIANTS, ids=lambda c: "x".join(map(str, c)))
def test_full_mask_every_reduce_variant(case, prec):
    from glfusion_amd import ops
    n, h, w, cin, cout, split = case
    with ops.precision_scope(prec):
        dy, x = _operands(n, h, w, cin, cout)
        kw = _kw(n, h, w, cin, cout, 1, (1 << 9) - 1, split, False)
        want = _two_step(ops, dy, x, cin, cout, kw)
        got = _fused(ops, dy, x, cin, cout, kw)
        torch.cuda.synchronize()
    assert not bool(torch.isnan(want).any())
    assert _bits(got, want)


@pytest.mark.parametrize("prec", ["f32", "f16x3"])
@pytest.mark.parametrize("split", [3, 9, 33])                  # plain, lanes<4>, lanes<16>: per-tap slice counts differ in rect mode
def test_rect_mode_centre_cleared_and_foreign_tap(split, prec):
    from glfusion_amd import ops
    n, h, w, cin, cout, dil = 3, 28, 28, 64, 32, 24
    with ops.precision_scope(prec):
        dy, x = _operands(n, h, w, cin, cout)
        mask = ops.tap_mask(1, h, w, h, w, 3, 3, 1, dil, dil) & ~CENTRE
        assert bin(mask).count("1") == 8
        kw = _kw(n, h, w, cin, cout, dil, mask, split, True)
        # the masked tap comes out as exact zeros
        want = _two_step(ops, dy, x, cin, cout, kw)
        got = _fused(ops, dy, x, cin, cout, kw)
        torch.cuda.synchronize()
        assert _bits(got, want)
        assert float(got[:, :, 1, 1].abs().max()) == 0.0 and float(got[:, :, 0, 0].abs().min()) > 0.0
        # the foreign centre tap: a row block of a wider buffer (row stride Cin + 8)
        src = torch.randn(4 * cout, cin + 8, generator=torch.Generator().manual_seed(2)).to(DEV)[2 * cout:3 * cout, :cin]
        want = _two_step(ops, dy, x, cin, cout, kw, (4, src))
        got = _fused(ops, dy, x, cin, cout, kw, (4, src))
        torch.cuda.synchronize()
        assert _bits(got, want) and _bits(got[:, :, 1, 1], src)


@pytest.mark.parametrize("prec", ["f32", "f16x3"])
def test_store_only_form(prec):
    """Dilation 36 on 28 x 28 keeps the centre tap alone; with that one foreign the mask is empty and nothing is contracted."""
    from glfusion_amd import ops
    n, h, w, cin, cout, dil = 3, 28, 28, 64, 32, 36
    with ops.precision_scope(prec):
        dy, x = _operands(n, h, w, cin, cout)
        mask = ops.tap_mask(1, h, w, h, w, 3, 3, 1, dil, dil)
        assert mask == CENTRE
        src = torch.randn(cout, cin, generator=torch.Generator().manual_seed(3)).to(DEV)
        ops.PROFILER = prof = []
        try:
            got = _fused(ops, dy, x, cin, cout, _kw(n, h, w, cin, cout, dil, 0, 1, False), (4, src))
        finally:
            ops.PROFILER = None
        torch.cuda.synchronize()
    assert not prof                                            # no contraction was launched
    assert _bits(got[:, :, 1, 1], src)
    rest = got.clone()
    rest[:, :, 1, 1] = 0
    assert _bits(rest, torch.zeros_like(rest))


@pytest.mark.parametrize("split", [3, 5])
def test_accumulate_adds_to_the_destination(split):
    from glfusion_amd import ops
    n, h, w, cin, cout, dil = 3, 28, 28, 64, 32, 24
    with ops.precision_scope("f16x3"):
        dy, x = _operands(n, h, w, cin, cout)
        mask = ops.tap_mask(1, h, w, h, w, 3, 3, 1, dil, dil) & ~CENTRE & ~1          # tap 0 masked out as well: it must keep d0
        kw = _kw(n, h, w, cin, cout, dil, mask, split, True)
        src = torch.randn(cout, cin, generator=torch.Generator().manual_seed(4)).to(DEV)
        r = _fused(ops, dy, x, cin, cout, kw, (4, src))
        # the store rounds destination + (the slices' sum in double) once; against destination + the ROUNDED result r that is
        # half an ulp of r and half an ulp of the sum apart.  The destination takes r's sign, so the sum is the larger of the two
        # and both halves fit into one ulp of it (with cancellation the first half would not).
        d0 = torch.randn(cout, cin, 3, 3, generator=torch.Generator().manual_seed(5)).to(DEV)
        torch.cuda.synchronize()
        d0 = torch.where(r != 0, d0.abs() * r.sign(), d0)
        got = _fused(ops, dy, x, cin, cout, kw, (4, src), into=d0.clone(), accumulate=True)
        torch.cuda.synchronize()
    want = d0.double() + r.double()
    assert bool(((got.double() - want).abs() <= want.abs() * 2.0 ** -23).all())
    assert _bits(got[:, :, 0, 0], d0[:, :, 0, 0])


def test_refused_forms():
    """What the fused store does not take is GLF_ERR_UNSUPPORTED (status -2) before anything is launched, and the destination is
    untouched; a foreign tap that is also in the mask is GLF_ERR_BAD_SHAPE (-1)."""
    from glfusion_amd import ops
    n, h, w, cin, cout = 2, 12, 10, 64, 32
    full = (1 << 9) - 1
    with ops.precision_scope("f16x3"):
        dy, x = _operands(n, h, w, cin, cout)
        kw = _kw(n, h, w, cin, cout, 1, full, 3, False)
        dw = torch.full((cout * cin * 9 + 4,), float("nan"), device=DEV)
        with pytest.raises(RuntimeError, match=r"status -2"):     # batch > 1
            ops.gemm("tn", dy, x, dw, oihw=True, **dict(kw, K=n * h * w // 2, geo=(1, h, w, h, w, 3, 3, 1, 1, 1)), batch=2,
                     bsa=cout * h * w, bsb=cin * h * w, bsc=cout * cin * 9)
        dy2, x2 = _operands(n, h, w, 66, cout)
        with pytest.raises(RuntimeError, match=r"status -2"):     # Cin % 4 != 0: the non-vector form
            ops.gemm("tn", dy2, x2, dw, oihw=True, **_kw(n, h, w, 66, cout, 1, full, 3, False))
        with pytest.raises(RuntimeError, match=r"status -2"):     # a destination that is not 16-byte aligned
            ops.gemm("tn", dy, x, dw[1:], oihw=True, **kw)
        with pytest.raises(RuntimeError, match=r"status -2"):     # a 4 x 4 kernel: more taps than the store's tile holds
            ops.gemm("tn", dy, x, dw, oihw=True, **dict(kw, taps=16, mask=(1 << 16) - 1, geo=(n, h, w, h, w, 4, 4, 1, 1, 1)))
        with pytest.raises(RuntimeError, match=r"status -2"):     # a foreign tap without the parameter-layout store
            p = dict(kw, mask=full & ~CENTRE)
            _raw_foreign_without_oihw(ops, dy, x, dw, p)
        with pytest.raises(RuntimeError, match=r"status -1"):     # the foreign tap is also a kept tap
            ops.gemm("tn", dy, x, dw, oihw=True, foreign=(4, x[:cout], cin), **kw)
        torch.cuda.synchronize()
    assert bool(torch.isnan(dw).all())


def _raw_foreign_without_oihw(ops, dy, x, dw, kw):
    """glf_gemm_tn with foreign_src set and c_oihw clear (ops.gemm never builds this)."""
    import ctypes as C
    from glfusion_amd._lib import GemmParams, check, lib
    p = GemmParams()
    p.M, p.N, p.K, p.lda, p.ldb, p.ldc = kw["M"], kw["N"], kw["K"], kw["lda"], kw["ldb"], kw["ldc"]
    p.taps, p.tap_mask, p.tap_stride_b, p.gather = kw["taps"], kw["mask"], kw["tap_stride_b"], kw["gather"]
    (p.n_img, p.hs, p.ws, p.hd, p.wd, p.kh, p.kw, p.stride, p.pad, p.dil) = kw["geo"]
    p.batch, p.alpha, p.split, p.precision = 1, 1.0, 1, 1
    p.foreign_tap, p.foreign_src, p.foreign_ld = 4, x.data_ptr(), kw["N"]
    check(lib.glf_gemm_tn(dy.data_ptr(), x.data_ptr(), dw.data_ptr(), C.byref(p), torch.cuda.current_stream().cuda_stream), "gemm_tn")
