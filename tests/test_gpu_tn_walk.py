"""Edge shapes of what the TN (reduction form) kernels and their second stage share (csrc/gemm_tn_walk.h): the tap of a block
row, the slice of a workgroup, the row state of a gathered reduction row, the fp32 store epilogue and the slab summation with
1, 4 and 16 slice lanes -- through direct ops.gemm("tn") calls, on every tile family (64 x 64, 128 x 128, 256-row 8-wave, the
exact-fp32 fallback) and under every contraction precision.

Gate: EVERY value of C against float64, `close` of test_gpu_ops.py / test_gpu_rows_walk.py at their 5e-5 for f32, bf16x6 and
f16x3.  Those tests have no elementwise f16 bound to take over, so it is worked out here: under f16 every operand is rounded to
11 bits once (relative error uniform within 2^-12: 1.4e-4 rms), a product is off by sqrt(2) of that, 2.0e-4 rms of itself, and a
product of two operands uniform in [-1, 1] has mean square 1/9.  The sum of K products is therefore off by 6.7e-5 sqrt(K) rms;
the bound is 9 of those, 6e-4 sqrt(K) -- 3.4e-3 at K = 33, 2e-2 at K = 1057 (where the mode's model-level 2e-2 is met)."""
import pytest
import torch

from test_gpu_rows_walk import close, geo_of, rnd, src_index

pytestmark = pytest.mark.gpu

DEV = "cuda"
PRECISIONS = ["f32", "bf16x6", "f16x3", "f16"]


def tol(prec, K):
    return 6e-4 * K ** 0.5 if prec == "f16" else 5e-5


SENTINEL = 7.0                  # what C holds before a call that does not accumulate: a tap outside the mask must keep it
NO_CORNERS = 0x1FF & ~(1 | 4 | 64 | 256)

# (M, N) per tile family: 64 x 64 tiles | 128 x 128 with a ragged column tile | the 256-row 8-wave form with a ragged second row
# tile | M % 4 != 0: the exact-fp32 kernel under every precision, and (N % 4 != 0) the scalar second stage
SMALL, MID, WIDE, ODD = (64, 68), (128, 132), (260, 132), (66, 70)


def plain(name, mn, K, split=1, batch=1, accumulate=False, amax=False):
    return dict(name=name, M=mn[0], N=mn[1], K=K, split=split, batch=batch, accumulate=accumulate, amax=amax, conv=None, mask=1, rect=False)


def gathered(name, conv, split=1, rect=False, mask=0x1FF):
    return dict(name=name, M=SMALL[0], N=SMALL[1], K=None, split=split, batch=1, accumulate=False, amax=False, conv=conv, mask=mask, rect=rect)


CASES = [
    # tile families at K = 33: one K tile plus one row
    plain("small_k33", SMALL, 33), plain("mid_k33", MID, 33), plain("wide_k33", WIDE, 33), plain("odd_k33", ODD, 33),
    # chunk 32: the scalar second stage adds a one-row slice.  (The exact-fp32 and bf16x6 kernels add one accumulator per K tile
    # onto their running sum, so a slice boundary on a K tile boundary -- here, and in the _s2 gathers below -- reproduces the
    # bits of the unsplit call under those precisions; the float64 gate does not depend on that.)
    plain("odd_k33_s2", ODD, 33, split=2),
    # slices.  K = 100, split 3: chunk rounds to 64, the third slice is empty and returns early, the second stage counts 2
    plain("small_k100_s3", SMALL, 100, split=3), plain("mid_k100_s3", MID, 100, split=3),
    # K = 33 * 32 + 1: split 9 -> chunk 128, 9 slices, 4 slice lanes; split 33 -> chunk 64, 17 of 33 slices, 16 slice lanes
    plain("small_k1057_s9", SMALL, 1057, split=9), plain("mid_k1057_s9", MID, 1057, split=9),
    plain("small_k1057_s33", SMALL, 1057, split=33), plain("mid_k1057_s33", MID, 1057, split=33),
    # batch 3 with its own strides
    plain("mid_k100_b3", MID, 100, batch=3), plain("mid_k100_b3_s3", MID, 100, batch=3, split=3),
    # accumulate onto seeded C: the single atomic add of split 1, the second stage's add of split 3
    plain("mid_k100_acc", MID, 100, accumulate=True), plain("mid_k100_acc_s3", MID, 100, split=3, accumulate=True),
    plain("small_k100_acc_s3", SMALL, 100, split=3, accumulate=True),
    # gathers, conv = (n, h, w, k, stride, pad, dil)
    gathered("g_3x3_p1", (2, 9, 7, 3, 1, 1, 1)), gathered("g_3x3_p1_s2", (2, 9, 7, 3, 1, 1, 1), split=2),       # 126 rows: slice 1 starts inside image 1
    gathered("g_3x3_stride2", (2, 9, 9, 3, 2, 1, 1)), gathered("g_3x3_stride2_s2", (2, 9, 9, 3, 2, 1, 1), split=2),
    # dilation 5 on 2 x 12 x 12: K = 288, split 4 -> chunk 96; in rect mode the centre tap (288 rows) uses 3 of the 4 slices, the
    # edge taps (168 rows) and the corner taps (98 rows) use 2: every tap leaves at least one slice empty
    gathered("g_dil5_s4", (2, 12, 12, 3, 1, 5, 5), split=4), gathered("g_dil5_s4_rect", (2, 12, 12, 3, 1, 5, 5), split=4, rect=True),
    gathered("g_dil5_s4_nocorners", (2, 12, 12, 3, 1, 5, 5), split=4, mask=NO_CORNERS),
    gathered("g_dil5_s4_rect_nocorners", (2, 12, 12, 3, 1, 5, 5), split=4, rect=True, mask=NO_CORNERS),
]
AMAX_CASES = [plain("amax_mid_k100", MID, 100, amax=True), plain("amax_mid_k100_s3", MID, 100, split=3, amax=True),
              plain("amax_wide_k100", WIDE, 100, amax=True), plain("amax_small_k100_s3", SMALL, 100, split=3, amax=True)]

_inputs = {}


def inputs(case):
    """Seeded operands, the initial C and the float64 reference of a case: made once, shared by the precisions, never changed."""
    if case["name"] in _inputs:
        return _inputs[case["name"]]
    M, N, batch = case["M"], case["N"], case["batch"]
    if case["conv"] is None:
        K = case["K"]
        sa, sb, sc = (K * M + 8, K * N + 12, M * N + 4) if batch > 1 else (0, 0, 0)
        A, B = rnd(batch * (K * M + 8), seed=1), rnd(batch * (K * N + 12), seed=2)
        c0 = rnd(batch * (M * N + 4), seed=3) if case["accumulate"] else torch.full((batch * (M * N + 4),), SENTINEL)
        ref = c0.double().clone()
        for b in range(batch):
            a2, b2 = A[b * sa:b * sa + K * M].view(K, M).double(), B[b * sb:b * sb + K * N].view(K, N).double()
            out = ref[b * sc:b * sc + M * N].view(M, N)
            out.copy_(a2.T @ b2 + (out if case["accumulate"] else 0.0))
        kw = dict(M=M, N=N, K=K, lda=M, ldb=N, ldc=N, batch=batch, bsa=sa, bsb=sb, bsc=sc, split=case["split"], accumulate=case["accumulate"])
    else:
        geo = geo_of(1, case["conv"])
        src = src_index(1, geo)
        K, rows_b = geo[0] * geo[3] * geo[4], geo[0] * geo[1] * geo[2]
        A, B = rnd(K * M, seed=1), rnd(rows_b * N, seed=2)
        c0 = torch.full((9 * M * N,), SENTINEL)
        ref = c0.double().clone().view(9, M, N)
        bz = torch.cat([B.view(rows_b, N).double(), torch.zeros(1, N, dtype=torch.float64)])
        for t in range(9):
            if (case["mask"] >> t) & 1:
                ref[t] = A.view(K, M).double().T @ bz[src[t]]
        ref = ref.reshape(-1)
        kw = dict(M=M, N=N, K=K, lda=M, ldb=N, ldc=N, taps=9, mask=case["mask"], tap_stride_b=M * N, gather=1, geo=geo, split=case["split"],
                  rect=case["rect"])
    _inputs[case["name"]] = (A, B, c0, ref, kw)
    return _inputs[case["name"]]


def run_case(ops, case):
    """-> (C as the call left it, the float64 reference, the amax_c slot or None)"""
    A, B, c0, ref, kw = inputs(case)
    c = c0.to(DEV)
    slot = ops.amax_slot(torch.device(DEV, 0)) if case["amax"] else None
    ops.gemm("tn", A.to(DEV), B.to(DEV), c, amax_c=slot, **kw)
    torch.cuda.synchronize()
    return c, ref, slot


@pytest.mark.parametrize("prec", PRECISIONS)
@pytest.mark.parametrize("case", CASES, ids=lambda c: c["name"])
def test_every_value_against_float64(case, prec):
    from glfusion_amd import ops
    with ops.precision_scope(prec):
        c, ref, _ = run_case(ops, case)
    assert close(c, ref, tol(prec, inputs(case)[4]["K"]))


@pytest.mark.parametrize("case", AMAX_CASES, ids=lambda c: c["name"])
def test_amax_c_is_the_maximum_of_what_was_stored(case):
    """f16x3: from the direct store (split 1) and from the second stage (split 3), bit for bit."""
    from glfusion_amd import ops
    with ops.precision_scope("f16x3"):
        c, ref, slot = run_case(ops, case)
    assert close(c, ref, tol("f16x3", case["K"]))
    assert torch.equal(slot.cpu(), c[:case["M"] * case["N"]].abs().max().reshape(1).cpu())       # (behind C: untouched sentinels)
