"""GPU: glf_s16_gemm_nt / glf_s16_gemm_tn (csrc/gemm_s16.hip) driven directly through ops16.gemm16 and judged element by element
against float64 on the same bf16 operands.

Three kinds of evidence, used together (the whole-tensor relative L2 gates of test_gpu_s16.py pass a truncating store and cannot
see one wrong element):
  (a) integer operands -- small integers in bf16, alpha a power of two, integer bias and old C, |alpha| |A| |B|^T + |bias| +
      |C_old| < 2^24 asserted on the CPU first: every product and partial sum is exact in fp32 whatever the order, so an fp32
      result must EQUAL the float64 reference and a bf16 result must equal reference.float().to(bfloat16) bit for bit (odd
      integers in [256, 512) are exact ties: round-to-nearest, ties-to-even is pinned at the store);
  (b) Gaussian operands -- per element, d = (n_terms + 4) 2^-23 (|alpha| |A| |B|^T + |bias| + |C_old|) is the worst-case fp32
      accumulation bound for any summation order (twice gamma_n for unspecified rounding inside the MFMA; + 4 for the alpha, bias
      and accumulate operations and the double -> float step of the check).  fp32 C: |got - ref| <= d; bf16 C:
      bf16_rne(ref - d) <= got <= bf16_rne(ref + d).  No element is excluded;
  (c) fp32 results also against a CPU emulation of the documented order (taps ascending, k ascending, 16-deep steps, fp32
      accumulator; TN: slices in order, then the slice sum): relL2(got, ref) <= 3 relL2(emulation, ref) (floor 1e-7).  The 3 is a
      margin for the unspecified order inside a 16-deep MFMA step, not a measurement.
Every operand is a view into a larger NaN-filled buffer (padding columns up to the row stride, rows behind the last one, gaps
between batches, offsets and strides multiples of 8 elements): a NaN read into a live output shows up, every logical C element
must come back finite, and the bit pattern of every C-buffer element outside the logical C must be unchanged.

Which kernel variant a case runs is computed here with the host formulas of gemm_s16.hip (nt_variant / tn_variant) and printed;
tests/test_s16_gemm_ref_cpu.py asserts on the CPU that the case tables reach every variant and that the gates accept a correct
result and reject a truncating store and a dropped k-step."""
import ctypes as C
import math
import os
import subprocess
import sys

import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

DEV = "cuda"
BF = torch.bfloat16
F32 = torch.float32
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CHILD_MARK = "GLF_S16_GEMM_TEST_CHILD"          # set in the child processes of test_stage_depths_in_child_processes
TM, TK_TN, TN_BN = 256, 64, 128                  # tile constants of gemm_s16.hip
ERR_BAD_SHAPE, ERR_UNSUPPORTED, ERR_WORKSPACE = -1, -2, -3   # include/glfusion.h


@pytest.fixture(autouse=True)
def _s16_mode():
    if not torch.cuda.is_available():
        yield
        return
    from glfusion_amd import ops
    ops.set_precision("bf16")
    yield
    ops.set_precision("f32")


# ----------------------------------------------------------------------------------------
# operand families: float64 tensors whose values are exactly representable in bf16
# ----------------------------------------------------------------------------------------
def _gen(seed):
    return torch.Generator(device="cpu").manual_seed(seed)


def dense_ints(shape, seed, lo=-3, hi=3):
    return torch.randint(lo, hi + 1, tuple(shape), generator=_gen(seed)).double()


def ternary(shape, seed, n_terms):
    """{-1, 0, 1} with density p = min(0.5, sqrt(96 / n_terms)): |A| |B|^T stays far below 255 for any reduction length."""
    p = min(0.5, math.sqrt(96.0 / n_terms))
    g = _gen(seed)
    keep = torch.rand(tuple(shape), generator=g) < p
    sign = torch.randint(0, 2, tuple(shape), generator=g).double() * 2 - 1
    return torch.where(keep, sign, torch.zeros(()).double())


def gauss(shape, seed, scale=1.0, dtype=BF):
    return (torch.randn(tuple(shape), generator=_gen(seed)) * scale).to(dtype).double()


def operand(family, shape, seed, n_terms):
    if family == "dense":
        return dense_ints(shape, seed)
    if family == "ternary":
        return ternary(shape, seed, n_terms)
    return gauss(shape, seed)


def f32_alpha(a):
    """alpha travels as a C float: the reference uses the value the kernel sees."""
    return float(torch.tensor(a, dtype=F32))


# ----------------------------------------------------------------------------------------
# rounding and gates
# ----------------------------------------------------------------------------------------
def bf16_rne(x):
    """float64 -> float32 -> bf16, both round-to-nearest-even, back as float64.  As an interval end this is valid for any fp32
    value v inside the interval: v >= lo implies v >= rne_f32(lo), and bf16 rounding is monotone."""
    return x.float().to(BF).double()


def bf16_trunc(x32):
    """fp32 -> bf16 by dropping the low 16 bits (the defect the interval gate must reject)."""
    return (x32.contiguous().view(torch.int32) & -65536).view(F32)


def rel_l2(a, b):
    a, b = a.double(), b.double()
    return float((a - b).norm()) / max(float(b.norm()), 1e-30)


def assert_exact_precondition(absref):
    assert float(absref.max()) < 2 ** 24, f"integer case is not exact in fp32: |.| reaches {float(absref.max())}"


def gate_exact(got, ref, c_bf16, what):
    assert torch.equal(ref.float().double(), ref), what + ": reference is not an fp32 value"
    want = ref.float().to(BF) if c_bf16 else ref.float()
    bad = got != want
    nbad = int(bad.sum())
    if nbad:
        i = tuple(int(v) for v in bad.nonzero()[0])
        raise AssertionError(f"{what}: {nbad} of {got.numel()} elements differ from float64; first at {i}: got {float(got[i])}, "
                             f"want {float(want[i])} (unrounded {float(ref[i])})")


def interval_violations(got, ref, absref, n_terms, c_bf16):
    """Elements outside the derived interval, and the largest |got - ref| / d (fp32) for the report."""
    d = (n_terms + 4) * 2.0 ** -23 * absref
    g = got.double()
    if c_bf16:
        bad = (g < bf16_rne(ref - d)) | (g > bf16_rne(ref + d))
    else:
        bad = (g - ref).abs() > d
    worst = float(((g - ref).abs() / d.clamp_min(1e-300)).max())
    return bad, worst


def gate_interval(got, ref, absref, n_terms, c_bf16, what):
    bad, worst = interval_violations(got, ref, absref, n_terms, c_bf16)
    nbad = int(bad.sum())
    print(f"    {what}: n_terms {n_terms}, max |got-ref|/d {worst:.3g}, outside {nbad} of {got.numel()}")
    if nbad:
        i = tuple(int(v) for v in bad.nonzero()[0])
        raise AssertionError(f"{what}: {nbad} of {got.numel()} elements outside the derived interval; first at {i}: got "
                             f"{float(got[i])}, ref {float(ref[i])}, sum|a||b| {float(absref[i])}")


def gate_emulation(got, emu, ref, what):
    e_got, e_emu = rel_l2(got, ref), rel_l2(emu, ref)
    print(f"    {what}: relL2(got, f64) {e_got:.3e}, relL2(emulation, f64) {e_emu:.3e}")
    assert e_got <= max(3.0 * e_emu, 1e-7), f"{what}: relL2 {e_got:.3e} > 3 x emulation {e_emu:.3e}"


# ----------------------------------------------------------------------------------------
# gather index arithmetic (gemm_common.h: map_src) and the float64 references
# ----------------------------------------------------------------------------------------
def conv_out(h, k, stride, pad, dil):
    return (h + 2 * pad - dil * (k - 1) - 1) // stride + 1


def geo_of(gather, conv):
    """glf_gemm_params geometry (n_img, hs, ws, hd, wd, kh, kw, stride, pad, dil) of conv = (n, h, w, k, stride, pad, dil):
    gather 1 maps output pixels to input pixels, gather 2 input pixels to output-gradient pixels."""
    n, h, w, k, stride, pad, dil = conv
    ho, wo = conv_out(h, k, stride, pad, dil), conv_out(w, k, stride, pad, dil)
    return (n, h, w, ho, wo, k, k, stride, pad, dil) if gather == 1 else (n, ho, wo, h, w, k, k, stride, pad, dil)


def src_index(gather, geo):
    """[taps][rows] source row of every destination row and tap, -1 where the tap falls into the padding."""
    n_img, hs, ws, hd, wd, kh, kw, stride, pad, dil = geo
    m = torch.arange(n_img * hd * wd)
    n, y, x = m // (hd * wd), (m // wd) % hd, m % wd
    out = []
    for t in range(kh * kw):
        ky, kx = divmod(t, kw)
        if gather == 1:
            sy, sx = y * stride - pad + ky * dil, x * stride - pad + kx * dil
            ok = (sy >= 0) & (sy < hs) & (sx >= 0) & (sx < ws)
        else:
            ny, nx = y + pad - ky * dil, x + pad - kx * dil
            ok = (ny >= 0) & (nx >= 0) & (ny % stride == 0) & (nx % stride == 0)
            sy, sx = torch.div(ny, stride, rounding_mode="floor"), torch.div(nx, stride, rounding_mode="floor")
            ok = ok & (sy < hs) & (sx < ws)
        out.append(torch.where(ok, (n * hs + sy) * ws + sx, torch.full_like(m, -1)))
    return torch.stack(out)


def mask_of(src):
    """tap_mask: bit t set when tap t is in range for some row."""
    return sum(1 << t for t in range(src.shape[0]) if bool((src[t] >= 0).any()))


def kept_taps(mask, taps):
    return [t for t in range(taps) if (mask >> t) & 1]


def gather_rows(A, idx):
    """A[idx] with zero rows where idx == -1."""
    return torch.cat([A, torch.zeros(1, A.shape[1], dtype=A.dtype)])[idx]


def nt_products(A, B, src, mask):
    """sum over kept taps of A[src_tap] @ B_tap^T and the same on magnitudes; A [rows][K], B [taps][N][K], float64."""
    P = torch.zeros(src.shape[1], B.shape[1], dtype=torch.float64)
    Q = torch.zeros_like(P)
    for t in kept_taps(mask, B.shape[0]):
        At = gather_rows(A, src[t])
        P += At @ B[t].T
        Q += At.abs() @ B[t].abs().T
    return P, Q


def nt_emulate(A, B, src, mask):
    """fp32 accumulator of the documented order: taps ascending, k ascending, 16-deep steps."""
    acc = torch.zeros(src.shape[1], B.shape[1], dtype=F32)
    for t in kept_taps(mask, B.shape[0]):
        At = gather_rows(A, src[t])
        for k0 in range(0, A.shape[1], 16):
            acc = (acc.double() + At[:, k0:k0 + 16] @ B[t][:, k0:k0 + 16].T).float()
    return acc


def nt_finish_emulation(acc, alpha, bias, cold):
    v = (acc.double() * alpha).float()
    if bias is not None:
        v = (v.double() + bias).float()
    if cold is not None:
        v = (v.double() + cold).float()
    return v


def tn_chunk(K, split):
    return ((((K + split - 1) // split) + TK_TN - 1) // TK_TN) * TK_TN


def tn_rows(src_t, K, rect):
    """reduction rows of one tap in kernel order: rectangle mode enumerates the in-range rows only."""
    return (src_t >= 0).nonzero().flatten() if rect else torch.arange(K)


def tn_products(A, B, src, mask):
    """C_tap = A^T @ B[src_tap] per kept tap (zeros elsewhere) and the same on magnitudes; A [K][M], B [rows][N]."""
    taps = src.shape[0]
    P = torch.zeros(taps, A.shape[1], B.shape[1], dtype=torch.float64)
    Q = torch.zeros_like(P)
    for t in kept_taps(mask, taps):
        Bt = gather_rows(B, src[t])
        P[t] = A.T @ Bt
        Q[t] = A.abs().T @ Bt.abs()
    return P, Q


def tn_emulate(A, B, src, mask, alpha, split, rect):
    """slices in order, each with an fp32 accumulator over 16-row steps, scaled by alpha; then the slice sum in fp32."""
    K = A.shape[0]
    chunk = tn_chunk(K, split)
    out = torch.zeros(src.shape[0], A.shape[1], B.shape[1], dtype=F32)
    for t in kept_taps(mask, src.shape[0]):
        rows = tn_rows(src[t], K, rect)
        Bt = gather_rows(B, src[t])
        total = None
        for r0 in range(0, max(int(rows.numel()), 1), chunk):
            rr = rows[r0:r0 + chunk]
            acc = torch.zeros(A.shape[1], B.shape[1], dtype=F32)
            for s in range(0, int(rr.numel()), 16):
                q = rr[s:s + 16]
                acc = (acc.double() + A[q].T @ Bt[q]).float()
            part = (acc.double() * alpha).float()
            total = part if total is None else (total.double() + part.double()).float()
        out[t] = total
    return out


def conv_fwd_ref(x, B, conv):
    """F.conv2d in float64: x [n][h][w][K], B [taps][N][K] -> [n*ho*wo][N]."""
    n, h, w, k, stride, pad, dil = conv
    wt = B.view(k, k, B.shape[1], B.shape[2]).permute(2, 3, 0, 1)
    y = F.conv2d(x.view(n, h, w, -1).permute(0, 3, 1, 2), wt, None, stride, pad, dil)
    return y.permute(0, 2, 3, 1).reshape(-1, B.shape[1])


def conv_dgrad_ref(dy, B, conv):
    """input gradient of F.conv2d by autograd in float64: dy [n][ho][wo][K = cout], B [taps][N = cin][K] -> [n*h*w][N]."""
    n, h, w, k, stride, pad, dil = conv
    ho, wo = conv_out(h, k, stride, pad, dil), conv_out(w, k, stride, pad, dil)
    wt = B.view(k, k, B.shape[1], B.shape[2]).permute(3, 2, 0, 1)
    x = torch.zeros(n, B.shape[1], h, w, dtype=torch.float64, requires_grad=True)
    y = F.conv2d(x, wt, None, stride, pad, dil)
    (dx,) = torch.autograd.grad(y, x, dy.view(n, ho, wo, -1).permute(0, 3, 1, 2))
    return dx.permute(0, 2, 3, 1).reshape(-1, B.shape[1])


def conv_wgrad_ref(dy, x, conv):
    """weight gradient of F.conv2d by autograd in float64: dy [n*ho*wo][M], x [n*h*w][N] -> [taps][M][N]."""
    n, h, w, k, stride, pad, dil = conv
    ho, wo = conv_out(h, k, stride, pad, dil), conv_out(w, k, stride, pad, dil)
    wt = torch.zeros(dy.shape[1], x.shape[1], k, k, dtype=torch.float64, requires_grad=True)
    y = F.conv2d(x.view(n, h, w, -1).permute(0, 3, 1, 2), wt, None, stride, pad, dil)
    (dw,) = torch.autograd.grad(y, wt, dy.view(n, ho, wo, -1).permute(0, 3, 1, 2))
    return dw.permute(2, 3, 0, 1).reshape(k * k, dy.shape[1], x.shape[1])


# ----------------------------------------------------------------------------------------
# which variant a call runs: the host formulas of glf_s16_gemm_nt / glf_s16_gemm_tn
# ----------------------------------------------------------------------------------------
def nt_variant(*, N, K, ldc, bsc=0, c_off=16, c_bf16=True, gather=0, geo=None, rect=0, taps=1, kept=1, env=None):
    force = int((os.environ if env is None else env).get("GLF_S16_TK", "0") or 0)
    bn = 64 if N <= 64 else 128
    tk32 = bn == 128 and ((force == 32) if force else rect != 2)
    tk = 32 if tk32 else 64
    wide = ldc % 8 == 0 and N % 8 == 0 and (c_off * (2 if c_bf16 else 4)) % 16 == 0 and bsc % 8 == 0
    census = bool(gather) and taps > 1 and not rect and TM < geo[4] * (geo[9] + 1)
    slow = gather == 2 and geo[7] > 1
    return {"kernel": f"s16_rows_kernel<{'true' if gather else 'false'}, {bn}, {tk}>", "bn": bn, "tk": tk, "wide": wide,
            "census": census, "slow_gather": slow, "region": rect == 2, "ntiles_max": kept * (K // tk)}


def tn_variant(*, M, N, K, split, gather=0, rect=0):
    chunk = tn_chunk(K, split)
    nvalid = min(split, (K + chunk - 1) // chunk)
    lanes = 0
    if split > 1:
        work, lanes = M * (N // 4), 1
        while lanes < 16 and lanes * 4 <= split and work * lanes < 65536:
            lanes *= 4
    return {"kernel": f"s16_tn_kernel<{'true' if gather else 'false'}>", "chunk": chunk, "nvalid": nvalid,
            "empty_slices": split - nvalid, "SL": lanes, "rect": rect, "k_tail": K % TK_TN}


# ----------------------------------------------------------------------------------------
# NaN-framed buffers
# ----------------------------------------------------------------------------------------
def _bits(t):
    return t.view(torch.int16 if t.dtype == BF else (torch.int64 if t.dtype == torch.float64 else torch.int32))


class Frame:
    """A logical tensor (dims, element strides) inside a larger 1-d buffer pre-filled with NaN: `off` elements in front, padding
    between rows / batches as the strides say, `tail` elements behind.  Everything is allocated at full size."""

    def __init__(self, dims, strides, dtype, off=16, tail=72):
        idx = torch.full(tuple(dims), off, dtype=torch.long)
        for ax, (n, s) in enumerate(zip(dims, strides)):
            shape = [1] * len(dims)
            shape[ax] = n
            idx = idx + (torch.arange(n) * s).view(shape)
        flat = idx.reshape(-1)
        assert flat.unique().numel() == flat.numel(), "overlapping layout"
        self.idx, self.off, self.dtype = idx, off, dtype
        self.host = torch.full((int(flat.max()) + 1 + tail,), float("nan"), dtype=dtype)
        self.dev = None

    def put(self, values):
        self.host[self.idx.reshape(-1)] = values.reshape(-1).to(self.dtype)
        return self

    def upload(self):
        self.dev = self.host.to(DEV)
        return self.dev[self.off:]

    def result(self, what="C"):
        """the logical tensor after the call; every buffer element outside it must have kept its bit pattern"""
        got = self.dev.cpu()
        outside = torch.ones(got.numel(), dtype=torch.bool)
        outside[self.idx.reshape(-1)] = False
        changed = (_bits(got) != _bits(self.host)) & outside
        assert not bool(changed.any()), (f"{what}: {int(changed.sum())} elements outside the logical tensor were overwritten, "
                                         f"first at buffer offset {int(changed.nonzero()[0])} (logical tensor starts at {self.off})")
        return got[self.idx]


def _sync():
    torch.cuda.synchronize()


def call16(mode, A, B, Cm, **kw):
    from glfusion_amd import ops16
    ops16.gemm16(mode, A, B, Cm, **kw)
    _sync()


# ----------------------------------------------------------------------------------------
# NT driver
# ----------------------------------------------------------------------------------------
def nt_spec(M=None, N=64, K=64, *, batch=1, bias=False, alpha=1.0, alpha_g=1.0 / 49, gather=0, conv=None, rect=0, lda=None, ldb=None,
            ldc=None, bsa=None, bsb=None, bsc=None, a_off=16, c_off=16, families=("dense", "gauss"), colstats=False,
            dtypes=(BF, F32), accumulates=(False, True), emulate=True, tap_mask=None):
    s = dict(locals())
    if gather:
        geo = geo_of(gather, conv)
        s["geo"], s["taps"] = geo, geo[5] * geo[6]
        s["M"] = geo[0] * geo[3] * geo[4]
        s["rows_a"] = geo[0] * geo[1] * geo[2]
    else:
        s["geo"], s["taps"], s["rows_a"] = None, 1, M
    s["lda"] = K + 8 if lda is None else lda
    s["ldb"] = K + 16 if ldb is None else ldb
    s["ldc"] = N + 8 if ldc is None else ldc
    s["tsb"] = N * s["ldb"] + 24 if gather else 0
    s["bsa"] = (s["rows_a"] * s["lda"] + 24 if bsa is None else bsa) if batch > 1 else 0
    s["bsb"] = (N * s["ldb"] + 40 if bsb is None else bsb) if batch > 1 else 0
    s["bsc"] = (s["M"] * s["ldc"] + 24 if bsc is None else bsc) if batch > 1 else 0
    return s


def nt_spec_variant(s, c_bf16=True, env=None):
    src = src_index(s["gather"], s["geo"]) if s["gather"] else None
    kept = bin(mask_of(src)).count("1") if s["gather"] else 1
    return nt_variant(N=s["N"], K=s["K"], ldc=s["ldc"], bsc=s["bsc"], c_off=s["c_off"], c_bf16=c_bf16, gather=s["gather"], geo=s["geo"],
                      rect=s["rect"], taps=s["taps"], kept=kept, env=env)


def run_nt(s, seed=1):
    M, N, K, batch, gather, conv, taps = s["M"], s["N"], s["K"], s["batch"], s["gather"], s["conv"], s["taps"]
    src = src_index(gather, s["geo"]) if gather else torch.arange(M).view(1, M)
    mask = mask_of(src) if gather else 1
    if s["tap_mask"] is not None:                  # a caller's mask: only some of the in-range taps are contracted
        mask &= s["tap_mask"]
    kept = bin(mask).count("1")
    n_terms = K * kept
    print(f"\n  NT M {M} N {N} K {K} batch {batch} gather {gather} conv {conv} rect {s['rect']} mask {mask:#x}: "
          f"{nt_spec_variant(s, True)}; fp32 C wide: {nt_spec_variant(s, False)['wide']}")
    for family in s["families"]:
        exact = family != "gauss"
        alpha = float(s["alpha"]) if exact else f32_alpha(s["alpha_g"])
        A = operand(family, (batch, s["rows_a"], K), seed, n_terms)
        B = operand(family, (batch, taps, N, K), seed + 1, n_terms)
        bias = None
        if s["bias"]:
            bias = dense_ints((N,), seed + 2, -8, 8) if exact else gauss((N,), seed + 2, dtype=F32)
        P, Q = zip(*(nt_products(A[b], B[b], src, mask) for b in range(batch)))
        P, Q = torch.stack(P), torch.stack(Q)
        if gather and batch == 1 and s["tap_mask"] is None:
            # the reference proper is F.conv2d (and its autograd) in float64; the index form gives the magnitudes and the emulation
            cref = (conv_fwd_ref if gather == 1 else conv_dgrad_ref)(A[0], B[0], conv)
            if exact:
                assert torch.equal(cref, P[0]), "F.conv2d reference and gather-index reference disagree on integers"
            P = cref.view(1, M, N)
        fa = Frame((batch, s["rows_a"], K), (s["bsa"], s["lda"], 1), BF, off=s["a_off"]).put(A)
        fb = Frame((batch, taps, N, K), (s["bsb"], s["tsb"], s["ldb"], 1), BF).put(B)
        dA, dB = fa.upload(), fb.upload()
        dbias = Frame((N,), (1,), F32, off=4, tail=12).put(bias).upload() if bias is not None else None
        emu_acc = None
        for cdt in s["dtypes"]:
            c_bf16 = cdt == BF
            for accumulate in s["accumulates"]:
                cold = None
                fc = Frame((batch, M, N), (s["bsc"], s["ldc"], 1), cdt, off=s["c_off"])
                if accumulate:
                    cold = dense_ints((batch, M, N), seed + 3, -64, 64) if exact else gauss((batch, M, N), seed + 3, dtype=cdt)
                    fc.put(cold)
                ref = alpha * P + (bias if bias is not None else 0.0) + (cold if cold is not None else 0.0)
                absref = abs(alpha) * Q + (bias.abs() if bias is not None else 0.0) + (cold.abs() if cold is not None else 0.0)
                what = f"nt {family} {'bf16' if c_bf16 else 'fp32'} C{' accumulate' if accumulate else ''}"
                stats = None
                if s["colstats"]:
                    if exact:
                        assert float(ref.abs().max()) <= 255, "ternary case leaves the exact range of the statistics"
                    start = dense_ints((2, N), seed + 4, 1, 9)
                    stats = start.to(DEV)
                if exact:
                    assert_exact_precondition(absref)
                call16("nt", dA, dB, fc.upload(), M=M, N=N, K=K, lda=s["lda"], ldb=s["ldb"], ldc=s["ldc"], bias=dbias, taps=taps, mask=mask,
                       tap_stride_b=s["tsb"], gather=gather, geo=s["geo"], batch=batch, bsa=s["bsa"], bsb=s["bsb"], bsc=s["bsc"],
                       alpha=alpha, accumulate=accumulate, rect=s["rect"], colstats=stats)
                got = fc.result(what)
                assert bool(torch.isfinite(got.float()).all()), what + ": non-finite element in the logical C"
                if exact:
                    gate_exact(got, ref, c_bf16, what)
                else:
                    gate_interval(got, ref, absref, n_terms, c_bf16, what)
                    if not c_bf16 and s["emulate"]:
                        if emu_acc is None:
                            emu_acc = [nt_emulate(A[b], B[b], src, mask) for b in range(batch)]
                        emu = torch.stack([nt_finish_emulation(emu_acc[b], alpha, bias, cold[b] if cold is not None else None)
                                           for b in range(batch)])
                        gate_emulation(got, emu, ref, what)
                if stats is not None:
                    # sums of the unrounded fp32 results alpha * acc + bias (what this call computed), added onto what was there
                    v = alpha * P[0] + (bias if bias is not None else 0.0)
                    want = start + torch.stack([v.sum(0), (v * v).sum(0)])
                    sgot = stats.cpu()
                    if exact:
                        assert torch.equal(sgot, want), f"{what}: column sums differ from float64 at {(sgot != want).nonzero()[:4].tolist()}"
                    else:
                        e0, e1 = rel_l2(sgot[0] - start[0], want[0] - start[0]), rel_l2(sgot[1] - start[1], want[1] - start[1])
                        print(f"    {what}: colstats relL2 {e0:.2e} {e1:.2e}")
                        assert e0 <= 1e-5 and e1 <= 1e-5


# plain NT: together M in {1, 37, 255, 256, 257, 517, 1100}, N in {8, 40, 64, 72, 128, 136, 260, 384}, K in {64, 128, 192, 512, 2048},
# lda > K, ldb > K, ldc > N (nt_spec defaults), batch in {1, 3} with gaps, alpha in {1, 0.5, -2}, with and without bias
NT_PLAIN = {
    "m1_n8_k64": nt_spec(1, 8, 64),
    "m37_n40_k128_b3": nt_spec(37, 40, 128, batch=3, bias=True, alpha=0.5),
    "m255_n64_k64": nt_spec(255, 64, 64, bias=True, alpha=-2.0),                  # one K-tile (BN 64, TK 64)
    "m256_n64_k128": nt_spec(256, 64, 128),                                       # two K-tiles
    "m256_n72_k192_b3": nt_spec(256, 72, 192, batch=3, alpha=0.5, alpha_g=1.0 / 196),
    "m257_n128_k64": nt_spec(257, 128, 64, bias=True),                            # two K-tiles at TK 32, one at TK 64
    "m517_n136_k512": nt_spec(517, 136, 512, bias=True, alpha=-2.0),
    "m1100_n260_k128": nt_spec(1100, 260, 128, ldc=272),                          # N % 8 != 0: narrow store; 4 | 2 K-tiles
    "m1100_n384_k2048": nt_spec(1100, 384, 2048, bias=True, alpha=0.5),
    "m517_n384_k192_b3": nt_spec(517, 384, 192, batch=3),
}
# the one-element-per-lane store loop, forced in each of its four ways
NT_NARROW = {
    "n5": nt_spec(300, 5, 128, ldc=16, bias=True),
    "n70": nt_spec(300, 70, 128, ldc=80, alpha=0.5),
    "ldc_odd_n64": nt_spec(300, 64, 128, ldc=67),
    "ldc_odd_n136": nt_spec(300, 136, 64, ldc=139, bias=True),
    "bsc_odd_b3": nt_spec(300, 72, 128, batch=3, bsc=300 * 80 + 4),
    "c_off_2": nt_spec(300, 136, 128, c_off=18, alpha=-2.0),
    "m257_n60": nt_spec(257, 60, 64, ldc=64, bias=True),                            # BN 64: one row past a tile, ragged columns
}
for _s in NT_NARROW.values():
    assert not nt_spec_variant(_s, True)["wide"] and not nt_spec_variant(_s, False)["wide"]
for _s in NT_PLAIN.values():
    assert nt_spec_variant(_s, True)["wide"] == nt_spec_variant(_s, False)["wide"] == (_s["N"] % 8 == 0)

# the attention-gradient call shapes of fusion16.Tpavi16Fn.backward (mode 'dot'), scaled down: n = 3 frames, L = 100, Ci = 64, C = 128
_AL, _ACI, _AC, _AN = 100, 64, 128, 3
_AC3 = 3 * _ACI
NT_ATTN = {
    # dth = dy @ M_n: A dense per batch, C the first Ci columns of dqkv [n L][3 Ci]
    "dtheta": nt_spec(_AL, _ACI, _ACI, batch=_AN, lda=_ACI, bsa=_AL * _ACI, ldb=_ACI, bsb=_ACI * _ACI, ldc=_AC3, bsc=_AL * _AC3, c_off=16),
    # dph = g @ dM / L: A the third column slice of qkv, C the second column slice of dqkv
    "dphi": nt_spec(_AL, _ACI, _ACI, batch=_AN, lda=_AC3, bsa=_AL * _AC3, a_off=16 + 2 * _ACI, ldb=_ACI, bsb=_ACI * _ACI, ldc=_AC3,
                    bsc=_AL * _AC3, c_off=16 + _ACI, alpha=0.5, alpha_g=1.0 / _AL),
    # dx += dqkv @ Wcat: accumulate with N = C
    "dx_accumulate": nt_spec(_AN * _AL, _AC, _AC3, lda=_AC3, ldb=_AC3, ldc=_AC, accumulates=(True,)),
}


@pytest.mark.parametrize("name", list(NT_PLAIN))
def test_nt_plain(name):
    run_nt(NT_PLAIN[name])


@pytest.mark.parametrize("name", list(NT_NARROW))
def test_nt_narrow_store(name):
    run_nt(NT_NARROW[name])


@pytest.mark.parametrize("name", list(NT_ATTN))
def test_nt_attention_gradient_shapes(name):
    run_nt(NT_ATTN[name])


# gathered NT, rect = 0, both gathers: conv = (n, h, w, k, stride, pad, dil).  13 x 17 with n = 3 gives 221 pixels per image: the
# 256-row tiles start in the middle of an image row and in the middle of an image.
NT_GATHER_CONVS = {
    "3x3_d1_13x17": dict(conv=(3, 13, 17, 3, 1, 1, 1), N=72, K=64),
    "3x3_d2_13x17": dict(conv=(3, 13, 17, 3, 1, 2, 2), N=64, K=128, bias=True),
    "3x3_d4_17x13": dict(conv=(3, 17, 13, 3, 1, 4, 4), N=136, K=64),
    "3x3_s2_9to5": dict(conv=(5, 9, 9, 3, 2, 1, 1), N=64, K=64),
    "3x3_s2_14to7": dict(conv=(3, 14, 14, 3, 2, 1, 1), N=72, K=64, bias=True),
    "3x3_s2_55to28": dict(conv=(2, 55, 55, 3, 2, 1, 1), N=64, K=64),
    "1x1_s2_14to7": dict(conv=(3, 14, 14, 1, 2, 0, 1), N=136, K=128),
    "3x3_d12_28x28_census": dict(conv=(2, 28, 28, 3, 1, 12, 12), N=64, K=64),
    "3x3_d4_60x72_census": dict(conv=(1, 60, 72, 3, 1, 4, 4), N=136, K=64),
    "3x3_d1_13x11_k2048": dict(conv=(2, 13, 11, 3, 1, 1, 1), N=136, K=2048, alpha=0.5, gathers=(1,)),   # 18 432 terms
    "3x3_d12_28x28_n1_census": dict(conv=(1, 28, 28, 3, 1, 12, 12), N=136, K=64),                       # 784 rows: a ragged last tile
    "3x3_s2_55to28_n1": dict(conv=(1, 55, 55, 3, 2, 1, 1), N=136, K=64, gathers=(2,)),                  # strided dgrad, 3025 rows
}
NT_GATHER = {f"g{g}_{k}": nt_spec(gather=g, **{a: b for a, b in v.items() if a != "gathers"})
             for k, v in NT_GATHER_CONVS.items() for g in v.get("gathers", (1, 2))}
# region mode (rect = 2: 3x3, stride 1, pad == dil, equal maps), both gathers, with bias and accumulate
NT_REGION_CONVS = {
    "d6_28x28": dict(conv=(2, 28, 28, 3, 1, 6, 6), N=64, K=64, bias=True),
    "d12_28x28": dict(conv=(2, 28, 28, 3, 1, 12, 12), N=136, K=64),
    "d24_28x28": dict(conv=(2, 28, 28, 3, 1, 24, 24), N=72, K=128, bias=True),
    "d6_13x17": dict(conv=(3, 13, 17, 3, 1, 6, 6), N=136, K=64, bias=True),       # regions narrower than one LDS-DMA instruction
    "d12_10x12_centre_only": dict(conv=(3, 10, 12, 3, 1, 12, 12), N=64, K=64),   # h, w <= dil: side regions empty
}
NT_REGION = {f"g{g}_{k}": nt_spec(gather=g, rect=2, **v) for k, v in NT_REGION_CONVS.items() for g in (1, 2)}
# a caller's tap mask under which the first corner region (y, x < 12) has no tap left: its rows are still stored (zeros plus bias),
# because this launch stores every element exactly once.  Forward gather: the corner reaches taps 4, 5, 7, 8; transposed: 0, 1, 3, 4.
NT_REGION["g1_d12_28x28_empty_region"] = nt_spec(gather=1, rect=2, conv=(1, 28, 28, 3, 1, 12, 12), N=136, K=64, bias=True, tap_mask=0x04F)
NT_REGION["g2_d12_28x28_empty_region"] = nt_spec(gather=2, rect=2, conv=(1, 28, 28, 3, 1, 12, 12), N=136, K=64, bias=True, tap_mask=0x1E4)


@pytest.mark.parametrize("name", list(NT_GATHER))
def test_nt_gather(name):
    run_nt(NT_GATHER[name])


@pytest.mark.parametrize("name", list(NT_REGION))
def test_nt_region(name):
    run_nt(NT_REGION[name])


# fused column statistics: ternary operands (exact), n_terms = 64, 2048, 576, 2304 and 18 432; one Gaussian case
_CS = dict(colstats=True, families=("ternary",), accumulates=(False,))
NT_COLSTATS = {
    "plain_k64": nt_spec(517, 40, 64, bias=True, **_CS),
    "plain_k2048": nt_spec(517, 136, 2048, **_CS),
    "g1_3x3_d2": nt_spec(gather=1, conv=(3, 13, 17, 3, 1, 2, 2), N=72, K=64, bias=True, **_CS),
    "g2_3x3_s2": nt_spec(gather=2, conv=(3, 14, 14, 3, 2, 1, 1), N=64, K=64, **_CS),
    "g1_3x3_d1_k2048": nt_spec(gather=1, conv=(2, 13, 11, 3, 1, 1, 1), N=136, K=2048, **_CS),
    "g1_region_d12_k256": nt_spec(gather=1, rect=2, conv=(2, 28, 28, 3, 1, 12, 12), N=136, K=256, bias=True, **_CS),
    "g2_region_d6": nt_spec(gather=2, rect=2, conv=(3, 13, 17, 3, 1, 6, 6), N=64, K=64, **_CS),
    "plain_gauss": nt_spec(517, 136, 512, bias=True, colstats=True, families=("gauss",), accumulates=(False,), alpha_g=1.0),
}


@pytest.mark.parametrize("name", list(NT_COLSTATS))
def test_nt_colstats(name):
    run_nt(NT_COLSTATS[name])


# ----------------------------------------------------------------------------------------
# TN driver
# ----------------------------------------------------------------------------------------
def tn_spec(K=None, M=64, N=64, *, split=1, batch=1, alpha=1.0, alpha_g=1.0 / 49, conv=None, rect=0, mask=None, families=("dense", "gauss"),
            dtypes=(BF, F32)):
    s = dict(locals())
    s["gather"] = 1 if conv is not None else 0
    if conv is not None:
        geo = geo_of(1, conv)
        s["geo"], s["taps"], s["K"], s["rows_b"] = geo, geo[5] * geo[6], geo[0] * geo[3] * geo[4], geo[0] * geo[1] * geo[2]
    else:
        s["geo"], s["taps"], s["rows_b"] = None, 1, K
    s["lda"], s["ldb"], s["ldc"] = M + 8, N + 16, N + 8
    s["tsb"] = M * s["ldc"] + 64 if conv is not None else 0
    s["bsa"] = s["K"] * s["lda"] + 24 if batch > 1 else 0
    s["bsb"] = s["rows_b"] * s["ldb"] + 40 if batch > 1 else 0
    s["bsc"] = M * s["ldc"] + 24 if batch > 1 else 0
    return s


def tn_spec_variant(s):
    return tn_variant(M=s["M"], N=s["N"], K=s["K"], split=s["split"], gather=s["gather"], rect=s["rect"])


def tn_direct(dA, dB, dC, s, mask, alpha, c_bf16, workspace, workspace_bytes=None):
    """glf_s16_gemm_tn through ctypes with a caller-made workspace (ops16.gemm16 always allocates its own)."""
    from glfusion_amd import ops
    from glfusion_amd._lib import GemmParams, lib
    p = GemmParams()
    p.M, p.N, p.K, p.lda, p.ldb, p.ldc = s["M"], s["N"], s["K"], s["lda"], s["ldb"], s["ldc"]
    p.taps, p.tap_mask, p.tap_stride_b, p.gather = s["taps"], mask, s["tsb"], s["gather"]
    (p.n_img, p.hs, p.ws, p.hd, p.wd, p.kh, p.kw, p.stride, p.pad, p.dil) = s["geo"] if s["geo"] is not None else (1, 1, 1, 1, 1, 1, 1, 1, 0, 1)
    p.batch, p.batch_stride_a, p.batch_stride_b, p.batch_stride_c = s["batch"], s["bsa"], s["bsb"], s["bsc"]
    p.alpha, p.accumulate, p.split, p.rect = alpha, 0, s["split"], s["rect"]
    p.c_dtype = 1 if c_bf16 else 0
    need = int(lib.glf_s16_gemm_tn_workspace_bytes(C.byref(p)))
    if workspace is not None:
        p.workspace, p.workspace_bytes = ops._p(workspace), need if workspace_bytes is None else workspace_bytes
    rc = lib.glf_s16_gemm_tn(ops._p(dA), ops._p(dB), ops._p(dC), C.byref(p), ops._stream())
    _sync()
    return rc, need


def run_tn(s, seed=11):
    M, N, K, batch, taps, conv, split, rect = s["M"], s["N"], s["K"], s["batch"], s["taps"], s["conv"], s["split"], s["rect"]
    src = src_index(1, s["geo"]) if conv is not None else torch.arange(K).view(1, K)
    true_mask = mask_of(src) if conv is not None else 1
    mask = true_mask if s["mask"] is None else s["mask"]
    assert mask & ~true_mask == 0
    live = kept_taps(mask, taps)
    n_terms = K
    print(f"\n  TN K {K} M {M} N {N} batch {batch} split {split} conv {conv} rect {rect} mask {mask:#x}: {tn_spec_variant(s)}")
    for family in s["families"]:
        exact = family != "gauss"
        alpha = float(s["alpha"]) if exact else f32_alpha(s["alpha_g"])
        A = operand(family, (batch, K, M), seed, n_terms)
        B = operand(family, (batch, s["rows_b"], N), seed + 1, n_terms)
        P, Q = zip(*(tn_products(A[b], B[b], src, mask) for b in range(batch)))
        P, Q = torch.stack(P), torch.stack(Q)                      # [batch][taps][M][N]
        if conv is not None:
            cref = conv_wgrad_ref(A[0], B[0], conv)
            if exact:
                assert torch.equal(cref[live], P[0][live]), "F.conv2d weight-gradient reference and gather-index reference disagree"
            P = P.clone()
            P[0][live] = cref[live]
        ref, absref = alpha * P[:, live], abs(alpha) * Q[:, live]
        if exact:
            assert_exact_precondition(absref)
        dA = Frame((batch, K, M), (s["bsa"], s["lda"], 1), BF).put(A).upload()
        dB = Frame((batch, s["rows_b"], N), (s["bsb"], s["ldb"], 1), BF).put(B).upload()
        emu = None
        for cdt in s["dtypes"]:
            c_bf16 = cdt == BF
            what = f"tn {family} {'bf16' if c_bf16 else 'fp32'} C"
            # only the slabs of the kept taps are logical C: the slabs of masked-out taps must stay untouched
            strides = (s["bsc"], s["tsb"], s["ldc"], 1)

            def c_frame():
                f = Frame((batch, taps, M, N), strides, cdt)
                f.idx = f.idx[:, live]
                return f
            fc = c_frame()
            call16("tn", dA, dB, fc.upload(), M=M, N=N, K=K, lda=s["lda"], ldb=s["ldb"], ldc=s["ldc"], taps=taps, mask=mask, tap_stride_b=s["tsb"],
                   gather=s["gather"], geo=s["geo"], batch=batch, bsa=s["bsa"], bsb=s["bsb"], bsc=s["bsc"], alpha=alpha, split=split, rect=rect)
            got = fc.result(what)
            assert bool(torch.isfinite(got.float()).all()), what + ": non-finite element in the logical C"
            if exact:
                gate_exact(got, ref, c_bf16, what)
            else:
                gate_interval(got, ref, absref, n_terms, c_bf16, what)
                if not c_bf16:
                    if emu is None:
                        emu = torch.stack([tn_emulate(A[b], B[b], src, mask, alpha, split, rect) for b in range(batch)])[:, live]
                    gate_emulation(got, emu, ref, what)
            if split > 1:
                # the reduction must read only slabs that a slice wrote: two workspaces pre-filled with different garbage
                for garbage in (float("nan"), 3.0e38):
                    f2 = c_frame()
                    rc, need = tn_direct(dA, dB, f2.upload(), s, mask, alpha, c_bf16, None)
                    assert rc == ERR_WORKSPACE
                    ws = torch.full((need // 4 + 64,), garbage, dtype=F32, device=DEV)
                    rc, _ = tn_direct(dA, dB, f2.upload(), s, mask, alpha, c_bf16, ws)
                    assert rc == 0
                    again = f2.result(what + " (garbage workspace)")
                    assert torch.equal(_bits(again), _bits(got)), f"{what}: result depends on the workspace's previous contents ({garbage})"
                    assert torch.equal(_bits(ws[need // 4:].cpu()), _bits(torch.full((64,), garbage, dtype=F32))), "workspace overrun"


# plain TN: K in {1, 63, 64, 65, 100, 1000, 4099}, M in {8, 64, 136, 256, 264}, N in {8, 64, 128, 200}, split in {1, 2, 3, 7, 16, 40},
# batch in {1, 3}.  Reduce variants (SL, from the `lanes` loop of glf_s16_gemm_tn) and empty trailing slices are asserted below.
TN_PLAIN = {
    "k1_m8_n8": tn_spec(1, 8, 8),
    "k63_m64_n64_s2_b3": tn_spec(63, 64, 64, split=2, batch=3, alpha=0.5),            # SL 1, second slice empty
    "k64_m136_n128": tn_spec(64, 136, 128, alpha=-2.0),
    "k65_m256_n200_s16": tn_spec(65, 256, 200, split=16),                              # SL 16, 14 of 16 slices empty
    "k100_m264_n8_s3": tn_spec(100, 264, 8, split=3, alpha=0.5),                       # SL 1, third slice empty
    "k1000_m264_n200_s7_b3": tn_spec(1000, 264, 200, split=7, batch=3, alpha_g=1.0 / 196),   # SL 4
    "k4099_m64_n64_s40": tn_spec(4099, 64, 64, split=40),                              # SL 16, 7 of 40 slices empty
    "k4099_m256_n128_s2": tn_spec(4099, 256, 128, split=2, alpha=-2.0),                # SL 1
    "k1000_m136_n64_b3": tn_spec(1000, 136, 64, batch=3),
}
assert [tn_spec_variant(TN_PLAIN[k])["SL"] for k in ("k63_m64_n64_s2_b3", "k65_m256_n200_s16", "k100_m264_n8_s3", "k1000_m264_n200_s7_b3",
                                                      "k4099_m64_n64_s40", "k4099_m256_n128_s2")] == [1, 16, 1, 4, 16, 1]
assert [tn_spec_variant(TN_PLAIN[k])["empty_slices"] for k in ("k63_m64_n64_s2_b3", "k65_m256_n200_s16", "k100_m264_n8_s3",
                                                                "k4099_m64_n64_s40")] == [1, 14, 1, 7]

# gathered TN (weight gradients): banded tile skipping (rect 0), per-tap rectangles (rect 1, split > 1), tap masks with holes
_CENTRE, _NO_CORNERS = 0x010, 0x0BA
TN_GATHER = {
    "band_d12": tn_spec(conv=(2, 28, 28, 3, 1, 12, 12), M=64, N=64),
    "band_d24_s3": tn_spec(conv=(2, 28, 28, 3, 1, 24, 24), M=136, N=64, split=3, alpha=0.5),
    "band_s2_55to28": tn_spec(conv=(1, 55, 55, 3, 2, 1, 1), M=64, N=72, split=2),
    "rect_d12_s4": tn_spec(conv=(2, 28, 28, 3, 1, 12, 12), M=64, N=136, split=4, rect=1),
    "rect_d24_s7": tn_spec(conv=(2, 28, 28, 3, 1, 24, 24), M=64, N=64, split=7, rect=1, alpha=-2.0),
    "rect_s2_14to7_s2": tn_spec(conv=(4, 14, 14, 3, 2, 1, 1), M=72, N=64, split=2, rect=1),
    "holes_centre_only": tn_spec(conv=(2, 13, 17, 3, 1, 2, 2), M=64, N=64, mask=_CENTRE),
    "holes_no_corners_s3": tn_spec(conv=(2, 13, 17, 3, 1, 2, 2), M=72, N=64, mask=_NO_CORNERS, split=3),
    "holes_no_corners_rect": tn_spec(conv=(2, 28, 28, 3, 1, 12, 12), M=64, N=64, mask=_NO_CORNERS, split=4, rect=1),
}


@pytest.mark.parametrize("name", list(TN_PLAIN))
def test_tn_plain(name):
    run_tn(TN_PLAIN[name])


@pytest.mark.parametrize("name", list(TN_GATHER))
def test_tn_gather(name):
    run_tn(TN_GATHER[name])


# ----------------------------------------------------------------------------------------
# both stage depths of the rows kernel
# ----------------------------------------------------------------------------------------
def test_stage_depths_in_child_processes():
    """GLF_S16_TK is read once per process: the whole NT matrix again with 64-deep stages (s16_rows_kernel<*, 128, 64>, otherwise
    unreachable without region mode) and with 32-deep stages forced (region mode on the TK = 32 kernels), each in one fresh child."""
    if os.environ.get(CHILD_MARK):
        return                                              # a child does not spawn children
    for tk in ("64", "32"):
        env = dict(os.environ, GLF_S16_TK=tk)
        env[CHILD_MARK] = "1"
        try:
            r = subprocess.run([sys.executable, "-m", "pytest", os.path.abspath(__file__), "-k", "nt", "-m", "gpu", "-q", "-x", "-p", "no:cacheprovider"],
                               cwd=ROOT, env=env, timeout=900, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
        except subprocess.TimeoutExpired as e:
            raise AssertionError(f"GLF_S16_TK={tk}: the child timed out; no further child is started\n{str(e.stdout)[-3000:]}")
        print(f"GLF_S16_TK={tk}: exit status {r.returncode}\n{r.stdout[-1500:]}")
        assert r.returncode == 0, f"GLF_S16_TK={tk}: child failed with status {r.returncode}; no further child is started\n{r.stdout[-6000:]}"
        assert " passed" in r.stdout and "skipped" not in r.stdout.splitlines()[-1]


# ----------------------------------------------------------------------------------------
# refusals: the documented status, and nothing launched (C keeps its NaN fill)
# ----------------------------------------------------------------------------------------
def _refused(mode, status, fragment, A, B, Cm, **kw):
    before = Cm.clone()
    with pytest.raises(RuntimeError, match=rf"status {status}\).*{fragment}"):
        call16(mode, A, B, Cm, **kw)
    _sync()
    assert torch.equal(_bits(Cm.cpu()), _bits(before.cpu())), "a refused call wrote to C"


def test_refusals():
    nan16 = lambda n: torch.full((n,), float("nan"), dtype=BF, device=DEV)
    A, B, Cm = torch.zeros(1 << 16, dtype=BF, device=DEV), torch.zeros(1 << 16, dtype=BF, device=DEV), nan16(1 << 16)
    Cf = torch.full((1 << 16,), float("nan"), dtype=F32, device=DEV)
    ok = dict(M=64, N=64, K=64, lda=64, ldb=64, ldc=64)
    conv3 = dict(taps=9, mask=0x1ff, tap_stride_b=64 * 64, gather=1)
    same = (1, 8, 8, 8, 8, 3, 3, 1, 1, 1)                       # 3x3 stride 1 pad 1 on 8 x 8: M = 64
    nt = lambda status, frag, a=A, **kw: _refused("nt", status, frag, a, B, Cm, **{**ok, **kw})
    tn = lambda status, frag, a=A, c=Cf, **kw: _refused("tn", status, frag, a, B, c, **{**ok, **kw})
    nt(ERR_UNSUPPORTED, "K must be a multiple of 64", K=96, lda=96, ldb=96)
    tn(ERR_UNSUPPORTED, "M and N must be multiples of 8", M=60)
    tn(ERR_UNSUPPORTED, "M and N must be multiples of 8", N=60)
    for mode in (nt, tn):
        mode(ERR_BAD_SHAPE, "multiples of 8 elements", lda=68)
        mode(ERR_BAD_SHAPE, "multiples of 8 elements", ldb=68)
        mode(ERR_BAD_SHAPE, "multiples of 8 elements", batch=2, bsa=4100, bsb=4096, bsc=4096)
        mode(ERR_BAD_SHAPE, "multiples of 8 elements", batch=2, bsa=4096, bsb=4100, bsc=4096)
        mode(ERR_BAD_SHAPE, "multiples of 8 elements", geo=same, **{**conv3, "tap_stride_b": 64 * 64 + 4})
        mode(ERR_BAD_SHAPE, "16-byte aligned", a=A[4:])
        mode(ERR_BAD_SHAPE, "tap_mask has bits beyond taps", geo=same, **{**conv3, "mask": 0x3ff})
    nt(ERR_UNSUPPORTED, "rect must be 0 or 2", geo=same, rect=1, **conv3)
    nt(ERR_UNSUPPORTED, "region mode needs", M=16, geo=(1, 8, 8, 4, 4, 3, 3, 2, 1, 1), rect=2, **conv3)       # stride 2
    nt(ERR_UNSUPPORTED, "region mode needs", geo=(1, 8, 8, 8, 8, 3, 3, 1, 2, 1), rect=2, **conv3)           # pad 2, dil 1
    stats = torch.zeros(2, 64, dtype=torch.float64, device=DEV)
    nt(ERR_UNSUPPORTED, "colstats needs batch 1", batch=2, bsa=4096, bsb=4096, bsc=4096, colstats=stats)
    tn(ERR_UNSUPPORTED, "colstats / accumulate", accumulate=True)
    tn(ERR_UNSUPPORTED, "colstats / accumulate", colstats=stats)
    assert float(stats.abs().sum()) == 0.0
    tn(ERR_UNSUPPORTED, "transposed gather", geo=same, **{**conv3, "gather": 2})
    tn(ERR_BAD_SHAPE, r"batch\*split too large", M=8, N=8, K=1 << 15, batch=2, split=40000)
    # split > 1 without a workspace, and with one a float short (ops16.gemm16 always brings its own: direct call)
    from glfusion_amd._lib import lib
    s = tn_spec(256, 64, 64, split=2)
    fa, fb = Frame((256, 64), (s["lda"], 1), BF).put(torch.zeros(256, 64)), Frame((256, 64), (s["ldb"], 1), BF).put(torch.zeros(256, 64))
    dA, dB = fa.upload(), fb.upload()
    before = Cf.clone()
    rc, need = tn_direct(dA, dB, Cf, s, 1, 1.0, False, None)
    assert rc == ERR_WORKSPACE and b"needs a workspace" in lib.glf_last_error() and need == 2 * 64 * 64 * 4
    ws = torch.zeros(need // 4, dtype=F32, device=DEV)
    rc, _ = tn_direct(dA, dB, Cf, s, 1, 1.0, False, ws, workspace_bytes=need - 4)
    assert rc == ERR_WORKSPACE and b"needs a workspace" in lib.glf_last_error()
    assert torch.equal(_bits(Cf.cpu()), _bits(before.cpu())), "a refused call wrote to C"
