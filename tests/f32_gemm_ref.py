"""Host side of tests/test_gpu_f32_gemm.py: the reference, the operand families, the case tables and the gates of the fp32-storage
contraction kernels (csrc/gemm_f32.hip, gemm_bf16s.hip, gemm_f16s.hip, gemm_f16s4.hip, gemm_rows_walk.h, gemm_tn_walk.h).  No GPU
code here; tests/test_f32_gemm_ref_cpu.py proves on the CPU that all of it has teeth.

The operand splits are emulated with IEEE element-wise torch operations, bit for bit: pow2_scale and split4h of csrc/split_f16.h
(x32 * s, .half(), the residual times 2048 in fp32, .half()) and split4 of csrc/gemm_bf16s.hip (three successive
round-to-nearest-even bf16 pieces of the fp32 residual).  From the pieces the IDEAL RESULT OF A PRECISION is evaluated in float64,
keeping exactly the products the kernels keep (PRODUCTS), summed over the kept taps and k:
    f32     a*b
    bf16x6  l*h, m*m, h*l, m*h, h*m, h*h                         (GLF_SIX)
    f16x3   (ha*hb + 2^-11 (ha*lb + la*hb)) / (sa*sb)
    f16     ha*hb / (sa*sb)
then alpha, bias or shift, residual, ReLU and the old C as the entry point defines them; `absref` is the same sum over the
magnitudes of the piece products plus |bias| + |residual| + |C_old|.  Only fp32 accumulation separates a correct kernel from
that ideal, so two gates judge every element (none is ever excluded):
  (a) integer operands chosen per precision (FAMILIES) so that every kept product and every partial sum is exact in fp32 in any
      order -- float atomics, the two-stage TN slab sum, the separate main and mixed accumulators of f16x3 folded by m * 2^-11:
      the result must EQUAL the reference.  The precondition is asserted first (exact_ratio): every term is a multiple of one
      power of two u (the product of the lowest set bits of the pieces), and sum |terms| / u < 2^24;
  (b) Gaussian operands, |got - ideal| <= (P n + 4) 2^-23 absref with P products per k and n = K x kept taps (TN: reduction rows
      plus the slices of the second stage): twice gamma_n at u = 2^-24, plus 4 for alpha, bias, accumulate and the double -> float
      step -- the convention of tests/test_gpu_s16_gemm.py, whose gate functions are used here by import.  The Gaussians are
      drawn so that every scaled fp16 piece is zero or normal (|x| >= 2^-10 amax, asserted), so the gate does not depend on the
      GPU's denormal mode; one separate case with elements down to 2^-27 amax adds one fp16 subnormal spacing per operand and
      term (2^-24 / s) to the bound;
  (c) CPU only: |ideal - float64| stays inside the models written in the kernel headers (3 * 2^-22 and 2^-22 times sum |a||b|).
Which kernel a case reaches is computed with the host formulas copied from the launchers (nt_variant / tn_variant).

Out of scope: the segmented region mode (nseg, glf_gemm_nt_seg_cols) and the colstats / colmax sums have their own tests."""
import math
import os

import torch

import test_gpu_s16_gemm as S16           # the shared gates, NaN-framed buffers and gather index arithmetic

F32, BF = torch.float32, torch.bfloat16
PRECISIONS = ("f32", "bf16x6", "f16x3", "f16")                 # ops.PRECISIONS order = the library's precision numbers 0..3
NPROD = {"f32": 1, "bf16x6": 6, "f16x3": 3, "f16": 1}
# (A piece, B piece, weight) of every product a precision keeps
PRODUCTS = {
    "f32": (("x", "x", 1.0),),
    "bf16x6": (("l", "h", 1.0), ("m", "m", 1.0), ("h", "l", 1.0), ("m", "h", 1.0), ("h", "m", 1.0), ("h", "h", 1.0)),
    "f16x3": (("h", "h", 1.0), ("h", "l", 2.0 ** -11), ("l", "h", 2.0 ** -11)),
    "f16": (("h", "h", 1.0),),
}
# integer operand families per precision (operand(), below); every precision also runs "gauss"
# (i13 is the one family with a non-zero DROPPED product, la * hb: the f16 ideal drops it as the kernel does, every kept term is
# still exact in fp32, and the result depends on how the split rounds A -- it pins round-to-nearest-even in integers.  Under f16x3
# no integer family can: with 13-bit A and an l piece in B, ha * hb and la * hb lie more than 24 bits apart.)
FAMILIES = {"f32": ("i32",), "bf16x6": ("a24b8", "a8b24", "a16b16"), "f16x3": ("a2b1", "a1b2"), "f16": ("i11", "i13")}
MODEL_BOUND = {"f16x3": 3 * 2.0 ** -22, "bf16x6": 2.0 ** -22}      # the claims of gemm_f16s.hip / gemm_bf16s.hip, times sum |a||b|
BK = 32                                                           # K tile of every fp32-storage kernel (gemm_common.h)

geo_of, src_index, mask_of, kept_taps, gather_rows = S16.geo_of, S16.src_index, S16.mask_of, S16.kept_taps, S16.gather_rows
f32_alpha, Frame, gate_exact, interval_violations = S16.f32_alpha, S16.Frame, S16.gate_exact, S16.interval_violations
assert_exact_precondition = S16.assert_exact_precondition


def popcount(m):
    return bin(m).count("1")


# ----------------------------------------------------------------------------------------
# the operand splits, bit for bit
# ----------------------------------------------------------------------------------------
def pow2_scale(amax):
    """split_f16.h: s with amax * s in [2^13, 2^14); no pointer, zero, denormal-range or non-finite amax: s = 1."""
    if amax is None:
        return 1.0
    e = (int(torch.tensor(float(amax), dtype=F32).view(torch.int32)) >> 23) & 0xff
    return 2.0 ** (140 - e) if 20 <= e <= 250 else 1.0


def f16_trunc(v32):
    """fp32 -> fp16 towards zero (normal fp16 range): a defect the gates must reject."""
    return (v32.contiguous().view(torch.int32) & ~0x1fff).view(F32).half().float()


def bf16_trunc(v32):
    return (v32.contiguous().view(torch.int32) & -65536).view(F32)


def split4h(x32, s, *, trunc=False, l_unscaled=False):
    """split_f16.h split4h: (h, l) as fp32 tensors holding fp16 values, x32 * s = h + 2^-11 l + e."""
    rnd = f16_trunc if trunc else (lambda v: v.half().float())
    xs = x32 * torch.tensor(s, dtype=F32)
    h = rnd(xs)
    r = xs - h
    return h, rnd(r if l_unscaled else r * torch.tensor(2048.0, dtype=F32))


def split4(x32, *, trunc=False):
    """gemm_bf16s.hip split4: (h, m, l) as fp32 tensors holding bf16 values."""
    rnd = bf16_trunc if trunc else (lambda v: v.to(BF).float())
    h = rnd(x32)
    r = x32 - h
    m = rnd(r)
    return h, m, rnd(r - m)


def pieces(x, prec, amax=None, **defect):
    """{piece name: float64 tensor} and the operand scale s of a float64 tensor of fp32 values."""
    x32 = x.float()
    assert torch.equal(x32.double(), x), "operand is not an fp32 value"
    if prec == "f32":
        return {"x": x}, 1.0
    if prec == "bf16x6":
        defect.pop("l_unscaled", None)
        return dict(zip("hml", (p.double() for p in split4(x32, **defect)))), 1.0
    s = pow2_scale(amax)
    return dict(zip("hl", (p.double() for p in split4h(x32, s, **defect)))), s


def packed_image(x, amax):
    """glf_split_f16_packed on the host: every aligned group of four fp32 elements -> {h0 h1 h2 h3 l0 l1 l2 l3} (fp16), returned
    as an fp32 tensor of the same shape holding those bits."""
    h, l = split4h(x.float(), pow2_scale(amax))
    g = x.shape[:-1] + (x.shape[-1] // 4, 4)
    return torch.cat([h.half().view(g), l.half().view(g)], -1).contiguous().view(F32).reshape(x.shape)


def pieces_normal(p, prec):
    """every fp16 piece zero or normal (bf16 pieces have fp32's exponent range)"""
    if prec not in ("f16x3", "f16"):
        return True
    return all(bool(((v == 0) | (v.abs() >= 2.0 ** -14)).all()) for v in p.values())


def lowbit(x):
    """the largest power of two that divides every non-zero element of a float64 tensor (inf for an all-zero one)"""
    x = x[x != 0]
    if x.numel() == 0:
        return math.inf
    m, e = torch.frexp(x)
    mi = (m.abs() * 2.0 ** 53).long()
    return float(((mi & -mi).double() * torch.pow(torch.tensor(2.0, dtype=torch.float64), (e - 53).double())).min())


# ----------------------------------------------------------------------------------------
# the contraction in float64
# ----------------------------------------------------------------------------------------
def contract(mode, A, B, src, mask):
    """nt: sum_t A[src_t] @ B_t^T, A [rows][K], B [taps][N][K] -> [M][N];  nn: sum_t A[src_t] @ B_t, B [taps][K][N];
    tn: C_t = A^T @ B[src_t] per kept tap, A [K][M], B [rows][N] -> [taps][M][N] (zeros for the other taps)."""
    taps = src.shape[0]
    if mode == "tn":
        out = torch.zeros(taps, A.shape[1], B.shape[1], dtype=torch.float64)
        for t in kept_taps(mask, taps):
            out[t] = A.T @ gather_rows(B, src[t])
        return out
    out = torch.zeros(src.shape[1], B.shape[1] if mode == "nt" else B.shape[2], dtype=torch.float64)
    for t in kept_taps(mask, taps):
        out += gather_rows(A, src[t]) @ (B[t].T if mode == "nt" else B[t])
    return out


def ideal(mode, A, B, src, mask, prec, amax_a=None, amax_b=None, *, drop=None, **defect):
    """(P, Q, unit): the ideal contraction of `prec` before alpha, the same over magnitudes, and the power of two every kept
    term is a multiple of.  drop = (A piece, B piece): that product left out; defect: trunc / l_unscaled (see split4h)."""
    pa, sa = pieces(A, prec, amax_a, **defect)
    pb, sb = pieces(B, prec, amax_b, **defect)
    P = Q = None
    unit = math.inf
    for na, nb, w in PRODUCTS[prec]:
        if (na, nb) == drop:
            continue
        p, q = w * contract(mode, pa[na], pb[nb], src, mask), w * contract(mode, pa[na].abs(), pb[nb].abs(), src, mask)
        P, Q = (p, q) if P is None else (P + p, Q + q)
        unit = min(unit, w * lowbit(pa[na]) * lowbit(pb[nb]))
    return P / (sa * sb), Q / (sa * sb), unit / (sa * sb)


def finish(P, Q, alpha, bias=None, res=None, relu=False, cold=None):
    """alpha, bias / shift, residual, ReLU, then the old C: the order of the store epilogues (gemm_rows_walk.h)."""
    ref, absref = alpha * P, abs(alpha) * Q
    for extra in (bias, res):
        if extra is not None:
            ref, absref = ref + extra, absref + extra.abs()
    if relu:
        ref = ref.clamp_min(0.0)
    if cold is not None:
        ref, absref = ref + cold, absref + cold.abs()
    return ref, absref


def exact_ratio(absref, unit, *others):
    """sum |terms| in units of the power of two that divides every term and every addend"""
    for o in others:
        if o is not None:
            unit = min(unit, lowbit(o))
    return absref / unit


def gate_interval(got, ref, absref, n_terms, what, extra=None):
    """S16.gate_interval's bound d = (n_terms + 4) 2^-23 absref, optionally plus an absolute term per element (`extra`, the
    subnormal case): the shared gate is called with absref raised by extra / ((n_terms + 4) 2^-23).  Returns max |got - ref| / d."""
    if extra is not None:
        absref = absref + extra / ((n_terms + 4) * 2.0 ** -23)
    bad, worst = interval_violations(got, ref, absref, n_terms, False)
    S16.gate_interval(got, ref, absref, n_terms, False, what)
    return worst


def close_old(a, b, tol=5e-5):
    """the elementwise gate of test_gpu_ops.py / test_gpu_rows_walk.py / test_gpu_tn_walk.py that this module tightens"""
    err = (a.double() - b.double()).abs()
    return bool((err <= tol + tol * b.double().abs()).all())


# ----------------------------------------------------------------------------------------
# operand families
# ----------------------------------------------------------------------------------------
def _gen(seed):
    return torch.Generator(device="cpu").manual_seed(seed)


def _tern(shape, seed, n_terms, thin=4):
    """sparse ternary digits, density sqrt(96 / thin / n_terms) at most 0.5 (S16.ternary's rule at 1 / sqrt(thin) of its density):
    about 96 / thin non-zero digit pairs per output element whatever the reduction length"""
    return S16.ternary(shape, seed, thin * n_terms)


def _digits(shape, seed, n_terms, spacing, levels):
    # spacing 512 (bf16 pieces: terms up to 2^18 in units of 1): a twelfth of S16.ternary's pairs keeps the sums below 2^23
    return sum(_tern(shape, seed + 101 * j, n_terms, 12 if spacing == 512 else 4) * float(spacing) ** j for j in range(levels))


def gauss(shape, seed):
    """N(0, 1) in fp32 with every |x| >= 2^-10 max |x| (smaller draws are redrawn)"""
    g = _gen(seed)
    x = torch.randn(tuple(shape), generator=g)
    for _ in range(64):
        small = x.abs() < x.abs().max() * 2.0 ** -10
        if not bool(small.any()):
            return x.double()
        x[small] = torch.randn(int(small.sum()), generator=g)
    raise AssertionError("gauss: could not clear the small draws")


def operand(family, side, shape, seed, n_terms):
    """float64 tensor of fp32 values.  Integer families (side 'a' / 'b'):
    i32     dense integers in [-15, 15] on both sides
    a24b8   A = d2 2^18 + d1 2^9 + d0 (three bf16 pieces), B one ternary digit; a8b24 the reverse
    a16b16  d1 2^9 + d0 on both sides (two pieces each)
    a2b1    A = p 2^11 + q (two fp16 pieces), B one ternary digit; a1b2 the reverse
    i11     dense integers in [-7, 7] on both sides (one fp16 piece)
    i13     A = p 2^12 + q with q in [-7, 7] (13 bits: h is rounded), B one ternary digit"""
    if family == "gauss":
        return gauss(shape, seed)
    if family == "i32":
        return S16.dense_ints(shape, seed, -15, 15)
    if family == "i11":
        return S16.dense_ints(shape, seed, -7, 7)
    if family == "i13":
        if side == "b":
            return _tern(shape, seed, n_terms)
        q = S16.dense_ints(shape, seed + 17, -7, 7)
        return _tern(shape, seed, n_terms) * 4096.0 + torch.where(_tern(shape, seed + 29, n_terms) != 0, q, torch.zeros(()).double())
    levels, spacing = {"a24b8": ((3, 1), 512), "a8b24": ((1, 3), 512), "a16b16": ((2, 2), 512), "a2b1": ((2, 1), 2048), "a1b2": ((1, 2), 2048)}[family]
    return _digits(shape, seed, n_terms, spacing, levels[0 if side == "a" else 1])


# ----------------------------------------------------------------------------------------
# cases
# ----------------------------------------------------------------------------------------
def rows_case(M=None, N=64, K=32, *, mode="nt", batch=1, bias=False, alpha=1.0, accumulate=False, gather=0, conv=None, rect=0, tap_mask=None,
              lda=None, ldb=None, ldc=None, a_off=16, b_off=16, c_off=16, pa=False, pb=False, epi=None, amax=None, amax_c=False,
              precs=PRECISIONS):
    """An NT / NN call.  conv = (n, h, w, k, stride, pad, dil) with gather; epi = (ld_res or None for no residual, relu);
    amax: 'self' (measured by the library), 'exact' or 'loose' (8x; device scalars from the caller)."""
    c = dict(locals())
    if gather:
        geo = geo_of(gather, conv)
        c.update(geo=geo, taps=geo[5] * geo[6], M=geo[0] * geo[3] * geo[4], rows_a=geo[0] * geo[1] * geo[2])
        src = src_index(gather, geo)
        c["mask"] = mask_of(src) & (0xffffffff if tap_mask is None else tap_mask)
    else:
        c.update(geo=None, taps=1, rows_a=M, mask=1)
    c["kept"] = popcount(c["mask"])
    rows_b, cols_b = (N, K) if mode == "nt" else (K, N)
    c["b_dims"] = (rows_b, cols_b)
    c["lda"] = K + 8 if lda is None else lda
    c["ldb"] = cols_b + 12 if ldb is None else ldb
    c["ldc"] = N + 8 if ldc is None else ldc
    c["tsb"] = rows_b * c["ldb"] + 24 if gather else 0
    c["bsa"] = c["rows_a"] * c["lda"] + 24 if batch > 1 else 0
    c["bsb"] = rows_b * c["ldb"] + 40 if batch > 1 else 0
    c["bsc"] = c["M"] * c["ldc"] + 24 if batch > 1 else 0
    c["amax"] = amax or ("exact" if (pa or pb) else "self")
    c["n"] = K * c["kept"]
    return c


def tn_case(K=None, M=64, N=64, *, split=1, batch=1, alpha=1.0, accumulate=False, conv=None, rect=0, tap_mask=None, oihw=False, foreign=None,
            pa=False, pb=False, amax=None, precs=PRECISIONS):
    """A TN call: A [K][M], B [rows][N] (gathered with conv), C_tap [M][N]; foreign = the tap copied from another buffer (oihw)."""
    c = dict(locals(), mode="tn", bias=False, epi=None, amax_c=False, a_off=16, b_off=16, c_off=16)
    c["gather"] = 1 if conv is not None else 0
    if conv is not None:
        geo = geo_of(1, conv)
        c.update(geo=geo, taps=geo[5] * geo[6], K=geo[0] * geo[3] * geo[4], rows_b=geo[0] * geo[1] * geo[2])
        c["mask"] = mask_of(src_index(1, geo)) & (0xffffffff if tap_mask is None else tap_mask)
    else:
        c.update(geo=None, taps=1, rows_b=K, mask=1)
    c["kept"] = popcount(c["mask"])
    c["lda"], c["ldb"], c["ldc"] = M + 8, N + 12, N + 8
    c["tsb"] = M * c["ldc"] + 64 if conv is not None else 0
    c["bsa"] = c["K"] * c["lda"] + 24 if batch > 1 else 0
    c["bsb"] = c["rows_b"] * c["ldb"] + 40 if batch > 1 else 0
    c["bsc"] = M * c["ldc"] + 24 if batch > 1 else 0
    c["amax"] = amax or ("exact" if (pa or pb) else "self")
    c["n"] = c["K"] + (split if (split > 1 or oihw) else 0)
    return c


def case_src(c):
    if c["gather"]:
        return src_index(c["gather"], c["geo"])
    return torch.arange(c["K"] if c["mode"] == "tn" else c["M"]).view(1, -1)


# ----------------------------------------------------------------------------------------
# which kernel a call reaches: the host formulas of glf_gemm_nt / _nn / _tn and their launchers
# ----------------------------------------------------------------------------------------
def _f16s4_mode():
    return int(os.environ.get("GLF_F16S4", "1") or 1)


def rows_variant(c, prec):
    """{'kernel', 'arith' (the precision whose arithmetic the kernel evaluates), ...} of an NT / NN case."""
    pi = PRECISIONS.index(prec)
    G = "true" if c["gather"] else "false"
    vec_a = c["a_off"] % 4 == 0 and c["lda"] % 4 == 0 and c["bsa"] % 4 == 0
    vec_b = c["b_off"] % 4 == 0 and c["ldb"] % 4 == 0 and c["bsb"] % 4 == 0 and c["tsb"] % 4 == 0
    M, N, K = c["M"], c["N"], c["K"]
    v = dict(vec_a=vec_a, vec_b=vec_b, k_tail=K % BK, skinny=False, use_f16s4=False)
    if c["mode"] == "nn":
        return dict(v, kernel=f"gemm_rows_kernel<1, {G}>", arith="f32", bf16s_rows_ok=False, f16s_rows_ok=False)
    rows_ok = vec_a and vec_b and K % BK == 0 and K >= BK
    v.update(bf16s_rows_ok=rows_ok, f16s_rows_ok=rows_ok and K <= (1 << 18))
    v["skinny"] = (c["epi"] is None and M <= 64 and not c["gather"] and c["taps"] == 1 and c["batch"] == 1 and not c["rect"] and not c["pa"]
                   and not c["pb"] and vec_a and vec_b and K % 16 == 0 and N >= 64)
    if v["skinny"]:
        return dict(v, kernel="gemm_skinny_nt_kernel", arith="f32")
    if pi == 1 and rows_ok:
        return dict(v, kernel=f"gemm_rows_bf16s8_kernel<{G}>", arith="bf16x6")
    if pi >= 2 and v["f16s_rows_ok"]:
        mode = _f16s4_mode()
        v["use_f16s4"] = mode == 2 or (mode != 0 and K * c["kept"] <= 256)
        np_ = 3 if pi == 2 else 1
        flags = f"{G}, {np_}, pa={int(c['pa'])}, pb={int(c['pb'])}, epi={int(c['epi'] is not None)}"
        wide_store = c["rect"] != 1 and c["ldc"] % 4 == 0 and N % 4 == 0 and c["c_off"] % 4 == 0 and c["bsc"] % 4 == 0
        return dict(v, kernel=("gemm_rows_f16s4_kernel<" if v["use_f16s4"] else "gemm_rows_f16s8_kernel<") + flags + ">", arith=prec,
                    wide_store=wide_store)
    assert c["epi"] is None and c["rect"] != 2 and not c["pa"] and not c["pb"], "the case would be refused by the launcher"
    return dict(v, kernel=f"gemm_rows_kernel<0, {G}>", arith="f32")


def tn_chunk(K, split):
    return (((K + split - 1) // split + BK - 1) // BK) * BK


def tn_tap_rows(c, tap):
    """reduction rows of a tap: K, or in rect mode the pixels of tap_rect() (stride 1)"""
    if not c["rect"]:
        return c["K"]
    n_img, hs, ws, hd, wd, kh, kw, stride, pad, dil = c["geo"]
    ky, kx = divmod(tap, kw)
    oy, ox = pad - ky * dil, pad - kx * dil
    y0, y1 = max(oy, 0), min(hs + oy, hd)
    x0, x1 = max(ox, 0), min(ws + ox, wd)
    return n_img * max(y1 - y0, 0) * max(x1 - x0, 0)


def tn_variant(c, prec):
    pi = PRECISIONS.index(prec)
    G = "true" if c["gather"] else "false"
    M, N, K, split = c["M"], c["N"], c["K"], c["split"]
    vec_a = c["lda"] % 4 == 0 and c["bsa"] % 4 == 0
    vec_b = c["ldb"] % 4 == 0 and c["bsb"] % 4 == 0
    tn_ok = vec_a and vec_b and M % 4 == 0 and N % 4 == 0 and M >= 4 and N >= 4
    small = (M <= 64 or N <= 64) and M <= 256 and N <= 256
    wide = not small and M > 128
    v = dict(f16s_tn_ok=tn_ok, small=False, wide=False, lanes=0, second_vec=None)
    if pi == 1 and tn_ok:
        v.update(kernel=f"gemm_tn_bf16s_kernel<{G}>", arith="bf16x6")
    elif pi >= 2 and tn_ok:
        tile = "f16s8_kernel" if wide else "f16s_kernel"
        v.update(kernel=f"gemm_tn_{tile}<{G}, {3 if pi == 2 else 1}, pa={int(c['pa'])}, pb={int(c['pb'])}{', small' if small else ''}>",
                 arith=prec, small=small, wide=wide)
    else:
        assert not c["pa"] and not c["pb"], "the case would be refused by the launcher"
        v.update(kernel=f"gemm_tn_kernel<{G}>", arith="f32")
    chunk = tn_chunk(K, split)
    nvalid = {t: min(split, (tn_tap_rows(c, t) + chunk - 1) // chunk) for t in kept_taps(c["mask"], c["taps"])}
    v.update(chunk=chunk, empty_slices=max(split - n for n in nvalid.values()) if nvalid else 0)
    if split > 1 or c["oihw"]:
        vec = c["oihw"] or (N % 4 == 0 and c["ldc"] % 4 == 0 and c["c_off"] % 4 == 0 and c["tsb"] % 4 == 0 and c["bsc"] % 4 == 0)
        work, lanes = (M * (N // 4) if vec else M * N), 1
        while vec and lanes < 16 and lanes * 4 <= split and work * lanes < 65536:
            lanes *= 4
        v.update(lanes=lanes, second_vec=bool(vec), second="tn_reduce_oihw_kernel" if c["oihw"] else ("tn_reduce_kernel" if lanes == 1 else "tn_reduce_lanes_kernel"))
    return v


def variant(c, prec):
    return tn_variant(c, prec) if c["mode"] == "tn" else rows_variant(c, prec)


# ----------------------------------------------------------------------------------------
# the data and the reference of one (case, arithmetic, family)
# ----------------------------------------------------------------------------------------
def make_data(c, arith, family, seed=1, *, subnormal=False):
    """Everything a run needs, as float64 host tensors: A [batch][rows][cols], B ([batch][taps][N][K] / [taps][K][N]; TN: [batch][rows][N]),
    bias / res / cold or None, alpha, amax_a / amax_b (the values the kernel scales with), ref and absref of the logical C
    ([batch][M][N]; TN: [batch][taps][M][N], oihw included), n_terms = P n, and for an integer family the exactness ratio.
    The CPU-side preconditions of the gates are asserted here."""
    exact = family != "gauss"
    mode, batch, taps, M, N, K = c["mode"], c["batch"], c["taps"], c["M"], c["N"], c["K"]
    n = c["n"]
    src = case_src(c)
    mask = c["mask"]
    if mode == "tn":
        a_shape, b_shape = (batch, K, M), (batch, c["rows_b"], N)
    else:
        a_shape, b_shape = (batch, c["rows_a"], K), (batch, taps) + c["b_dims"]
    A, B = operand(family, "a", a_shape, seed, n), operand(family, "b", b_shape, seed + 1, n)
    if subnormal:
        # every fourth element becomes +-4 * 2^-u, u uniform in [0, 27): h stays normal (|x s| > 2^-14), l may be subnormal or zero
        for X, sd in ((A, seed + 7), (B, seed + 8)):
            u = torch.rand(X.shape, generator=_gen(sd), dtype=torch.float64) * 27.0
            low = torch.rand(X.shape, generator=_gen(sd + 50)) < 0.25
            X.copy_(torch.where(low, X.sign() * 4.0 * torch.pow(torch.tensor(2.0, dtype=torch.float64), -u), X.clamp(-4.0, 4.0)))
            X.view(-1)[0] = 4.0                                          # the maximum itself
        A, B = A.float().double(), B.float().double()
    alpha = float(c["alpha"]) if exact else f32_alpha(c["alpha"] / 7.0)
    d = dict(A=A, B=B, alpha=alpha, exact=exact, n_terms=NPROD[arith] * n, src=src, mask=mask, bias=None, res=None, cold=None, relu=False, extra=None)
    # the maxima the kernels scale with: measured over exactly the elements the call can read (self_amax), or given by the caller
    live_b = B if mode == "tn" else B[:, kept_taps(mask, taps)]
    loose = 8.0 if c["amax"] == "loose" else 1.0
    d["amax_a"], d["amax_b"] = (float(A.abs().max()) * loose, float(live_b.abs().max()) * loose) if arith in ("f16x3", "f16") else (None, None)
    small = lambda shape, sd, lo, hi: S16.dense_ints(shape, sd, lo, hi) if exact else gauss(shape, sd)
    if c["bias"] or c["epi"] is not None:
        d["bias"] = small((N,), seed + 2, -8, 8)
    if c["epi"] is not None:
        d["relu"] = bool(c["epi"][1])
        if c["epi"][0] is not None:
            d["res"] = small((batch, M, N), seed + 4, -16, 16)
    c_shape = (batch, taps, M, N) if mode == "tn" else (batch, M, N)
    if c["accumulate"]:
        d["cold"] = small(c_shape, seed + 3, -64, 64)
    if mode == "tn" and c["foreign"] is not None:
        d["foreign"] = small((M, N), seed + 5, -32, 32)
    P, Q, unit = zip(*(ideal(mode, A[b], B[b], src, mask, arith, d["amax_a"], d["amax_b"]) for b in range(batch)))
    P, Q, unit = torch.stack(P), torch.stack(Q), min(unit)
    d["P"], d["Q"] = P, Q
    ref, absref = finish(P, Q, alpha, d["bias"], d["res"], d["relu"], d["cold"])
    if mode == "tn" and c["foreign"] is not None:
        t = c["foreign"]
        ref[0, t] = ref[0, t] + d["foreign"]
        absref[0, t] = absref[0, t] + d["foreign"].abs()
    d["ref"], d["absref"] = ref, absref
    pa, sa = pieces(A, arith, d["amax_a"])
    pb, sb = pieces(live_b, arith, d["amax_b"])
    if subnormal:
        assert arith in ("f16x3", "f16")
        assert bool(((pa["h"] == 0) | (pa["h"].abs() >= 2.0 ** -14)).all()) and bool(((pb["h"] == 0) | (pb["h"].abs() >= 2.0 ** -14)).all())
        assert not pieces_normal(pa, arith) or not pieces_normal(pb, arith), "the subnormal case has no subnormal piece"
        # one fp16 subnormal spacing per operand and term: da = 2^-24 / sa on every a, db = 2^-24 / sb on every b
        da, db = 2.0 ** -24 / sa, 2.0 ** -24 / sb
        ones_a, ones_b = torch.ones_like(A[0]), torch.ones_like(B[0])
        d["extra"] = abs(alpha) * torch.stack([da * contract(mode, ones_a, B[b].abs(), src, mask) + db * contract(mode, A[b].abs(), ones_b, src, mask)
                                               + da * db * contract(mode, ones_a, ones_b, src, mask) for b in range(batch)])
    else:
        assert pieces_normal(pa, arith) and pieces_normal(pb, arith), f"{family}: an fp16 piece is subnormal"
    if exact:
        d["ratio"] = exact_ratio(absref, abs(alpha) * unit, d["bias"], d["res"], d["cold"], d.get("foreign"))
        assert_exact_precondition(d["ratio"])
        assert torch.equal(ref.float().double(), ref)
    return d


def piece_coverage(c, arith, family, seed=1):
    """{(A piece, B piece): max over the output of sum |A piece| |B piece|} for every pair of pieces of one integer family"""
    d = make_data(c, arith, family, seed)
    pa, _ = pieces(d["A"][0], arith, d["amax_a"])
    pb, _ = pieces(d["B"][0], arith, d["amax_b"])
    return {(na, nb): float(contract(c["mode"], pa[na].abs(), pb[nb].abs(), d["src"], d["mask"]).max()) for na in pa for nb in pb}


# ----------------------------------------------------------------------------------------
# case tables: the smallest shapes that reach each code path (nothing beyond about 520 x 264 x 320)
# ----------------------------------------------------------------------------------------
SPLIT16 = ("f16x3", "f16")
NO_CENTRE = 0x1EF                      # 3x3 with a hole: 8 taps x K = 32 = 256 -> the 4-wave kernel
_D12, _D24 = (1, 28, 28, 3, 1, 12, 12), (1, 28, 28, 3, 1, 24, 24)
_S1, _S2 = (2, 13, 17, 3, 1, 1, 1), (1, 55, 55, 3, 2, 1, 1)
_D12_3, _S2_2 = (3, 28, 20, 3, 1, 12, 12), (2, 23, 23, 3, 2, 1, 1)

NT_CASES = {
    # geometry, under every precision: K = 32 -> bf16x6 8-wave / split-fp16 4-wave, K = 288 -> 8-wave; f32 -> the exact rows kernel
    "m129_n132_k32": rows_case(129, 132, 32),                                           # one row past a 128-row tile, wide store, ragged column tile
    "m257_n70_k288": rows_case(257, 70, 288),                                           # one row past a 256-row tile, one-dword store
    "m127_n4_k32_alpha_bias": rows_case(127, 4, 32, alpha=0.5, bias=True),
    "m255_n132_k288_acc": rows_case(255, 132, 288, accumulate=True, bias=True),
    "m257_n132_k32": rows_case(257, 132, 32, bias=True),
    "m129_n70_k32_b3": rows_case(129, 70, 32, batch=3, bias=True, alpha=0.5),           # batches with gaps
    "m129_n72_k288_b3_acc": rows_case(129, 72, 288, batch=3, accumulate=True),
    # unaligned K: every precision falls back to the exact kernel; lda % 4 == 0 with K % 4 != 0 is its vector path with a tail
    "m129_n70_k33": rows_case(129, 70, 33, lda=40, ldb=44, bias=True),
    "m127_n132_k52": rows_case(127, 132, 52, lda=56, ldb=60, alpha=0.5, bias=True, accumulate=True),
    # misaligned layouts: every precision on the exact kernel's scalar loads
    "odd_lda": rows_case(129, 70, 32, lda=41, ldb=45),
    "base_plus_one_float": rows_case(129, 72, 32, a_off=17, b_off=17),
    # skinny
    "skinny_m1_k16": rows_case(1, 64, 16),
    "skinny_m61_n67_k48": rows_case(61, 67, 48, alpha=0.5, bias=True, accumulate=True, amax_c=True),
    "m129_n132_k288_amax_c": rows_case(129, 132, 288, bias=True, amax_c=True, precs=SPLIT16),
    # gathers of a 3x3 conv, stride 1 and stride 2 (55 -> 28), both directions; a tap mask with holes
    "g1_s1": rows_case(gather=1, conv=_S1, N=72, K=32, bias=True),
    "g2_s1": rows_case(gather=2, conv=_S1, N=72, K=32),
    "g1_s1_holes": rows_case(gather=1, conv=_S1, N=72, K=32, tap_mask=NO_CENTRE),
    "g2_s1_holes_acc": rows_case(gather=2, conv=_S1, N=70, K=32, tap_mask=0x0BA, accumulate=True),
    "g1_s2_55to28": rows_case(gather=1, conv=_S2, N=72, K=32, alpha=0.5),
    "g2_s2_55to28": rows_case(gather=2, conv=_S2, N=72, K=32, tap_mask=NO_CENTRE),
    "g1_s1_k64": rows_case(gather=1, conv=_S1, N=132, K=64),
    # pad = dil = 12 / 24 on 28 x 28: rect 0 (tap census), 1 (per-tap rectangles, float atomics into a zero-filled C), 2 (regions)
    "g1_d12_rect0": rows_case(gather=1, conv=_D12, N=72, K=32),
    "g2_d12_rect0": rows_case(gather=2, conv=_D12, N=72, K=64, tap_mask=NO_CENTRE),
    "g1_d24_rect0": rows_case(gather=1, conv=_D24, N=72, K=32, bias=True),
    "g1_d12_rect1": rows_case(gather=1, conv=_D12, N=72, K=32, rect=1),
    "g2_d12_rect1": rows_case(gather=2, conv=_D12, N=70, K=64, rect=1, tap_mask=NO_CENTRE),
    "g1_d24_rect1": rows_case(gather=1, conv=_D24, N=72, K=32, rect=1, alpha=0.5),
    "g2_d24_rect1": rows_case(gather=2, conv=_D24, N=72, K=32, rect=1),
    "g1_d12_rect2": rows_case(gather=1, conv=_D12, N=72, K=32, rect=2, bias=True, precs=SPLIT16),
    "g2_d12_rect2_acc": rows_case(gather=2, conv=_D12, N=70, K=64, rect=2, accumulate=True, precs=SPLIT16),
    "g1_d24_rect2": rows_case(gather=1, conv=_D24, N=72, K=32, rect=2, precs=SPLIT16),
    "g2_d24_rect2": rows_case(gather=2, conv=_D24, N=72, K=32, rect=2, bias=True, alpha=0.5, precs=SPLIT16),
    # three images of a non-square map: a thread's rows (32 or 64 apart) wrap several lines of a rectangle and cross images.
    # rect 1: the corner taps have 16 x 8 rectangles = 384 rows (three full 128-row tiles; one full and one ragged 256-row tile),
    # the centre tap 1 680 rows (ragged in both tile heights); rect 0: the census runs on tiles that straddle two images
    "g1_3img_d12_rect1": rows_case(gather=1, conv=_D12_3, N=72, K=32, rect=1),
    "g2_3img_d12_rect1": rows_case(gather=2, conv=_D12_3, N=72, K=32, rect=1),
    "g1_3img_d12_rect0": rows_case(gather=1, conv=_D12_3, N=72, K=32, tap_mask=NO_CENTRE),
    "g2_3img_d12_rect0": rows_case(gather=2, conv=_D12_3, N=72, K=32),
    # the dgrad of a strided conv over two images (the one gather without the fast form), 1 058 rows: a ragged last tile in both heights
    "g2_s2_2img_23to12": rows_case(gather=2, conv=_S2_2, N=72, K=32),
}
# the split-fp16 kernels with pre-split operands: plain and gather x (a, b, both) x 4-wave and 8-wave
for _k, _w in ((32, "4w"), (288, "8w")):
    for _pa, _pb in ((True, False), (False, True), (True, True)):
        _t = f"pa{int(_pa)}_pb{int(_pb)}_{_w}"
        NT_CASES["plain_" + _t] = rows_case(129 if _k == 32 else 257, 132, _k, pa=_pa, pb=_pb, bias=True, precs=SPLIT16,
                                            amax="loose" if (_pa and _pb) else None)
        NT_CASES["g1_" + _t] = rows_case(gather=1, conv=_S1, N=72, K=32 if _k == 32 else 64, tap_mask=NO_CENTRE if _k == 32 else None,
                                         pa=_pa, pb=_pb, precs=SPLIT16)
# the fused epilogue (glf_gemm_nt_epilogue): residual with ld_res != ldc, ReLU on and off, both tile configurations
NT_CASES.update({
    "epi_res_relu_4w": rows_case(129, 132, 32, epi=(148, True), precs=SPLIT16),
    "epi_res_8w": rows_case(257, 132, 288, epi=(144, False), alpha=0.5, precs=SPLIT16),
    "epi_relu_n70_8w": rows_case(255, 70, 288, epi=(None, True), precs=SPLIT16),
    "epi_res_relu_g1_rect2": rows_case(gather=1, conv=_D12, N=72, K=32, rect=2, epi=(77, True), precs=SPLIT16),
    "epi_res_relu_pa_pb_4w": rows_case(127, 72, 64, epi=(84, True), pa=True, pb=True, precs=SPLIT16),
})
# NN runs on the exact kernel whatever the precision setting
_NNP = ("f32", "f16x3")
NN_CASES = {
    "nn_plain": rows_case(129, 70, 33, mode="nn", precs=_NNP),
    "nn_g2_s1": rows_case(mode="nn", gather=2, conv=_S1, N=72, K=32, bias=True, precs=_NNP),
    "nn_g2_d24_rect1": rows_case(mode="nn", gather=2, conv=_D24, N=72, K=32, rect=1, precs=_NNP),
    "nn_g2_3img_d12_rect1": rows_case(mode="nn", gather=2, conv=_D12_3, N=72, K=32, rect=1, precs=_NNP),
    "nn_b3_alpha_bias_acc": rows_case(127, 132, 52, mode="nn", batch=3, alpha=0.5, bias=True, accumulate=True, precs=_NNP),
}
_W5 = (2, 16, 12, 3, 1, 5, 5)
TN_CASES = {
    # tile families: 64 x 64 (small), 128 x 128, 256-row 8-wave (wide), the exact fallback, and bf16x6 for each
    "k1_m64_n72": tn_case(1, 64, 72),                                                  # one reduction row: P + 4 roundings at most
    "k3_m64_n72": tn_case(3, 64, 72, alpha=0.5),
    "k100_m64_n72": tn_case(100, 64, 72),
    "k320_m128_n132": tn_case(320, 128, 132, alpha=0.5),
    "k96_m260_n72": tn_case(96, 260, 72),
    "k100_m66_n72_exact": tn_case(100, 66, 72),
    # slices: split 3 with an empty slice, 9 -> 4 slice lanes, 33 -> 16 slice lanes, the scalar second stage
    "k40_m64_n72_s3_empty": tn_case(40, 64, 72, split=3),
    "k300_m132_n72_s9": tn_case(300, 132, 72, split=9, alpha=0.5),
    "k1056_m64_n72_s33": tn_case(1056, 64, 72, split=33),
    "k100_m64_n70_s3_scalar": tn_case(100, 64, 70, split=3),
    "k100_m132_n72_acc": tn_case(100, 132, 72, accumulate=True),
    "k100_m64_n72_s3_acc": tn_case(100, 64, 72, split=3, accumulate=True),
    "k100_m260_n72_b3": tn_case(100, 260, 72, batch=3, alpha=0.5),
    "k100_m64_n72_s3_b3": tn_case(100, 64, 72, split=3, batch=3),
    # gathered 3x3 (weight gradients): stride 1, stride 2, dilation 5, with and without per-tap rectangles
    "w_s1": tn_case(conv=_S1, M=64, N=72),
    "w_s1_s3": tn_case(conv=_S1, M=132, N=72, split=3, alpha=0.5),
    "w_s2_55to28_s2": tn_case(conv=_S2, M=64, N=72, split=2),
    "w_d5": tn_case(conv=_W5, M=64, N=72, tap_mask=NO_CENTRE),
    "w_d5_rect_s4": tn_case(conv=_W5, M=64, N=72, split=4, rect=1),
    "w_d12_rect_s7": tn_case(conv=_D12, M=128, N=72, split=7, rect=1, alpha=0.5),
    "w_s1_rect": tn_case(conv=_S1, M=260, N=72, rect=1, split=2),
    # the parameter-layout store, with and without a foreign tap
    "w_s1_oihw": tn_case(conv=_S1, M=64, N=72, oihw=True),
    "w_d5_oihw_s4_rect": tn_case(conv=_W5, M=64, N=72, oihw=True, split=4, rect=1, accumulate=True),
    "w_d12_oihw_foreign": tn_case(conv=_D12, M=132, N=72, oihw=True, split=3, rect=1, tap_mask=NO_CENTRE, foreign=4),
    # pre-split operands
    "k100_m64_n72_pa": tn_case(100, 64, 72, pa=True, precs=SPLIT16),
    "k320_m128_n132_pb": tn_case(320, 128, 132, pb=True, split=3, precs=SPLIT16),
    "w_s1_pa_pb": tn_case(conv=_S1, M=260, N=72, pa=True, pb=True, split=2, precs=SPLIT16, amax="loose"),
}
ALL_CASES = {**NT_CASES, **NN_CASES, **TN_CASES}
# the one case with elements down to 2^-27 of the maximum (split-fp16 arithmetic only)
SUBNORMAL_CASE = rows_case(129, 72, 64, precs=SPLIT16)


def runs(cases=None):
    """(name, precision) of every run, in table order"""
    return [(k, p) for k, c in (ALL_CASES if cases is None else cases).items() for p in c["precs"]]


def families_of(arith):
    return FAMILIES[arith] + ("gauss",)


def split_probe(rows=37, cols=72, seed=5):
    """(x, [exact maximum, a maximum 8x loose, 0.0 = no maximum: s = 1]) for pinning the packed images: Gaussians, exact fp16
    ties of the scaled value, the maximum itself and zeros; every value has pieces that are zero or normal under all three
    settings (the few Gaussians that have not are replaced by zeros)."""
    x = gauss((rows, cols), seed).float()
    amax = float(x.abs().max())
    s = torch.tensor(pow2_scale(amax), dtype=F32)
    k = torch.arange(cols, dtype=F32)
    sign = 1.0 - 2.0 * (torch.arange(cols) % 2).float()
    x[1] = sign * (2049.0 + 2.0 * k) / s              # x s in [2048, 4096): fp16 spacing 2, odd integers are ties
    x[2] = -sign * (4098.0 + 4.0 * k) / s             # x s in [4096, 8192): spacing 4
    x[3] = 0.0
    x = x.double()
    settings = [amax, 8.0 * amax, 0.0]
    for _ in range(4):
        bad = torch.zeros_like(x, dtype=torch.bool)
        for am in settings:
            for v in pieces(x, "f16x3", am)[0].values():
                bad |= (v != 0) & (v.abs() < 2.0 ** -14)
        if not bool(bad.any()):
            break
        x[bad] = 0.0
    assert not bool(bad.any()) and float(x.abs().max()) == amax and int((x == 0).sum()) >= cols
    h, _ = split4h(x[1:3].float(), float(s))
    assert bool(((x[1:3].float() * s - h).abs() * 2 == torch.where(h.abs() >= 4096, 4.0, 2.0)).all()), "rows 1 and 2 are not exact ties"
    return x, settings
