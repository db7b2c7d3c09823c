"""Helpers of tests/test_gpu_s16_stream.py and tests/test_s16_stream_ref_cpu.py: guarded buffers, the two input families, and the
float64 / magnitude references of the 16-bit-storage streaming kernels (csrc/norm.hip and csrc/s16_ops.hip).  A plain module, not a conftest.

Inputs are float64 tensors whose values bf16 holds exactly (vectors of coefficients: fp32).  Two families:
  integer -- x, w in {-3..3}; dy, dy2, dz, residual in {-2..2}; given mean in {-1, 0, 1}; given invstd, gamma, LN gamma in
             {0.5, 1, 2}; beta in {-1, 0, 1} (+ 0.125 where a ReLU sign is taken: BN(x) is a multiple of 0.25, so no pre-ReLU
             value is nearer to zero than 0.125).  Every product and every column or row sum is an integer or a dyadic with few
             bits; assert_exact(magnitude) asserts < 2^24 from the reference alone; such results are gated for EQUALITY;
  gauss   -- randn scaled and shifted (means are not zero), rounded to bf16; coefficient vectors uniform, fp32.

The interval gate (tests/test_gpu_s16_gemm.py): d = (k + 4) 2^-23 magnitude, where the magnitude is the reference expression with
every input and every partial sum replaced by its absolute value and k is the number of fp32 roundings on the path to the output;
fp32 (and double) outputs: |got - ref| <= d; bf16 outputs: bf16_rne(ref - d) <= got <= bf16_rne(ref + d).  -ffp-contract=fast may
fuse a multiply with the following add: that removes roundings, never adds one.  x and mean are exact fp32 operands of x - mean,
so its one rounding is relative to |x - mean| (not to |x| + |mean|): that is the magnitude of this partial sum (with one row the
batch mean IS x, the difference is zero, and BN(x) = beta without any error).  k per output, counted in norm.hip / s16_ops.hip:

  colstats sum x       k = rpt                          x is exact in fp32; rpt adds of one thread (below); LDS fold and atomics in double
  colstats sum x^2     k = rpt                          a bf16 square has 16 bits: exact in fp32
  colsum db            k = rpt + 1                      + the double -> float store
  bn_apply mean/invstd within one fp32 ulp of the mirrored double formula (sums / rows, E[x^2] - mean^2 clamped at 0, 1 / sqrt(var + eps))
  bn_apply y           k = 5                            x - mean, * invstd, * gamma, + beta, + residual  (bn_val, then the residual)
  bn_bwd dres          k = 1                            dy + dy2 (none without dy2); the mask selects
  bn_bwd dbeta         k = 1 + rpt + 1                  dy + dy2; rpt adds; (float) of the double sum
  bn_bwd dgamma        k = 4 + rpt + 1                  dy + dy2, x - mean, * invstd, * g; rpt adds; (float)
  bn_bwd dx, eval      k = 2                            g * gamma, * invstd (the dy + dy2 add, where present, is one of the + 4)
  bn_bwd dx, train     k = 10                           gamma * invstd, x - mean, * invstd, * s2, s1 +, g -, *  (7) and on the way to
                                                        s1 / s2: (float) sum, fl(1 / n), * (3); reference and magnitude take the
                                                        dbeta / dgamma the kernel wrote (they ARE its s1 n, s2 n), gated first
  tail u = BN(w) + x   k = 5                            as bn_apply y; A = mag(u) + |row_mean| below
  tail row_mean        k = 5 + 32 + 6 + 1 = 44          u; 8 LN_NV adds of a lane; six wave_sum steps; / c.  magnitude mean_c mag(u)
  tail row_rstd        k = 13 + 32 + 6 + 1 + 1 = 53     with the row_mean the kernel wrote: dlt = u - mean carries 5 + 1 roundings of A,
                                                        dlt^2 twice that + 1 (|dlt| <= A); lane adds, wave steps, / c, + eps.  With V =
                                                        var + eps and MV = mean_c A^2 + eps, rstd = V^-1/2 moves by rstd MV / (2 V) per unit
                                                        of relative error in V; sqrtf and the division add 3 roundings of rstd itself:
                                                        magnitude rstd (MV / (2 V) + 1)
  tail z               k = 9                            u (5), - mean, * rstd, * g, + b with the row statistics the kernel wrote
  tail du              k = 58                           uhat = (u - mean) rstd carries 7 roundings of MUH = A rstd; gz = dz g (1);
                                                        m2 = mean gz uhat: 9 per term + 32 + 6 + 1 = 48; then uhat * m2, the subtraction,
                                                        * rstd: 7 + 48 + 3 = 58 on the longest path.  magnitude rstd (|gz| + mean|gz| + MUH
                                                        mean(|gz| MUH))
  tail dln_gamma       k = 8 + 16 + 3 + 1 = 28          dz * uhat (7 + 1); 16 rows of a wave; three LDS folds; (float) of the double slab sum
  tail dln_beta        k = 16 + 3 + 1 = 20              exact in the integer family
  sum_rows y           k = ceil(p / 8) + 7 + 1          a row lane's adds; seven LDS folds; * scale  (exact in the integer family, scale 0.5)
rpt = rows one thread of a reduction adds = ceil(ceil(rows / slices) / (256 / threads-per-row)) (red_geometry mirrors red_geom of csrc/col_reduce.h).

ReLU signs: an element whose float64 pre-ReLU value v has |v| <= d(v) is "unsure": the fp32 sign may legitimately differ.  Mask
bits and ReLU-dependent outputs are compared on the others; a column sum's d grows by the magnitude of its unsure terms.  A case
must have at most UNSURE_CAP of its elements unsure (asserted from the reference alone)."""
import functools
import math

import torch

from test_gpu_s16_gemm import assert_exact_precondition, bf16_rne, gate_exact, interval_violations

DEV = "cuda"
BF, F32, F64 = torch.bfloat16, torch.float32, torch.float64
U = 2.0 ** -23
GUARD = 64
SENT16 = 0x7FA5                                           # a NaN no kernel produces
SENT_F = float(torch.tensor(-1234.56789, dtype=F32))
SENT_B = 0xA5
SENT_I = -0x5A5A5A5A
UNSURE_CAP = 1e-4
EPS = float(torch.tensor(1e-5, dtype=F32))                # eps and momentum travel as C floats
MOM = float(torch.tensor(0.1, dtype=F32))
LN_EPS = float(torch.tensor(1e-5, dtype=F32))
LN_NV, LN_ROWS, APPLY_MAX_C, LN_MAX_C = 4, 64, 4096, 2048

ROWS = [1, 5, 70, 297, 1031, 4100]
CHANNELS = [8, 24, 72, 128, 136, 2048, 4096]
BN_SHAPES = [(r, c) for r in ROWS for c in CHANNELS if r * c <= 1031 * 4096 or (r, c) == (4100, 2048)]
BIG_SHAPE = (8500, 4096)                                   # the slice cap of red_geom<8>
# row-stride pads per strided operand, in argument order: none, all, and each operand alone -- every pair of operands has
# different strides in some pattern, so a kernel that indexes one operand with another's stride cannot pass
def _pad_patterns(names):
    pats = {"p0": (0,) * len(names), "p8": (8,) * len(names)}
    for i, n in enumerate(names):
        pats[n + "8"] = tuple(8 if j == i else 0 for j in range(len(names)))
    return pats


APPLY_PADS = _pad_patterns(("x", "res", "y"))
BWD_PADS = _pad_patterns(("dy", "dy2", "x", "dx", "dres"))
TAIL_C = [8, 512, 520, 1024, 2048]
TAIL_ROWS = [1, 3, 17, 64, 65, 200, 1100]
SUM_N, SUM_P, SUM_C = [1, 3], [1, 7, 8, 9, 31, 32, 33, 100], [8, 248, 256, 264]


# ------------------------------------------------------------------------------------------------------------------ buffers
class Guarded:
    """[rows][ld] output of dtype fp32 / double / uint8 / int64 whose first c columns the kernel may write: everything else
    (GUARD elements before and after, the columns c .. ld of every row) holds a sentinel that must survive."""
    SENT = {torch.float32: SENT_F, torch.float64: SENT_F, torch.uint8: SENT_B, torch.int64: SENT_I, torch.int16: SENT16}

    def __init__(self, rows, c, ld=None, dtype=F32, device=DEV):
        ld = c if ld is None else ld
        self.sent = self.SENT[dtype]
        self.buf = torch.full((GUARD + rows * ld + GUARD,), self.sent, dtype=dtype, device=device)
        self.body = self.buf[GUARD:GUARD + rows * ld].view(rows, ld)
        self.t = self.body[:, :c]
        self.rows, self.ld, self.c = rows, ld, c

    @property
    def ptr(self):
        return self.body.data_ptr()

    def fill(self, values):
        self.t.copy_(values.to(self.t.dtype))
        return self

    def dense(self):
        return self.t.contiguous()

    def f64(self):
        return self.t.double()

    def intact(self):
        ok = bool((self.buf[:GUARD] == self.sent).all()) and bool((self.buf[-GUARD:] == self.sent).all())
        return ok and (self.ld == self.c or bool((self.body[:, self.c:] == self.sent).all()))

    def written(self, allow=None):
        """every element differs from the sentinel (uint8: except where `allow` says the sentinel byte is the expected value)"""
        left = self.t == self.sent
        if allow is not None:
            left = left & ~allow
        return not bool(left.any())

    def untouched(self):
        """a refused call: the whole buffer still holds the sentinel"""
        return bool((self.buf == self.sent).all())


class Guarded16(Guarded):
    """The bf16 counterpart: [rows][ld] uint16 storage (held as int16) with the sentinel bit pattern in the guards and in the
    columns c .. ld; dense() is the bf16 view of the live part."""

    def __init__(self, rows, c, ld=None, device=DEV):
        super().__init__(rows, c, ld, dtype=torch.int16, device=device)

    def fill(self, values):
        self.t.copy_(values.to(BF).view(torch.int16))
        return self

    def dense(self):
        return self.t.contiguous().view(BF)

    def f64(self):
        return self.dense().double()


def put16(values, ld=None, device=DEV):
    """a bf16 input [rows][ld] on the device, NaN in the columns beyond the logical ones (a read of the pad shows up)"""
    rows, c = values.shape
    ld = c if ld is None else ld
    out = torch.full((rows, ld), float("nan"), dtype=BF, device=device)
    out[:, :c] = values.to(device=device, dtype=BF)
    assert torch.equal(out[:, :c].double(), values.to(device)), "input is not representable in bf16"
    return out


def vec32(values, device=DEV):
    out = values.to(device=device, dtype=F32).contiguous()
    assert torch.equal(out.double(), values.to(device)), "coefficient is not an fp32 value"
    return out


def ptr(t):
    return None if t is None else (t.ptr if isinstance(t, Guarded) else t.data_ptr())


# ------------------------------------------------------------------------------------------------------------------- inputs
def _gen(seed):
    return torch.Generator(device="cpu").manual_seed(seed)


def ints(shape, seed, lo, hi):
    return torch.randint(lo, hi + 1, tuple(shape), generator=_gen(seed)).double()


def pick(shape, seed, values):
    v = torch.tensor(values, dtype=F64)
    return v[torch.randint(0, len(values), tuple(shape), generator=_gen(seed))]


def gauss(shape, seed, scale=1.0, shift=0.0):
    return (torch.randn(tuple(shape), generator=_gen(seed)) * scale + shift).to(BF).double()


def uniform32(shape, seed, lo, hi):
    return (torch.rand(tuple(shape), generator=_gen(seed)) * (hi - lo) + lo).float().double()


class Bag(dict):
    __getattr__ = dict.__getitem__
    __setattr__ = dict.__setitem__


@functools.lru_cache(maxsize=6)
def bn_inputs(family, rows, c, device=DEV):
    """x, res, dy, dy2 [rows][c]; gamma, beta, given mean / invstd [c]: float64 on `device` (the inputs are cached here; the
    references taken from them are cached by the tests that share them among pad patterns)"""
    if family == "int":
        b = Bag(x=ints((rows, c), 1, -3, 3), res=ints((rows, c), 2, -2, 2), dy=ints((rows, c), 3, -2, 2), dy2=ints((rows, c), 4, -2, 2),
                mean=pick((c,), 5, [-1.0, 0.0, 1.0]), invstd=pick((c,), 6, [0.5, 1.0, 2.0]), gamma=pick((c,), 7, [0.5, 1.0, 2.0]),
                beta=pick((c,), 8, [-1.0, 0.0, 1.0]) + 0.125)
    else:
        x = gauss((rows, c), 11, 2.0, 0.7)
        b = Bag(x=x, res=gauss((rows, c), 12, 1.0, 0.3), dy=gauss((rows, c), 13, 1.0, 0.1), dy2=gauss((rows, c), 14, 0.5, -0.2),
                mean=uniform32((c,), 15, 0.5, 0.9), invstd=uniform32((c,), 16, 0.4, 0.6), gamma=uniform32((c,), 17, 0.5, 1.5),
                beta=uniform32((c,), 18, -0.5, 0.5))
    return Bag({k: v.to(device) for k, v in b.items()})


@functools.lru_cache(maxsize=4)
def tail_inputs(family, rows, c, device=DEV):
    if family == "int":
        b = Bag(w=ints((rows, c), 21, -3, 3), x=ints((rows, c), 22, -2, 2), dz=ints((rows, c), 23, -2, 2),
                mean=pick((c,), 24, [-1.0, 0.0, 1.0]), invstd=pick((c,), 25, [0.5, 1.0, 2.0]), bn_g=pick((c,), 26, [0.5, 1.0, 2.0]),
                bn_b=pick((c,), 27, [-1.0, 0.0, 1.0]), ln_g=pick((c,), 28, [0.5, 1.0, 2.0]), ln_b=pick((c,), 29, [-1.0, 0.0, 1.0]))
    else:
        b = Bag(w=gauss((rows, c), 31, 2.0, 0.7), x=gauss((rows, c), 32, 1.0, 0.3), dz=gauss((rows, c), 33, 1.0, 0.1),
                mean=uniform32((c,), 34, 0.5, 0.9), invstd=uniform32((c,), 35, 0.4, 0.6), bn_g=uniform32((c,), 36, 0.5, 1.5),
                bn_b=uniform32((c,), 37, -0.5, 0.5), ln_g=uniform32((c,), 38, 0.5, 1.5), ln_b=uniform32((c,), 39, -0.5, 0.5))
    return Bag({k: v.to(device) for k, v in b.items()})


def sum_inputs(family, n, p, c, device=DEV):
    x = ints((n * p, c), 41, -3, 3) if family == "int" else gauss((n * p, c), 42, 2.0, 0.7)
    return x.to(device)


# ------------------------------------------------------------------------------------------------------------------- gates
RATIOS = {}            # output name -> [gated tensors, largest |got - ref| / d, largest share of a bf16 tensor that is not bf16_rne(ref)]


def tol(k, mag):
    return (k + 4) * U * mag


def assert_exact(*mags):
    for m in mags:
        assert_exact_precondition(m)


def gate(got, ref, mag, k, bf16, what, name, sure=None, extra=None):
    """the interval gate on every element (on the `sure` ones), recording the largest |got - ref| / d under `name`; `extra`
    (same shape as ref) widens d by an absolute amount that the caller derived (unsure terms of a sum)"""
    got, ref, mag = got.double(), ref.double(), mag.double()
    if extra is not None:
        mag = mag + extra / ((k + 4) * U)
    if sure is not None:
        got, ref, mag = got[sure], ref[sure], mag[sure]
    if got.numel() == 0:
        return
    assert bool(torch.isfinite(got).all()), what + ": non-finite element"
    bad, worst = interval_violations(got, ref, mag, k, bf16)
    rec = RATIOS.setdefault(name, [0, 0.0, 0.0])
    rec[0] += 1
    rec[1] = max(rec[1], worst)
    if bf16:                                              # |got - ref| / d of a bf16 output is mostly its own store rounding: also
        rec[2] = max(rec[2], float((got != bf16_rne(ref)).double().mean()))      # the share that is not bf16_rne(ref)
    nbad = int(bad.sum())
    if nbad:
        i = int(bad.reshape(-1).nonzero()[0])
        g, r, m = got.reshape(-1)[i], ref.reshape(-1)[i], mag.reshape(-1)[i]
        raise AssertionError(f"{what}: {nbad} of {got.numel()} elements outside the derived interval (k = {k}); first at flat index {i}: got "
                             f"{float(g)!r}, ref {float(r)!r}, magnitude {float(m)!r}, |got - ref| / d = {float((g - r).abs() / tol(k, m).clamp_min(1e-300)):.3g}")


def exact(got, ref, bf16, what, name, sure=None):
    if sure is not None:
        got, ref = got[sure], ref[sure]
    rec = RATIOS.setdefault(name + " (exact)", [0, 0.0, 0.0])
    rec[0] += 1
    gate_exact(got.double() if got.dtype == F64 else got, ref, bf16, what)


def within_ulps(got32, ref64, n=1):
    """|got - ref| <= n fp32 ulps of ref"""
    _, e = torch.frexp(ref64.abs())
    ulp = torch.ldexp(torch.ones_like(ref64), e - 24).clamp_min(2.0 ** -149)
    return bool(((got32.double() - ref64).abs() <= n * ulp).all())


def close(a, b, tol_):
    a, b = a.double(), b.double()
    return bool(((a - b).abs() <= tol_ + tol_ * b.abs()).all())


def sign_bytes(positive, w=8):
    """[rows][c] bool -> [rows][c / w] bytes, bit j of byte i = channel w i + j (w = 8: bf16 storage, w = 4: fp32 storage)"""
    rows, c = positive.shape
    bit = torch.tensor([1 << j for j in range(w)], dtype=torch.int32, device=positive.device)
    return (positive.reshape(rows, c // w, w).to(torch.int32) * bit).sum(-1).to(torch.uint8).contiguous()


def unsure_share(unsure):
    return float(unsure.double().mean())


# --------------------------------------------------------------------------- reduction geometry (col_reduce.h: red_geom<W>)
def red_geometry(rows, c, w=8):
    """(threads per row, rows per pass, slices, rows per slice, rows one thread adds) of the single-stage column reductions at
    access width w: 8 elements per 16-byte access for bf16 storage, 4 for fp32"""
    cw = c // w if c > w else 1
    tpr = min(cw, 16)
    rpp = 256 // tpr
    s = (rows + 16 * rpp - 1) // (16 * rpp)
    cblocks = (cw + tpr - 1) // tpr
    cap = max(1, 1024 // cblocks)
    slices = max(1, min(s, cap))
    per = (rows + slices - 1) // slices
    return tpr, rpp, slices, per, (per + rpp - 1) // rpp


# --------------------------------------------------------------------------------------------------------------- BatchNorm
def colstats_ref(x):
    """(sum x, sum x^2) [2][c] and the same on magnitudes"""
    s = torch.stack([x.sum(0), (x * x).sum(0)])
    return s, torch.stack([x.abs().sum(0), (x * x).sum(0)])


def bn_stats_from_sums(sums, rows, eps=EPS):
    """the kernel's double formula: mean, invstd, unbiased variance"""
    m = sums[0] / rows
    var = (sums[1] / rows - m * m).clamp_min(0.0)
    return m, 1.0 / torch.sqrt(var + eps), (var * rows / (rows - 1) if rows > 1 else var)


def bn_fwd_ref(x, mean, invstd, gamma, beta, res=None):
    """pre-ReLU value v = (x - mean) invstd gamma + beta [+ res] and its magnitude"""
    v = (x - mean) * invstd * gamma + beta
    mag = (x - mean).abs() * invstd.abs() * gamma.abs() + beta.abs()
    if res is not None:
        v, mag = v + res, mag + res.abs()
    return v, mag


K_Y, K_V_NORES = 5, 4


def unsure_of(v, mag, k):
    return v.abs() <= tol(k, mag)


def bn_bwd_ref(dy, dy2, x, mean, invstd, mask):
    """g = (dy + dy2) mask; s1 = sum g; s2 = sum g xhat, each with its magnitude.  mask: float64 0 / 1 or None"""
    g0 = dy if dy2 is None else dy + dy2
    g0mag = dy.abs() if dy2 is None else dy.abs() + dy2.abs()
    m = 1.0 if mask is None else mask
    g, gmag = g0 * m, g0mag * m
    xh = (x - mean) * invstd
    xhmag = xh.abs()
    return Bag(g=g, gmag=gmag, g0mag=g0mag, xh=xh, xhmag=xhmag, s1=g.sum(0), s1mag=gmag.sum(0), s2=(g * xh).sum(0), s2mag=(gmag * xhmag).sum(0))


def bn_bwd_dx_eval(b, gamma, invstd):
    return b.g * gamma * invstd, b.gmag * gamma.abs() * invstd.abs()


def bn_bwd_dx_train(b, gamma, invstd, s1, s2, rows):
    """with s1 = dbeta and s2 = dgamma as given (float64 sums, or the fp32 values the kernel wrote)"""
    k = gamma * invstd
    return k * (b.g - (s1 + b.xh * s2) / rows), k.abs() * (b.gmag + (s1.abs() + b.xhmag * s2.abs()) / rows)


K_DRES, K_DX_EVAL, K_DX_TRAIN = 1, 2, 10


def k_dbeta(rows, c):
    return 1 + red_geometry(rows, c)[4] + 1


def k_dgamma(rows, c):
    return 4 + red_geometry(rows, c)[4] + 1


# -------------------------------------------------------------------------------------------------------------- TPAVI tail
K_ROW_MEAN, K_ROW_RSTD, K_Z, K_DU, K_DLN_G, K_DLN_B = 44, 53, 9, 58, 28, 20


def tail_u(i):
    """u = BN(w) + x and its magnitude"""
    return bn_fwd_ref(i.w, i.mean, i.invstd, i.bn_g, i.bn_b, i.x)


def tail_row_mean(u, umag):
    return u.mean(1), umag.mean(1)


def tail_row_rstd(u, umag, row_mean, eps=LN_EPS):
    """rstd with the given row mean, and the magnitude rstd (MV / (2 V) + 1)"""
    m = row_mean[:, None]
    V = ((u - m) ** 2).mean(1) + eps
    MV = ((umag + m.abs()) ** 2).mean(1) + eps
    rstd = 1.0 / torch.sqrt(V)
    return rstd, rstd * (MV / (2.0 * V) + 1.0)


def tail_z(u, umag, row_mean, row_rstd, ln_g, ln_b):
    m, r = row_mean[:, None], row_rstd[:, None]
    return (u - m) * r * ln_g + ln_b, (umag + m.abs()) * r.abs() * ln_g.abs() + ln_b.abs()


def tail_bwd_ref(u, umag, dz, row_mean, row_rstd, ln_g):
    """du, dln_gamma, dln_beta with magnitudes"""
    m, r = row_mean[:, None], row_rstd[:, None]
    uh, uhmag = (u - m) * r, (umag + m.abs()) * r.abs()
    gz, gzmag = dz * ln_g, dz.abs() * ln_g.abs()
    m1, m1mag = gz.mean(1, keepdim=True), gzmag.mean(1, keepdim=True)
    m2, m2mag = (gz * uh).mean(1, keepdim=True), (gzmag * uhmag).mean(1, keepdim=True)
    return Bag(du=r * (gz - m1 - uh * m2), dumag=r.abs() * (gzmag + m1mag + uhmag * m2mag),
               dg=(dz * uh).sum(0), dgmag=(dz.abs() * uhmag).sum(0), db=dz.sum(0), dbmag=dz.abs().sum(0))


# ---------------------------------------------------------------------------------------------------------------- row sums
def sum_rows_ref(x, n, p, scale):
    c = x.shape[1]
    return scale * x.view(n, p, c).sum(1), abs(scale) * x.abs().view(n, p, c).sum(1)


def k_sum_rows(p):
    return math.ceil(p / 8) + 7 + 1


# ------------------------------------------------------------------------------------------------------------------- casts
def cast_specials():
    """fp32 bit patterns: exact halfway cases between two bf16 values with even and odd kept mantissa, just above / below them, the
    largest finite value that rounds to infinity and the one below it that does not, both zeros, denormals (also those that round
    up into the smallest normal), infinities; 8 k values"""
    bits = []
    for hi in (0x3F80, 0x3F81, 0x4049, 0x7F7E, 0x0001, 0x0080, 0x007F, 0x0000):
        for lo in (0x0000, 0x0001, 0x7FFF, 0x8000, 0x8001, 0xFFFF):
            bits += [(hi << 16) | lo, 0x80000000 | (hi << 16) | lo]
    bits += [0x7F7FFFFF, 0xFF7FFFFF, 0x7F7F8000, 0x7F7F7FFF, 0x7F800000, 0xFF800000, 0x00000000, 0x80000000, 0x00000001, 0x80000001,
             0x007FFFFF, 0x807FFFFF, 0x00008000, 0x00018000]
    bits += [0] * (-len(bits) % 8)
    t = torch.tensor(bits, dtype=torch.int64)
    return torch.where(t >= 2 ** 31, t - 2 ** 32, t).to(torch.int32)


def cast_nans():
    t = torch.tensor([0x7FC00000, 0xFFC00000, 0x7F800001, 0x7FFFFFFF, 0x7F808000, 0x7F80FFFF, 0xFF800001, 0x7FA00000], dtype=torch.int64)
    return torch.where(t >= 2 ** 31, t - 2 ** 32, t).to(torch.int32)
