"""Helpers of tests/test_gpu_pointwise.py and tests/test_pointwise_ref_cpu.py: float64 references, shape lists and the derivation of
every k for the pointwise kernels of csrc/pointwise.hip (fp32 storage: Stream<float, 1> / <float, 4>; bf16 storage: <u16, 8>).
A plain module, not a conftest.  Buffers, input families and the two gates are those of tests/s16_stream_ref.py (re-exported).

Families: integer (small integers, dyadic coefficients: the float64 reference is an fp32 value, assert_exact asserts < 2^24 on
the magnitude, bf16 outputs stay <= 256 in magnitude) -> EQUALITY; Gaussian -> the interval d = (k + 4) 2^-23 magnitude, bf16
outputs bf16_rne(ref - d) <= got <= bf16_rne(ref + d).  -ffp-contract=fast only removes roundings.  Selections and copies (relu,
max-pool values / indices / routing, copies, transposes, re-layouts, dropout, overlap counts) are always equality.

expf / log1pf: charged 4 fp32 ulps of the function's value per call.  This is a margin over the 1-2 ulp ROCm documents for its
device library, NOT a measurement; tests/test_pointwise_ref_cpu.py shows torch's own fp32 evaluation of every formula inside the
same intervals.  (Observed on the MI355X, profiles/pointwise_gate.txt: this build's expf carries about |x| / 2 ulp at large |x|,
because -ffp-contract=fast fuses a subtraction inside the compiler's own expansion of expf; the outputs stay inside these
intervals, the charge was not changed.)  sigmoid(x) = 1 / (1 + expf(-x)) therefore carries 4 E / (1 + E) + 2 <= 6 roundings of its value (E = exp(-x));
where its true value is below the smallest normal fp32 (x <= -87.4: 1 + inf -> 0) the absolute error is at most 2^-126 (`extra`).

k per output (U = 2^-23; "rel" = the per-element k of gate_rel: d = (kelem + 4) U |ref|):
  axpby out            k = 3                    a x, b y, +
  add_n out            k = inputs - 1
  add_frames dst       k = 1
  sum_rows y           fp32-sum kernel (c % 4 != 0 or ld % 4 != 0 or a pointer off 16 bytes): k = ceil(p / 4) + 3 + 1 (a row lane's
                       adds, three LDS adds, * scale); double-sum kernel (everything else): k = 1 (the (float) store).  avgpool is
                       sum_rows with ld = c and scale = fl32(1 / p): the reference multiplies by that fp32 value
  bcast_rows y         k = 1;  bcast_rows_add y: k = 2 (scale * x, + y)
  softmax p            rel: |x - m| / 2 + 4 (t = x - m: one rounding of |t|, which moves exp(t) by |t| 2^-24 of its value; expf)
                       + S + 2 (1 / s, e * inv) with S = sum_j e_j (|x_j - m| / 2 + 4) / s + ceil(cols / 256) + 9 (a thread's adds,
                       six shuffle steps, three wave partials); the maximum m is a selection.  extra 2^-126: an e below the
                       smallest normal may be flushed; elements with p >= 2^-100 are gated again WITHOUT the extra
  softmax_bwd dp       k = ceil(cols / 256) + 12: p dy (1), a thread's adds, 6 + 3 (s); dy - s (1); * p (1).  magnitude p (|dy| +
                       sum |p dy|)
  bilinear y           k = 7 + h + w: 1 - lx, * v, +, 1 - ly, *, + on the longest path (7 with the lx / ly products); the source
                       coordinate s = (o + 0.5) scale - 0.5 is one fused or two separate roundings: it moves by at most ulp(s) <=
                       size 2^-23 per axis between the two, and the blend moves by that times the sum of |x| over its source pixels, which
                       is the magnitude of this output (h + w).  The reference
                       takes the separate form (numpy float32, as ATen's host arithmetic); the CPU test asserts that the fused form
                       picks the same source pixels at every shape used
  bilinear dx          k = contributing columns + contributing rows (the two running sums) + 6 (wx: up to 2, wx g: 1, wy: up to 2,
                       wy rowacc: 1) + h + w.  magnitude: sum of |g| over the contributing outputs
  gate a               rel: 14 |u| (1 - a) + 6 with u = weight best cc: best and cc are sigmoids (6 each), two products (2); a =
                       sigmoid(u) moves by a (1 - a) |du|, and adds its own 6
  gate y, df           EQUALITY with fl32(f a) for the a the kernel wrote / was given (one fp32 product; bf16: then bf16_rne)
  gate da (internal)   fp32: k_da = 1 + 3 ceil(c / 256) + 6 (product; per 16-byte access two pairwise levels and the running add; six
                       shuffle steps); bf16: k_da = 1 + 8 ceil(c / 512) + 6 (sequential).  0 in the integer family (exact sums)
  gate dcls[argmax]    rel on the magnitude M_da a (1 - a) w cc m (1 - m): k_da + 4 (1 - a and three products) + 6 (m) + 6 (cc) +
                       6 m / (1 - m) + 1 (1 - m: m's error relative to 1 - m, and the subtraction) + 3 (products); off the argmax
                       column: exactly 0
  gate dctr            the same with cc / (1 - cc) in place of m / (1 - m)
  bce loss             k = 7 on sum_i (max(x, 0) + |x t| + L + E), E = exp(-|x|), L = log1p(E): x t, -, + (3), log1pf (4); expf's 4
                       ulps of E pass through log1p with slope <= 1 (the E in the magnitude).  The sum is a double and is stored as
                       one (atomicAdd on a double): no (float) store
  bce dx               k = 9: sigmoid (6), - t, gscale * *grad_scale_dev, * on (sigmoid + |t|) |g|; extra 2^-126 |g|; elements with
                       |x| <= 80 are gated again WITHOUT the extra
  stem y               k = 49 (the fmaf chain on |bias| + sum |x| |w|)
  stem dw, db          k = pixels of the largest 16 x 16 tile + 1 (one thread's chain over its tile; tiles meet in double; (float))
  stem pool y          k = 49 + 4 on maxpool(relu-free magnitude): (a - mean) invstd gamma + beta; relu and max are 1-Lipschitz, so
                       the interval of a window is the largest interval in it
"""
import functools
import math

import numpy as np
import torch
import torch.nn.functional as F

from s16_stream_ref import (BF, DEV, F32, F64, U, GUARD, SENT_B, SENT_F, SENT_I, SENT16, RATIOS, Bag, Guarded, Guarded16, _pad_patterns,
                            assert_exact, exact, gate, gauss, ints, pick, ptr, put16, tol, uniform32, vec32)
from test_gpu_s16_gemm import assert_exact_precondition, bf16_rne, gate_exact, interval_violations

Guarded.SENT.setdefault(torch.int32, SENT_I)
TINY = 2.0 ** -126                  # smallest normal fp32
K_TRANS = 4                         # fp32 ulps charged per expf / log1pf call
K_SIG = 6                           # roundings of a sigmoid's value

# ------------------------------------------------------------------------------------------------------------------ shapes
MI355X_CUS = 256


def cap(cus=MI355X_CUS):
    """threads of the largest grid stream_grid launches: 8 workgroups of 256 per CU"""
    return 8 * cus * 256


def big(cus=MI355X_CUS):
    """accesses of the one second-trip case per kernel: the grid-stride loop turns once more, raggedly"""
    return cap(cus) + 3 * 256 + 5


AXPBY_GRID = 8192 * 256             # glf_axpby caps its grid at 8192 workgroups (not stream_grid): its own second trip


RELU_NUMEL = [1, 7, 8, 255, 256, 257]
AXPBY_NUMEL = [1, 3, 4, 5, 1023, 1027]
AXPBY_COEF = [(1.0, 1.0), (1.0, -1.0), (0.5, 2.0), (-1.0, 0.5), (2.0, -1.0)]
FRAME_N, FRAME_INNER = [1, 3], [1, 5, 1000]                  # inner in units of W
FRAME_PADS3 = _pad_patterns(("a", "b", "dst"))
FRAME_PADS2 = _pad_patterns(("src", "dst"))
DROP_P = [0.0, 0.1, 0.5, 0.9, 0.999]
DROP_SEED = [0, 1, 2 ** 63 + 12345]
DROP_STEP = [None, 0, 3]
DROP_NUMEL = [1, 7, 8, 257, 264]
POOL_SHAPES = [(1, 1, 1), (1, 1, 4), (1, 2, 2), (2, 3, 5), (1, 8, 6), (2, 13, 11), (1, 16, 16)]
POOL_C = [4, 8, 12, 64, 72]
POOL_BIG = (2, 130, 130)
GATE_ROWS, GATE_NCLS = [1, 3, 4, 5, 9, 1027], [1, 2, 5]
GATE_C = {"f32": [4, 252, 256, 264, 2048], "bf16": [8, 256, 264, 2048]}
GATE_WEIGHT = 2.5
ROWS_N, ROWS_P, ROWS_C = [1, 3], [1, 15, 16, 17, 63, 64, 65, 113, 196], [1, 3, 4, 60, 64, 68, 260]
ROWS_C16 = [8, 64, 264]
SOFT_ROWS, SOFT_COLS, SOFT_PAD = [1, 3], [1, 2, 255, 256, 257, 301, 1030], [0, 1, 7]
BIL_SHAPES = [(1, 1, 1, 1), (1, 1, 5, 3), (2, 3, 2, 3), (3, 2, 8, 5), (5, 7, 13, 29), (7, 5, 28, 20), (2, 2, 37, 41)]
BIL_C, BIL_N = [1, 5], [1, 2]
BCE_NUMEL = [1, 63, 64, 65, 257]
BCE_PLANTS = [0.0, 20.0, -20.0, 90.0, -90.0, 104.0, -104.0]
STEM_SHAPES = [(7, 7, 0), (1, 1, 3), (22, 22, 0), (23, 38, 0), (20, 35, 2), (12, 9, 3)]
STEM_N = [1, 2]
TR_DIMS = {"f32": [1, 31, 32, 33, 70], "bf16": [1, 63, 64, 65, 130]}
TR_TILE = {"f32": 32, "bf16": 64}
TR_BATCH = [1, 3]
RELAYOUT = [(1, 1, 1), (3, 5, 9), (64, 1, 49), (7, 13, 1)]


# ------------------------------------------------------------------------------------------------------------------ buffers
class GuardedMask:
    """A flat output of `total` elements of which the kernel may write exactly those where `live` is set (frames with padded
    strides, a strided transpose): the rest, and GUARD elements on either side, hold a sentinel that must survive."""

    def __init__(self, live, dtype=F32, device=DEV):
        self.sent = Guarded.SENT[dtype]
        total = live.numel()
        self.live = live.to(device).reshape(-1)
        self.buf = torch.full((GUARD + total + GUARD,), self.sent, dtype=dtype, device=device)
        self.body = self.buf[GUARD:GUARD + total]

    @property
    def ptr(self):
        return self.body.data_ptr()

    def intact(self):
        return (bool((self.buf[:GUARD] == self.sent).all()) and bool((self.buf[-GUARD:] == self.sent).all())
                and bool((self.body[~self.live] == self.sent).all()))

    def written(self):
        return not bool((self.body[self.live] == self.sent).any())

    def untouched(self):
        return bool((self.buf == self.sent).all())

    def values(self):
        v = self.body[self.live]
        return v.view(BF) if self.buf.dtype == torch.int16 else v


def strided_live(batch, rows, cols, ld, bs):
    """live mask and flat offsets of a [batch][rows][cols] view with row stride ld and batch stride bs"""
    off = (torch.arange(batch).view(-1, 1, 1) * bs + torch.arange(rows).view(1, -1, 1) * ld + torch.arange(cols).view(1, 1, -1)).reshape(-1)
    total = (batch - 1) * bs + (rows - 1) * ld + cols
    live = torch.zeros(total, dtype=torch.bool)
    live[off] = True
    assert int(live.sum()) == off.numel(), "the view overlaps itself"
    return live, off


def put32(values, ld=None, device=DEV):
    """an fp32 input [rows][ld] on the device, NaN in the columns beyond the logical ones (a read of the pad shows up)"""
    rows, c = values.shape
    ld = c if ld is None else ld
    out = torch.full((rows, ld), float("nan"), dtype=F32, device=device)
    out[:, :c] = values.to(device=device, dtype=F32)
    assert torch.equal(out[:, :c].double(), values.to(device)), "input is not an fp32 value"
    return out


def put(st, values, ld=None, device=DEV):
    return put32(values, ld, device) if st == "f32" else put16(values, ld, device)


def out_buf(st, rows, c, ld=None, device=DEV):
    return Guarded(rows, c, ld, device=device) if st == "f32" else Guarded16(rows, c, ld, device=device)


def width(st):
    return 4 if st == "f32" else 8


def _gen(seed):
    return torch.Generator(device="cpu").manual_seed(seed)


def gauss32(shape, seed, scale=1.0, shift=0.0):
    """fp32 Gaussians with all 24 bits in use"""
    return (torch.randn(tuple(shape), generator=_gen(seed)) * scale + shift).float().double()


def gaussian(st, shape, seed, scale=1.0, shift=0.0):
    return gauss32(shape, seed, scale, shift) if st == "f32" else gauss(shape, seed, scale, shift)


def gate_rel(got, ref, kelem, bf16, what, name, extra=None, sure=None):
    """the interval gate with a k of its own per element: d = (kelem + 4) U |ref| (+ extra), on the `sure` elements"""
    gate(got, ref, ref.abs() * (kelem + 4.0) / 4.0, 0, bf16, what, name, sure=sure, extra=extra)


def same_values(got, want):
    """equality that lets NaN match NaN"""
    return bool(((got == want) | (got.isnan() & want.isnan())).all())


# -------------------------------------------------------------------------------------------------------------------- relu
def relu_specials(st):
    """+-0, +-inf, fp32 denormals (fp32 storage only), bf16 denormals, the smallest normals, ordinary values: float64"""
    v = [0.0, 2.0 ** -133, 2.0 ** -127, 2.0 ** -126, 1.5, 2.0 ** 127, float("inf")]
    if st == "f32":
        v += [2.0 ** -149, 2.0 ** -127 + 2.0 ** -149, 1.0 + 2.0 ** -23]
    t = torch.tensor(v, dtype=F64)
    t = torch.cat([t, -t])
    assert torch.equal(t.float().double(), t) and (st == "f32" or torch.equal(t.to(BF).double(), t))
    return t


def relu_inputs(st, numel, seed=101):
    """x (specials first, then Gaussians) and dy"""
    sp = relu_specials(st)
    x = gaussian(st, (numel,), seed)
    m = min(numel, sp.numel())
    x[:m] = sp[torch.randperm(sp.numel(), generator=_gen(seed + 1))][:m]
    return x, gaussian(st, (numel,), seed + 2)


def relu_fwd_ref(x):
    return torch.where(x > 0, x, torch.zeros_like(x))


def relu_bwd_ref(dy, y):
    return torch.where(y > 0, dy, torch.zeros_like(dy))


# ------------------------------------------------------------------------------------------------------------- axpby, add_n
K_AXPBY = 3


def axpby_ref(x, y, a, b):
    return a * x + b * y, abs(a) * x.abs() + abs(b) * y.abs()


def add_n_ref(xs):
    return sum(xs), sum(x.abs() for x in xs)


# ----------------------------------------------------------------------------------------------------------------- dropout
_M64 = (1 << 64) - 1


def mix64_scalar(z):
    """the kernel's hash of one 64-bit value in Python integers (the definition the vector form is checked against)"""
    z = (z + 0x9E3779B97F4A7C15) & _M64
    z = ((z ^ (z >> 30)) * 0xBF58476D1CE4E5B9) & _M64
    z = ((z ^ (z >> 27)) * 0x94D049BB133111EB) & _M64
    z ^= z >> 31
    return z >> 40


def effective_seed(seed, step):
    return seed & _M64 if step is None else (seed + step * 0xD1B54A32D192ED03) & _M64


@functools.lru_cache(maxsize=12)
def dropout_hash(seed, step, n):
    """top 24 bits of mix64(seed' * 0x100000001B3 + index) for index 0 .. n - 1: numpy uint64, which wraps"""
    base = (effective_seed(seed, step) * 0x100000001B3) & _M64
    z = np.arange(n, dtype=np.uint64) + np.uint64(base)
    z += np.uint64(0x9E3779B97F4A7C15)
    z = (z ^ (z >> np.uint64(30))) * np.uint64(0xBF58476D1CE4E5B9)
    z = (z ^ (z >> np.uint64(27))) * np.uint64(0x94D049BB133111EB)
    z ^= z >> np.uint64(31)
    return (z >> np.uint64(40)).astype(np.uint32)


def dropout_threshold(p):
    return np.uint32(np.float32(p) * np.float32(16777216.0))


def dropout_keep(seed, step, n, p, per_access=None):
    """bool [n]; per_access = W reproduces the defect 'index i * W in place of i * W + j'"""
    h = dropout_hash(seed, step, n)
    if per_access:
        h = h[(np.arange(n) // per_access) * per_access]
    return torch.from_numpy(h >= dropout_threshold(p))


def dropout_ref(x, keep, p):
    """fl32(x * fl32(1 / (1 - p))) where kept, 0 elsewhere (float64 holding fp32 values)"""
    scale = np.float32(1.0) / (np.float32(1.0) - np.float32(p))
    y = (x.float().cpu().numpy() * scale).astype(np.float32)
    return torch.where(keep, torch.from_numpy(y), torch.zeros(())).double()


@functools.lru_cache(maxsize=4)
def dropout_input(st, numel, seed=201):
    """nowhere zero, so the kept set shows in the output"""
    x = gaussian(st, (numel,), seed)
    return torch.where(x == 0, torch.ones_like(x), x)


# ---------------------------------------------------------------------------------------------------------------- max-pool
def pool_out(h):
    return (h + 2 - 3) // 2 + 1


def pool_input(n, h, w, c, kind, seed=301):
    """[n][h][w][c] integers in {-2..2}; 'relu': clamped at 0; 'special': -inf and NaN planted, also in the first and the last tap
    of a window"""
    x = ints((n, h, w, c), seed, -2, 2)
    if kind == "relu":
        x = x.clamp_min(0.0)
    if kind == "special":
        g = _gen(seed + 1)
        for v in (float("-inf"), float("nan")):
            k = max(1, x.numel() // 7)
            x.view(-1)[torch.randint(0, x.numel(), (k,), generator=g)] = v
        # window (oy, ox) = (1, 1) covers rows / columns 1 .. 3 where they exist: its first and last tap, in channels 0 and 1
        if h >= 4 and w >= 4:
            x[0, 1:4, 1:4, 0:2] = 1.0
            x[0, 1, 1, 0], x[0, 3, 3, 0] = float("nan"), 2.0
            x[0, 1, 1, 1], x[0, 3, 3, 1] = 2.0, float("nan")
            if c > 2:
                x[0, 1:4, 1:4, 2] = float("-inf")
    return x


def maxpool_ref(x):
    """x [n][h][w][c] -> y [n][ho][wo][c], window code ky * 3 + kx (uint8) and ATen's flat index, from F.max_pool2d on the CPU"""
    n, h, w, c = x.shape
    y, ind = F.max_pool2d(x.permute(0, 3, 1, 2).contiguous().float(), 3, 2, 1, return_indices=True)
    ho, wo = y.shape[2], y.shape[3]
    ky = ind // w - (2 * torch.arange(ho).view(1, 1, -1, 1) - 1)
    kx = ind % w - (2 * torch.arange(wo).view(1, 1, 1, -1) - 1)
    assert bool(((ky >= 0) & (ky < 3) & (kx >= 0) & (kx < 3)).all())
    code = (ky * 3 + kx).to(torch.uint8)
    return y.permute(0, 2, 3, 1).contiguous().double(), code.permute(0, 2, 3, 1).contiguous(), ind


def maxpool_bwd_ref(dy, ind, h, w):
    """dy [n][ho][wo][c], ATen's flat indices [n][c][ho][wo] -> dx [n][h][w][c]"""
    n, ho, wo, c = dy.shape
    dx = torch.zeros(n, c, h * w, dtype=F64)
    dx.scatter_add_(2, ind.reshape(n, c, -1), dy.permute(0, 3, 1, 2).reshape(n, c, -1))
    return dx.view(n, c, h, w).permute(0, 2, 3, 1).contiguous()


# ------------------------------------------------------------------------------------------------- row sums and broadcasts
def sum_rows_uses_double(c, ld, base_off=0, y_off=0):
    """glf_sum_rows_fwd takes sum_rows4_kernel (16-byte loads, double sums) iff c % 4 == 0, ld % 4 == 0 and both pointers sit on 16
    bytes (base_off / y_off: element offsets from an aligned allocation); otherwise sum_rows_kernel (scalar, fp32 sums)"""
    return c % 4 == 0 and ld % 4 == 0 and base_off % 4 == 0 and y_off % 4 == 0


def k_sum_rows(p, double_sums):
    return 1 if double_sums else math.ceil(p / 4) + 3 + 1


def sum_rows_ref(x, n, p, scale):
    c = x.shape[1]
    return scale * x.view(n, p, c).sum(1), abs(scale) * x.abs().view(n, p, c).sum(1)


def bcast_ref(x, p, scale, y0=None):
    """x [n][c] -> y [n * p][c] = scale x (+ y0)"""
    y = (scale * x).repeat_interleave(p, 0)
    mag = y.abs()
    return (y, mag) if y0 is None else (y + y0, mag + y0.abs())


K_BCAST, K_BCAST_ADD = 1, 2


def rows_ld(c, which, w=4):
    """the three strides of the issue: c, c + 4, c + 1 (16-bit storage: c, c + 8)"""
    return {"c": c, "cw": c + w, "c1": c + 1}[which]


# ----------------------------------------------------------------------------------------------------------------- softmax
def softmax_input(rows, cols, seed=401):
    """Gaussians scaled by 5 (fp32 values); in row 0 one entry dominates the rest of its row by 60"""
    x = gauss32((rows, cols), seed, 5.0)
    j = (7 * cols) // 11
    others = torch.cat([x[0, :j], x[0, j + 1:]])
    x[0, j] = (float(others.max()) if cols > 1 else 0.0) + 60.0
    return x.float().double()


def softmax_ref(x):
    """p, the per-element k (docstring above) -- float64"""
    cols = x.shape[1]
    m = x.max(1, keepdim=True).values
    t = x - m
    e = torch.exp(t)
    s = e.sum(1, keepdim=True)
    ke = t.abs() / 2 + K_TRANS
    S = (e * ke).sum(1, keepdim=True) / s + math.ceil(cols / 256) + 9
    return e / s, ke + S + 2


def softmax_bwd_inputs(fam, rows, cols, seed=411):
    if fam == "int":
        return pick((rows, cols), seed, [0.0, 0.25, 0.5]), ints((rows, cols), seed + 1, -2, 2)
    p = torch.softmax(gauss32((rows, cols), seed, 2.0), 1).float().double()
    return p, gauss32((rows, cols), seed + 1)


def softmax_bwd_ref(p, dy):
    s = (p * dy).sum(1, keepdim=True)
    smag = (p * dy).abs().sum(1, keepdim=True)
    return p * (dy - s), p.abs() * (dy.abs() + smag)


def k_softmax_bwd(cols):
    return math.ceil(cols / 256) + 12


# ---------------------------------------------------------------------------------------------------------------- bilinear
def bil_index(out_size, in_size, fused=False):
    """i0, i1, lambda1 per output coordinate, in fp32 as the kernel (numpy float32).  fused: s in ONE rounding (an fma)"""
    scale = np.float32(in_size) / np.float32(out_size)
    o = np.arange(out_size, dtype=np.float32) + np.float32(0.5)
    if fused:
        s = (o.astype(np.float64) * np.float64(scale) - 0.5).astype(np.float32)      # the product of two fp32 is exact in double
    else:
        s = (o * scale).astype(np.float32) - np.float32(0.5)
    s = np.maximum(s, np.float32(0.0)).astype(np.float32)
    i0 = np.minimum(s.astype(np.int64), in_size - 1)
    i1 = i0 + (i0 < in_size - 1)
    l1 = (s - i0.astype(np.float32)).astype(np.float32)
    return torch.from_numpy(i0), torch.from_numpy(i1), torch.from_numpy(l1.astype(np.float64))


def bil_matrix(out_size, in_size, unit=False):
    """[out][in] float64 interpolation weights from the fp32 indices and lambdas; unit: 1 at both source pixels of an output
    whatever their weights (the magnitude: a coordinate that moves shifts weight between the two)"""
    i0, i1, l1 = bil_index(out_size, in_size)
    m = torch.zeros(out_size, in_size, dtype=F64)
    r = torch.arange(out_size)
    if unit:
        m[r, i0] = 1.0
        m[r, i1] = 1.0
        return m
    m[r, i0] += 1.0 - l1
    m[r, i1] += l1
    return m


def bilinear_fwd_ref(x, ho, wo):
    """x [n][h][w][c] channels-last -> y [n][c][ho][wo] and its magnitude: the sum of |x| over the (up to) four source pixels"""
    n, h, w, c = x.shape
    my, mx = bil_matrix(ho, h), bil_matrix(wo, w)
    return torch.einsum("oh,nhwc,pw->ncop", my, x, mx), torch.einsum("oh,nhwc,pw->ncop", bil_matrix(ho, h, True), x.abs(), bil_matrix(wo, w, True))


def bilinear_bwd_ref(dy, h, w):
    """the exact adjoint: dy [n][c][ho][wo] -> dx [n][h][w][c], magnitude, and the largest number of contributing rows / columns"""
    ho, wo = dy.shape[2], dy.shape[3]
    my, mx = bil_matrix(ho, h), bil_matrix(wo, w)
    dx = torch.einsum("oh,ncop,pw->nhwc", my, dy, mx)
    mag = torch.einsum("oh,ncop,pw->nhwc", bil_matrix(ho, h, True), dy.abs(), bil_matrix(wo, w, True))
    return dx, mag, int((my != 0).sum(0).max()), int((mx != 0).sum(0).max())


def k_bilinear_fwd(h, w):
    return 7 + h + w


def k_bilinear_bwd(h, w, rows_c, cols_c):
    return rows_c + cols_c + 6 + h + w


# --------------------------------------------------------------------------------------------------------------------- gate
def gate_inputs(rows, ncls, seed=501):
    """class logits: multiples of 1/64 within +-8, so two logits of a row are bit-equal or at least 2^-6 apart (the issue asks for
    2^-10); every third row has its maximum planted twice (bit-equal: the first must win); centre logits within +-4.  Rows differ
    strongly: neighbouring rows' a are many intervals apart (asserted by gate_conditions)."""
    cls = ints((rows, ncls), seed, -512, 512) / 64.0
    if ncls > 1:
        for r in range(0, rows, 3):
            j = int(cls[r].argmax())
            cls[r, (j + 1 + r % (ncls - 1)) % ncls if ncls > 2 else 1 - j] = cls[r, j]
    ctr = ints((rows,), seed + 1, -256, 256) / 64.0
    return cls, ctr


def gate_conditions(cls):
    """from the inputs alone: two class logits of a row are bit-equal or differ by >= 2^-10 (the stated condition), and their
    sigmoids then differ by more than twice the 6 roundings charged to each (the derived one)"""
    d = (cls[:, :, None] - cls[:, None, :]).abs()
    ok1 = bool(((d == 0) | (d >= 2.0 ** -10)).all())
    s = torch.sigmoid(cls)
    ds = (s[:, :, None] - s[:, None, :]).abs()
    ok2 = bool(((d == 0) | (ds > 2 * (K_SIG + 4) * U)).all())
    return ok1 and ok2


def gate_fwd_ref(cls, ctr, weight=GATE_WEIGHT):
    """argmax (first maximum), a, and the per-row k of a"""
    best, bi = torch.sigmoid(cls).max(1)
    bi = (cls == cls.max(1, keepdim=True).values).int().argmax(1)          # the FIRST maximum, whatever torch.max returns
    cc = torch.sigmoid(ctr)
    u = weight * best * cc
    a = torch.sigmoid(u)
    return bi.to(torch.int32), a, 14.0 * u.abs() * (1.0 - a) + K_SIG


def product32(x, a32):
    """fl32(x a) for fp32 values x, a held in float64: the double product is exact, .float() rounds it once"""
    return (x * a32).float().double()


def k_gate_da(st, c, fam):
    if fam == "int":
        return 0
    return 1 + 3 * math.ceil(c / 256) + 6 if st == "f32" else 1 + 8 * math.ceil(c / 512) + 6


def gate_bwd_ref(dy, f, cls, ctr, a, bi, weight=GATE_WEIGHT):
    """dcls [rows][ncls], dctr [rows] with the magnitudes and the per-row k beyond k_da"""
    rows, ncls = cls.shape
    da, dam = (dy * f).sum(1), (dy * f).abs().sum(1)
    m = torch.sigmoid(cls.gather(1, bi.long().view(-1, 1))[:, 0])
    cc = torch.sigmoid(ctr)
    dt, dtm = da * a * (1 - a) * weight, dam * a * (1 - a) * abs(weight)
    hot = torch.zeros(rows, ncls, dtype=F64).scatter_(1, bi.long().view(-1, 1), 1.0).to(cls.device)
    dcls, dclsm = dt * cc * m * (1 - m), dtm * cc * m * (1 - m)
    dctr, dctrm = dt * m * cc * (1 - cc), dtm * m * cc * (1 - cc)
    base = 4 + K_SIG + K_SIG + 1 + 3
    return Bag(dcls=dcls[:, None] * hot, dclsm=dclsm[:, None] * hot, hot=hot.bool(), kcls=base + K_SIG * m / (1 - m),
               dctr=dctr, dctrm=dctrm, kctr=base + K_SIG * cc / (1 - cc))


# --------------------------------------------------------------------------------------------------------- BCE and overlap
def bce_inputs(numel, seed=601):
    """logits scaled by 6 with 0, +-20, +-90, +-104 planted; targets 0 / 1 with some 0.25 (non-zero, not 1)"""
    x = gauss32((numel,), seed, 6.0)
    x = torch.where((x != 0) & (x.abs() < 1e-3), torch.full_like(x, 0.5), x)
    k = min(numel, len(BCE_PLANTS))
    pos = torch.randperm(numel, generator=_gen(seed + 1))[:k]
    x[pos] = torch.tensor(BCE_PLANTS[:k], dtype=F64)
    t = pick((numel,), seed + 2, [0.0, 0.0, 1.0, 1.0, 0.25])
    return x, t


def overlap_condition(x):
    """no logit in (0, 1e-6) in magnitude except exact 0"""
    return bool(((x == 0) | (x.abs() >= 1e-6)).all())


K_BCE, K_BCE_DX = 7, 9


def bce_ref(x, t, g):
    """loss (sum), its magnitude; dx and its magnitude"""
    E = torch.exp(-x.abs())
    L = torch.log1p(E)
    loss = (x.clamp_min(0) - x * t + L).sum()
    mag = (x.clamp_min(0) + (x * t).abs() + L + E).sum()
    sg = torch.sigmoid(x)
    return loss, mag, (sg - t) * g, (sg + t.abs()) * abs(g)


def overlap_ref(x, t):
    pr, gt = x > 0, t != 0
    return torch.tensor([int((pr & gt).sum()), int((pr & ~gt).sum()), int((~pr & gt).sum()), int((~pr & ~gt).sum())], dtype=torch.int64)


# -------------------------------------------------------------------------------------------------------------------- stem
def stem_inputs(fam, n, h, w, pad, seed=701):
    ho, wo = h + 2 * pad - 6, w + 2 * pad - 6
    if fam == "int":
        b = Bag(x=ints((n, h, w), seed, 0, 1), w=ints((64, 49), seed + 1, -1, 1), bias=ints((64,), seed + 2, -1, 1),
                dy=ints((n, ho, wo, 64), seed + 3, -2, 2), mean=pick((64,), seed + 4, [-1.0, 0.0, 1.0]),
                invstd=pick((64,), seed + 5, [0.5, 1.0, 2.0]), gamma=pick((64,), seed + 6, [0.5, 1.0, 2.0]),
                beta=ints((64,), seed + 7, -8, 8) / 4.0)
    else:
        b = Bag(x=gauss32((n, h, w), seed, 1.0, 0.3), w=gauss32((64, 49), seed + 1, 0.3), bias=gauss32((64,), seed + 2, 0.5),
                dy=gauss((n, ho, wo, 64), seed + 3, 1.0, 0.1), mean=uniform32((64,), seed + 4, -0.5, 0.5),
                invstd=uniform32((64,), seed + 5, 0.4, 0.6), gamma=uniform32((64,), seed + 6, 0.5, 1.5), beta=uniform32((64,), seed + 7, -0.5, 0.5))
    b.ho, b.wo = ho, wo
    return b


def stem_fwd_ref(x, w, bias, pad):
    """x [n][h][w], w [64][49] -> y [n][ho][wo][64] and its magnitude"""
    f = lambda xx, ww, bb: F.conv2d(xx[:, None], ww.view(64, 1, 7, 7), bb, padding=pad).permute(0, 2, 3, 1).contiguous()
    return f(x, w, bias), f(x.abs(), w.abs(), bias.abs())


K_STEM_FWD, K_STEM_POOL = 49, 49 + 4


def stem_wgrad_ref(x, dy, pad):
    """dw [64][49], db [64] with magnitudes"""
    g = dy.permute(0, 3, 1, 2).contiguous()
    f = lambda xx, gg: torch.nn.grad.conv2d_weight(xx[:, None], (64, 1, 7, 7), gg, padding=pad).reshape(64, 49)
    return f(x, g), f(x.abs(), g.abs()), g.sum((0, 2, 3)), g.abs().sum((0, 2, 3))


def k_stem_wgrad(ho, wo):
    return min(16, ho) * min(16, wo) + 1


def stem_pool_ref(y, ymag, mean, invstd, gamma, beta):
    """maxpool3x3s2p1(relu(bn(y))) on [n][ho][wo][64] and the magnitude of the window's widest interval"""
    v = (y - mean) * invstd * gamma + beta
    vm = (ymag + mean.abs()) * invstd.abs() * gamma.abs() + beta.abs()
    pool = lambda t: F.max_pool2d(t.permute(0, 3, 1, 2), 3, 2, 1).permute(0, 2, 3, 1).contiguous()
    return pool(torch.relu(v)), pool(vm)


# --------------------------------------------------------------------------------------------- transposes and re-layouts
def rows_pads(rows, tile):
    return sorted({rows, rows + 1, (rows + tile - 1) // tile * tile + 1})


def relayout_refs(w):
    """w [cout][cin][taps] -> tap-major [taps][cout][cin] and its dgrad form [taps][cin][cout]"""
    return w.permute(2, 0, 1).contiguous(), w.permute(2, 1, 0).contiguous()
