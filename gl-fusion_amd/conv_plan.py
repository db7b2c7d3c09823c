"""The launch plan of a convolution pass: which taps can reach the map, whether the pass runs dense, as per-tap rectangles or in
region mode, how many reduction slices the weight gradient is cut into, whether the output must be zero-filled first and whether
fused column statistics can be honoured.  ONE pure function, plan(), for every pass, precision and storage; the slice-count
rules of the TN kernels live beside it.  Every wrapper asks it: the 16-bit-storage ones of ops16 and the fp32-storage ones of ops
(Conv2dFn, the fallback loops of AsppCentreFn, conv_stats_fusable, fold_plan).  ops holds none of the rules; it re-exports
tap_mask, rect_fraction, RECT_THRESHOLD and CENTRE_TAP as these very objects.  Pure Python (no torch, no library):
glf_conv2d_plan of csrc/conv_api.hip is the same policy for C hosts (fp32 storage, no `keep`), and tests/test_abi_cpu.py holds the
C plan to this planner field by field and to the rules restated one by one; tests/test_conv_plan_cpu.py holds the planner to a
table recorded from the rules as ops and ops16 spelled them before it existed."""
from __future__ import annotations

from functools import lru_cache
from typing import NamedTuple, Optional, Tuple

PASSES = ("fwd", "dgrad", "wgrad", "fwd_folded")          # passes 0..3 of glf_conv2d_plan
S16 = 4                                                   # index of "bf16" (16-bit storage) in ops.PRECISIONS
CENTRE_TAP = 1 << 4                                       # of a 3x3 kernel

# use rect mode when less than this fraction of the kept taps' work is in range (per conv pass)
# The rectangle GEMMs sum their taps with float atomics; dgrad writes the widest outputs (Cin = 2048 columns for
# ASPP) over the shortest reductions (Cout = 256), so once the MFMA work is cheap (f16x3) the atomics cost more
# than the padding work they avoid unless most of it is padding: measured on the ASPP shapes, rate 12 (51 % in
# range) is faster dense, rate 24 (18 %) faster as rectangles.
# (plan() is memoised: whoever changes an entry calls plan.cache_clear())
RECT_THRESHOLD = {"fwd": 0.8, "dgrad": 0.8, "wgrad": 0.8, "dgrad_f16x3": 0.35, "region": 0.8}


def conv_out(h: int, k: int, stride: int, pad: int, dil: int) -> int:
    return (h + 2 * pad - dil * (k - 1) - 1) // stride + 1


def _axis_valid(gather: int, hd: int, hs: int, k: int, stride: int, pad: int, dil: int):
    if gather == 1:
        return [any(0 <= y * stride - pad + t * dil < hs for y in range(hd)) for t in range(k)]
    return [any(v >= 0 and v % stride == 0 and v // stride < hs for v in (y + pad - t * dil for y in range(hd))) for t in range(k)]


@lru_cache(maxsize=None)
def tap_mask(gather: int, hd: int, wd: int, hs: int, ws: int, kh: int, kw: int, stride: int, pad: int, dil: int) -> int:
    """Bit t set = tap t can be in range for some destination pixel.  gather 1: destination = output map (forward, wgrad);
    gather 2: destination = input map (dgrad)."""
    vy, vx = _axis_valid(gather, hd, hs, kh, stride, pad, dil), _axis_valid(gather, wd, ws, kw, stride, pad, dil)
    return sum(1 << (ky * kw + kx) for ky in range(kh) for kx in range(kw) if vy[ky] and vx[kx])


@lru_cache(maxsize=None)
def rect_fraction(gather: int, hd: int, wd: int, hs: int, ws: int, kh: int, kw: int, pad: int, dil: int, mask: int) -> float:
    """sum over kept taps of (in-range rectangle area) / (kept taps x full area), stride 1 (mirrors tap_rect
    in gemm_f32.hip).  Small values = most tap work is padding => the tap-parallel rect mode pays."""
    tot, n = 0, 0
    for t in range(kh * kw):
        if not (mask >> t) & 1:
            continue
        ky, kx = divmod(t, kw)
        oy = pad - ky * dil if gather == 1 else ky * dil - pad
        ox = pad - kx * dil if gather == 1 else kx * dil - pad
        tot += max(0, min(hs + oy, hd) - max(oy, 0)) * max(0, min(ws + ox, wd) - max(ox, 0))
        n += 1
    return tot / max(1, n * hd * wd)


def tn_split(rows: int, m: int, n: int, ntaps: int, batch: int = 1, prec: int = 0) -> int:
    """Reduction slices for the fp32-storage TN (wgrad) kernels under precision `prec`: fill ~4 waves of 512 resident workgroups,
    keep >= 16 K-tiles (512 rows) per slice."""
    tiles = ((m + 127) // 128) * ((n + 127) // 128) * max(ntaps, 1) * batch
    # workgroups to aim for: 2048 128x128 tiles on the fp32 / bf16x6 kernels (two per CU); the f16x3 kernel has 256-wide
    # tiles, one workgroup per CU, and shares the chip with other streams: 1024 measured best (293.5 vs 299.2 ms / step)
    target = 1024 if prec >= 2 else 2048
    want = max(1, (target + tiles - 1) // tiles)
    cap = max(1, rows // 512)
    hi = 65535 // max(batch, 1)
    if prec >= 2:
        # among the slice counts around the target, the one whose workgroups (256-wide tiles, one per CU) fill whole
        # rounds of the 256 CUs best
        wg = ((m + 255) // 256) * ((n + 127) // 128) * max(ntaps, 1) * batch
        best, best_score = want, -1.0
        for s in range(max(1, want // 2), max(1, min(want * 2, cap, hi)) + 1):
            b = wg * s
            score = b / (((b + 255) // 256) * 256.0) - 0.004 * s
            if score > best_score:
                best, best_score = s, score
        want = best
    return int(max(1, min(want, cap, hi)))


def tn_split16(rows: int, m: int, n: int, ntaps: int, batch: int = 1) -> int:
    """Reduction slices of glf_s16_gemm_tn: 256 x 128 tiles, one workgroup per CU.  Aim for ~2 rounds of the 256 CUs and, among the
    slice counts around that, take the one whose workgroups fill whole rounds best (576 workgroups = 2.25 rounds run as long as
    768 = 3); keep at least 512 rows per slice (every slice costs an [M][N] fp32 slab written and read back)."""
    tiles = ((m + 255) // 256) * ((n + 127) // 128) * max(ntaps, 1) * batch
    want = max(1, (512 + tiles - 1) // tiles)
    cap = max(1, min(rows // 512, 65535 // max(batch, 1)))
    best, best_score = min(want, cap), -1.0
    for sp in range(max(1, want // 2), max(1, min(2 * want, cap)) + 1):
        b = tiles * sp
        score = b / (((b + 255) // 256) * 256.0) - 0.01 * sp
        if score > best_score:
            best, best_score = sp, score
    return int(max(1, min(best, cap)))


def wgrad_split(rows_o: int, frac: float, cout: int, cin: int, ntap: int, rect: bool, prec: int) -> int:
    """Reduction slices of a convolution's weight gradient.  A slice is ceil(rows / split) rows of EVERY tap's reduction; in rect
    mode (ASPP: most taps reach only a small rectangle of the map) a tap uses as many slices as its rectangle is long, so the count
    is scaled up by the in-range fraction to keep the launch at its target size -- and all workgroups reduce the same number of
    rows (before: every tap was cut into `split` pieces of its own rectangle, the centre tap's workgroups ran 3 x (rate 12) to
    50 x (rate 24) longer than the corner taps')."""
    if prec == S16:
        if not rect:
            return tn_split16(rows_o, cout, cin, ntap)
        s_in = tn_split16(max(512, int(rows_o * frac)), cout, cin, ntap)
        return max(2, min(int(s_in / max(frac, 0.02) + 0.999), max(2, rows_o // 512), 65535))
    split = tn_split(max(512, int(rows_o * frac)) if rect else rows_o, cout, cin, ntap, 1, prec)
    if rect:
        # (measured on the 2048 -> 256 ASPP convs, profiles/r03_aspp_wgrad_probe.txt: half of split / frac is the sweet spot --
        # rate 12: 7 slices 1.01 ms, 14 slices 1.22 ms; rate 24: 19 slices 0.48 ms, 39 slices 0.50 ms, 78 slices 0.57 ms)
        s2 = max(split, int(split / (2.0 * max(frac, 0.02)) + 0.999))
        split = max(1, min(s2, max(1, rows_o // 512), 65535))
    return split


class ConvPlan(NamedTuple):
    ho: int
    wo: int
    taps: int
    plain: bool                       # a 1x1 stride-1 unpadded conv: a plain contraction, no gather
    mask: int                         # the taps the launch contracts
    kept: int                         # their number
    rect: int                         # 0 dense, 1 per-tap rectangles (float atomics), 2 regions with a constant tap set
    split: int                        # reduction slices (wgrad)
    zero_fill: bool                   # the destination must hold zeros before the launch
    gather: int
    geo: Optional[Tuple[int, ...]]    # the 10-tuple gemm() takes; None for a plain conv
    M: int
    N: int
    K: int
    colstats_ok: bool                 # fwd: fused column statistics are honoured

    @property
    def workspace_bytes(self) -> int:
        """Of the two-stage reduction of a sliced weight gradient (glf_conv_plan.workspace_bytes)."""
        return self.split * self.kept * self.M * self.N * 4 if self.split > 1 else 0


@lru_cache(maxsize=None)
def plan(pass_: str, geom: Tuple[int, ...], prec: int, keep: Optional[int] = None, bias: bool = False) -> ConvPlan:
    """The plan of pass `pass_` (one of PASSES) of the conv geom = (n, h, w, cin, cout, kh, kw, stride, pad, dil) under precision
    `prec` (index into ops.PRECISIONS; S16 = bf16 storage).  bias: the forward adds one (per-tap rectangles cannot).
    keep: a tap bit mask of the ASPP centre-tap callers, which evaluate the centre tap elsewhere -- two semantics, as introduced:
      fwd / dgrad ("Evaluate the centre taps of the ASPP branches as one contraction"): the branch keeps the launch it would use
        alone -- the mode is decided on the FULL mask, the launch then runs mask & keep and adds into what the stacked launch
        stored (no zero fill);
      wgrad ("Stack the ASPP centre-tap weight gradients; reduce 3x3 wgrads to OIHW"): a reduction of its own over the remaining
        taps -- the mode and the slice count are decided on the REDUCED mask."""
    n, h, w, cin, cout, kh, kw, stride, pad, dil = geom
    ho, wo = conv_out(h, kh, stride, pad, dil), conv_out(w, kw, stride, pad, dil)
    taps = kh * kw
    plain = taps == 1 and stride == 1 and pad == 0
    to_input = pass_ == "dgrad"
    # destination grid = what the GEMM rows enumerate (dgrad: the input map); source grid = what is gathered
    grids = (2, h, w, ho, wo) if to_input else (1, ho, wo, h, w)
    mask = 1 if plain else tap_mask(*grids, kh, kw, stride, pad, dil)
    if keep is not None and pass_ == "wgrad":
        mask &= keep
    kept = bin(mask).count("1")
    frac = 1.0 if plain or stride != 1 else rect_fraction(*grids, kh, kw, pad, dil, mask)
    tapwise = not plain and taps > 1 and stride == 1 and kept > 1               # more than one tap to run side by side
    same3 = taps == 9 and kh == 3 and stride == 1 and pad == dil and ho == h and wo == w and kept > 1       # what region mode covers
    thr = RECT_THRESHOLD
    rect, split = 0, 1
    if pass_ == "wgrad":
        rect = int(tapwise and frac < thr["wgrad"] and (prec != S16 or n * ho * wo >= 2048))
        split = wgrad_split(n * ho * wo, frac if rect else 1.0, cout, cin, kept, bool(rect), prec) if kept else 1
    elif prec == S16:
        rect = 2 if same3 and frac < thr["region"] else 0                       # the 16-bit kernels store every element once
    elif to_input:
        # region mode (f16x3 kernels): no padding work, no atomics, no zero fill.  Used for the dgrad of the ASPP rate-12 / 24 convs
        # (2048-column outputs): 14.4 -> 11.2 ms and 7.6 -> 6.7 ms per step against dense / per-tap rectangles with atomics.
        # Measured NOT to pay elsewhere: the forward of the same convs (256-column outputs, 392 workgroups) is faster as per-tap
        # rectangles -- the regions' blocks are fewer and of uneven length (4 / 6 / 9 taps) -- and for dilations 1-4 the 5-18 % of
        # padding work saved is less than the extra partial tiles and the per-element pixel arithmetic of the epilogue cost.
        if prec >= 2 and same3 and cout % 32 == 0 and frac < thr["region"]:
            rect = 2
        else:
            rect = int(tapwise and frac < thr["dgrad_f16x3" if prec >= 2 else "dgrad"])
    else:
        rect = int(tapwise and not bias and frac < thr["fwd"])
        # folded forward: the epilogue needs every element stored once -- regions instead of per-tap rectangles where they exist
        if pass_ == "fwd_folded" and rect and prec >= 2 and same3 and cin % 32 == 0:
            rect = 2
    full = mask == (1 << taps) - 1
    if keep is not None and pass_ != "wgrad":
        mask &= keep
        kept = bin(mask).count("1")
    if pass_ == "wgrad":
        zero_fill, (M, N, K) = not full, (cout, cin, n * ho * wo)               # taps outside the mask stay zero
    else:
        zero_fill = keep is None and (rect == 1 or (to_input and mask == 0))
        M, N, K = (n * h * w, cin, cout) if to_input else (n * ho * wo, cout, cin)
    stats = pass_ == "fwd" and (cin % 64 == 0 and cout % 64 == 0 if prec == S16 else prec >= 2 and cin % 32 == 0 and cout % 4 == 0 and rect == 0)
    geo = None if plain else ((n, ho, wo, h, w) if to_input else (n, h, w, ho, wo)) + (kh, kw, stride, pad, dil)
    return ConvPlan(ho, wo, taps, plain, mask, kept, rect, split, zero_fill, 0 if plain else grids[0], geo, M, N, K, stats)
