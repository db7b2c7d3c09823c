"""16-bit-storage ("S16") autograd nodes: BASELINE.json configs[2] / [4] -- bf16 activations, saved-for-backward tensors and
activation gradients in HBM, fp32 master weights and weight gradients, fp32 MFMA accumulation.

`ops.set_precision("bf16")` selects the mode; the public functions of glfusion_amd.ops dispatch here on the tensor's dtype
(torch.bfloat16), so the model code is the same for every precision.  Every function launches glf_s16_* kernels from
libglfusion_hip.so on the current HIP stream; nothing here is a torch compute op and there is no fallback.

Only what the storage mode does differently lives here: the contractions, convolutions, BatchNorm and the casts (the fusion block: fusion16.py).
The streaming ops in between (ReLU, dropout, pooling, broadcast, gate, axpby, fan-in sums, view stacking) are the nodes of
glfusion_amd.ops, which serve both storage dtypes.

What stays fp32 in this mode: the input images, the 5- / 1-channel head logits and everything after them (bilinear
up-sampling, loss, metrics), per-channel statistics and every parameter / parameter gradient.
"""
from __future__ import annotations

import ctypes as C
import os
from typing import Optional, Sequence

import torch
from torch.autograd import Function
from torch.autograd.function import once_differentiable

from ._lib import GemmParams, S16GemmEpilogue, WJ_CVT_BF16, check, lib
from . import conv_plan, ops as _o
from .conv_plan import S16, tn_split16          # (fusion16 takes its slice counts from here)

BF, DT_F32, DT_BF16 = _o.BF, _o.DT_F32, _o.DT_BF16
_p, _stream, _contig = _o._p, _o._stream, _o._contig
# block sequences (fusion16.Tpavi16Fn, mode 'dot') through their single-call C entry points (glf_s16_tpavi_fwd / _bwd); 0 = composed
# from Python, the same launches.  A switch of the storage mode, read at call time
BLOCK_CALLS = os.environ.get("GLF_BLOCK_CALLS", "1") != "0"


def weight16(layout: torch.Tensor, owner: torch.Tensor, tag: str) -> torch.Tensor:
    """bf16 image of a dense fp32 weight layout derived from the parameter `owner` (tap-major / transposed / stacked forms of
    ops.tap_major & co), made once per weight update: a registered job of the multi-tensor refresh (GLF_WJ_CVT_BF16)."""
    n = layout.numel()
    if n % 8 != 0 or not layout.is_contiguous():
        raise RuntimeError("glfusion_amd: a 16-bit weight image needs a contiguous layout of 8n elements")
    im, fresh = _o._wimage(owner, "s16:" + tag, WJ_CVT_BF16, layout, (n, 0, 0), lambda: torch.empty(layout.shape, dtype=BF, device=layout.device))
    if fresh:
        check(lib.glf_s16_cast(_p(layout), DT_F32, _p(im.dst), DT_BF16, n, _stream()), "s16_cast(weight)")
    return im.dst


KERNEL_NAMES = {("nt", False): "s16_rows_kernel<false>", ("nt", True): "s16_rows_kernel<true>",
                ("tn", False): "s16_tn_kernel<false>", ("tn", True): "s16_tn_kernel<true>"}


def gemm16(mode: str, A: torch.Tensor, B: torch.Tensor, Cm: torch.Tensor, *, M: int, N: int, K: int, lda: int, ldb: int, ldc: int,
           bias: Optional[torch.Tensor] = None, taps: int = 1, mask: int = 1, tap_stride_b: int = 0, gather: int = 0, geo=None,
           batch: int = 1, bsa: int = 0, bsb: int = 0, bsc: int = 0, alpha: float = 1.0, accumulate: bool = False, split: int = 1,
           rect: int = 0, colstats: Optional[torch.Tensor] = None, epilogue=None) -> None:
    """glf_s16_gemm_nt / glf_s16_gemm_tn (include/glfusion.h).  A, B: bf16; Cm: bf16 or fp32 (its dtype is what is stored).
    epilogue ('nt' only): (bf16 residual or None, its row stride, relu) -- the call goes to glf_s16_gemm_nt_epilogue, which stores
    bf16(act(alpha * acc + bias[n] + residual[m][n])) once (bias is then required: the folded BatchNorm shift)."""
    p = GemmParams()
    p.M, p.N, p.K, p.lda, p.ldb, p.ldc = M, N, K, lda, ldb, ldc
    p.taps, p.tap_mask, p.tap_stride_b, p.gather = taps, mask, tap_stride_b, gather
    (p.n_img, p.hs, p.ws, p.hd, p.wd, p.kh, p.kw, p.stride, p.pad, p.dil) = geo if geo is not None else (1, 1, 1, 1, 1, 1, 1, 1, 0, 1)
    p.batch, p.batch_stride_a, p.batch_stride_b, p.batch_stride_c = batch, bsa, bsb, bsc
    p.alpha, p.accumulate, p.split, p.rect = alpha, int(accumulate), split, int(rect)
    p.colstats = _p(colstats)
    p.c_dtype = DT_BF16 if Cm.dtype == BF else DT_F32
    ws = None
    if mode == "tn" and split > 1:
        nbytes = int(lib.glf_s16_gemm_tn_workspace_bytes(C.byref(p)))
        ws = torch.empty(nbytes // 4, dtype=torch.float32, device=Cm.device)
        p.workspace, p.workspace_bytes = _p(ws), nbytes
    prof = _o.PROFILER
    if prof is not None:
        ev0 = torch.cuda.Event(enable_timing=True)
        ev0.record()
    if mode == "nt" and epilogue is not None:
        e = S16GemmEpilogue()
        e.shift, e.residual, e.ld_res, e.relu = _p(bias), _p(epilogue[0]), int(epilogue[1]), int(bool(epilogue[2]))
        check(lib.glf_s16_gemm_nt_epilogue(_p(A), _p(B), _p(Cm), C.byref(p), C.byref(e), _stream()), "s16_gemm_nt_epilogue")
    elif epilogue is not None:
        raise ValueError("gemm16: the fused epilogue exists for mode 'nt' only")
    elif mode == "nt":
        check(lib.glf_s16_gemm_nt(_p(A), _p(B), _p(bias), _p(Cm), C.byref(p), _stream()), "s16_gemm_nt")
    elif mode == "tn":
        check(lib.glf_s16_gemm_tn(_p(A), _p(B), _p(Cm), C.byref(p), _stream()), "s16_gemm_tn")
    else:
        raise ValueError(mode)
    if prof is not None:
        ev1 = torch.cuda.Event(enable_timing=True)
        ev1.record()
        kept = bin(mask).count("1")
        dense = 2.0 * M * N * K * taps * batch
        src_rows = (geo[0] * geo[1] * geo[2]) if geo else None
        in_range = conv_plan.rect_fraction(gather, geo[3], geo[4], geo[1], geo[2], geo[5], geo[6], geo[8], geo[9], mask) if (rect and geo and gather) else 1.0
        csz = 2 if Cm.dtype == BF else 4
        if mode == "tn":
            abytes = batch * (2.0 * (K * M + (src_rows if src_rows else K) * N) + csz * M * N * kept)
        else:
            abytes = batch * (2.0 * ((src_rows if src_rows else M) * K + N * K * kept) + csz * M * N * (2 if accumulate else 1))
        prof.append((KERNEL_NAMES[(mode, gather != 0)], dense, dense * kept / taps * in_range, ev0, ev1,
                     (M, N, K, taps, kept, batch, split, geo[8] if geo else 0, geo[9] if geo else 0), abytes))


def s16_conv_ok(cin: int, cout: int) -> bool:
    """A convolution runs on the 16-bit kernels when forward (K = Cin), dgrad (K = Cout) and wgrad (M = Cout, N = Cin) all fit."""
    return cin % 64 == 0 and cout % 64 == 0


# ----------------------------------------------------------------------------------------
# casts at the border of the 16-bit domain
# ----------------------------------------------------------------------------------------
class ToF32Fn(Function):
    @staticmethod
    def forward(ctx, x):
        x = _contig(_o._chk(x, "cast input", BF))
        y = torch.empty(x.shape, dtype=torch.float32, device=x.device)
        check(lib.glf_s16_cast(_p(x), DT_BF16, _p(y), DT_F32, x.numel(), _stream()), "s16_cast")
        return y

    @staticmethod
    @once_differentiable
    def backward(ctx, dy):
        dy = _contig(dy)
        dx = torch.empty(dy.shape, dtype=BF, device=dy.device)
        check(lib.glf_s16_cast(_p(dy), DT_F32, _p(dx), DT_BF16, dy.numel(), _stream()), "s16_cast")
        return dx


class ToBF16Fn(Function):
    @staticmethod
    def forward(ctx, x):
        x = _contig(_o._chk(x, "cast input"))
        y = torch.empty(x.shape, dtype=BF, device=x.device)
        check(lib.glf_s16_cast(_p(x), DT_F32, _p(y), DT_BF16, x.numel(), _stream()), "s16_cast")
        return y

    @staticmethod
    @once_differentiable
    def backward(ctx, dy):
        dy = _contig(dy)
        dx = torch.empty(dy.shape, dtype=torch.float32, device=dy.device)
        check(lib.glf_s16_cast(_p(dy), DT_BF16, _p(dx), DT_F32, dy.numel(), _stream()), "s16_cast")
        return dx


def to_f32(x):
    return ToF32Fn.apply(x)


def to_bf16(x):
    return ToBF16Fn.apply(x)


def colsum16(dy2d: torch.Tensor, rows: int, c: int, ld: Optional[int] = None) -> torch.Tensor:
    db = torch.empty(c, dtype=torch.float32, device=dy2d.device)
    ws = torch.empty(2 * c, dtype=torch.float64, device=dy2d.device)
    check(lib.glf_s16_colsum(_p(dy2d), ld if ld is not None else c, _p(db), rows, c, _p(ws), _stream()), "s16_colsum")
    return db


# ----------------------------------------------------------------------------------------
# conv2d
# ----------------------------------------------------------------------------------------
class Conv2d16Fn(Function):
    """F.conv2d on bf16 [N,H,W,Cin] with the fp32 torch-layout weight [Cout,Cin,kh,kw] (groups = 1); bf16 result."""

    @staticmethod
    def forward(ctx, x, weight, bias, stride: int, pad: int, dil: int, colstats=None):
        _o._chk(x, "conv input", BF); _o._chk(weight, "conv weight")
        x = _contig(x)
        n, h, w, cin = x.shape
        cout, cin_w, kh, kw = weight.shape
        if cin_w != cin:
            raise RuntimeError(f"conv2d: input has {cin} channels, weight expects {cin_w}")
        geom = (n, h, w, cin, cout, kh, kw, stride, pad, dil)
        pl = conv_plan.plan("fwd", geom, S16)
        if pl.ho <= 0 or pl.wo <= 0:
            raise RuntimeError("conv2d: empty output")
        wt = weight16(_o.tap_major(weight), weight, "w")
        y = torch.empty(n, pl.ho, pl.wo, cout, dtype=BF, device=x.device)
        gemm16("nt", x, wt, y, M=pl.M, N=cout, K=cin, lda=cin, ldb=cin, ldc=cout, bias=bias, taps=pl.taps, mask=pl.mask,
               tap_stride_b=cout * cin, gather=pl.gather, geo=pl.geo, rect=pl.rect, colstats=colstats)
        ctx.save_for_backward(x)
        ctx.weight_ref = weight
        ctx.cfg = (geom, bias is not None, tuple(weight.shape))
        return y

    @staticmethod
    @once_differentiable
    def backward(ctx, dy):
        (x,) = ctx.saved_tensors
        geom, has_bias, wshape = ctx.cfg
        cin, cout = geom[3], geom[4]
        weight = ctx.weight_ref
        dy = _contig(dy)
        dx = dw = db = None

        def dgrad():
            pl = conv_plan.plan("dgrad", geom, S16)
            if pl.mask == 0:
                return _o.zeros(x.shape, dtype=BF, device=x.device)
            dx = torch.empty_like(x)
            wT = weight16(_o.tap_major_T(weight), weight, "wT")
            gemm16("nt", dy, wT, dx, M=pl.M, N=cin, K=cout, lda=cout, ldb=cout, ldc=cin, taps=pl.taps, mask=pl.mask,
                   tap_stride_b=cout * cin, gather=pl.gather, geo=pl.geo, rect=pl.rect)
            return dx

        def wgrad():
            # taps that fall mostly into the padding (ASPP rates 12 / 24) on a map of >= 2048 rows: rectangle mode -- a tap reduces over
            # its in-range output pixels only.  A slice is the same number of rows for every tap (a short rectangle uses fewer slices),
            # so the slice count is the one of the in-range rows scaled back up to the whole map (conv_plan.wgrad_split).
            pl = conv_plan.plan("wgrad", geom, S16)
            taps = pl.taps
            if taps == 1 and not pl.zero_fill:
                dwt = _o.grad_out(weight, (1, cout, cin), x.device)
            else:
                dwt = (_o.zeros if pl.zero_fill else torch.empty)(taps, cout, cin, dtype=torch.float32, device=x.device)
            gemm16("tn", dy, x, dwt, M=cout, N=cin, K=pl.K, lda=cout, ldb=cin, ldc=cin, taps=taps, mask=pl.mask, tap_stride_b=cout * cin,
                   gather=pl.gather, geo=pl.geo, split=pl.split, rect=pl.rect)
            if taps == 1:
                return dwt.view(wshape)
            dw = _o.grad_out(weight, wshape, x.device)
            check(lib.glf_tap_major_to_oihw(_p(dwt), _p(dw), cout, cin, taps, _stream()), "tap_major_to_oihw")
            return dw

        if ctx.needs_input_grad[0]:
            dx = dgrad()
        if ctx.needs_input_grad[1]:
            dw = wgrad()
        if has_bias and ctx.needs_input_grad[2]:
            db = colsum16(dy, dy.numel() // cout, cout)
        return dx, dw, db, None, None, None, None


def conv2d(x, weight, bias=None, stride: int = 1, pad: int = 0, dil: int = 1, colstats=None):
    cout, cin = weight.shape[0], weight.shape[1]
    if not s16_conv_ok(cin, cout):
        # narrow outputs (the 5- / 1-channel head logits): through the exact fp32 kernels, result stays fp32
        if colstats is not None:
            raise RuntimeError("glfusion_amd: fused statistics need a convolution that runs on the 16-bit kernels")
        return _o.Conv2dFn.apply(to_f32(x), weight, bias, stride, pad, dil, None)
    return Conv2d16Fn.apply(x, weight, bias, stride, pad, dil, colstats)


class ConvCat16Fn(Function):
    """1x1 conv over the channel concatenation of inputs that ARE the column slices of one [..., ctot] bf16 buffer (ASPP project,
    deeplabv3.py:153-165): one K = ctot contraction."""

    @staticmethod
    def forward(ctx, weight, bias, colstats, *xs):
        _o._chk(weight, "weight")
        cout, ctot = weight.shape[0], weight.shape[1]
        t0 = _o._chk(xs[0], "input", BF)
        offs = [0]
        for t in xs:
            offs.append(offs[-1] + t.shape[-1])
        cat = (offs[-1] == ctot and t0.stride(-1) == 1 and t0.stride(-2) == ctot
               and all(_o._chk(t, "input", BF).stride() == t0.stride() and t.shape[:-1] == t0.shape[:-1]
                       and t.data_ptr() == t0.data_ptr() + 2 * o for t, o in zip(xs, offs)))
        if not cat:
            raise RuntimeError("glfusion_amd: 16-bit conv1x1_cat needs its inputs to be the column slices of one buffer")
        rows = t0.numel() // t0.shape[-1]
        w2 = _contig(weight.detach()).view(cout, ctot)
        y = torch.empty(*t0.shape[:-1], cout, dtype=BF, device=t0.device)
        gemm16("nt", t0, weight16(w2, weight, "w"), y, M=rows, N=cout, K=ctot, lda=ctot, ldb=ctot, ldc=cout, bias=bias, colstats=colstats)
        ctx.save_for_backward(*xs)
        ctx.weight_ref = weight
        ctx.cfg = (rows, cout, ctot, bias is not None, tuple(weight.shape))
        return y

    @staticmethod
    @once_differentiable
    def backward(ctx, dy):
        xs = ctx.saved_tensors
        rows, cout, ctot, has_bias, wshape = ctx.cfg
        weight = ctx.weight_ref
        dy = _contig(dy)
        t0 = xs[0]
        dw = db = None
        grads = [None] * len(xs)
        w2 = _contig(weight.detach()).view(cout, ctot)
        if any(ctx.needs_input_grad[3:]):
            dcat = torch.empty(*t0.shape[:-1], ctot, dtype=BF, device=dy.device)
            gemm16("nt", dy, weight16(_o.weight_T(w2, weight), weight, "T2"), dcat, M=rows, N=ctot, K=cout, lda=cout, ldb=cout, ldc=ctot)
            off = 0
            grads = []
            for t in xs:
                grads.append(dcat[..., off:off + t.shape[-1]])
                off += t.shape[-1]
        if ctx.needs_input_grad[0]:
            dw = _o.grad_out(weight, (cout, ctot), dy.device)
            gemm16("tn", dy, t0, dw, M=cout, N=ctot, K=rows, lda=cout, ldb=ctot, ldc=ctot, split=tn_split16(rows, cout, ctot, 1))
            dw = dw.view(wshape)
        if has_bias and ctx.needs_input_grad[1]:
            db = colsum16(dy, rows, cout)
        return (dw, db, None, *grads)


def conv1x1_cat(weight, xs: Sequence[torch.Tensor], bias=None, colstats=None):
    return ConvCat16Fn.apply(weight, bias, colstats, *xs)


# ----------------------------------------------------------------------------------------
# Folded-BatchNorm inference under 16-bit storage (opt-in: ops.set_fold_bn_s16).  Unfolded, the conv result is rounded to bf16 and
# THEN normalised; folded, W' = W * s_o is the bf16 B operand, the shift (and the residual, and the clamp) are applied to the fp32
# accumulator and the value is rounded to bf16 once, after normalisation.
# ----------------------------------------------------------------------------------------
_fold_cache16 = {}          # keyed apart from ops._fold_cache: one model may run folded under 'f16x3' and under 'bf16' in one process


def fold_plan16(x: torch.Tensor, weight: torch.Tensor, bn, stride: int, pad: int, dil: int):
    """(plain, mask, rect, ho, wo) when conv(x, weight) -> bn runs on the folded 16-bit path right now, else None: switch on,
    precision 'bf16', no autograd graph, BatchNorm in eval mode with running statistics and affine parameters, a bf16 NHWC device
    tensor, a conv the 16-bit kernels take, more than 64 output rows (the ASPP pooled branch keeps its path) and at least one tap
    that can touch the map.  Every conv forward of this mode stores each element once (the ASPP rates run in region mode), so
    nothing has to be planned around."""
    if not _o._FOLD_BN_S16[0] or not _o._S16[0] or torch.is_grad_enabled():
        return None
    if bn.training or bn.running_mean is None or bn.running_var is None or bn.weight is None or bn.bias is None:
        return None
    if x.dim() != 4 or x.dtype != BF or not x.is_cuda:
        return None
    n, h, w, cin = x.shape
    cout, cin_w, kh, kw = weight.shape
    if cin_w != cin or not s16_conv_ok(cin, cout) or cin > (1 << 18):
        return None
    pl = conv_plan.plan("fwd_folded", (n, h, w, cin, cout, kh, kw, stride, pad, dil), S16)
    if pl.ho <= 0 or pl.wo <= 0 or pl.M <= 64 or pl.mask == 0:
        return None
    return pl.plain, pl.mask, pl.rect, pl.ho, pl.wo


def _folded_images16(weight: torch.Tensor, bias: Optional[torch.Tensor], bn):
    """(folded tap-major bf16 weights [taps][Cout][Cin], fp32 shift [Cout]): ops._folded_images with a cache of its own and
    glf_s16_fold_bn as the fold -- the same stamp of the six sources, re-folded in place only when it differs."""
    cout, cin, kh, kw = weight.shape
    hit, stamp = _o._fold_entry(_fold_cache16, weight, bias, bn, BF)
    if hit.stamp != stamp:
        wt = _o.tap_major(weight)
        check(lib.glf_s16_fold_bn(_p(wt), _p(bias.detach()) if bias is not None else None, _p(bn.weight.detach()), _p(bn.bias.detach()),
                                  _p(bn.running_mean), _p(bn.running_var), float(bn.eps), _p(hit.wf), _p(hit.shift), kh * kw, cout, cin,
                                  _stream()), "s16_fold_bn")
        _o.FOLD_COUNT[0] += 1
        hit.gen += 1
        hit.stamp = stamp
    return hit.wf, hit.shift


def conv_bn_folded16(x, weight, bias, bn, stride: int, pad: int, dil: int, relu: bool, residual=None, plan=None):
    """relu?(bn_eval(conv(x)) + residual?) in ONE glf_s16_gemm_nt_epilogue launch on bf16 NHWC tensors; plan = fold_plan16(...)
    (not None).  Writes into a pending ops.output_into view (the ASPP branches' column slices of the shared buffer)."""
    if plan is None:
        raise RuntimeError("conv_bn_folded16: needs the plan of fold_plan16 (None = this conv does not run folded)")
    plain, mask, rect, ho, wo = plan
    x = _contig(_o._chk(x, "conv input", BF))
    n, h, w, cin = x.shape
    cout, _, kh, kw = weight.shape
    wf, shift = _folded_images16(weight, bias, bn)
    res, ldr = (None, 0)
    if residual is not None:
        res, ldr = _o._rows_view(_o._chk(residual, "bn residual", BF))
        if res.numel() // res.shape[-1] != n * ho * wo or res.shape[-1] != cout:
            raise RuntimeError("conv_bn_folded16: residual shape does not match the conv output")
    y, ldy, _ = _o._take_out((n, ho, wo, cout), x.device, BF)
    gemm16("nt", x, wf, y, M=n * ho * wo, N=cout, K=cin, lda=cin, ldb=cin, ldc=ldy, bias=shift, taps=kh * kw, mask=mask,
           tap_stride_b=cout * cin, gather=0 if plain else 1, geo=None if plain else (n, h, w, ho, wo, kh, kw, stride, pad, dil), rect=rect,
           epilogue=(res, ldr, relu))
    return y


# ----------------------------------------------------------------------------------------
# stem
# ----------------------------------------------------------------------------------------
class Stem16Fn(Function):
    @staticmethod
    def forward(ctx, x, weight, bias, pad: int):
        _o._chk(x, "stem input"); _o._chk(weight, "stem weight")
        x = _contig(x)
        n, h, w, _ = x.shape
        cout = weight.shape[0]
        y = torch.empty(n, h + 2 * pad - 6, w + 2 * pad - 6, cout, dtype=BF, device=x.device)
        check(lib.glf_s16_stem7x7_fwd(_p(x), _p(_contig(weight.detach())), _p(bias), _p(y), n, h, w, cout, pad, _stream()), "s16_stem7x7_fwd")
        ctx.save_for_backward(x, weight)
        ctx.cfg = (n, h, w, cout, pad, tuple(weight.shape), bias is not None)
        return y

    @staticmethod
    @once_differentiable
    def backward(ctx, dy):
        x, weight = ctx.saved_tensors
        n, h, w, cout, pad, wshape, has_bias = ctx.cfg
        dy = _contig(dy)
        dx = None
        if ctx.needs_input_grad[0]:                     # the image is itself computed: early_fusion's learned mix of the views
            dx = torch.empty_like(x)
            check(lib.glf_s16_stem7x7_dgrad(_p(dy), _p(_contig(weight.detach())), _p(dx), n, h, w, cout, pad, _stream()), "s16_stem7x7_dgrad")
        dw = torch.empty(wshape, dtype=torch.float32, device=dy.device)
        db = torch.empty(cout, dtype=torch.float32, device=dy.device) if has_bias else None
        part = torch.empty(int(lib.glf_stem7x7_wgrad_workspace(n, h, w, cout, pad)), dtype=torch.float32, device=dy.device)
        check(lib.glf_s16_stem7x7_wgrad(_p(x), _p(dy), _p(dw), _p(db), _p(part), n, h, w, cout, pad, _stream()), "s16_stem7x7_wgrad")
        return dx, dw, db, None


def stem7x7(x, weight, bias, pad: int):
    return Stem16Fn.apply(x, weight, bias, pad)


# ----------------------------------------------------------------------------------------
# BatchNorm (+ residual, + ReLU)
# ----------------------------------------------------------------------------------------
class BatchNormAct16Fn(Function):
    @staticmethod
    def forward(ctx, x, gamma, beta, residual, running_mean, running_var, nbt, training: bool, momentum: float, eps: float, relu: bool, sums=None):
        _o._chk(x, "bn input", BF); _o._chk(gamma, "bn weight"); _o._chk(beta, "bn bias")
        x = _contig(x)
        c = x.shape[-1]
        rows = x.numel() // c
        dev = x.device
        mean = torch.empty(c, dtype=torch.float32, device=dev)
        invstd = torch.empty(c, dtype=torch.float32, device=dev)
        if training:
            if sums is None:                     # no producing contraction left them: one pass over x
                sums = _o.stats_slot(c, dev)
                check(lib.glf_s16_colstats(_p(x), c, rows, c, _p(sums), _stream()), "s16_colstats")
        else:
            if running_mean is None or running_var is None:
                raise RuntimeError("batch_norm in eval mode needs running statistics")
            check(lib.glf_bn_eval_coeffs(_p(running_mean), _p(running_var), eps, _p(mean), _p(invstd), c, _stream()), "bn_eval_coeffs")
            sums = None
        if residual is not None:
            residual = _contig(_o._chk(residual, "bn residual", BF))
        y, ldy, _ = _o._take_out(x.shape, dev, BF)
        # (grad mode is always off inside Function.forward: what says that a backward may follow is needs_input_grad)
        need_mask = relu and residual is not None and any(ctx.needs_input_grad[:4])
        mask = torch.empty(rows * (c // 8), dtype=torch.uint8, device=dev) if need_mask else None
        check(lib.glf_s16_bn_apply(_p(x), c, _p(residual), c, _p(y), ldy, _p(sums), rows, c, eps, momentum, _p(gamma), _p(beta), _p(mean), _p(invstd),
                                   _p(running_mean) if training else None, _p(running_var) if training else None, _p(nbt) if training else None,
                                   int(relu), _p(mask), _stream()), "s16_bn_apply")
        ctx.save_for_backward(x, mask, mean, invstd, gamma, beta if relu else None)
        ctx.cfg = (rows, c, relu, training, residual is not None)
        ctx.param_refs = (gamma, beta)
        _o._last_bn[0] = (mean, invstd, rows)
        return y

    @staticmethod
    @once_differentiable
    def backward(ctx, dy):
        x, mask, mean, invstd, gamma, beta = ctx.saved_tensors
        rows, c, relu, training, has_res = ctx.cfg
        dy2 = getattr(dy, "_glf_addend", None)
        lddy2 = 0
        dy, lddy = _o._rows_view(dy)
        if dy2 is not None:
            if dy2.shape != dy.shape:
                raise RuntimeError("glfusion_amd: the two addends of a lazy fan-in gradient differ in shape")
            dy2, lddy2 = _o._rows_view(dy2)
        dev = dy.device
        dx = torch.empty_like(x)
        dres = torch.empty_like(x) if (has_res and ctx.needs_input_grad[3]) else None
        dgamma = _o.grad_out(ctx.param_refs[0], (c,), dev)
        dbeta = _o.grad_out(ctx.param_refs[1], (c,), dev)
        sums = _o.stats_slot(c, dev)
        check(lib.glf_s16_bn_bwd(_p(dy), lddy, _p(dy2), lddy2, _p(x), c, _p(mean), _p(invstd), _p(gamma), _p(beta), _p(dx), c, _p(dres), c,
                                 _p(dgamma), _p(dbeta), rows, c, int(relu), int(training), _p(sums), _p(mask), _stream()), "s16_bn_bwd")
        return dx, dgamma, dbeta, dres, None, None, None, None, None, None, None, None


def transpose16(x: torch.Tensor, rows: int, cols: int, batch: int = 1) -> torch.Tensor:
    out = torch.empty(batch * rows * cols, dtype=BF, device=x.device)
    check(lib.glf_s16_transpose2d(_p(x), _p(out), rows, cols, batch, _stream()), "s16_transpose2d")
    return out
