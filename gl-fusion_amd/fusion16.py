"""The fusion block (fusion.py) under 16-bit storage, precision "bf16": the same node -- head, core(mode), tail -- on the glf_s16_*
kernels.  x, qkv, y, w, z and every activation gradient are bf16; parameters, statistics, parameter gradients and what a mode keeps
for its backward pass besides (scores statistics, a | b of 'concatenate') are fp32.  The geometry record, the input checks and the
tuple of returned gradients are fusion.py's.  Mode 'dot' has a single-call fast path: the whole pass as one C entry point.
"""
from __future__ import annotations

import ctypes as C

import torch
from torch.autograd import Function
from torch.autograd.function import once_differentiable

from ._lib import TpaviParams, check, lib
from . import fusion, ops as _o, ops16
from .fusion import _attn_params, _block, _grads, _pair_params, _qkv_weights, _slices, _unpack
from .ops16 import BF, _contig, _p, _stream, colsum16, gemm16, tn_split16, transpose16, weight16

PAIR16_MAXCI = 1024        # widths of csrc/attn_pair_s16.hip: Ci % 64 == 0, Ci <= 1024
GAUSS16_BYTES = 12         # per score element of a frame group: S, dP fp32; P, dS bf16 (dS^T takes P's place once dg is out)


def _gauss_frames16(n: int, L: int, lp: int) -> int:
    """Frames per group of 'gaussian': ALL score-shaped buffers alive at once stay within fusion.CHUNK_BYTES."""
    return max(1, min(n, fusion.CHUNK_BYTES // (L * lp * GAUSS16_BYTES)))


def transposed16(src: torch.Tensor, ld: int, rows: int, cols: int, rows_pad: int, batch: int, out: torch.Tensor) -> None:
    """out[b] = the [cols, rows_pad] transposes of the bf16 [rows, cols] matrices src[b] (row stride ld, frame stride rows * ld), zero
    for rows <= r < rows_pad: a reduction extent padded to the NT kernel's K granule."""
    check(lib.glf_s16_transpose2d_strided(_p(src), ld, rows * ld, _p(out), rows_pad, cols * rows_pad, rows, cols, rows_pad, batch, _stream()),
          "s16_transpose2d_strided")


def _gauss_scores16(x2, f0: int, gc: int, L: int, lp: int, c: int, S, P) -> None:
    """S[0:gc] = x_f x_f^T (fp32, rows of stride lp) and P = softmax_rows(S) as bf16 with zero pad columns, frames f0 .. f0 + gc."""
    xf = x2[f0 * L:]
    gemm16("nt", xf, xf, S, M=L, N=L, K=c, lda=c, ldb=c, ldc=lp, batch=gc, bsa=L * c, bsb=L * c, bsc=L * lp)
    check(lib.glf_s16_softmax_rows_fwd(_p(S), _p(P), gc * L, L, lp, lp, _stream()), "s16_softmax_rows_fwd")


# One core per mode: fwd(G, x, qkv, wf) -> (y, attT), attT being what the mode keeps for its backward pass;
# bwd(G, x, qkv, attT, y, dy, dqkv, du, wf) fills dqkv ('gaussian' also adds into du) -> (dW_f, db_f).
# wf = (W_f weight, the forward pass's copies of its row and of its bias) of 'concatenate'.
def _dot_fwd16(G, x, qkv, wf):
    # M_n^T[a][b] = sum_r g[r][a] phi[r][b] / L  (TN with A = g, B = phi): the B operand of y_n = theta_n M_n as it stands
    n, L, ci, c3, bq = G.n, G.L, G.ci, G.c3, G.bq
    th, ph, g = _slices(G, qkv)
    y = torch.empty(G.rows, ci, dtype=BF, device=G.dev)
    attT = torch.empty(n, ci, ci, dtype=BF, device=G.dev)
    gemm16("tn", g, ph, attT, M=ci, N=ci, K=L, lda=c3, ldb=c3, ldc=ci, batch=n, bsa=bq, bsb=bq, bsc=ci * ci, alpha=1.0 / L)
    gemm16("nt", th, attT, y, M=L, N=ci, K=ci, lda=c3, ldb=ci, ldc=ci, batch=n, bsa=bq, bsb=ci * ci, bsc=L * ci)
    return y, attT


def _dot_bwd16(G, x, qkv, attT, y, dy, dqkv, du, wf):
    n, L, ci, c3, bq, bs = G.n, G.L, G.ci, G.c3, G.bq, G.bs
    th, ph, g = _slices(G, qkv)
    dth, dph, dg = _slices(G, dqkv)
    att = transpose16(attT, ci, ci, n)                     # M_n
    gemm16("nt", dy, att, dth, M=L, N=ci, K=ci, lda=ci, ldb=ci, ldc=c3, batch=n, bsa=bs, bsb=ci * ci, bsc=bq)
    dM = torch.empty(n, ci, ci, dtype=BF, device=G.dev)    # dM_n = theta_n^T dy_n
    gemm16("tn", th, dy, dM, M=ci, N=ci, K=L, lda=c3, ldb=ci, ldc=ci, batch=n, bsa=bq, bsb=bs, bsc=ci * ci)
    gemm16("nt", g, dM, dph, M=L, N=ci, K=ci, lda=c3, ldb=ci, ldc=c3, batch=n, bsa=bq, bsb=ci * ci, bsc=bq, alpha=1.0 / L)
    dMT = transpose16(dM, ci, ci, n)
    gemm16("nt", ph, dMT, dg, M=L, N=ci, K=ci, lda=c3, ldb=ci, ldc=c3, batch=n, bsa=bq, bsb=ci * ci, bsc=bq, alpha=1.0 / L)
    return None, None


def _embedded_fwd16(G, x, qkv, wf):
    # y_n = softmax(theta_n phi_n^T, dim=-1) g_n, fused (csrc/attn_s16.hip); attT holds the row log-sum-exp that backward
    # recomputes the scores against
    th, ph, g = _slices(G, qkv)
    y = torch.empty(G.rows, G.ci, dtype=BF, device=G.dev)
    attT = torch.empty(G.rows, **G.f32)
    check(lib.glf_s16_attn_softmax_fwd(_p(th), _p(ph), _p(g), _p(y), _p(attT), C.byref(_attn_params(G.n, G.L, G.ci, G.c3, G.ci)), _stream()),
          "s16_attn_softmax_fwd")
    return y, attT


def _embedded_bwd16(G, x, qkv, attT, y, dy, dqkv, du, wf):
    # attT is the row log-sum-exp here; one call writes all three column slices of dqkv
    th, ph, g = _slices(G, qkv)
    dth, dph, dg = _slices(G, dqkv)
    dsum = torch.empty(G.rows, **G.f32)
    check(lib.glf_s16_attn_softmax_bwd(_p(th), _p(ph), _p(g), _p(y), _p(dy), _p(attT), _p(dth), _p(dph), _p(dg), _p(dsum),
                                       C.byref(_attn_params(G.n, G.L, G.ci, G.c3, G.ci)), _stream()), "s16_attn_softmax_bwd")
    return None, None


def _gaussian_fwd16(G, x, qkv, wf):
    # per group of frames (fusion.py's route on the 16-bit contractions): S = x x^T over C into fp32, P = softmax(S) as bf16 with
    # the reduction extent padded to the NT kernel's K granule, y = P g against g^T; backward recomputes S and P
    n, L, c, ci, dev = G.n, G.L, G.c, G.ci, G.dev
    g = _slices(G, qkv)[2]
    y = torch.empty(G.rows, ci, dtype=BF, device=dev)
    attT = torch.empty(1, **G.f32)
    x2 = x.view(G.rows, c)
    lp = (L + 63) // 64 * 64
    gpc = _gauss_frames16(n, L, lp)
    S = torch.empty(gpc, L, lp, **G.f32)
    P = torch.empty(gpc, L, lp, dtype=BF, device=dev)
    gT = torch.empty(gpc, ci, lp, dtype=BF, device=dev)
    for f0 in range(0, n, gpc):
        gc = min(gpc, n - f0)
        _gauss_scores16(x2, f0, gc, L, lp, c, S, P)
        transposed16(g[f0 * L:], G.c3, L, ci, lp, gc, gT)
        gemm16("nt", P, gT, y[f0 * L:], M=L, N=ci, K=lp, lda=lp, ldb=lp, ldc=ci, batch=gc, bsa=L * lp, bsb=ci * lp, bsc=L * ci)
    return y, attT


def _gaussian_bwd16(G, x, qkv, attT, y, dy, dqkv, du, wf):
    # per group of frames: S, P recomputed from x; dP = dY g^T (fp32); dg = P^T dY; dS = P (dP - rowsum(P dP)) as bf16; x is
    # BOTH operands of the scores, so dx (= du, which already holds the residual's gradient) += dS x, then += dS^T x: two NT
    # launches that accumulate in this order against x^T (the TN kernel does not accumulate)
    n, L, c, ci, c3, bq, bs, dev = G.n, G.L, G.c, G.ci, G.c3, G.bq, G.bs, G.dev
    g, dg = _slices(G, qkv)[2], _slices(G, dqkv)[2]
    x2 = x.view(G.rows, c)
    lp = (L + 63) // 64 * 64
    gpc = _gauss_frames16(n, L, lp)
    S = torch.empty(gpc, L, lp, **G.f32)
    dP = torch.empty(gpc, L, lp, **G.f32)
    P = torch.empty(gpc, L, lp, dtype=BF, device=dev)
    dS = torch.empty(gpc, L, lp, dtype=BF, device=dev)
    xT = torch.empty(gpc, c, lp, dtype=BF, device=dev)
    for f0 in range(0, n, gpc):
        gc = min(gpc, n - f0)
        _gauss_scores16(x2, f0, gc, L, lp, c, S, P)
        gemm16("nt", dy[f0 * L:], g[f0 * L:], dP, M=L, N=L, K=ci, lda=ci, ldb=c3, ldc=lp, batch=gc, bsa=bs, bsb=bq, bsc=L * lp)
        gemm16("tn", P, dy[f0 * L:], dg[f0 * L:], M=L, N=ci, K=L, lda=lp, ldb=ci, ldc=c3, batch=gc, bsa=L * lp, bsb=bs, bsc=bq)
        check(lib.glf_s16_softmax_rows_bwd(_p(S), _p(dP), _p(dS), gc * L, L, lp, lp, lp, _stream()), "s16_softmax_rows_bwd")
        transposed16(x2[f0 * L:], c, L, c, lp, gc, xT)
        gemm16("nt", dS, xT, du[f0 * L:], M=L, N=c, K=lp, lda=lp, ldb=lp, ldc=c, batch=gc, bsa=L * lp, bsb=c * lp, bsc=L * c,
               accumulate=True)
        dST = P                                            # dg is out: P's buffer takes dS^T
        transposed16(dS, lp, L, L, lp, gc, dST)
        gemm16("nt", dST, xT, du[f0 * L:], M=L, N=c, K=lp, lda=lp, ldb=lp, ldc=c, batch=gc, bsa=L * lp, bsb=c * lp, bsc=L * c,
               accumulate=True)
    return None, None


def _concatenate_fwd16(G, x, qkv, wf):
    # a = theta w_theta, b = phi w_phi (one fp32 scalar per position), then ONE kernel forms the relu(a_i + b_j + c) tiles and
    # contracts them with g on the bf16 MFMA (csrc/attn_pair_s16.hip); attT keeps a | b for the backward pass
    n, L, ci, c3, rows = G.n, G.L, G.ci, G.c3, G.rows
    th, ph, g = _slices(G, qkv)
    _, wrow, wf_c = wf
    y = torch.empty(rows, ci, dtype=BF, device=G.dev)
    attT = torch.empty(2, rows, **G.f32)
    check(lib.glf_s16_attn_pair_proj_fwd(_p(th), _p(ph), c3, _p(wrow), _p(attT[0]), _p(attT[1]), rows, ci, _stream()), "s16_attn_pair_proj_fwd")
    check(lib.glf_s16_attn_pair_relu_fwd(_p(attT[0]), _p(attT[1]), _p(wf_c), _p(g), _p(y), C.byref(_pair_params(n, L, ci, c3, ci, ci, c3)), _stream()),
          "s16_attn_pair_relu_fwd")
    return y, attT


def _concatenate_bwd16(G, x, qkv, attT, y, dy, dqkv, du, wf):
    # dg, da, db, dc from the fused kernels (every element written once, fixed summation order), then the skinny ends:
    # dtheta = da w_theta^T, dphi = db w_phi^T as bf16 into dqkv, and W_f's gradient [theta^T da | phi^T db] in fp32
    n, L, ci, c3, rows = G.n, G.L, G.ci, G.c3, G.rows
    th, ph, g = _slices(G, qkv)
    dth, dph, dg = _slices(G, dqkv)
    wf_w, wrow, wf_c = wf
    dab = torch.empty(2, rows, **G.f32)
    dwf_w = torch.empty(2 * ci, **G.f32)
    dwf_b = torch.empty(1, **G.f32)
    pp = _pair_params(n, L, ci, c3, ci, ci, c3)
    nb = int(lib.glf_s16_attn_pair_relu_workspace_bytes(C.byref(pp)))
    pws = torch.empty(nb // 4, **G.f32)
    check(lib.glf_s16_attn_pair_relu_bwd(_p(attT[0]), _p(attT[1]), _p(wf_c), _p(g), _p(dy), _p(dg), _p(dab[0]), _p(dab[1]), _p(dwf_b),
                                         _p(pws), nb, C.byref(pp), _stream()), "s16_attn_pair_relu_bwd")
    nb = int(lib.glf_s16_attn_pair_proj_workspace_bytes(rows, ci))
    pws = torch.empty(nb // 4, **G.f32)
    check(lib.glf_s16_attn_pair_proj_bwd(_p(th), _p(ph), c3, _p(wrow), _p(dab[0]), _p(dab[1]), _p(dth), _p(dph), c3, _p(dwf_w), _p(pws), nb,
                                         rows, ci, _stream()), "s16_attn_pair_proj_bwd")
    return dwf_w.view(wf_w.shape), dwf_b


_CORES16 = {"dot": (_dot_fwd16, _dot_bwd16), "embedded": (_embedded_fwd16, _embedded_bwd16), "gaussian": (_gaussian_fwd16, _gaussian_bwd16),
            "concatenate": (_concatenate_fwd16, _concatenate_bwd16)}


def _check16(G, mode: str) -> None:
    c, ci, L = G.c, G.ci, G.L
    if c % 64 != 0 or ci % 64 != 0:
        raise RuntimeError(f"glfusion_amd: TPAVI mode {mode!r} under 16-bit storage needs channel counts that are multiples of 64 "
                           f"(got C = {c}, Ci = {ci})")
    if mode == "concatenate" and ci > PAIR16_MAXCI:
        raise RuntimeError(f"glfusion_amd: TPAVI mode 'concatenate' under 16-bit storage is built for Ci % 64 == 0, Ci <= {PAIR16_MAXCI} "
                           f"(got {ci})")
    if mode == "gaussian" and L % 8 != 0:
        raise RuntimeError(f"glfusion_amd: TPAVI mode 'gaussian' under 16-bit storage needs L = V h w to be a multiple of 8 (got {L}): "
                           "dg = P^T dY runs on the TN kernel, whose M is L")


def _single_call(mode: str) -> bool:
    """The whole pass as ONE C call (include/glfusion.h: glf_s16_tpavi_fwd / _bwd); the composed sequence is the same launches, kept
    for the per-contraction profiler hooks and the other modes (tests/test_gpu_s16.py checks the two bit for bit)."""
    return ops16.BLOCK_CALLS and _o.PROFILER is None and mode == "dot"


class Tpavi16Fn(Function):
    @staticmethod
    def forward(ctx, x, th_w, th_b, ph_w, ph_b, g_w, g_b, wz_w, wz_b, bn_g, bn_b, ln_g, ln_b, rmean, rvar, nbt, training: bool,
                momentum: float, bn_eps: float, ln_eps: float, mode: str, wf_w=None, wf_b=None):
        """th_* / ph_*: None for 'gaussian' (the mode owns no theta / phi); wf_w [1, 2 Ci, 1, 1], wf_b [1]: W_f of 'concatenate'."""
        x, G = _unpack(x, g_w, mode, BF)
        _check16(G, mode)
        n, L, c, ci, c3, rows, dev = G.n, G.L, G.c, G.ci, G.c3, G.rows, G.dev
        zW = _contig(wz_w.detach()).view(wz_w.shape[0], wz_w.shape[1])
        Wcat, bcat = _qkv_weights((g_w, g_b) if G.npj == 1 else (th_w, ph_w, g_w, th_b, ph_b, g_b))
        qkv = torch.empty(rows, c3, dtype=BF, device=dev)
        single = _single_call(mode)
        ctx.wf = (None, None, None)
        if single:
            attT = torch.empty(n, ci, ci, dtype=BF, device=dev)
            y = torch.empty(rows, ci, dtype=BF, device=dev)
        else:
            gemm16("nt", x, weight16(Wcat, Wcat, "w"), qkv, M=rows, N=c3, K=c, lda=c, ldb=c, ldc=c3, bias=bcat)
            if mode == "concatenate":
                # copies of the W_f row and bias: backward masks with the c the forward used, whatever happens to the parameters in between
                ctx.wf = (wf_w, wf_w.detach().reshape(2 * ci).clone(), wf_b.detach().clone())
            y, attT = _CORES16[mode][0](G, x, qkv, ctx.wf)
        wz = torch.empty(rows, c, dtype=BF, device=dev)
        mean, invstd = torch.empty(c, **G.f32), torch.empty(c, **G.f32)
        z = torch.empty_like(x)
        rmu, rrs = torch.empty(rows, **G.f32), torch.empty(rows, **G.f32)
        if single:
            tp = TpaviParams(n, L, c, ci, int(training), bn_eps, momentum, ln_eps)
            nws = int(lib.glf_s16_tpavi_workspace_bytes(C.byref(tp), 0))
            ws = torch.empty(nws, dtype=torch.uint8, device=dev)
            check(lib.glf_s16_tpavi_fwd(_p(x), _p(weight16(Wcat, Wcat, "w")), _p(bcat), _p(weight16(zW, wz_w, "w")), _p(wz_b), _p(bn_g), _p(bn_b),
                                        _p(rmean), _p(rvar), _p(nbt), _p(ln_g), _p(ln_b), _p(z), _p(qkv), _p(attT), _p(y), _p(wz), _p(mean), _p(invstd),
                                        _p(rmu), _p(rrs), C.byref(tp), _p(ws), nws, _stream()), "s16_tpavi_fwd")
        else:
            sums = _o.stats_slot(c, dev) if training else None
            gemm16("nt", y, weight16(zW, wz_w, "w"), wz, M=rows, N=c, K=ci, lda=ci, ldb=ci, ldc=c, bias=wz_b, colstats=sums)
            if training:
                check(lib.glf_bn_stats_from_sums(_p(sums), rows, c, bn_eps, momentum, _p(mean), _p(invstd), _p(rmean), _p(rvar), _p(nbt), _stream()),
                      "bn_stats_from_sums")
            else:
                check(lib.glf_bn_eval_coeffs(_p(rmean), _p(rvar), bn_eps, _p(mean), _p(invstd), c, _stream()), "bn_eval_coeffs")
            check(lib.glf_s16_bn_res_ln_fwd(_p(wz), _p(x), _p(mean), _p(invstd), _p(bn_g), _p(bn_b), _p(ln_g), _p(ln_b), ln_eps, _p(z), _p(rmu), _p(rrs),
                                            rows, c, _stream()), "s16_bn_res_ln_fwd")
        ctx.save_for_backward(x, qkv, attT, y, wz, mean, invstd, rmu, rrs, Wcat, zW, bn_g, bn_b, ln_g)
        ctx.cfg = (n, L, c, ci, training, tuple(g_w.shape), tuple(wz_w.shape), mode)
        ctx.owners = (wz_w,)
        return z

    @staticmethod
    @once_differentiable
    def backward(ctx, dz):
        (x, qkv, attT, y, wz, mean, invstd, rmu, rrs, Wcat, zW, bn_g, bn_b, ln_g) = ctx.saved_tensors
        n, L, c, ci, training, pshape, zshape, mode = ctx.cfg
        (wz_o,) = ctx.owners
        G = _block(n, L, c, ci, mode, dz.device)
        c3, rows, dev = G.c3, G.rows, G.dev
        dz = _contig(dz)
        du = torch.empty(rows, c, dtype=BF, device=dev)        # the residual's gradient; the projections' dgrad adds onto it: dx
        dzW = torch.empty(c, ci, **G.f32)
        dbn_g, dbn_b, dln_g, dln_b = (torch.empty(c, **G.f32) for _ in range(4))
        if _single_call(mode):
            tp = TpaviParams(n, L, c, ci, int(training), 0.0, 0.0, 0.0)
            dWcat, dbcat, dzb = torch.empty(c3, c, **G.f32), torch.empty(c3, **G.f32), torch.empty(c, **G.f32)
            nws = int(lib.glf_s16_tpavi_workspace_bytes(C.byref(tp), 1))
            ws = torch.empty(nws, dtype=torch.uint8, device=dev)
            check(lib.glf_s16_tpavi_bwd(_p(dz), _p(x), _p(qkv), _p(attT), _p(y), _p(wz), _p(mean), _p(invstd), _p(rmu), _p(rrs),
                                        _p(weight16(_o.weight_T(Wcat, Wcat), Wcat, "T2")), _p(weight16(_o.weight_T(zW, wz_o), wz_o, "T2")),
                                        _p(bn_g), _p(bn_b), _p(ln_g), _p(du), _p(dWcat), _p(dbcat), _p(dzW), _p(dzb), _p(dbn_g), _p(dbn_b),
                                        _p(dln_g), _p(dln_b), C.byref(tp), _p(ws), nws, _stream()), "s16_tpavi_bwd")
            return _grads(G, x, du, dWcat, dbcat, pshape, dzW.view(zshape), dzb, dbn_g, dbn_b, dln_g, dln_b)
        ws = torch.empty(int(lib.glf_s16_bn_res_ln_workspace(rows, c)) // 4, **G.f32)
        check(lib.glf_s16_bn_res_ln_bwd(_p(dz), _p(wz), _p(x), _p(mean), _p(invstd), _p(bn_g), _p(bn_b), _p(ln_g), _p(rmu), _p(rrs), _p(du), _p(dln_g),
                                        _p(dln_b), rows, c, _p(ws), _stream()), "s16_bn_res_ln_bwd")
        dwz = torch.empty(rows, c, dtype=BF, device=dev)
        check(lib.glf_s16_bn_bwd(_p(du), c, None, 0, _p(wz), c, _p(mean), _p(invstd), _p(bn_g), None, _p(dwz), c, None, 0, _p(dbn_g), _p(dbn_b),
                                 rows, c, 0, int(training), _p(_o.stats_slot(c, dev)), None, _stream()), "s16_bn_bwd")
        gemm16("tn", dwz, y, dzW, M=c, N=ci, K=rows, lda=c, ldb=ci, ldc=ci, split=tn_split16(rows, c, ci, 1))
        # train mode: the bias feeds a BatchNorm, its gradient is zero in exact arithmetic (fusion._tail_bwd)
        dzb = _o.zeros(c, device=dev) if training else colsum16(dwz, rows, c)
        dy = torch.empty(rows, ci, dtype=BF, device=dev)
        gemm16("nt", dwz, weight16(_o.weight_T(zW, wz_o), wz_o, "T2"), dy, M=rows, N=ci, K=c, lda=c, ldb=c, ldc=ci)
        del dwz
        dqkv = torch.empty(rows, c3, dtype=BF, device=dev)
        dwf_w, dwf_b = _CORES16[mode][1](G, x, qkv, attT, y, dy, dqkv, du, ctx.wf)
        del dy
        dWcat = torch.empty(c3, c, **G.f32)
        gemm16("tn", dqkv, x, dWcat, M=c3, N=c, K=rows, lda=c3, ldb=c, ldc=c, split=tn_split16(rows, c3, c, 1))
        dbcat = colsum16(dqkv, rows, c3)
        gemm16("nt", dqkv, weight16(_o.weight_T(Wcat, Wcat), Wcat, "T2"), du, M=rows, N=c, K=c3, lda=c3, ldb=c3, ldc=c, accumulate=True)
        return _grads(G, x, du, dWcat, dbcat, pshape, dzW.view(zshape), dzb, dbn_g, dbn_b, dln_g, dln_b, dwf_w, dwf_b)
