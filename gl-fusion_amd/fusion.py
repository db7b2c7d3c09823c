"""The Global-Local cross-view attention block (TPAVIModule.forward, reference
models/ours.py:845-917) as ONE autograd node over the HIP contraction engine.

x is [N, V, h, w, C] channels-last, i.e. the matrix [N*L, C] with L = V*h*w positions per
frame (what the reference builds with unsqueeze(2)+cat(dim=2), ours.py:1819-1820).

mode 'dot' (the shipped model, ours.py:1746-1747):  f = theta^T phi, y = (f / L) g.  It is linear,
so we re-associate exactly:  M_n = phi_n^T g_n / L  ([Ci,Ci] per frame), y_n = theta_n M_n.  The
[N,L,L] score matrix (1.4 GB at config 2, 983 MB *per frame* at the 5-view 224^2 config) is never
formed and the matmul work drops from 2*L*L*Ci to 2*L*Ci*Ci MACs per frame.
mode 'embedded' (softmax, ours.py:896-897): scores are materialised per frame, normalised by a
row-softmax kernel, then contracted with g.
mode 'gaussian' (ours.py:871-875): the softmax of x x^T -- no theta / phi, the scores contract over C.  Scores per group of
frames (at most CHUNK_BYTES alive), row softmax, P g; backward recomputes them and adds dS x and dS^T x into dx.
mode 'concatenate' (ours.py:883-894): f_ij = relu(w_theta . theta_i + w_phi . phi_j + c), y = (f / L) g.  The score is the
sum of two scalars per position, a = theta w_theta and b = phi w_phi: one fused kernel (csrc/attn_pair.hip) forms the
relu(a_i + b_j + c) tiles on the fly; the reference's [N, 2 Ci, L, L] tensor and the [N, L, L] scores never exist.

Tail (ours.py:908-915): w = W_z y + b;  z = LayerNorm_C( BatchNorm3d(w) + x ) in one fused pass.

The node reads head -> core(mode) -> tail: _project (the stacked theta | phi | g projection), one forward / backward pair per mode
(_CORES), _tail; backward runs _tail_bwd, the core, _project_bwd.  fusion16.py is the same node under 16-bit storage.
"""
from __future__ import annotations

import ctypes as C
import os
import weakref
from types import SimpleNamespace

import torch
from torch.autograd import Function
from torch.autograd.function import once_differentiable

from ._lib import AttnPairParams, AttnParams, check, lib
from .ops import (_chk, _contig, _p, _stream, _tn_split, _ws, _wimage, _registry, WJ_COPY, stats_slot, bnbwd_slot, amax_of, amax_slot, colsum, gemm, set_amax, split_mode,
                  transpose2d, weight_T, weight_packed, nt_presplit_ok, tn_presplit_ok, act_packed, act_packed_colsum, packed_hit, pick, zeros,
                  _ones4)


FUSED_SOFTMAX = os.environ.get("GLF_FUSED_SOFTMAX", "1") != "0"
# Exact-fp32 precision only: the block's NT / NN contractions run as K / EXACT_KCHUNK launches that accumulate into C.  The fp32 MFMA
# adds its K products ONE AFTER THE OTHER into the accumulator -- up to a 3 072-long fp32 chain (dx = du + dqkv Wcat) -- and this
# block's gradients cancel to ~1e-3 of their terms: unchunked, theta.weight sat at 4.5e-3 of its norm and the encoder gradients
# behind the block at 2e-3 (the split-fp16 kernels add 16 products per instruction: 5e-4).  Which roundings such a tensor collects is
# a matter of luck at any single chain length (1 024: 1.0e-3 with a dense ASPP forward, 3.6e-3 with per-tap launches; 512: 2.2e-3);
# 256-deep chains were within 1e-3 in every regime measured (5.6e-4 / 9.5e-4), for +14 % on the strict-precision leg
# (profiles/r04_exact_leg_spread.txt -- measurable since the leg is reproducible, see ops.Conv2dFn.forward).
EXACT_KCHUNK = int(os.environ.get("GLF_EXACT_KCHUNK", "256"))
# The tail's backward in one walk: du, the LayerNorm parameter gradients and the BatchNorm-backward sums of w from ONE pass over
# dz / w / x (glf_bn_res_ln_bwd_sums) instead of three, and the stacked projection's bias gradient from the pass that packs dqkv
# (glf_split_f16_packed_colsum) instead of a second one.  0 = the separate passes (A/B, profiles/tail_bwd_fused.txt).
TAIL_BWD_FUSED = os.environ.get("GLF_TAIL_BWD_FUSED", "1") != "0"
_gemm = gemm


def gemm(mode, A, B, Cm, **kw):          # noqa: F811  (every contraction of this module goes through here)
    K = kw["K"]
    if split_mode() or mode == "tn" or EXACT_KCHUNK <= 0 or K <= EXACT_KCHUNK or kw.get("taps", 1) != 1:
        return _gemm(mode, A, B, Cm, **kw)
    first = True
    for k0 in range(0, K, EXACT_KCHUNK):
        kk = dict(kw)
        kk["K"] = min(EXACT_KCHUNK, K - k0)
        if not first:
            kk["bias"] = None
            kk["accumulate"] = True
        _gemm(mode, A[..., k0:], B[..., k0:] if mode == "nt" else B[..., k0:, :], Cm, **kk)
        first = False
# 'embedded' under the split 16-bit contraction precisions: scores per group of frames through the split-fp16 MFMA kernels (QK^T, PV,
# dP, dS^T theta, dS phi, P^T dY as plain contractions, softmax statistics in fp32, at most CHUNK_BYTES of scores alive) instead of
# the fused exact-fp32 kernel -- 3-4x its rate at the model's shapes; 0 = the fused kernel under every precision
CHUNKED_SOFTMAX = os.environ.get("GLF_CHUNKED_SOFTMAX", "1") != "0"
CHUNK_BYTES = int(os.environ.get("GLF_SOFTMAX_CHUNK_BYTES", str(2 << 30)))


def chunked_softmax_ok(ci: int, L: int) -> bool:
    return CHUNKED_SOFTMAX and split_mode() and ci % 32 == 0 and L % 4 == 0


def gaussian_chunked_ok(ci: int) -> bool:
    """'gaussian' runs the frame-group route under EVERY precision (exact fp32 included: the same bounded buffers on the exact
    contractions); only widths the split kernels' K = 32 granularity excludes (toy modules) materialise the scores."""
    return ci % 32 == 0


def pair_relu_ok(ci: int) -> bool:
    """Widths of the fused pairwise-ReLU kernel (glf_attn_pair_relu_*): the fused softmax kernel's."""
    return ci % 32 == 0 and ci <= 1024


def _frames_per_chunk(n: int, L: int) -> int:
    lp = (L + 31) // 32 * 32
    return max(1, min(n, CHUNK_BYTES // (L * lp * 4)))


def _scores(th, ph, f0, g, L, lp, ci, c3, am_q, S):
    """S[0:g] = softmax_rows(theta_f phi_f^T) for frames f0 .. f0 + g: rows of stride lp (a multiple of 32: the matrices are K
    operands of the next contractions), padding columns zero."""
    bq = L * c3
    gemm("nt", th[f0 * L:], ph[f0 * L:], S, M=L, N=L, K=ci, lda=c3, ldb=c3, ldc=lp, batch=g, bsa=bq, bsb=bq, bsc=L * lp,
         amax_a=am_q, amax_b=am_q)
    check(lib.glf_softmax_rows_ld(_p(S), g * L, L, lp, _stream()), "softmax_rows_ld")


def _transposed(src, f0, g, L, lp, ci, c3, out):
    """out[0:g] = the [ci, lp] transposes of the [L, ci] column slices src (row stride c3) of frames f0 .. f0 + g, zero beyond L."""
    check(lib.glf_transpose2d_strided(_p(src[f0 * L:]), c3, L * c3, _p(out), lp, ci * lp, L, ci, lp, g, _stream()), "transpose2d_strided")


def fused_softmax_ok(ci: int) -> bool:
    """The fused QK^T / softmax / PV kernel covers Ci % 32 == 0, Ci <= 1024 (the model: Ci = 1024); other widths (toy
    modules) materialise the scores per frame."""
    return FUSED_SOFTMAX and ci % 32 == 0 and ci <= 1024


def _pair_params(n: int, L: int, ci: int, ldg: int, ldy: int, lddy: int, lddg: int) -> AttnPairParams:
    """glf_attn_pair_params of 'concatenate': g / dg column slices of the qkv / dqkv buffers (row strides ldg / lddg), y and dy dense."""
    pp = AttnPairParams()
    pp.frames, pp.L, pp.ci = n, L, ci
    pp.ldg, pp.ldy, pp.lddy, pp.lddg = ldg, ldy, lddy, lddg
    return pp


def _attn_params(n: int, L: int, ci: int, ldqkv: int, ldy: int) -> AttnParams:
    """glf_attn_params of the fused softmax attention (fp32 and 16-bit): theta / phi / g / dtheta / dphi / dg are column slices of the
    qkv / dqkv buffers (row stride ldqkv), y and dy dense (row stride ldy)."""
    ap = AttnParams()
    ap.frames, ap.L, ap.ci = n, L, ci
    ap.ldq = ap.ldk = ap.ldv = ldqkv
    ap.ldy, ap.lddy, ap.ldd = ldy, ldy, ldqkv
    return ap


_qkv_cache = {}


def _qkv_weights(params):
    """theta | phi | g weights (params = the k weights, then their k biases; k = 1 for 'gaussian', which projects g alone)
    stacked as ONE [k*ci, c] operand (+ the stacked bias), so the projections run as a single contraction over the shared input.  The stacked buffers live as long as theta's weight; each of the six slices is
    a registered weight image (ops._wimage: re-copied when its source parameter changed, or by ops.refresh_weights), and the
    stacked operand carries the combined version stamp of its sources for the images derived from IT (maximum, transpose,
    packed forms)."""
    k = len(params) // 2
    ws_, bs_ = params[:k], params[k:]
    th_w = ws_[0]
    ci, c = th_w.shape[0], th_w.shape[1]
    if ci % 4 != 0:                                    # odd toy widths only (the 16-byte copy kernel does not apply)
        Wcat = torch.cat([_contig(t.detach()).view(ci, c) for t in ws_], dim=0)
        bcat = torch.cat([t.detach() for t in bs_], dim=0)
        return Wcat, bcat
    key = id(th_w)
    hit = _qkv_cache.get(key)
    if hit is None or hit[0]() is not th_w or hit[1].device != th_w.device or hit[1].shape != (k * ci, c):
        Wcat = torch.empty(k * ci, c, dtype=torch.float32, device=th_w.device)
        bcat = torch.empty(k * ci, dtype=torch.float32, device=th_w.device)
        refs = [weakref.ref(t) for t in params]
        Wcat._glf_version_fn = lambda refs=refs: tuple((r()._version, r().data_ptr()) if r() is not None else None for r in refs)
        Wcat._glf_sources = refs
        hit = _qkv_cache[key] = (weakref.ref(th_w, lambda _r, k=key: _qkv_cache.pop(k, None)), Wcat, bcat)
    _, Wcat, bcat = hit
    for i, (w, b) in enumerate(zip(ws_, bs_)):
        for t, dst, n in ((w, Wcat[i * ci:(i + 1) * ci], ci * c), (b, bcat[i * ci:(i + 1) * ci], ci)):
            src = _contig(t.detach())
            im, fresh = _wimage(t, "qkvcat", WJ_COPY, src, (n, 0, 0), lambda dst=dst: dst)
            if im.dst.data_ptr() != dst.data_ptr():   # the stacked buffers were re-created: re-register
                _registry(t.device).drop(im.key)
                im, fresh = _wimage(t, "qkvcat", WJ_COPY, src, (n, 0, 0), lambda dst=dst: dst)
            if fresh:
                check(lib.glf_copy_frames(_p(src), n, _p(im.dst), n, 1, n, _stream()), "qkv_weights")
    return Wcat, bcat


def _block(n: int, L: int, c: int, ci: int, mode: str, dev) -> SimpleNamespace:
    """Geometry of one block call, built here for both passes of both autograd nodes (fusion16.Tpavi16Fn is the other): n frames of
    L = V h w positions, rows = n L.  qkv / dqkv are [rows, c3], the npj projections side by side (3: theta | phi | g; 1: 'gaussian'
    projects g alone, its scores are x x^T); bq / bs: the frame strides inside qkv / dqkv and inside the dense [rows, ci] y / dy."""
    npj = 1 if mode == "gaussian" else 3
    return SimpleNamespace(n=n, L=L, c=c, ci=ci, npj=npj, c3=npj * ci, rows=n * L, bq=L * npj * ci, bs=L * ci, dev=dev,
                           f32=dict(dtype=torch.float32, device=dev))


def _slices(G, qkv):
    """theta | phi | g column slices of qkv (d theta | d phi | d g of dqkv); 'gaussian': g is the whole matrix, the others unused"""
    return qkv[:, 0:G.ci], qkv[:, G.ci:2 * G.ci], qkv[:, (G.npj - 1) * G.ci:]


def _unpack(x, g_w, mode: str, dtype=torch.float32):
    """The node's input, checked and contiguous, and the geometry of the call."""
    x = _contig(_chk(x, "TPAVI input", dtype))
    if x.dim() != 5:
        raise RuntimeError("TPAVI input must be [N, V, h, w, C]")
    if mode not in _CORES:
        raise RuntimeError(f"TPAVI mode {mode!r} is not on the path (built: 'dot', 'embedded', 'gaussian', 'concatenate')")
    n, v, h, w_, c = x.shape
    return x, _block(n, v * h * w_, c, g_w.shape[0], mode, x.device)


def _grads(G, x, dx, dWcat, dbcat, pshape, dzW, dzb, dbn_g, dbn_b, dln_g, dln_b, dwf_w=None, dwf_b=None):
    """The gradients of a node's 23 forward arguments: dWcat / dbcat sliced per projection (None for the theta / phi 'gaussian' does
    not own), None for the statistics buffers and the settings."""
    ci = G.ci
    gw = [None] * (3 - G.npj) + [dWcat[i * ci:(i + 1) * ci].reshape(pshape) for i in range(G.npj)]
    gb = [None] * (3 - G.npj) + [dbcat[i * ci:(i + 1) * ci] for i in range(G.npj)]
    return (dx.view_as(x), gw[0], gb[0], gw[1], gb[1], gw[2], gb[2], dzW, dzb, dbn_g, dbn_b, dln_g, dln_b,
            None, None, None, None, None, None, None, None, dwf_w, dwf_b)


# The two softmax routes that 'embedded' and 'gaussian' share.  scores = (Q, K, row stride, contraction width, amax): the theta /
# phi slices of qkv, or x twice.  sink = (dst of dS K, dst of dS^T Q, row stride, accumulate, amax_c slot): the d theta / d phi
# slices of dqkv, or du twice, added onto the residual's gradient.
def _group_softmax_fwd(G, scores, g, am_q, y) -> None:
    """Per group of frames: S = Q K^T, P = softmax(S) in place, y = P g -- three launches + one transpose of g; nothing of size
    L x L is kept (the backward pass recomputes P group by group), at most CHUNK_BYTES of scores are alive."""
    Q, K, ld, k, am = scores
    n, L, ci, dev = G.n, G.L, G.ci, G.dev
    lp = (L + 31) // 32 * 32
    gpc = _frames_per_chunk(n, L)
    S = torch.empty(gpc, L, lp, **G.f32)
    gT = torch.empty(gpc, ci, lp, **G.f32)
    one = _ones4(dev)[:1]                                            # max P <= 1
    am_y = amax_slot(dev)
    for f0 in range(0, n, gpc):
        gc = min(gpc, n - f0)
        _scores(Q, K, f0, gc, L, lp, k, ld, am, S)
        _transposed(g, f0, gc, L, lp, ci, G.c3, gT)
        gemm("nt", S, gT, y[f0 * L:], M=L, N=ci, K=lp, lda=lp, ldb=lp, ldc=ci, batch=gc, bsa=L * lp, bsb=ci * lp, bsc=L * ci,
             amax_a=one, amax_b=am_q, amax_c=am_y)
    set_amax(y, am_y)


def _group_softmax_bwd(G, scores, g, am_q, dy, am_dy, dqkv, am_dq_slot, sink) -> None:
    """Per group of frames: P recomputed; dP = dY g^T; dg = P^T dY; dS = P (dP - rowsum(dP P)); then dS K and dS^T Q into the sink."""
    Q, K, ld, k, am = scores
    dQ, dK, ldd, acc, am_d = sink
    n, L, ci, c3, bq, bs, dev = G.n, G.L, G.ci, G.c3, G.bq, G.bs, G.dev
    dg = _slices(G, dqkv)[2]
    lp = (L + 31) // 32 * 32
    gpc = _frames_per_chunk(n, L)
    S = torch.empty(gpc, L, lp, **G.f32)
    dP = torch.empty(gpc, L, lp, **G.f32)
    KT = torch.empty(gpc, k, lp, **G.f32)
    one = _ones4(dev)[:1]
    for f0 in range(0, n, gpc):
        gc = min(gpc, n - f0)
        _scores(Q, K, f0, gc, L, lp, k, ld, am, S)
        am_dP = amax_slot(dev)
        gemm("nt", dy[f0 * L:], g[f0 * L:], dP, M=L, N=L, K=ci, lda=ci, ldb=c3, ldc=lp, batch=gc, bsa=bs, bsb=bq, bsc=L * lp,
             amax_a=am_dy, amax_b=am_q, amax_c=am_dP)
        gemm("tn", S, dy[f0 * L:], dg[f0 * L:], M=L, N=ci, K=L, lda=lp, ldb=ci, ldc=c3, batch=gc, bsa=L * lp, bsb=bs, bsc=bq,
             amax_a=one, amax_b=am_dy, amax_c=am_dq_slot)
        check(lib.glf_softmax_rows_bwd_ld(_p(S), _p(dP), gc * L, L, lp, _stream()), "softmax_rows_bwd_ld")       # dP <- dS
        am_dS = amax_slot(dev)                                       # |dS| <= P (|dP| + |sum dP P|) <= 2 max|dP|
        if am_dS is not None:
            check(lib.glf_amax_combine(_p(am_dP), None, 2.0, 0, _p(am_dS), _stream()), "amax_combine")
        _transposed(K, f0, gc, L, lp, k, ld, KT)
        gemm("nt", dP, KT, dQ[f0 * L:], M=L, N=k, K=lp, lda=lp, ldb=lp, ldc=ldd, batch=gc, bsa=L * lp, bsb=k * lp, bsc=L * ldd,
             accumulate=acc, amax_a=am_dS, amax_b=am, amax_c=am_d)
        gemm("tn", dP, Q[f0 * L:], dK[f0 * L:], M=L, N=k, K=L, lda=lp, ldb=ld, ldc=ldd, batch=gc, bsa=L * lp, bsb=L * ld, bsc=L * ldd,
             accumulate=acc, amax_a=am_dS, amax_b=am, amax_c=am_d)
    if am_dq_slot is not None:
        set_amax(dqkv, am_dq_slot)


def _full_softmax_fwd(G, scores, g, y):
    """att = softmax(Q K^T) of every frame, materialised and kept for backward, y = att g: the widths no other route takes (toy modules)."""
    Q, K, ld, k, am = scores
    n, L, ci = G.n, G.L, G.ci
    att = torch.empty(n, L, L, **G.f32)
    gemm("nt", Q, K, att, M=L, N=L, K=k, lda=ld, ldb=ld, ldc=L, batch=n, bsa=L * ld, bsb=L * ld, bsc=L * L, amax_a=am, amax_b=am)
    check(lib.glf_softmax_rows(_p(att), n * L, L, _stream()), "softmax_rows")
    gemm("nn", att, g, y, M=L, N=ci, K=L, lda=L, ldb=G.c3, ldc=ci, batch=n, bsa=L * L, bsb=G.bq, bsc=L * ci)
    return att


def _full_softmax_bwd(G, scores, att, g, am_q, dy, am_dy, dqkv, sink) -> None:
    """y_n = P_n g_n ; P_n = softmax(Q_n K_n^T), P_n = att saved by the forward pass."""
    Q, K, ld, k, am = scores
    dQ, dK, ldd, acc, _ = sink
    n, L, ci, c3, bq, bs = G.n, G.L, G.ci, G.c3, G.bq, G.bs
    dg = _slices(G, dqkv)[2]
    dP = torch.empty(n, L, L, **G.f32)
    gemm("nt", dy, g, dP, M=L, N=L, K=ci, lda=ci, ldb=c3, ldc=L, batch=n, bsa=bs, bsb=bq, bsc=L * L, amax_a=am_dy, amax_b=am_q)
    gemm("tn", att, dy, dg, M=L, N=ci, K=L, lda=L, ldb=ci, ldc=c3, batch=n, bsa=L * L, bsb=bs, bsc=bq,
         amax_a=amax_of(att), amax_b=am_dy)
    check(lib.glf_softmax_rows_bwd(_p(att), _p(dP), n * L, L, _stream()), "softmax_rows_bwd")   # dP <- dS
    gemm("nn", dP, K, dQ, M=L, N=k, K=L, lda=L, ldb=ld, ldc=ldd, batch=n, bsa=L * L, bsb=L * ld, bsc=L * ldd, accumulate=acc)
    gemm("tn", dP, Q, dK, M=L, N=k, K=L, lda=L, ldb=ld, ldc=ldd, batch=n, bsa=L * L, bsb=L * ld, bsc=L * ldd, accumulate=acc,
         amax_a=amax_of(dP), amax_b=am)


# One core per mode: fwd(G, x, qkv, am_x, am_q, wf) -> (y, att), att being what the mode keeps for its backward pass;
# bwd(G, x, qkv, att, y, am_q, dy, am_dy, dqkv, am_dq_slot, du, wf) fills dqkv ('gaussian' also adds into du) -> (dW_f, db_f).
# wf = (W_f weight, W_f bias) of 'concatenate'.  Score-shaped buffers are locals of these functions: dead when they return.
def _dot_fwd(G, x, qkv, am_x, am_q, wf):
    n, L, ci, c3, bq, dev = G.n, G.L, G.ci, G.c3, G.bq, G.dev
    th, ph, g = _slices(G, qkv)
    y = torch.empty(G.rows, ci, **G.f32)
    att = torch.empty(n, ci, ci, **G.f32)                              # M_n = phi_n^T g_n / L
    am_att = amax_slot(dev)
    gemm("tn", ph, g, att, M=ci, N=ci, K=L, lda=c3, ldb=c3, ldc=ci, batch=n, bsa=bq, bsb=bq,
         bsc=ci * ci, alpha=1.0 / L, amax_a=am_q, amax_b=am_q, amax_c=am_att)
    set_amax(att, am_att)
    if split_mode() and ci % 32 == 0:      # y_n = theta_n M_n as NT against M_n^T (split-bf16 kernels are NT / TN only)
        attT = transpose2d(att, ci, ci, n)
        am_y = amax_slot(dev)
        gemm("nt", th, attT, y, M=L, N=ci, K=ci, lda=c3, ldb=ci, ldc=ci, batch=n, bsa=bq, bsb=ci * ci, bsc=L * ci,
             amax_a=am_q, amax_b=am_att, amax_c=am_y)                  # a transpose keeps the maximum
        set_amax(y, am_y)
    else:
        gemm("nn", th, att, y, M=L, N=ci, K=ci, lda=c3, ldb=ci, ldc=ci, batch=n, bsa=bq, bsb=ci * ci, bsc=L * ci)
    return y, att


def _dot_bwd(G, x, qkv, att, y, am_q, dy, am_dy, dqkv, am_dq_slot, du, wf):
    # y_n = th_n M_n ;  M_n = ph_n^T g_n / L
    n, L, ci, c3, bq, bs, dev = G.n, G.L, G.ci, G.c3, G.bq, G.bs, G.dev
    th, ph, g = _slices(G, qkv)
    dth, dph, dg = _slices(G, dqkv)
    gemm("nt", dy, att, dth, M=L, N=ci, K=ci, lda=ci, ldb=ci, ldc=c3, batch=n, bsa=bs, bsb=ci * ci, bsc=bq,
         amax_a=am_dy, amax_b=amax_of(att), amax_c=am_dq_slot)
    dM = torch.empty(n, ci, ci, **G.f32)
    am_dM = amax_slot(dev)
    gemm("tn", th, dy, dM, M=ci, N=ci, K=L, lda=c3, ldb=ci, ldc=ci, batch=n, bsa=bq, bsb=bs, bsc=ci * ci,
         amax_a=am_q, amax_b=am_dy, amax_c=am_dM)
    set_amax(dM, am_dM)
    gemm("nt", g, dM, dph, M=L, N=ci, K=ci, lda=c3, ldb=ci, ldc=c3, batch=n, bsa=bq, bsb=ci * ci, bsc=bq, alpha=1.0 / L,
         amax_a=am_q, amax_b=am_dM, amax_c=am_dq_slot)
    if _split_dgrad(G):
        dMT = transpose2d(dM, ci, ci, n)
        gemm("nt", ph, dMT, dg, M=L, N=ci, K=ci, lda=c3, ldb=ci, ldc=c3, batch=n, bsa=bq, bsb=ci * ci, bsc=bq, alpha=1.0 / L,
             amax_a=am_q, amax_b=am_dM, amax_c=am_dq_slot)
        if am_dq_slot is not None:
            set_amax(dqkv, am_dq_slot)
    else:
        gemm("nn", ph, dM, dg, M=L, N=ci, K=ci, lda=c3, ldb=ci, ldc=c3, batch=n, bsa=bq, bsb=ci * ci, bsc=bq, alpha=1.0 / L)
    return None, None


def _embedded_fwd(G, x, qkv, am_x, am_q, wf):
    n, L, ci, c3 = G.n, G.L, G.ci, G.c3
    th, ph, g = _slices(G, qkv)
    y = torch.empty(G.rows, ci, **G.f32)
    if chunked_softmax_ok(ci, L):          # the frame-group route on the split-fp16 kernels
        att = torch.empty(1, **G.f32)
        _group_softmax_fwd(G, (th, ph, c3, ci, am_q), g, am_q, y)
    elif fused_softmax_ok(ci):
        # ONE kernel: 64-query blocks, key tiles through LDS, online row max / sum, P g in MFMA accumulators; the
        # [L, L] scores are never written.  `att` holds the row log-sum-exp the backward pass recomputes them against.
        att = torch.empty(n * L, **G.f32)
        ap = _attn_params(n, L, ci, c3, ci)
        check(lib.glf_attn_softmax_fwd(_p(th), _p(ph), _p(g), _p(y), _p(att), C.byref(ap), _stream()), "attn_softmax_fwd")
    else:
        att = _full_softmax_fwd(G, (th, ph, c3, ci, am_q), g, y)
    return y, att


def _embedded_bwd(G, x, qkv, att, y, am_q, dy, am_dy, dqkv, am_dq_slot, du, wf):
    n, L, ci, c3 = G.n, G.L, G.ci, G.c3
    th, ph, g = _slices(G, qkv)
    dth, dph, dg = _slices(G, dqkv)
    if chunked_softmax_ok(ci, L):          # dtheta = dS phi; dphi = dS^T theta
        _group_softmax_bwd(G, (th, ph, c3, ci, am_q), g, am_q, dy, am_dy, dqkv, am_dq_slot, (dth, dph, c3, False, am_dq_slot))
    elif fused_softmax_ok(ci):
        # recompute the score tiles from theta / phi and the saved row log-sum-exp: three passes (dg, dphi, dtheta), each
        # writing its slice of dqkv exactly once
        ap = _attn_params(n, L, ci, c3, ci)
        dsum = torch.empty(G.rows, **G.f32)
        check(lib.glf_attn_softmax_bwd(_p(th), _p(ph), _p(g), _p(y), _p(dy), _p(att), _p(dth), _p(dph), _p(dg), _p(dsum), C.byref(ap),
                                       _stream()), "attn_softmax_bwd")
    else:
        _full_softmax_bwd(G, (th, ph, c3, ci, am_q), att, g, am_q, dy, am_dy, dqkv, (dth, dph, c3, False, None))
    return None, None


def _gaussian_fwd(G, x, qkv, am_x, am_q, wf):
    # the routes of 'embedded' with theta = phi = x: S = x x^T over C, P = softmax(S), y = P g
    c, g = G.c, _slices(G, qkv)[2]
    x2 = x.view(G.rows, c)
    y = torch.empty(G.rows, G.ci, **G.f32)
    if gaussian_chunked_ok(G.ci):
        att = torch.empty(1, **G.f32)
        _group_softmax_fwd(G, (x2, x2, c, c, am_x), g, am_q, y)
    else:
        att = _full_softmax_fwd(G, (x2, x2, c, c, am_x), g, y)
    return y, att


def _gaussian_bwd(G, x, qkv, att, y, am_q, dy, am_dy, dqkv, am_dq_slot, du, wf):
    # x is BOTH operands of the scores, so dx (= du, which already holds the residual's gradient) += dS x + dS^T x
    c, g = G.c, _slices(G, qkv)[2]
    x2 = x.view(G.rows, c)
    scores, sink = (x2, x2, c, c, amax_of(x)), (du, du, c, True, None)
    if gaussian_chunked_ok(G.ci):
        _group_softmax_bwd(G, scores, g, am_q, dy, am_dy, dqkv, am_dq_slot, sink)
    else:
        _full_softmax_bwd(G, scores, att, g, am_q, dy, am_dy, dqkv, sink)
    return None, None


def _concatenate_fwd(G, x, qkv, am_x, am_q, wf):
    # a = theta w_theta, b = phi w_phi (one scalar per position), then ONE kernel forms the relu(a_i + b_j + c) tiles in LDS
    # and contracts them with g; `att` keeps a | b for the backward pass
    n, L, ci, c3, rows = G.n, G.L, G.ci, G.c3, G.rows
    th, ph, g = _slices(G, qkv)
    wf_w, wf_b = wf
    if not pair_relu_ok(ci):
        raise RuntimeError(f"TPAVI mode 'concatenate' is built for Ci % 32 == 0, Ci <= 1024 (got {ci})")
    y = torch.empty(rows, ci, **G.f32)
    wrow = _contig(wf_w.detach()).view(2 * ci)
    att = torch.empty(2, rows, **G.f32)
    check(lib.glf_attn_pair_proj_fwd(_p(th), _p(ph), c3, _p(wrow), _p(att[0]), _p(att[1]), rows, ci, _stream()), "attn_pair_proj_fwd")
    pp = _pair_params(n, L, ci, c3, ci, ci, c3)
    check(lib.glf_attn_pair_relu_fwd(_p(att[0]), _p(att[1]), _p(wf_b), _p(g), _p(y), C.byref(pp), _stream()), "attn_pair_relu_fwd")
    return y, att


def _concatenate_bwd(G, x, qkv, att, y, am_q, dy, am_dy, dqkv, am_dq_slot, du, wf):
    # dg, da, db, dc from the fused kernels (every element written once, fixed summation order), then the skinny ends:
    # dtheta = da w_theta^T, dphi = db w_phi^T into dqkv, and W_f's gradient [theta^T da | phi^T db]
    n, L, ci, c3, rows = G.n, G.L, G.ci, G.c3, G.rows
    th, ph, g = _slices(G, qkv)
    dth, dph, dg = _slices(G, dqkv)
    wf_w, wf_b = wf
    wrow = _contig(wf_w.detach()).view(2 * ci)
    dab = torch.empty(2, rows, **G.f32)
    dwf_w = torch.empty(2 * ci, **G.f32)
    dwf_b = torch.empty(1, **G.f32)
    pp = _pair_params(n, L, ci, c3, ci, ci, c3)
    nb = int(lib.glf_attn_pair_relu_workspace_bytes(C.byref(pp)))
    ws = torch.empty(nb // 4, **G.f32)
    check(lib.glf_attn_pair_relu_bwd(_p(att[0]), _p(att[1]), _p(wf_b), _p(g), _p(dy), _p(dg), _p(dab[0]), _p(dab[1]), _p(dwf_b),
                                     _p(ws), nb, C.byref(pp), _stream()), "attn_pair_relu_bwd")
    nb = int(lib.glf_attn_pair_proj_workspace_bytes(rows, ci))
    ws = torch.empty(nb // 4, **G.f32)
    check(lib.glf_attn_pair_proj_bwd(_p(th), _p(ph), c3, _p(wrow), _p(dab[0]), _p(dab[1]), _p(dth), _p(dph), c3, _p(dwf_w), _p(ws), nb,
                                     rows, ci, _stream()), "attn_pair_proj_bwd")
    return dwf_w.view(wf_w.shape), dwf_b


_CORES = {"dot": (_dot_fwd, _dot_bwd), "embedded": (_embedded_fwd, _embedded_bwd), "gaussian": (_gaussian_fwd, _gaussian_bwd),
          "concatenate": (_concatenate_fwd, _concatenate_bwd)}


def _split_dgrad(G) -> bool:
    """The block's dgrad contractions run as NT on the split kernels (against cached transposed weights)."""
    return split_mode() and G.ci % 32 == 0 and G.c % 32 == 0


# Head (the stacked projection) and tail (W_z, BatchNorm, residual, LayerNorm) that every mode shares
def _project(G, x, Wcat, bcat):
    """theta | phi | g in ONE contraction over the shared input: qkv[rows, 3*ci] (x is read once; the cores' operands are column
    slices with row stride 3*ci).  -> qkv, max|x|, max|qkv|, the packed image of x to retain (or None)."""
    rows, c, c3 = G.rows, G.c, G.c3
    qkv = torch.empty(rows, c3, **G.f32)
    am_x = amax_of(x)
    am_q = amax_slot(G.dev)                # max|qkv| from the epilogue: one bound for the theta | phi | g column slices
    am_wc = amax_of(Wcat)
    ok = nt_presplit_ok(c, c, c)
    wb, pb = pick(Wcat, weight_packed(Wcat, Wcat, "w", am_wc) if ok else None, ok)
    xa, pa = pick(x, act_packed(x, am_x) if ok else None, ok)       # read again by the weight gradient of the projections
    gemm("nt", xa, wb, qkv, M=rows, N=c3, K=c, lda=c, ldb=c, ldc=c3, bias=bcat, amax_a=am_x, amax_b=am_wc, amax_c=am_q,
         a_packed=pa, b_packed=pb)
    x_packed = (xa, am_x) if (pa and packed_hit(x, am_x) is not None) else None      # retained while memory allows
    set_amax(qkv, am_q)
    return qkv, am_x, am_q, x_packed


def _project_bwd(G, x, dqkv, Wcat, du, x_packed):
    """The three projections as one, qkv = x Wcat^T + bcat: -> dWcat, dbcat; the dgrad is added onto du (one RMW)."""
    rows, c, c3 = G.rows, G.c, G.c3
    sp = _tn_split(rows, c3, c, 1)
    if not split_mode():
        # exact fp32: this weight gradient's terms cancel to ~1e-3 of their size, and the exact TN kernel adds its K-tile sums in
        # ONE fp32 chain per slice -- slices of at most 512 rows (16 K-tiles; the second stage adds the slabs in double) keep the
        # strict-precision leg at least as accurate as the split-fp16 one (3e-3 -> 1.5e-3 on the smoke fixture)
        sp = max(sp, min((rows + 511) // 512, 65535))
    dWcat = torch.empty(c3, c, **G.f32)
    am_dq = amax_of(dqkv)
    ok = tn_presplit_ok(c3, c, c3, c)
    dbcat = None
    if ok and TAIL_BWD_FUSED and rows < (1 << 31) // c3:
        _, dbcat = act_packed_colsum(dqkv, am_dq, rows, c3)          # the image is found again by act_packed
    dq_a, pa = pick(dqkv, act_packed(dqkv, am_dq, True) if ok else None, ok)
    am_x = x_packed[1] if x_packed is not None else amax_of(x)
    xb, pb = pick(x, x_packed[0] if x_packed is not None else None, ok)
    gemm("tn", dq_a, xb, dWcat, M=c3, N=c, K=rows, lda=c3, ldb=c, ldc=c, split=sp, amax_a=am_dq, amax_b=am_x, a_packed=pa, b_packed=pb)
    if dbcat is None:
        dbcat = colsum(dqkv, rows, c3)
    if _split_dgrad(G):
        WcatT = weight_T(Wcat, Wcat)                        # cached with the stacked operand (one rebuild per weight update)
        am_wc = amax_of(Wcat)
        ok = nt_presplit_ok(c3, c3, c3)
        wb, pb = pick(WcatT, weight_packed(WcatT, Wcat, "T2", am_wc), ok)
        da, pa = pick(dqkv, act_packed(dqkv, am_dq, True) if ok else None, ok)
        gemm("nt", da, wb, du, M=rows, N=c, K=c3, lda=c3, ldb=c3, ldc=c, accumulate=True, amax_a=am_dq, amax_b=am_wc,
             a_packed=pa, b_packed=pb)
    else:
        gemm("nn", dqkv, Wcat, du, M=rows, N=c, K=c3, lda=c3, ldb=c, ldc=c, accumulate=True)
    return dWcat, dbcat


def _tail(G, x, y, zW, wz_w, wz_b, bn_g, bn_b, ln_g, ln_b, rmean, rvar, nbt, training, momentum, bn_eps, ln_eps):
    """w = W_z y + b;  z = LayerNorm_C( BatchNorm3d(w) + x ).  -> z, w, mean, invstd, the LayerNorm row statistics, the packed image
    of y to retain (or None)."""
    rows, c, ci, dev = G.rows, G.c, G.ci, G.dev
    wz = torch.empty(rows, c, **G.f32)
    am_zw = amax_of(wz_w)
    ok = nt_presplit_ok(ci, ci, ci)
    wb, pb = pick(zW, weight_packed(zW, wz_w, "w", am_zw) if ok else None, ok)
    am_y = amax_of(y)
    ya, pa = pick(y, act_packed(y, am_y) if ok else None, ok)
    # train(): the BatchNorm statistics of w come out of the contraction's own epilogue (column sums of w and w^2 in double,
    # glf_gemm_params.colstats) -- no separate pass over the 1.2 GB tensor
    fuse_stats = training and split_mode() and nt_presplit_ok(ci, ci, ci) and c % 4 == 0
    sums = stats_slot(c, dev) if fuse_stats else None
    gemm("nt", ya, wb, wz, M=rows, N=c, K=ci, lda=ci, ldb=ci, ldc=c, bias=wz_b, amax_a=am_y, amax_b=am_zw, a_packed=pa, b_packed=pb,
         colstats=sums)
    y_packed = (ya, am_y) if (pa and packed_hit(y, am_y) is not None) else None
    mean = torch.empty(c, **G.f32)
    invstd = torch.empty(c, **G.f32)
    if fuse_stats:
        check(lib.glf_bn_stats_from_sums(_p(sums), rows, c, bn_eps, momentum, _p(mean), _p(invstd), _p(rmean), _p(rvar), _p(nbt),
                                         _stream()), "bn_stats_from_sums")
    elif training:
        check(lib.glf_bn_stats(_p(wz), c, rows, c, bn_eps, momentum, _p(mean), _p(invstd), _p(rmean), _p(rvar), _p(nbt),
                               _p(_ws(rows, c, dev)), _stream()), "bn_stats")
    else:
        check(lib.glf_bn_eval_coeffs(_p(rmean), _p(rvar), bn_eps, _p(mean), _p(invstd), c, _stream()), "bn_eval_coeffs")
    z = torch.empty_like(x)
    rmu = torch.empty(rows, **G.f32)
    rrs = torch.empty(rows, **G.f32)
    am_z = amax_slot(dev)                      # max|z|: the heads' first convolutions read z (through the global + local sum)
    check(lib.glf_bn_res_ln_fwd(_p(wz), _p(x), _p(mean), _p(invstd), _p(bn_g), _p(bn_b), _p(ln_g), _p(ln_b), ln_eps,
                                _p(z), _p(rmu), _p(rrs), rows, c, _p(am_z), _stream()), "bn_res_ln_fwd")
    set_amax(z, am_z)
    return z, wz, mean, invstd, rmu, rrs, y_packed


def _tail_bwd(G, dz, x, y, wz, mean, invstd, rmu, rrs, zW, wz_o, bn_g, bn_b, ln_g, training, y_packed):
    """-> du (gradient of u = BN(w) + x: also the residual's gradient), dy, (dzW, dzb, dbn_g, dbn_b, dln_g, dln_b).  dwz and its
    packed image die here, before dqkv is allocated."""
    rows, c, ci, dev = G.rows, G.c, G.ci, G.dev
    du = torch.empty(rows, c, **G.f32)
    dln_g = torch.empty(c, **G.f32)
    dln_b = torch.empty(c, **G.f32)
    # BatchNorm3d backward on w.  Its result dwz has three readers: the weight gradient and the dgrad of W_z -- contractions --
    # and W_z's bias gradient, the column sum of dwz.  In train mode that sum is ZERO in exact arithmetic (the bias feeds a
    # BatchNorm: sum_r dwz = -gamma invstd (sum_r xhat) sum(g xhat) / n and sum_r xhat = 0); what fp32 kernels -- the
    # reference's included -- return there is rounding noise.  So in train mode dwz is written ONCE, as the packed image
    # the two contractions read (glf_bn_bwd packed_dx), and the bias gradient is returned as the exact value.
    split = _split_dgrad(G)
    dwz = torch.empty(rows, c, **G.f32)
    am_dwz_slot = amax_slot(dev)
    dbn_g = torch.empty(c, **G.f32)
    dbn_b = torch.empty(c, **G.f32)
    dwz_pk = bool(training and split and am_dwz_slot is not None and nt_presplit_ok(c, c, c) and tn_presplit_ok(c, ci, c, ci))
    if TAIL_BWD_FUSED:
        # one walk over dz / w / x: du, the LayerNorm parameter gradients, the BatchNorm sums (kept in `keep` for the apply half) and,
        # for the packed image, its bound -- then the apply half alone (packed_dx 3: the packed image, 4: plain fp32)
        keep = torch.empty(2 * c, **G.f32)
        ws = _ws(rows, c, dev)
        check(lib.glf_bn_res_ln_bwd_sums(_p(dz), _p(wz), _p(x), _p(mean), _p(invstd), _p(bn_g), _p(bn_b), _p(ln_g), _p(rmu), _p(rrs),
                                         _p(du), _p(dln_g), _p(dln_b), _p(dbn_g), _p(dbn_b), _p(keep), _p(am_dwz_slot) if dwz_pk else None,
                                         rows, c, int(training), _p(ws), _stream()), "bn_res_ln_bwd_sums")
        check(lib.glf_bn_bwd(_p(du), c, _p(wz), c, None, c, _p(mean), _p(invstd), _p(bn_g), None, _p(dwz), c, None, c,
                             None, None, rows, c, 0, int(training), _p(ws), _p(am_dwz_slot), 3 if dwz_pk else 4, None, None, 0, _p(keep),
                             _stream()), "bn_bwd")
    else:
        check(lib.glf_bn_res_ln_bwd(_p(dz), _p(wz), _p(x), _p(mean), _p(invstd), _p(bn_g), _p(bn_b), _p(ln_g), _p(rmu), _p(rrs),
                                    _p(du), _p(dln_g), _p(dln_b), rows, c, _p(_ws(rows, c, dev)), _stream()), "bn_res_ln_bwd")
        fused = bnbwd_slot(c, dev) if c <= 4096 else None
        check(lib.glf_bn_bwd(_p(du), c, _p(wz), c, None, c, _p(mean), _p(invstd), _p(bn_g), None, _p(dwz), c, None, c,
                             _p(dbn_g), _p(dbn_b), rows, c, 0, int(training), None if fused is not None else _p(_ws(rows, c, dev)), _p(am_dwz_slot),
                             int(dwz_pk), None, None, 0, _p(fused), _stream()), "bn_bwd")
    set_amax(dwz, am_dwz_slot)
    # W_z: w = y zW^T + b
    sp = _tn_split(rows, c, ci, 1)
    if not split_mode():
        sp = max(sp, min((rows + 511) // 512, 65535))          # (as for the projections' weight gradient)
    dzW = torch.empty(c, ci, **G.f32)
    am_dwz = amax_of(dwz)
    ok = tn_presplit_ok(c, ci, c, ci)
    dwz_a, pa = (dwz, True) if dwz_pk else pick(dwz, act_packed(dwz, am_dwz, True) if ok else None, ok)       # shared with the NT contraction below
    am_y = y_packed[1] if y_packed is not None else amax_of(y)
    yb, pb = pick(y, y_packed[0] if y_packed is not None else None, ok)
    gemm("tn", dwz_a, yb, dzW, M=c, N=ci, K=rows, lda=c, ldb=ci, ldc=ci, split=sp, amax_a=am_dwz, amax_b=am_y, a_packed=pa, b_packed=pb)
    dzb = zeros(c, device=dev) if dwz_pk else colsum(dwz, rows, c)
    dy = torch.empty(rows, ci, **G.f32)
    if split:
        am_dy_slot = amax_slot(dev)
        zWT, am_zw = weight_T(zW, wz_o), amax_of(wz_o)
        ok = nt_presplit_ok(c, c, c)
        wb, pb = pick(zWT, weight_packed(zWT, wz_o, "T2", am_zw), ok)
        da, pa = (dwz, True) if dwz_pk else pick(dwz, act_packed(dwz, am_dwz, True) if ok else None, ok)
        gemm("nt", da, wb, dy, M=rows, N=ci, K=c, lda=c, ldb=c, ldc=ci, amax_a=am_dwz, amax_b=am_zw,
             amax_c=am_dy_slot, a_packed=pa, b_packed=pb)
        set_amax(dy, am_dy_slot)
    else:
        gemm("nn", dwz, zW, dy, M=rows, N=ci, K=c, lda=c, ldb=ci, ldc=ci)
    return du, dy, (dzW, dzb, dbn_g, dbn_b, dln_g, dln_b)


class TpaviFn(Function):
    @staticmethod
    def forward(ctx, x, th_w, th_b, ph_w, ph_b, g_w, g_b, wz_w, wz_b, bn_g, bn_b, ln_g, ln_b,
                rmean, rvar, nbt, training: bool, momentum: float, bn_eps: float, ln_eps: float, mode: str, wf_w=None, wf_b=None):
        """th_* / ph_*: None for 'gaussian' (the mode owns no theta / phi); wf_w [1, 2 Ci, 1, 1], wf_b [1]: W_f of 'concatenate'."""
        x, G = _unpack(x, g_w, mode)
        zW = _contig(wz_w.detach()).view(wz_w.shape[0], wz_w.shape[1])       # Conv3d 1x1x1 weight -> [out, in]
        Wcat, bcat = _qkv_weights((g_w, g_b) if G.npj == 1 else (th_w, ph_w, g_w, th_b, ph_b, g_b))      # [npj*ci, c], [npj*ci]
        qkv, am_x, am_q, ctx.x_packed = _project(G, x, Wcat, bcat)
        ctx.qkv_owner = g_w if G.npj == 1 else th_w    # parameter the stacked operand (and its cached transpose) is keyed on
        ctx.wf = (wf_w, wf_b)
        y, att = _CORES[mode][0](G, x, qkv, am_x, am_q, ctx.wf)
        z, wz, mean, invstd, rmu, rrs, ctx.y_packed = _tail(G, x, y, zW, wz_w, wz_b, bn_g, bn_b, ln_g, ln_b, rmean, rvar, nbt,
                                                            training, momentum, bn_eps, ln_eps)
        ctx.save_for_backward(x, qkv, att, y, wz, mean, invstd, rmu, rrs, Wcat, zW, bn_g, bn_b, ln_g)
        ctx.cfg = (G.n, G.L, G.c, G.ci, training, mode, tuple(g_w.shape), tuple(wz_w.shape))
        ctx.owners = (wz_w,)                      # parameter owning zW (transposed-copy cache key)
        return z

    @staticmethod
    @once_differentiable
    def backward(ctx, dz):
        (x, qkv, att, y, wz, mean, invstd, rmu, rrs, Wcat, zW, bn_g, bn_b, ln_g) = ctx.saved_tensors
        n, L, c, ci, training, mode, pshape, zshape = ctx.cfg
        G = _block(n, L, c, ci, mode, dz.device)
        du, dy, (dzW, dzb, dbn_g, dbn_b, dln_g, dln_b) = _tail_bwd(G, _contig(dz), x, y, wz, mean, invstd, rmu, rrs, zW, ctx.owners[0],
                                                                  bn_g, bn_b, ln_g, training, ctx.y_packed)
        dqkv = torch.empty(G.rows, G.c3, **G.f32)             # [d theta | d phi | d g], row stride 3*ci
        am_dq_slot = amax_slot(G.dev)                         # its writers (in the core) all report into one slot
        dwf_w, dwf_b = _CORES[mode][1](G, x, qkv, att, y, amax_of(qkv), dy, amax_of(dy), dqkv, am_dq_slot, du, ctx.wf)
        del dy
        dWcat, dbcat = _project_bwd(G, x, dqkv, Wcat, du, ctx.x_packed)      # dx = du: the residual's gradient, accumulated in place
        return _grads(G, x, du, dWcat, dbcat, pshape, dzW.view(zshape), dzb, dbn_g, dbn_b, dln_g, dln_b, dwf_w, dwf_b)


def tpavi_forward(x5: torch.Tensor, mod) -> torch.Tensor:
    """x5: [N, V, h, w, C]; mod: a models.ours.TPAVIModule (parameter container)."""
    bn = mod.W_z[1]
    training = bn.training
    if training and bn.momentum is None:
        raise RuntimeError("glfusion_amd: cumulative-average BatchNorm (momentum=None) is not built")
    fn = TpaviFn
    if x5.dtype == torch.bfloat16:
        from .fusion16 import Tpavi16Fn
        fn = Tpavi16Fn
    theta, phi = getattr(mod, "theta", None), getattr(mod, "phi", None)          # 'gaussian' owns neither
    args = (x5, theta.weight if theta is not None else None, theta.bias if theta is not None else None,
            phi.weight if phi is not None else None, phi.bias if phi is not None else None, mod.g.weight, mod.g.bias,
            mod.W_z[0].weight, mod.W_z[0].bias, bn.weight, bn.bias, mod.norm_layer.weight, mod.norm_layer.bias,
            bn.running_mean, bn.running_var, bn.num_batches_tracked if training else None,
            training, float(bn.momentum or 0.0), float(bn.eps), float(mod.norm_layer.eps), mod.mode)
    wf = mod.W_f[0] if mod.mode == "concatenate" else None
    args += (wf.weight if wf is not None else None, wf.bias if wf is not None else None)
    return fn.apply(*args)
