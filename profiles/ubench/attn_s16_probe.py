#!/usr/bin/env python3
"""The fused 16-bit softmax attention kernels alone (TPAVIModule mode='embedded' under precision "bf16":
glf_s16_attn_softmax_fwd / _bwd, csrc/attn_s16.hip) at the C2 fusion-block shape (N = 64 frames, L = 2352, Ci = 1024) and the
config-5 shape (N = 2, L = 15 680): ms per pass, TFLOP/s and the fraction of the 2.5 PF dense bf16 MFMA peak.

Counting convention (one unit = one L x L x Ci product = 2 L^2 Ci FLOP per frame):
  algorithmic: forward 2 units (S = theta phi^T, P g); backward 5 units (S recomputed once, dP = dY g^T, dg, dphi, dtheta)
  executed:    forward 2 units; backward 8 units (the four-pass split recomputes S in each of DV / DK / DQ and dP in DK and DQ)
The backward time includes the D = rowsum(dY o Y) pass.  Run under rocprofv3 --kernel-trace --stats / --pmc
SQ_VALU_MFMA_BUSY_CYCLES for the per-kernel rows.  Usage: attn_s16_probe.py [iters]"""
import ctypes as C
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
import torch
from glfusion_amd._lib import AttnParams, check, lib

PEAK = 2500.0
iters = int(sys.argv[1]) if len(sys.argv) > 1 else 5
dev = torch.device("cuda", 0)
g = torch.Generator(device=dev).manual_seed(0)
for n, L, ci in ((64, 2352, 1024), (2, 15680, 1024)):
    rows = n * L
    qkv = (torch.randn(rows, 3 * ci, device=dev, generator=g) * (4.0 / ci ** 0.5) ** 0.5).to(torch.bfloat16)
    th, ph, gg = qkv[:, :ci], qkv[:, ci:2 * ci], qkv[:, 2 * ci:]
    y = torch.empty(rows, ci, device=dev, dtype=torch.bfloat16)
    lse = torch.empty(rows, device=dev)
    dy = torch.randn(rows, ci, device=dev, generator=g).to(torch.bfloat16)
    dqkv = torch.empty_like(qkv)
    dsum = torch.empty(rows, device=dev)
    ap = AttnParams()
    ap.frames, ap.L, ap.ci = n, L, ci
    ap.ldq = ap.ldk = ap.ldv = ap.ldd = 3 * ci
    ap.ldy, ap.lddy = ci, ci
    p = lambda t: C.c_void_p(t.data_ptr())  # noqa: E731
    fwd = lambda: check(lib.glf_s16_attn_softmax_fwd(p(th), p(ph), p(gg), p(y), p(lse), C.byref(ap), None), "fwd")  # noqa: E731
    bwd = lambda: check(lib.glf_s16_attn_softmax_bwd(p(th), p(ph), p(gg), p(y), p(dy), p(lse), p(dqkv[:, :ci]), p(dqkv[:, ci:2 * ci]),  # noqa: E731
                                                     p(dqkv[:, 2 * ci:]), p(dsum), C.byref(ap), None), "bwd")
    unit = 2.0 * n * L * L * ci
    for fn, name, alg, exe in ((fwd, "forward ", 2, 2), (bwd, "backward", 5, 8)):
        fn(); torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(iters):
            fn()
        torch.cuda.synchronize()
        dt = (time.perf_counter() - t0) / iters
        ta, te = alg * unit / dt / 1e12, exe * unit / dt / 1e12
        print(f"N={n} L={L} Ci={ci} {name}: {dt * 1e3:8.2f} ms  algorithmic {ta:6.1f} TFLOP/s ({ta / PEAK:.3f} of {PEAK:.0f} TF)  "
              f"executed {te:6.1f} TFLOP/s ({te / PEAK:.3f})", flush=True)
    del qkv, y, dy, dqkv
