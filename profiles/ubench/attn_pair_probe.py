#!/usr/bin/env python3
"""The fused pairwise-ReLU attention kernels (TPAVIModule mode='concatenate': glf_attn_pair_relu_fwd / _bwd) against the fused
exact-fp32 softmax attention (mode='embedded': glf_attn_softmax_fwd / _bwd) IN THE SAME PROCESS at the C2 shape (N = 64 frames,
L = 2352, Ci = 1024): median of 20 timed calls after 5 warm-ups, HIP events around each call.
Expectation: the pair forward does the P g half of the softmax forward's MFMA work and none of its QK^T; the pair
backward does one score-type and one product-type contraction per tile pair against the softmax backward's five and three.
Usage: attn_pair_probe.py  (run the GPU step under a time limit of its own: timeout -k 10 300 python ...)"""
import ctypes as C
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
import torch
from glfusion_amd._lib import AttnPairParams, AttnParams, check, lib

WARM, ITERS = 5, 20
dev = torch.device("cuda", 0)
gen = torch.Generator(device=dev).manual_seed(0)
n, L, ci = 64, 2352, 1024
rows = n * L
qkv = (torch.rand(rows, 3 * ci, device=dev, generator=gen) - 0.5) * 0.2
th, ph, gg = qkv[:, :ci], qkv[:, ci:2 * ci], qkv[:, 2 * ci:]
y = torch.empty(rows, ci, device=dev)
lse = torch.empty(rows, device=dev)
dy = torch.rand(rows, ci, device=dev, generator=gen) - 0.5
dqkv = torch.empty_like(qkv)
dsum = torch.empty(rows, device=dev)
a = torch.rand(rows, device=dev, generator=gen) - 0.5          # about half of the pairs pass the ReLU
b = torch.rand(rows, device=dev, generator=gen) - 0.5
c = torch.full((1,), 0.01, device=dev)
da, db, dc = torch.empty(rows, device=dev), torch.empty(rows, device=dev), torch.empty(1, device=dev)
ap = AttnParams()
ap.frames, ap.L, ap.ci = n, L, ci
ap.ldq = ap.ldk = ap.ldv = 3 * ci
ap.ldy, ap.lddy, ap.ldd = ci, ci, 3 * ci
pp = AttnPairParams()
pp.frames, pp.L, pp.ci = n, L, ci
pp.ldg, pp.ldy, pp.lddy, pp.lddg = 3 * ci, ci, ci, 3 * ci
nb = int(lib.glf_attn_pair_relu_workspace_bytes(C.byref(pp)))
ws = torch.empty(nb // 4, device=dev)
p = lambda t: C.c_void_p(t.data_ptr())
calls = {
    "softmax forward ": lambda: check(lib.glf_attn_softmax_fwd(p(th), p(ph), p(gg), p(y), p(lse), C.byref(ap), None), "fwd"),
    "softmax backward": lambda: check(lib.glf_attn_softmax_bwd(p(th), p(ph), p(gg), p(y), p(dy), p(lse), p(dqkv[:, :ci]), p(dqkv[:, ci:2 * ci]),
                                                                 p(dqkv[:, 2 * ci:]), p(dsum), C.byref(ap), None), "bwd"),
    "pair forward    ": lambda: check(lib.glf_attn_pair_relu_fwd(p(a), p(b), p(c), p(gg), p(y), C.byref(pp), None), "pair fwd"),
    "pair backward   ": lambda: check(lib.glf_attn_pair_relu_bwd(p(a), p(b), p(c), p(gg), p(dy), p(dqkv[:, 2 * ci:]), p(da), p(db), p(dc), p(ws), nb,
                                                                   C.byref(pp), None), "pair bwd"),
}
med = {}
for name, fn in calls.items():
    for _ in range(WARM):
        fn()
    torch.cuda.synchronize()
    ts = []
    for _ in range(ITERS):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(); fn(); e1.record()
        e1.synchronize()
        ts.append(e0.elapsed_time(e1))
    med[name] = statistics.median(ts)
    print(f"N={n} L={L} Ci={ci} {name}: median {med[name]:8.2f} ms  (min {min(ts):.2f}, max {max(ts):.2f}; {ITERS} calls after {WARM} warm-ups)", flush=True)
print(f"pair / softmax: forward {med['pair forward    '] / med['softmax forward ']:.3f}, backward {med['pair backward   '] / med['softmax backward']:.3f}"
      f"  (workspace of the pair backward: {nb / 2 ** 20:.1f} MiB)")
