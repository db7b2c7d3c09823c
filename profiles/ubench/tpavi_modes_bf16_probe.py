#!/usr/bin/env python3
"""Forward and backward time of TPAVIModule(2048, mode) for mode = 'gaussian' and 'concatenate' at N = 64, V = 3, 28 x 28 (L = 2352,
Ci = 1024) under precision 'bf16' and, IN THE SAME PROCESS, under 'f16x3' (fp32 storage, the split-fp16 contractions: code that
existed before the bf16 modes), so the comparison is against existing code.  Median of 10 timed calls after 3 warm-ups, HIP events
around each direction; the backward is timed on a fresh forward graph each time (its forward is outside the events).
Usage: tpavi_modes_bf16_probe.py  (run the GPU step under a time limit of its own: timeout -k 10 500 python ...)"""
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
import torch
from glfusion_amd import ops
from glfusion_amd.models.ours import TPAVIModule

WARM, ITERS = 3, 10
dev = torch.device("cuda", 0)
n, v, h, w, c = 64, 3, 28, 28, 2048


def fill(mod, seed):
    g = torch.Generator().manual_seed(seed)
    with torch.no_grad():
        for p in mod.parameters():
            if p.dim() > 1:
                p.copy_(torch.randn(p.shape, generator=g) * (2.0 / p[0].numel()) ** 0.5)
            else:
                p.copy_(1.0 + 0.1 * torch.randn(p.shape, generator=g))


x32 = 0.25 * torch.randn(n, v, h, w, c, generator=torch.Generator().manual_seed(1))
for mode in ("gaussian", "concatenate"):
    for prec in ("bf16", "f16x3"):
        ops.set_precision(prec)
        mod = TPAVIModule(c, mode=mode)
        fill(mod, 2)
        mod = mod.to(dev).train()
        x = x32.to(dev).to(torch.bfloat16 if prec == "bf16" else torch.float32).requires_grad_(True)
        gz = torch.ones_like(x)
        tf, tb = [], []
        for it in range(WARM + ITERS):
            e = [torch.cuda.Event(enable_timing=True) for _ in range(4)]
            e[0].record(); z = mod.forward_nvhwc(x); e[1].record()
            e[2].record(); z.backward(gz); e[3].record()
            torch.cuda.synchronize()
            x.grad = None
            for p in mod.parameters():
                p.grad = None
            if it >= WARM:
                tf.append(e[0].elapsed_time(e[1])); tb.append(e[2].elapsed_time(e[3]))
        print(f"TPAVIModule({c}, {mode!r}) N={n} L={v * h * w} {prec:6s}: forward median {statistics.median(tf):8.2f} ms (min {min(tf):.2f}, max {max(tf):.2f}), "
              f"backward median {statistics.median(tb):8.2f} ms (min {min(tb):.2f}, max {max(tb):.2f}); {ITERS} calls after {WARM} warm-ups, "
              f"peak {torch.cuda.max_memory_allocated() / 2 ** 30:.1f} GiB", flush=True)
        del mod, x, gz, z
        torch.cuda.empty_cache()
        torch.cuda.reset_peak_memory_stats()
ops.set_precision("f32")
