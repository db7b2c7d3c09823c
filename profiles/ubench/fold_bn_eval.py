#!/usr/bin/env python3
"""Eval-forward latency with and without folded BatchNorm (ops.set_fold_bn) under f16x3: Global_and_Local in eval(), one clip of
40 frames x 3 views x 112^2, median of 20 timed forwards after 5 warm-ups, fold off against fold on in the same process.
Usage: fold_bn_eval.py [off|on|both] [frames]   -- `off` / `on` time one setting only (for a rocprofv3 --kernel-trace --stats run
of each, in a run of its own); `both` (default) prints the two medians and their ratio."""
import os
import statistics
import subprocess
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
import torch
from glfusion_amd import ops
from glfusion_amd.models import Global_and_Local

VIEWS = ["1", "3", "4"]
which = sys.argv[1] if len(sys.argv) > 1 else "both"
frames = int(sys.argv[2]) if len(sys.argv) > 2 else 40
WARMUP, STEPS = 5, 20

ops.set_precision("f16x3")
dev = torch.device("cuda", 0)
torch.manual_seed(0)
model = Global_and_Local(VIEWS).to(dev).eval()
gen = torch.Generator().manual_seed(1)
imgs = {v: torch.rand(frames, 1, 112, 112, generator=gen).to(dev) for v in VIEWS}


def median_ms(flag: bool) -> float:
    ops.set_fold_bn(flag)
    times = []
    with torch.no_grad():
        for i in range(WARMUP + STEPS):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            model(imgs)
            e1.record()
            torch.cuda.synchronize()
            if i >= WARMUP:
                times.append(e0.elapsed_time(e1))
    ops.set_fold_bn(False)
    return statistics.median(times)


try:
    commit = subprocess.run(["git", "rev-parse", "--short", "HEAD"], capture_output=True, text=True, cwd=os.path.dirname(os.path.abspath(__file__))).stdout.strip()
except OSError:
    commit = ""
print(f"fold_bn_eval: f16x3, eval forward, {frames} frames x {len(VIEWS)} views x 112^2, median of {STEPS} after {WARMUP} warm-ups; commit {commit or 'unknown'}")
res = {}
for name, flag in (("off", False), ("on", True)):
    if which in (name, "both"):
        before = ops.FOLD_COUNT[0]
        res[name] = median_ms(flag)
        print(f"fold {name:3s}: {res[name]:9.3f} ms per clip forward   ({ops.FOLD_COUNT[0] - before} glf_fold_bn launches in total)")
if len(res) == 2:
    print(f"ratio on / off: {res['on'] / res['off']:.4f}   (speed-up {res['off'] / res['on']:.3f}x)")
