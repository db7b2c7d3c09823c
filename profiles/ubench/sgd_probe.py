#!/usr/bin/env python3
"""The fused SGD kernel (glf_sgd_step) over the model's real parameter list -- every parameter of the three-view Global_and_Local
that receives a gradient in training (all but the dead `network.*` template) -- without momentum (8 B read + 4 B written per
element) and with a momentum buffer (12 B + 8 B), next to glf_adam_step (16 B + 12 B) over the same table IN THE SAME PROCESS:
median of 20 timed calls after 5 warm-ups, HIP events around each call.  All three are HBM-bound; GB/s is the yardstick.
Usage: sgd_probe.py [out.txt]   (default profiles/sgd_step.txt; run the GPU step under a time limit of its own:
timeout -k 10 300 python ...)"""
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
import torch
from glfusion_amd import optim
from glfusion_amd._lib import check, lib
from glfusion_amd.models import Global_and_Local
from glfusion_amd.ops import _p

WARM, ITERS = 5, 20
out_path = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "profiles", "sgd_step.txt")
dev = torch.device("cuda", 0)
model = Global_and_Local(view_num=["1", "3", "4"]).to(dev)
params = [p for name, p in model.named_parameters() if not name.startswith("network.")]
gen = torch.Generator(device=dev).manual_seed(0)
grads = [torch.randn(p.shape, device=dev, generator=gen) * 1e-2 for p in params]
m = [torch.zeros_like(p) for p in params]
v = [torch.zeros_like(p) for p in params]
elems = sum(p.numel() for p in params)
rows = optim._chunk_rows([(p.data_ptr(), g.data_ptr(), a.data_ptr(), b.data_ptr(), p.numel()) for p, g, a, b in zip(params, grads, m, v)])
table = torch.from_numpy(rows).to(dev)
no_m = rows.copy()
no_m[:, 2:4] = 0                                                # momentum == 0: the buffer column may be null
table0 = torch.from_numpy(no_m).to(dev)
n = rows.shape[0]
lr, wd = 1e-6, 1e-5
step = [0]


def adam():
    step[0] += 1
    check(lib.glf_adam_step(_p(table), n, lr, 0.9, 0.999, 1e-8, wd, step[0], None), "adam_step")


calls = [
    ("glf_sgd_step  momentum 0              ", 12, lambda: check(lib.glf_sgd_step(_p(table0), n, lr, 0.0, 0.0, wd, 0, 0, None), "sgd_step")),
    ("glf_sgd_step  momentum 0.9            ", 20, lambda: check(lib.glf_sgd_step(_p(table), n, lr, 0.9, 0.0, wd, 0, 0, None), "sgd_step")),
    ("glf_sgd_step  momentum 0.9, nesterov  ", 20, lambda: check(lib.glf_sgd_step(_p(table), n, lr, 0.9, 0.0, wd, 1, 0, None), "sgd_step")),
    ("glf_sgd_step  momentum 0.9, first step", 16, lambda: check(lib.glf_sgd_step(_p(table), n, lr, 0.9, 0.0, wd, 0, 1, None), "sgd_step")),
    ("glf_adam_step                         ", 28, adam),
]
lines = [f"{len(params)} parameters, {elems} elements, {n} table rows of at most {optim.CHUNK} elements; "
         f"median of {ITERS} calls after {WARM} warm-ups, HIP events"]
for name, bytes_per_elem, fn in calls:
    for _ in range(WARM):
        fn()
    torch.cuda.synchronize()
    ts = []
    for _ in range(ITERS):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(); fn(); e1.record()
        e1.synchronize()
        ts.append(e0.elapsed_time(e1))
    med = statistics.median(ts)
    lines.append(f"{name}: {med:7.3f} ms  (min {min(ts):.3f}, max {max(ts):.3f})  {bytes_per_elem} B/element  "
                 f"{bytes_per_elem * elems / med / 1e6:7.1f} GB/s")
    print(lines[-1], flush=True)
with open(out_path, "w") as f:
    f.write("\n".join(lines) + "\n")
print(lines[0])
