#!/usr/bin/env python3
"""Global-norm gradient clipping over the model's real parameter list -- every parameter of the three-view Global_and_Local that
receives a gradient in training (all but the dead `network.*` template), the table of sgd_probe.py -- IN ONE PROCESS:
  * the norm: glf_grad_sumsq + glf_grad_clip_coef (4 B read per element), timed as the pair and each alone;
  * glf_adam_step against glf_adam_step_clipped (16 B + 12 B), glf_sgd_step against glf_sgd_step_clipped with a momentum buffer
    (12 B + 8 B) and without (8 B + 4 B): the two of a pair ALTERNATE call by call, so that both see the same machine;
  * glf_grad_scale (4 B + 4 B), the in-place form behind optim.clip_grad_norm_.
Median of 20 timed calls after 5 warm-ups, HIP events around each call.  All are HBM-bound; GB/s is the yardstick.  The record
the clipped kernels read holds a clipping coefficient (max_norm 1 against gradients of norm ~136), so the multiply is live.
Usage: grad_clip_probe.py [out.txt]   (default profiles/grad_clip.txt; run the GPU step under a time limit of its own:
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
out_path = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "profiles", "grad_clip.txt")
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
partials = torch.empty(n, dtype=torch.float64, device=dev)
record = torch.zeros(4, dtype=torch.float32, device=dev)
skipped = torch.zeros((), dtype=torch.int64, device=dev)
half = torch.tensor([0.0, 0.5, 1.0, 0.0], device=dev)          # glf_grad_scale's record: ok, and a coef that makes it write (1 would not)
step = [0]


def sumsq():
    check(lib.glf_grad_sumsq(_p(table), n, _p(partials), None), "grad_sumsq")


def finish():
    check(lib.glf_grad_clip_coef(_p(partials), n, 1.0, _p(record), _p(skipped), None), "grad_clip_coef")


def norm():
    sumsq()
    finish()


def adam(clipped):
    def fn():
        step[0] += 1
        args = (_p(table), n, lr, 0.9, 0.999, 1e-8, wd, step[0])
        if clipped:
            check(lib.glf_adam_step_clipped(*args, _p(record), None), "adam_step_clipped")
        else:
            check(lib.glf_adam_step(*args, None), "adam_step")
    return fn


def sgd(tab, momentum, clipped):
    def fn():
        args = (_p(tab), n, lr, momentum, 0.0, wd, 0, 0)
        if clipped:
            check(lib.glf_sgd_step_clipped(*args, _p(record), None), "sgd_step_clipped")
        else:
            check(lib.glf_sgd_step(*args, None), "sgd_step")
    return fn


def scale():
    # the gradients halve per call (20 + 5 calls: 1e-2 * 2^-25 stays a normal float)
    check(lib.glf_grad_scale(_p(table), n, _p(half), None), "grad_scale")


def timed(fn):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record(); fn(); e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1)


def measure(fns):
    """The calls of one group alternate: call 1 of each, call 2 of each, ..."""
    for _ in range(WARM):
        for fn in fns:
            fn()
    torch.cuda.synchronize()
    ts = [[] for _ in fns]
    for _ in range(ITERS):
        for t, fn in zip(ts, fns):
            t.append(timed(fn))
    return ts


groups = [
    [("glf_grad_sumsq + glf_grad_clip_coef   ", 4, norm)],
    [("glf_grad_sumsq                        ", 4, sumsq)],
    [("glf_grad_clip_coef                    ", 0, finish)],
    [("glf_adam_step                         ", 28, adam(False)), ("glf_adam_step_clipped                 ", 28, adam(True))],
    [("glf_sgd_step          momentum 0.9    ", 20, sgd(table, 0.9, False)), ("glf_sgd_step_clipped  momentum 0.9    ", 20, sgd(table, 0.9, True))],
    [("glf_sgd_step          momentum 0      ", 12, sgd(table0, 0.0, False)), ("glf_sgd_step_clipped  momentum 0      ", 12, sgd(table0, 0.0, True))],
    [("glf_grad_scale        coef 0.5        ", 8, scale)],
]
lines = [f"{len(params)} parameters, {elems} elements, {n} table rows of at most {optim.CHUNK} elements; "
         f"median of {ITERS} calls after {WARM} warm-ups, HIP events; the calls of a pair alternate"]
norm()
torch.cuda.synchronize()
lines.append(f"gradient norm {float(record[0]):.6g}, coef {float(record[1]):.6g}, ok {float(record[2]):.0f}, skipped {int(skipped)}")
print(lines[-1], flush=True)
for group in groups:
    for (name, bytes_per_elem, _), ts in zip(group, measure([fn for _, _, fn in group])):
        med = statistics.median(ts)
        rate = f"{bytes_per_elem} B/element  {bytes_per_elem * elems / med / 1e6:7.1f} GB/s" if bytes_per_elem else f"{n} partials, one workgroup"
        lines.append(f"{name}: {med:7.3f} ms  (min {min(ts):.3f}, max {max(ts):.3f})  {rate}")
        print(lines[-1], flush=True)
with open(out_path, "w") as f:
    f.write("\n".join(lines) + "\n")
print(lines[0])
