#!/usr/bin/env python3
"""Cross pseudo supervision at the config-2 shape (3 views, batch 4 x 16 frames of 112 x 112; unlabelled clips of 40 frames: masks
[40,5,112,112] = 2 508 800 logits per view and network) -- IN ONE PROCESS:
  * glf_cps_bce_sum forward (with stats, and with stats NULL) and backward on one view's pair of masks, against the same result
    composed from existing pieces: thresholds with torch, two glf_bce_logits_sum each way and, where the counts are part of the
    result, glf_overlap_counts.  The two of a pair ALTERNATE call by call; median of 20 timed calls after 5 warm-ups, HIP events
    around each call;
  * Trainer.train_step of Global_and_Local_CPS on a labelled batch plus a clip (cycle term on), cps_weight 0 against 0.5: the clip
    forward is paid either way, the difference is the CPS term and its backward through network 2's clip forward.  Median of 5
    steps after 3 warm-ups, a host clock around a step that ends in a device synchronise.
Usage: cps_step.py [out.txt]   (default profiles/cps_step.txt; run the GPU step under a time limit of its own:
timeout -k 10 500 python ...)"""
import os
import statistics
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
import torch
from glfusion_amd import ops
from glfusion_amd._lib import check, lib
from glfusion_amd.ops import _p

WARM, ITERS = 5, 20
VIEWS, BATCH_FRAMES, CLIP = ["1", "3", "4"], 64, 40
out_path = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "profiles", "cps_step.txt")
dev = torch.device("cuda", 0)
gen = torch.Generator(device=dev).manual_seed(0)
shape = (CLIP, 5, 112, 112)
a = torch.randn(shape, device=dev, generator=gen) * 6
b = torch.randn(shape, device=dev, generator=gen) * 6
n = a.numel()
loss = torch.empty(1, dtype=torch.float64, device=dev)
loss2 = torch.empty(1, dtype=torch.float64, device=dev)
stats = torch.empty(4, dtype=torch.int64, device=dev)
stats2 = torch.empty(4, dtype=torch.int64, device=dev)
da, db = torch.empty_like(a), torch.empty_like(b)
up = torch.tensor([0.5], device=dev)


def fused_fwd():
    check(lib.glf_cps_bce_sum(_p(a), _p(b), _p(loss), _p(stats), None, None, 1.0, None, n, None), "cps fwd")


def fused_fwd_no_stats():
    check(lib.glf_cps_bce_sum(_p(a), _p(b), _p(loss), None, None, None, 1.0, None, n, None), "cps fwd")


def fused_bwd():
    check(lib.glf_cps_bce_sum(_p(a), _p(b), _p(loss), None, _p(da), _p(db), 1.0, _p(up), n, None), "cps bwd")


def composed_fwd():
    ta, tb = (a > 0).float(), (b > 0).float()
    check(lib.glf_bce_logits_sum(_p(a), _p(tb), _p(loss), None, 1.0, None, n, None), "bce")
    check(lib.glf_bce_logits_sum(_p(b), _p(ta), _p(loss2), None, 1.0, None, n, None), "bce")
    return loss + loss2


def composed_fwd_stats():
    total = composed_fwd()
    check(lib.glf_overlap_counts(_p(a), _p((b > 0).float()), _p(stats2), n, None), "overlap_counts")
    return total


def composed_bwd():
    ta, tb = (a > 0).float(), (b > 0).float()
    check(lib.glf_bce_logits_sum(_p(a), _p(tb), _p(loss), _p(da), 1.0, _p(up), n, None), "bce")
    check(lib.glf_bce_logits_sum(_p(b), _p(ta), _p(loss2), _p(db), 1.0, _p(up), n, None), "bce")


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


lines = [f"masks {list(shape)} = {n} logits per view and network; kernels: median of {ITERS} calls after {WARM} warm-ups, HIP events, the "
         "two of a pair alternate"]
fused_fwd()
got = float(loss)
want = float(composed_fwd_stats())
assert stats.tolist() == stats2.tolist(), (stats.tolist(), stats2.tolist())
lines.append(f"loss fused {got:.6f}, composed {want:.6f}; agreement counts (11, 10, 01, 00) {stats.tolist()}, the same composed")
print(lines[-1], flush=True)
# bytes the fused kernel moves: forward 2 reads, backward 2 reads + 2 writes of 4 B
groups = [[("glf_cps_bce_sum forward (+ stats)         ", 8, fused_fwd), ("3 thresholds + 2 bce fwd + overlap_counts ", 0, composed_fwd_stats)],
          [("glf_cps_bce_sum forward, stats NULL       ", 8, fused_fwd_no_stats), ("2 thresholds + 2 glf_bce_logits_sum fwd   ", 0, composed_fwd)],
          [("glf_cps_bce_sum backward (both gradients) ", 16, fused_bwd), ("2 thresholds + 2 glf_bce_logits_sum bwd   ", 0, composed_bwd)]]
for group in groups:
    for (name, bytes_per_elem, _), ts in zip(group, measure([fn for _, _, fn in group])):
        med = statistics.median(ts)
        rate = f"  {bytes_per_elem} B/element {bytes_per_elem * n / med / 1e6:7.1f} GB/s" if bytes_per_elem else ""
        lines.append(f"{name}: {med:7.4f} ms  (min {min(ts):.4f}, max {max(ts):.4f}){rate}")
        print(lines[-1], flush=True)
del a, b, da, db

# ---- the CPS model's step ----
from glfusion_amd.engine import Trainer

STEP_WARM, STEP_ITERS = 3, 5


def trainer(w):
    cfg = {"train": {"batch_size": BATCH_FRAMES, "num_epochs": 1, "clip_length": CLIP, "view_num": VIEWS, "test_view": VIEWS, "dense_cyc": False,
                     "save_dir": os.path.join(tempfile.gettempdir(), "cps_step_ckpt"), "iters_per_epoch": 1, "global_rank": 0, "precision": "f16x3", "cps_weight": w},
           "net": {"model": "Global_and_Local_CPS", "opt": {"opt_name": "Adam", "lr": 1e-5, "weight_decay": 1e-5}}}
    t = Trainer(cfg)
    t.model.train()
    return t


def step_times(t, imgs, masks, video):
    ts = []
    for k in range(STEP_WARM + STEP_ITERS):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        t.train_step(imgs, masks, video)
        torch.cuda.synchronize()
        if k >= STEP_WARM:
            ts.append((time.perf_counter() - t0) * 1e3)
    return ts


lines.append(f"Global_and_Local_CPS, views {VIEWS}, {BATCH_FRAMES} labelled frames + a {CLIP}-frame clip per view, f16x3, eager step with the cycle "
             f"term: median of {STEP_ITERS} steps after {STEP_WARM} warm-ups, host clock around a synchronised step")
for w in (0.0, 0.5):
    t = trainer(w)
    imgs, masks = t.loader.batch()
    video = t.video_loader.batch()[0]
    ts = step_times(t, imgs, masks, video)
    lines.append(f"train_step cps_weight {w}: {statistics.median(ts):8.1f} ms  (min {min(ts):.1f}, max {max(ts):.1f})")
    print(lines[-1], flush=True)
    del t, imgs, masks, video
    torch.cuda.empty_cache()
with open(out_path, "w") as f:
    f.write("\n".join(lines) + "\n")
print(lines[0])
