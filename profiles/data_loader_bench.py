#!/usr/bin/env python3
"""Cost of one training batch from patient volumes: data.BatchLoader (store warm) against the per-sample way -- B x ds[i] and
torch.stack per view, SegPAHDataset.__getitem__ -- and the frame-sum kernel on one volume.  Host call to torch.cuda.synchronize().

    python profiles/data_loader_bench.py [--out FILE] [--h0 600 --w0 800 --t 100 --batch 4 --patients 4]
"""
import argparse
import os
import random
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import numpy as np
import torch

STEP_MS = 245.0          # the training step at the benchmark's C2 shape the loader's cost is set against


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--h0", type=int, default=600)
    ap.add_argument("--w0", type=int, default=800)
    ap.add_argument("--t", type=int, default=100)
    ap.add_argument("--batch", type=int, default=4)
    ap.add_argument("--patients", type=int, default=4)
    ap.add_argument("--loader-epochs", type=int, default=10)
    ap.add_argument("--dataset-iterations", type=int, default=5)
    args = ap.parse_args()
    from glfusion_amd import data
    if not torch.cuda.is_available():
        raise SystemExit("data_loader_bench: needs the GPU (no CPU fallback, no CPU timing)")
    views, dev = ["1", "3", "4"], torch.device("cuda", 0)
    rs = np.random.RandomState(0)
    infos = {}
    for k in range(args.patients):
        shape = (args.h0, args.w0, args.t)
        infos[f"0_{k}"] = {"dataset_name": "rmyy", "fold": "0",
                           "views_images": {v: rs.randint(0, 256, size=shape, dtype=np.uint8) for v in views},
                           "views_labels": {v: rs.randint(0, 5, size=shape, dtype=np.uint8) for v in views}}

    def datasets(store=None):
        return {v: data.SegPAHDataset(infos, is_train=True, data_list=list(infos), view_num=[v], single_frame=True, device=dev,
                                      crop_seed=int(v), store=store) for v in views}

    # the loader, store warm: epoch 0 uploads every volume and takes its frame sums; the epochs after it are timed
    store = data.VolumeStore(dev, 16 << 30)
    loader = data.BatchLoader(datasets(), args.batch, store)
    random.seed(1)
    for _ in loader:
        pass
    torch.cuda.synchronize()
    new_ms = []
    for _ in range(args.loader_epochs):
        it = iter(loader)
        while True:
            t0 = time.perf_counter()
            try:
                imgs, masks = next(it)
            except StopIteration:
                break
            torch.cuda.synchronize()
            new_ms.append((time.perf_counter() - t0) * 1e3)
    # the per-sample way: B x ds[i] and torch.stack per view (one untimed iteration first)
    sets = datasets()
    old_ms = []
    for k in range(args.dataset_iterations + 1):
        idxs = range(k * args.batch, (k + 1) * args.batch)
        t0 = time.perf_counter()
        for v in views:
            items = [sets[v][i % len(sets[v])] for i in idxs]
            imgs, masks = torch.stack([x[0] for x in items]), torch.stack([x[1] for x in items])
        torch.cuda.synchronize()
        if k:
            old_ms.append((time.perf_counter() - t0) * 1e3)
    # the frame-sum kernel on one resident label volume, device events
    lab = store.volume("0_0", "4", "label", infos["0_0"]["views_labels"]["4"])
    for _ in range(3):
        data.frame_label_sums(lab)
    sum_ms = []
    for _ in range(30):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        data.frame_label_sums(lab)
        b.record()
        torch.cuda.synchronize()
        sum_ms.append(a.elapsed_time(b))
    new, old, sm = statistics.median(new_ms), statistics.median(old_ms), statistics.median(sum_ms)
    nbytes = lab.numel() * lab.element_size()
    lines = [
        f"command: python profiles/data_loader_bench.py --h0 {args.h0} --w0 {args.w0} --t {args.t} --batch {args.batch} --patients {args.patients}",
        f"device: {torch.cuda.get_device_name(0)}; {len(views)} views, B = {args.batch} per view, {args.patients} patients, uint8 volumes "
        f"{args.h0} x {args.w0} x {args.t}; host call to torch.cuda.synchronize(), medians",
        f"BatchLoader iteration, store warm: {new:.3f} ms (min {min(new_ms):.3f}, max {max(new_ms):.3f}, {len(new_ms)} iterations)",
        f"per-sample way, B x ds[i] + torch.stack per view (SegPAHDataset.__getitem__, which this change leaves as it was): "
        f"{old:.1f} ms (min {min(old_ms):.1f}, max {max(old_ms):.1f}, {len(old_ms)} iterations)",
        f"loader's share of a {STEP_MS:.0f} ms step: {100.0 * new / STEP_MS:.2f} % (per-sample way: {100.0 * old / STEP_MS:.0f} %)",
        f"glf_frame_label_sums on one {nbytes / 1e6:.0f} MB uint8 volume: {sm * 1e3:.1f} us (device events, median of {len(sum_ms)}; "
        f"min {min(sum_ms) * 1e3:.1f}), {nbytes / (sm * 1e-3) / 1e9:.0f} GB/s read",
    ]
    text = "\n".join(lines) + "\n"
    print(text, end="")
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(text)


if __name__ == "__main__":
    main()
