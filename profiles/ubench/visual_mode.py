"""The visual pass under the kernel tracer (profiles/visual_mode.txt).

  rocprofv3 --kernel-trace --stats -f csv -d DIR -o visual -- python profiles/ubench/visual_mode.py run [frames] [patients]
  python profiles/ubench/visual_mode.py report DIR [frames] > profiles/visual_mode.txt

`run`: Trainer.test_visualize with main.py's views (1, 3, 4) on synthetic patients of `frames` frames (200 x 160 volumes), all
outputs on, written to a temporary directory.  `report`: per call of render_labels_kernel / restore_labels_kernel in DIR's kernel
trace, the time next to the bytes the call cannot avoid moving (its floor at the HBM peak of 8 TB/s, MI355X)."""
import csv
import glob
import os
import statistics
import sys
import tempfile
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))

VIEWS, H0, W0, C, HW = ["1", "3", "4"], 200, 160, 5, 112
HBM_PEAK = 8.0e12


def run(frames: int, n_patients: int) -> None:
    import torch
    from glfusion_amd.engine import Trainer
    cfg = {"train": {"batch_size": 1, "num_epochs": 1, "clip_length": frames, "view_num": VIEWS, "test_view": VIEWS, "save_dir": "./result/ckpt",
                     "iters_per_epoch": 1, "global_rank": 0, "eval_patients": n_patients},
           "net": {"opt": {"opt_name": "Adam", "lr": 3e-4, "params": (0.9, 0.999), "weight_decay": 1e-5}}}
    t = Trainer(cfg)
    with tempfile.TemporaryDirectory() as out:
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        manifest = t.test_visualize("profile", out_root=out)
        torch.cuda.synchronize()
        dt = time.perf_counter() - t0
        files = sum(len(fs) for _, _, fs in os.walk(out))
    print(f"visual pass: {len(manifest)} patients x {len(VIEWS)} views x {frames} frames, {files} files, {dt:.2f} s wall clock under the tracer "
          f"(model forward, kernels, copies, PNG / NIfTI compression and writes)")


def report(directory: str, frames: int) -> None:
    rows = []
    for path in glob.glob(os.path.join(directory, "**", "*kernel_trace.csv"), recursive=True):
        with open(path, newline="") as f:
            rows += list(csv.DictReader(f))
    if not rows:
        raise SystemExit(f"no *kernel_trace.csv under {directory}")
    total = sum(int(r["End_Timestamp"]) - int(r["Start_Timestamp"]) for r in rows) / 1e3
    floors = {"render_labels_kernel": ("N C H W 4 read + N H W 5 written", frames * C * HW * HW * 4 + frames * HW * HW * 5),
              "restore_labels_kernel": ("T C oh ow 4 read + H0 W0 T written", frames * C * HW * HW * 4 + H0 * W0 * frames)}
    print(f"Visual pass (Trainer.test_visualize), MI355X, rocprofv3 --kernel-trace --stats, written by profiles/ubench/visual_mode.py")
    print(f"views {VIEWS}, {frames} frames per clip, volumes {H0} x {W0}, predictions [{frames}][{C}][{HW}][{HW}]; {len(rows)} kernel launches, "
          f"{total / 1e3:.2f} ms of kernel time in all")
    for name, (formula, nbytes) in floors.items():
        us = [(int(r["End_Timestamp"]) - int(r["Start_Timestamp"])) / 1e3 for r in rows if name in r["Kernel_Name"]]
        if not us:
            raise SystemExit(f"{name}: not in the trace")
        floor_us = nbytes / HBM_PEAK * 1e6
        print(f"{name:<22}: calls {len(us):3d}  median {statistics.median(us):7.2f} us  (min {min(us):.2f}, max {max(us):.2f})  total {sum(us) / 1e3:.3f} ms"
              f" = {100 * sum(us) / total:.3f} % of the kernel time;  bytes {formula} = {nbytes / 1e6:.2f} MB -> floor {floor_us:.2f} us,"
              f" median = {statistics.median(us) / floor_us:.1f} x floor, {nbytes / statistics.median(us) / 1e3:.0f} GB/s")
    print("render_labels_kernel runs three times per (patient, view): prediction, masks, overlay (which reads the frame as well: + N H W 4).")
    print("restore_labels_kernel reads only the channels its view shows (2 of 5 for views 1 and 3, 4 of 5 for view 4): its floor above counts all 5.")


if __name__ == "__main__":
    if len(sys.argv) > 1 and sys.argv[1] == "run":
        run(int(sys.argv[2]) if len(sys.argv) > 2 else 40, int(sys.argv[3]) if len(sys.argv) > 3 else 2)
    elif len(sys.argv) > 2 and sys.argv[1] == "report":
        report(sys.argv[2], int(sys.argv[3]) if len(sys.argv) > 3 else 40)
    else:
        raise SystemExit(__doc__)
