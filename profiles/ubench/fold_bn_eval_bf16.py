#!/usr/bin/env python3
"""Eval-forward latency with and without folded BatchNorm under 16-bit storage (ops.set_fold_bn_s16, precision bf16): Global_and_Local
in eval(), one clip of 40 frames x 3 views x 112^2, median of 20 timed forwards after 5 warm-ups.

  fold_bn_eval_bf16.py child off|on [frames]
      one setting in this process; prints `median_ms`, the quartiles and the extremes of the 20 samples.
  fold_bn_eval_bf16.py [--parent TREE] [--out FILE] [--repeats N] [--trace-dir DIR]
      the driver: every GPU step is a child process of its own under `timeout`, and nothing more is started after one fails.
      N alternating rounds of: switch off, switch on and -- with --parent TREE, a checkout of the parent commit with its library
      built -- the parent's forward through the same child (the parent has no switch: that is its only setting); then one
      `rocprofv3 --kernel-trace --stats` run per setting, from which the BatchNorm-apply launches per forward are counted.
      Writes FILE (default profiles/fold_bn_eval_bf16.txt).  The run-to-run spread is the range of the N process medians."""
import csv
import glob
import os
import statistics
import subprocess
import sys
import tempfile

HERE = os.path.abspath(__file__)
ROOT = os.path.dirname(os.path.dirname(os.path.dirname(HERE)))
VIEWS = ["1", "3", "4"]
WARMUP, STEPS = 5, 20


def child(which: str, frames: int) -> None:
    sys.path.insert(0, os.environ.get("GLF_TREE") or ROOT)
    import torch
    from glfusion_amd import ops
    from glfusion_amd.models import Global_and_Local
    ops.set_precision("bf16")
    dev = torch.device("cuda", 0)
    torch.manual_seed(0)
    model = Global_and_Local(VIEWS).to(dev).eval()
    gen = torch.Generator().manual_seed(1)
    imgs = {v: torch.rand(frames, 1, 112, 112, generator=gen).to(dev) for v in VIEWS}
    if which == "on":
        ops.set_fold_bn_s16(True)
    elif hasattr(ops, "set_fold_bn_s16"):
        ops.set_fold_bn_s16(False)
    before = ops.FOLD_COUNT[0]
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
    q = statistics.quantiles(times, n=4)
    print(f"median_ms {statistics.median(times):.3f} q1 {q[0]:.3f} q3 {q[2]:.3f} min {min(times):.3f} max {max(times):.3f} "
          f"folds {ops.FOLD_COUNT[0] - before} forwards {WARMUP + STEPS}", flush=True)


def run_child(which: str, frames: int, tree=None, prefix=(), limit=300):
    env = dict(os.environ)
    if tree:
        env["GLF_TREE"] = os.path.abspath(tree)
    cmd = ["timeout", "-k", "10", str(limit), *prefix, sys.executable, HERE, "child", which, str(frames)]
    r = subprocess.run(cmd, env=env, capture_output=True, text=True)
    line = next((l for l in r.stdout.splitlines() if l.startswith("median_ms")), None)
    if r.returncode != 0 or line is None:
        sys.stderr.write(r.stdout[-2000:] + r.stderr[-2000:])
        raise SystemExit(f"fold_bn_eval_bf16: step {' '.join(cmd)} failed with status {r.returncode}; nothing more is started")
    f = line.split()
    return {f[i]: float(f[i + 1]) for i in range(0, len(f), 2)}


def kernel_stats(trace_dir: str, tag: str):
    """{kernel name: (calls, total ms)} of the kernel_stats CSV that the traced run `tag` left under trace_dir."""
    paths = glob.glob(os.path.join(trace_dir, "**", f"{tag}_kernel_stats.csv"), recursive=True)
    if not paths:
        raise SystemExit(f"fold_bn_eval_bf16: no {tag}_kernel_stats.csv under {trace_dir}")
    out = {}
    with open(paths[0]) as fh:
        for row in csv.DictReader(fh):
            out[row["Name"]] = (int(row["Calls"]), float(row["TotalDurationNs"]) / 1e6)
    return out


def short(name: str) -> str:
    name = name.replace("void ", "").replace("(anonymous namespace)::", "")
    return name.split("(")[0]


def main(argv) -> None:
    opts = {"--parent": None, "--out": os.path.join(ROOT, "profiles", "fold_bn_eval_bf16.txt"), "--repeats": "3",
            "--trace-dir": None, "--frames": "40"}
    it = iter(argv)
    for a in it:
        if a not in opts:
            raise SystemExit(__doc__)
        opts[a] = next(it)
    frames, repeats, parent = int(opts["--frames"]), int(opts["--repeats"]), opts["--parent"]
    settings = [("off", None), ("on", None)] + ([("parent", parent)] if parent else [])
    runs = {name: [] for name, _ in settings}
    for _ in range(repeats):                                    # alternating: a drift of the machine hits every setting alike
        for name, tree in settings:
            runs[name].append(run_child("off" if name == "parent" else name, frames, tree))
            print(name, runs[name][-1], flush=True)
    if opts["--trace-dir"] is None:                             # the traces are working files: a temporary directory unless one is named
        opts["--trace-dir"] = tempfile.mkdtemp(prefix="fold_bn_eval_bf16_trace_")
    os.makedirs(opts["--trace-dir"], exist_ok=True)
    stats = {}
    for name in ("off", "on"):
        run_child(name, frames, prefix=("rocprofv3", "--kernel-trace", "--stats", "-d", opts["--trace-dir"], "-o", name, "--output-format", "csv", "--"),
                  limit=600)
        stats[name] = kernel_stats(opts["--trace-dir"], name)
    med = {name: statistics.median(r["median_ms"] for r in rs) for name, rs in runs.items()}
    lines = ["Eval forward with and without folded BatchNorm under 16-bit storage (ops.set_fold_bn_s16), MI355X, written by "
             "profiles/ubench/fold_bn_eval_bf16.py",
             f"bf16, eval forward, {frames} frames x {len(VIEWS)} views x 112^2; per process: median of {STEPS} after {WARMUP} warm-ups; "
             f"{repeats} processes per setting, alternating; every process under its own timeout",
             ""]
    label = {"off": "switch off", "on": "switch on ", "parent": "parent    "}
    for name, rs in runs.items():
        ms = [r["median_ms"] for r in rs]
        lines.append(f"{label[name]}: {med[name]:8.3f} ms per clip forward   process medians {', '.join(f'{m:.3f}' for m in ms)}   "
                     f"(range {max(ms) - min(ms):.3f} ms; within a process q1-q3 {statistics.median(r['q1'] for r in rs):.3f}-"
                     f"{statistics.median(r['q3'] for r in rs):.3f}; {int(rs[0]['folds'])} folds)")
    spread = max(max(r["median_ms"] for r in rs) - min(r["median_ms"] for r in rs) for rs in runs.values())
    lines.append(f"run-to-run spread (largest range of process medians of one setting): {spread:.3f} ms")
    lines.append(f"ratio on / off: {med['on'] / med['off']:.4f}   (speed-up {med['off'] / med['on']:.3f}x)")
    if parent:
        lines.append(f"ratio on / parent: {med['on'] / med['parent']:.4f}; off / parent: {med['off'] / med['parent']:.4f}   "
                     f"(on - parent = {med['on'] - med['parent']:+.3f} ms against a spread of {spread:.3f} ms)")
    fw = WARMUP + STEPS
    lines += ["", f"rocprofv3 --kernel-trace --stats, one run per setting ({fw} forwards each), top kernels by total time:"]
    for name in ("off", "on"):
        total = sum(t for _, t in stats[name].values())
        lines.append(f"switch {name}:")
        for k, (calls, ms) in sorted(stats[name].items(), key=lambda kv: -kv[1][1])[:12]:
            lines.append(f"  {short(k):58s} calls {calls:6d}  total {ms:9.2f} ms  avg {1e3 * ms / calls:8.1f} us  {100 * ms / total:5.2f} %")

    def count(name, needle):
        hit = [(c, t) for k, (c, t) in stats[name].items() if needle in k]
        return sum(c for c, _ in hit), sum(t for _, t in hit)
    lines.append("")
    for needle, what in (("s16_bn_apply_kernel", "BatchNorm-apply launches (s16_bn_apply_kernel)"), ("bn_eval_coeffs_kernel", "bn_eval_coeffs_kernel launches"),
                         ("s16_rows_kernel", "all s16_rows_kernel launches"), ("s16_fold_bn_kernel", "s16_fold_bn_kernel launches")):
        (c0, t0), (c1, t1) = count("off", needle), count("on", needle)
        lines.append(f"{what}: switch off {c0} ({c0 / fw:.1f} per forward, {t0:.1f} ms), switch on {c1} ({c1 / fw:.1f} per forward, {t1:.1f} ms)")
    lines.append("Kernel times under the tracer are not the wall-clock medians above (several streams overlap).")
    with open(opts["--out"], "w") as fh:
        fh.write("\n".join(lines) + "\n")
    print("\n".join(lines))


if __name__ == "__main__":
    if len(sys.argv) > 1 and sys.argv[1] == "child":
        child(sys.argv[2], int(sys.argv[3]) if len(sys.argv) > 3 else 40)
    else:
        main(sys.argv[1:])
