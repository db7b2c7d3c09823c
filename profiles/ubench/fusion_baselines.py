"""The fusion baselines: step time, peak memory, and the view-mix kernels against their byte floors (profiles/fusion_baselines.txt).

  python profiles/ubench/fusion_baselines.py steps > steps.txt
  rocprofv3 --kernel-trace --stats -f csv -d DIR -o fusion -- python profiles/ubench/fusion_baselines.py kernels
  python profiles/ubench/fusion_baselines.py report DIR steps.txt > profiles/fusion_baselines.txt

`steps`: forward + backward (BCE-sum over output 0) of early_fusion, late_fusion and MLP_fusion at 4 clips x 3 views x 16 frames x
112 x 112 (64 frames per view) under f16x3 and bf16; ms per step over 5 steps after 2 warm-up steps (device events), peak allocated
memory.  `kernels` (the one traced pass): ops.view_mix forward, input gradient and weight gradient, 10 calls each, at the two shapes
those steps meet -- rows = 802 816 (64 x 112 x 112 pixels), c = 1, V = 3 and rows = 50 176 (64 x 28 x 28 positions), c = 5, V = 3 --
and the stem's input gradient at 64 x 112 x 112.  `report`: per kernel the median time next to the bytes the call cannot avoid
moving, at 6.3 TB/s."""
import csv
import glob
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))

VIEWS, FRAMES, HW = ["1", "3", "4"], 64, 112
HBM = 6.3e12
SHAPES = [(FRAMES * HW * HW, 1), (FRAMES * (HW // 4) * (HW // 4), 5)]          # (rows, c) at V = 3


def steps() -> None:
    import torch
    from glfusion_amd import models as M
    from glfusion_amd import ops
    dev = torch.device("cuda", 0)
    gen = torch.Generator(device=dev).manual_seed(5)
    imgs = {v: torch.rand(FRAMES, 1, HW, HW, device=dev, generator=gen) for v in VIEWS}
    tgts = {v: (torch.rand(FRAMES, 5, HW, HW, device=dev, generator=gen) < 0.3).float() for v in VIEWS}
    for name in ("early_fusion", "late_fusion", "MLP_fusion"):
        for prec in ("f16x3", "bf16"):
            torch.manual_seed(0)
            model = getattr(M, name)(VIEWS).to(dev).train()
            with ops.precision_scope(prec):
                def step():
                    for p in model.parameters():
                        p.grad = None
                    out = model(imgs)[0]
                    loss = sum(ops.bce_with_logits_sum(out[v], tgts[v]) for v in VIEWS)
                    loss.backward()
                    return loss
                for _ in range(2):
                    step()
                torch.cuda.synchronize()
                torch.cuda.reset_peak_memory_stats(dev)
                ev = [torch.cuda.Event(enable_timing=True) for _ in range(6)]
                ev[0].record()
                for i in range(5):
                    loss = step()
                    ev[i + 1].record()
                torch.cuda.synchronize()
            ms = sorted(ev[i].elapsed_time(ev[i + 1]) for i in range(5))
            print(f"{name:<13} {prec:<6}: forward + backward {ms[2]:8.2f} ms per step (median of 5; min {ms[0]:.2f}, max {ms[4]:.2f}), "
                  f"peak memory {torch.cuda.max_memory_allocated(dev) / 2 ** 30:.2f} GiB, loss {float(loss.detach()):.1f}")
            del model
            torch.cuda.empty_cache()


def kernels() -> None:
    import torch
    from glfusion_amd import ops
    dev = torch.device("cuda", 0)
    v = len(VIEWS)
    for rows, c in SHAPES:
        xs = [torch.rand(rows, c, device=dev).requires_grad_(True) for _ in range(v)]
        ws = [torch.rand(c, v * c, 1, 1, device=dev).requires_grad_(True) for _ in range(v)]
        bs = [torch.rand(c, device=dev).requires_grad_(True) for _ in range(v)]
        dys = [torch.rand(rows, c, device=dev) for _ in range(v)]
        for _ in range(10):
            for t in xs + ws + bs:
                t.grad = None
            torch.autograd.backward(ops.view_mix(xs, ws, bs), dys)
    img = torch.rand(FRAMES, HW, HW, 1, device=dev).requires_grad_(True)
    w = torch.rand(64, 1, 7, 7, device=dev).requires_grad_(True)
    dy = torch.rand(FRAMES, HW, HW, 64, device=dev)
    for prec in ("f32", "bf16"):
        with ops.precision_scope(prec):
            for _ in range(10):
                img.grad = w.grad = None
                y = ops.stem7x7(img, w, None, 3)
                y.backward(dy.to(y.dtype))
    torch.cuda.synchronize()


def floors():
    """[(kernel name fragment, which half of that kernel's calls in the trace, label, bytes)]"""
    out = []
    for i, (rows, c) in enumerate(SHAPES):
        t = rows * c * 4 * len(VIEWS)                     # the V tensors of one side
        out.append(("view_mix_kernel", i, f"rows {rows} c {c}: V inputs read + V outputs written (forward; dgrad the same)", 2 * t))
        out.append(("view_mix_wgrad_kernel", i, f"rows {rows} c {c}: V inputs + V gradients read", 2 * t))
    pix = FRAMES * HW * HW
    out.append(("stem_dgrad_kernel", 0, "fp32: N H W 64 gradient read + N H W written", pix * 64 * 4 + pix * 4))
    out.append(("stem_dgrad_kernel", 1, "bf16: N H W 64 gradient read + N H W written", pix * 64 * 2 + pix * 4))
    return out


def report(directory: str, steps_file: str) -> None:
    rows = []
    for path in glob.glob(os.path.join(directory, "**", "*kernel_trace.csv"), recursive=True):
        with open(path, newline="") as f:
            rows += list(csv.DictReader(f))
    if not rows:
        raise SystemExit(f"no *kernel_trace.csv under {directory}")
    rows.sort(key=lambda r: int(r["Start_Timestamp"]))
    print("Fusion baselines (early_fusion, late_fusion, MLP_fusion), MI355X, written by profiles/ubench/fusion_baselines.py")
    print(f"views {VIEWS}, {FRAMES} frames per view (4 clips x 16 frames), {HW} x {HW}")
    print(open(steps_file).read().rstrip())
    print("view-mix kernels and the stem's input gradient, rocprofv3 --kernel-trace --stats, 10 calls each, floor at 6.3 TB/s:")
    for frag, shape_i, label, nbytes in floors():
        us = [(int(r["End_Timestamp"]) - int(r["Start_Timestamp"])) / 1e3 for r in rows if frag in r["Kernel_Name"]]
        per = len(us) // 2                               # the trace holds the first shape's (storage's) calls, then the second's
        us = us[shape_i * per:(shape_i + 1) * per]
        if not us:
            raise SystemExit(f"{frag}: not in the trace")
        floor_us, med = nbytes / HBM * 1e6, statistics.median(us)
        print(f"{frag:<26} calls {len(us):3d}  median {med:8.2f} us  (min {min(us):.2f}, max {max(us):.2f});  bytes {label} = "
              f"{nbytes / 1e6:.1f} MB -> floor {floor_us:.2f} us, median = {med / floor_us:.2f} x floor, {nbytes / med / 1e3:.0f} GB/s")
    print("view_mix_kernel: forward and dgrad are one kernel moving the same bytes; the median is over both (20 calls).")


if __name__ == "__main__":
    if sys.argv[1:2] == ["steps"]:
        steps()
    elif sys.argv[1:2] == ["kernels"]:
        kernels()
    elif len(sys.argv) == 4 and sys.argv[1] == "report":
        report(sys.argv[2], sys.argv[3])
    else:
        raise SystemExit(__doc__)
