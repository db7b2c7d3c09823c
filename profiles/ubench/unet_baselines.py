"""The U-Net baselines: step time, peak memory, and the new streaming kernels against their byte floors (profiles/unet_baselines.txt).

  python profiles/ubench/unet_baselines.py steps > steps.txt
  rocprofv3 --kernel-trace --stats -f csv -d DIR -o unet -- python profiles/ubench/unet_baselines.py kernels
  python profiles/ubench/unet_baselines.py report DIR steps.txt > profiles/unet_baselines.txt

`steps`: forward + backward (BCE-sum over head 0) of baseline_unet and multiview_unet at 4 clips x 3 views x 16 frames x 112 x 112
(64 frames per view) under f16x3 and bf16; ms per step over 5 steps after 2 warm-up steps (device events), peak allocated memory.
`kernels` (the one traced pass): every new streaming kernel, both storages, 10 calls each at the largest shape it meets in that step --
64 frames of 112 x 112 x 64 channels (the up-sampling: 56 x 56 x 128 in, its gradient 112 x 112 x 128).  `report`: per kernel the
median time next to the bytes the call cannot avoid moving, at 6.3 TB/s."""
import csv
import glob
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))

VIEWS, FRAMES, HW = ["1", "3", "4"], 64, 112
HBM = 6.3e12
N, C = FRAMES, 64
PIX = N * HW * HW


def steps() -> None:
    import torch
    from glfusion_amd import models as M
    from glfusion_amd import ops
    dev = torch.device("cuda", 0)
    gen = torch.Generator(device=dev).manual_seed(5)
    imgs = {v: torch.rand(FRAMES, 1, HW, HW, device=dev, generator=gen) for v in VIEWS}
    tgts = {v: (torch.rand(FRAMES, 5, HW, HW, device=dev, generator=gen) < 0.3).float() for v in VIEWS}
    for name in ("baseline_unet", "multiview_unet"):
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
            print(f"{name:<15} {prec:<6}: forward + backward {ms[2]:8.2f} ms per step (median of 5; min {ms[0]:.2f}, max {ms[4]:.2f}), "
                  f"peak memory {torch.cuda.max_memory_allocated(dev) / 2 ** 30:.2f} GiB, loss {float(loss.detach()):.1f}")
            del model
            torch.cuda.empty_cache()


def kernels() -> None:
    import torch
    from glfusion_amd import ops
    dev = torch.device("cuda", 0)
    for prec in ("f32", "bf16"):
        dt = torch.bfloat16 if prec == "bf16" else torch.float32
        with ops.precision_scope(prec):
            img = torch.rand(N, HW, HW, 1, device=dev)
            w = torch.rand(64, 1, 3, 3, device=dev).requires_grad_(True)
            b = torch.rand(64, device=dev).requires_grad_(True)
            act = torch.rand(N, HW, HW, C, device=dev).to(dt).requires_grad_(True)
            act2 = torch.rand(N, HW, HW, C, device=dev).to(dt).requires_grad_(True)
            low = torch.rand(N, HW // 2, HW // 2, 2 * C, device=dev).to(dt).requires_grad_(True)
            for _ in range(10):
                for t in (w, b, act, act2, low):
                    t.grad = None
                y = ops.conv3x3_c1(img, w, b)
                y.backward(act.detach())
                y = ops.maxpool2x2s2(act)
                y.backward(y.detach())
                y = ops.upsample2x(low)
                y.backward(y.detach())
                y = ops.concat_channels(act, act2)
                y.backward(y.detach())
                del y
        torch.cuda.synchronize()


def floors(es: int):
    """{kernel: (formula, bytes)} for elements of es bytes (4: fp32 storage, 2: bf16)."""
    a = PIX * C * es                     # one 112 x 112 x 64 activation
    return {
        "conv3x3_c1_fwd_kernel": ("image read + N H W 64 written", PIX * 4 + a),
        "conv3x3_c1_wgrad_kernel": ("image + N H W 64 gradient read", PIX * 4 + a),
        "maxpool2_fwd_kernel": ("N H W C read + N H/2 W/2 C (value + 1-byte index) written", a + a // 4 + PIX * C // 4),
        "maxpool2_bwd_kernel": ("N H/2 W/2 C (gradient + index) read + N H W C written", a // 4 + PIX * C // 4 + a),
        "upsample2x_fwd_kernel": ("N H/2 W/2 128 read + N H W 128 written", 2 * a // 4 + 2 * a),
        "upsample2x_bwd_kernel": ("N H W 128 read + N H/2 W/2 128 written", 2 * a + 2 * a // 4),
        "concat2_kernel": ("two N H W 64 sources and one N H W 128 tensor, each moved once", 4 * a),
    }


def report(directory: str, steps_file: str) -> None:
    rows = []
    for path in glob.glob(os.path.join(directory, "**", "*kernel_trace.csv"), recursive=True):
        with open(path, newline="") as f:
            rows += list(csv.DictReader(f))
    if not rows:
        raise SystemExit(f"no *kernel_trace.csv under {directory}")
    print("U-Net baselines (baseline_unet, multiview_unet), MI355X, written by profiles/ubench/unet_baselines.py")
    print(f"views {VIEWS}, {FRAMES} frames per view (4 clips x 16 frames), {HW} x {HW}")
    print(open(steps_file).read().rstrip())
    print(f"new streaming kernels, rocprofv3 --kernel-trace --stats, 10 calls each at {N} x {HW} x {HW} x {C} (up-sampling: 128 channels), floor at 6.3 TB/s:")
    for es, tag, tname in ((4, "fp32", "<float"), (2, "bf16", "<unsigned short")):
        for name, (formula, nbytes) in floors(es).items():
            us = [(int(r["End_Timestamp"]) - int(r["Start_Timestamp"])) / 1e3 for r in rows if name + tname in r["Kernel_Name"]]
            if not us:
                raise SystemExit(f"{name}{tname}: not in the trace")
            floor_us, med = nbytes / HBM * 1e6, statistics.median(us)
            print(f"{name:<24} {tag}: calls {len(us):3d}  median {med:8.2f} us  (min {min(us):.2f}, max {max(us):.2f});  bytes {formula} = "
                  f"{nbytes / 1e6:.1f} MB -> floor {floor_us:.2f} us, median = {med / floor_us:.2f} x floor, {nbytes / med / 1e3:.0f} GB/s")
    print("concat2_kernel: forward and backward are one kernel (two instantiations) moving the same bytes; the median is over both.")


if __name__ == "__main__":
    if sys.argv[1:2] == ["steps"]:
        steps()
    elif sys.argv[1:2] == ["kernels"]:
        kernels()
    elif len(sys.argv) == 4 and sys.argv[1] == "report":
        report(sys.argv[2], sys.argv[3])
    else:
        raise SystemExit(__doc__)
