"""Per-shape contraction rows of ONE ASPP head at the flagship shape (64 frames of 28x28, 2048 -> 256, rates 12 / 24 / 36), fused
route against GLF_ASPP_CENTRE=0, from ops.PROFILER's event brackets; then the rate-12 / rate-24 off-centre dgrad as accumulating
region launches against "separate outputs + three-input add_n".  Medians over ITERS forward + backward passes after WARM."""
import ctypes as C
import statistics
import sys

import torch

sys.path.insert(0, ".")
from glfusion_amd import ops  # noqa: E402
from glfusion_amd.models.deeplabv3 import ASPP  # noqa: E402

DEV = torch.device("cuda:0")
N, H, W, CIN, COUT, RATES = 64, 28, 28, 2048, 256, (12, 24, 36)
WARM, ITERS = 3, 10


def head(fused):
    ops.ASPP_CENTRE = fused
    torch.manual_seed(0)
    m = ASPP(CIN, list(RATES), COUT).to(DEV).train()
    x = torch.randn(N, CIN, H, W, device=DEV).requires_grad_(True)
    rows = {}
    for it in range(WARM + ITERS):
        ops.PROFILER = prof = [] if it >= WARM else None
        y = m(x)
        y.sum().backward()
        torch.cuda.synchronize()
        if prof is None:
            continue
        seen = {}
        for p in prof:
            key = (p[0], p[5])
            seen[key] = seen.get(key, 0) + 1
            rows.setdefault(key + (seen[key],), []).append((p[3].elapsed_time(p[4]), p[2]))
        for q in m.parameters():
            q.grad = None
        x.grad = None
    ops.PROFILER = None
    total = 0.0
    print(f"--- GLF_ASPP_CENTRE={int(fused)}: contraction launches of one head, forward + backward ---")
    for key, v in rows.items():
        ms = statistics.median(t for t, _ in v)
        total += ms
        print(f"  {key[0]:28s} {str(key[1]):44s} #{key[2]}  {ms:7.3f} ms  {v[0][1] / ms * 1e-9:7.1f} TF executed")
    print(f"  sum of medians {total:.3f} ms")


def timed(fn):
    ts = []
    for it in range(WARM + ITERS):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        torch.cuda.synchronize()
        if it >= WARM:
            ts.append(e0.elapsed_time(e1))
    return statistics.median(ts)


def store_ab():
    rows = N * H * W
    g = torch.Generator().manual_seed(1)
    dy = torch.randn(rows, COUT, generator=g).to(DEV)
    wT = torch.randn(9, CIN, COUT, generator=g).to(DEV)
    dx = torch.randn(rows, CIN, generator=g).to(DEV)
    sep = [torch.empty(rows, CIN, device=DEV) for _ in range(2)]
    out = torch.empty(rows, CIN, device=DEV)
    am_a, am_b = ops.amax_of(dy), ops.amax_of(wT)
    torch.cuda.synchronize()

    def launch(d, dst, acc):
        mask = ops.tap_mask(2, H, W, H, W, 3, 3, 1, d, d) & ~ops.CENTRE_TAP
        ops.gemm("nt", dy, wT, dst, M=rows, N=CIN, K=COUT, lda=COUT, ldb=COUT, ldc=CIN, taps=9, mask=mask, tap_stride_b=COUT * CIN,
                 gather=2, geo=(N, H, W, H, W, 3, 3, 1, d, d), rect=2, accumulate=acc, amax_a=am_a, amax_b=am_b)

    def add3():
        arr = (C.c_void_p * 3)(dx.data_ptr(), sep[0].data_ptr(), sep[1].data_ptr())
        ops._launch("add_n", out, arr, 3, out, out.numel())

    print("--- off-centre dgrad of rates 12 / 24 (region mode, centre bit cleared, fp32 operands split in the kernel) ---")
    a12, a24 = timed(lambda: launch(12, dx, True)), timed(lambda: launch(24, dx, True))
    s12, s24 = timed(lambda: launch(12, sep[0], False)), timed(lambda: launch(24, sep[1], False))
    t3 = timed(add3)
    print(f"  accumulate = 1 into dx:        rate 12 {a12:.3f} ms, rate 24 {a24:.3f} ms            -> {a12 + a24:.3f} ms per head")
    print(f"  separate outputs + add_n(3):   rate 12 {s12:.3f} ms, rate 24 {s24:.3f} ms, add_n {t3:.3f} ms -> {s12 + s24 + t3:.3f} ms per head")
    print("  (a separate output of a region launch with the centre bit cleared leaves rate 24's interior unwritten: that form would")
    print("   also need a zero fill or a region-aware add, which is not counted here)")


if __name__ == "__main__":
    with ops.precision_scope("f16x3"):
        head(True)
        head(False)
        store_ab()
