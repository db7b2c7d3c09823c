"""The input-gradient launches of ONE ASPP head at the flagship shape (64 frames of 28x28, 2048 -> 256, rates 12 / 24 / 36) with
ops.ASPP_DGRAD_ONE off (the stacked centre launch + two accumulating region launches) and on (one segmented region launch),
from ops.PROFILER's event brackets: medians over ITERS forward + backward passes after WARM, and the rate of the EXECUTED
(in-range) fp32-equivalent FLOPs.  Then the weight-image refresh of the head's parameters under both settings."""
import statistics
import sys

import torch

sys.path.insert(0, ".")
from glfusion_amd import ops  # noqa: E402
from glfusion_amd.models.deeplabv3 import ASPP  # noqa: E402

DEV = torch.device("cuda:0")
N, H, W, CIN, COUT, RATES = 64, 28, 28, 2048, 256, (12, 24, 36)
WARM, ITERS = 3, 10


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


def head(one):
    ops.ASPP_DGRAD_ONE = one
    ops.reset_weight_images()
    torch.manual_seed(0)
    m = ASPP(CIN, list(RATES), COUT).to(DEV).train()
    x = torch.randn(N, CIN, H, W, device=DEV).requires_grad_(True)
    rows_all, rows = N * H * W, {}
    for it in range(WARM + ITERS):
        ops.PROFILER = prof = [] if it >= WARM else None
        y = m(x)
        y.sum().backward()
        torch.cuda.synchronize()
        if prof is None:
            continue
        seen = {}
        for p in prof:
            if not (p[0].startswith("gemm_rows_kernel<0") and p[5][0] == rows_all and p[5][1] == CIN):
                continue                    # the head's dgrad launches: NT, M = all pixels, N = Cin
            key = (p[0], p[5])
            seen[key] = seen.get(key, 0) + 1
            rows.setdefault(key + (seen[key],), []).append((p[3].elapsed_time(p[4]), p[2], p[1]))
        for q in m.parameters():
            q.grad = None
        x.grad = None
    ops.PROFILER = None
    total = 0.0
    print(f"--- GLF_ASPP_DGRAD_ONE={int(one)}: dgrad launches of one head ---")
    for key, v in rows.items():
        ms = statistics.median(t for t, _, _ in v)
        total += ms
        print(f"  {key[0]:26s} {str(key[1]):44s} #{key[2]}  {ms:7.3f} ms  {v[0][1] / ms * 1e-9:7.1f} TF executed "
              f"({v[0][1] * 1e-9:.1f} GFLOP executed, {v[0][2] * 1e-9:.1f} dense)")
    print(f"  sum of medians {total:.3f} ms")
    # per-update weight work of this head: every registered image recomputed (four launches)
    t = timed(ops.refresh_weights)
    n_img = sum(len(r.images) for r in ops._wreg.values())
    print(f"  weights refresh of the head's {n_img} images: {t:.3f} ms")
    del m
    return total


if __name__ == "__main__":
    with ops.precision_scope("f16x3"):
        off = head(False)
        on = head(True)
        print(f"per head: {off:.3f} -> {on:.3f} ms ({on - off:+.3f} ms)")
