"""The forward conv launches of ONE ASPP head at the flagship shape (64 frames of 28x28, 2048 -> 256, rates 12 / 24 / 36) with
ops.ASPP_FWD_ONE off (the stacked centre launch, two adding launches of per-tap rectangles, and the statistics reduces of the
two BatchNorms those leave without sums) and on (one segmented launch with column groups and fused statistics), each timed
apart: contraction launches from ops.PROFILER's event brackets, statistics reduces from event brackets around glf_bn_stats.
Medians over ITERS forward passes after WARM, and the rate of the EXECUTED (in-range) fp32-equivalent FLOPs.  Then the
weight-image refresh of the head's parameters under both settings (after a forward + backward pass, so that every image the
head uses is registered)."""
import statistics
import sys

import torch

sys.path.insert(0, ".")
from glfusion_amd import _lib, ops  # noqa: E402
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
    ops.ASPP_FWD_ONE = one
    ops.reset_weight_images()
    torch.manual_seed(0)
    m = ASPP(CIN, list(RATES), COUT).to(DEV).train()
    x = torch.randn(N, CIN, H, W, device=DEV).requires_grad_(True)
    rows_all, rows, reduces = N * H * W, {}, []
    dll = _lib.lib.load()
    real = dll.glf_bn_stats

    def stats_spy(*a):                      # (x, ldx, rows, c, ...): the reduces over a branch's slice of U
        if not (a[2] == rows_all and a[3] == COUT and a[1] == 4 * COUT):
            return real(*a)
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        rc = real(*a)
        e1.record()
        reduces[-1].append((e0, e1))
        return rc
    dll.glf_bn_stats = stats_spy
    try:
        for it in range(WARM + ITERS):
            ops.PROFILER = prof = [] if it >= WARM else None
            reduces.append([])
            y = m(x)                            # (grad mode, as in a train step: the route depends on it)
            torch.cuda.synchronize()
            del y
            if prof is None:
                reduces.pop()
                continue
            seen = {}
            for p in prof:
                if not (p[0].startswith("gemm_rows_kernel<0") and p[5][0] == rows_all and p[5][2] == CIN and p[5][1] in (COUT, 4 * COUT)):
                    continue                    # the head's forward conv launches: NT, M = all pixels, K = Cin
                key = (p[0], p[5])
                seen[key] = seen.get(key, 0) + 1
                rows.setdefault(key + (seen[key],), []).append((p[3].elapsed_time(p[4]), p[2], p[1]))
    finally:
        dll.glf_bn_stats = real
        ops.PROFILER = None
    total = 0.0
    print(f"--- GLF_ASPP_FWD_ONE={int(one)}: forward conv launches of one head ---")
    for key, v in rows.items():
        ms = statistics.median(t for t, _, _ in v)
        total += ms
        print(f"  {key[0]:26s} {str(key[1]):44s} #{key[2]}  {ms:7.3f} ms  {v[0][1] / ms * 1e-9:7.1f} TF executed "
              f"({v[0][1] * 1e-9:.1f} GFLOP executed, {v[0][2] * 1e-9:.1f} dense)")
    per_call = list(zip(*[[e0.elapsed_time(e1) for e0, e1 in r] for r in reduces])) if reduces and reduces[0] else []
    for i, ts in enumerate(per_call):
        ms = statistics.median(ts)
        total += ms
        print(f"  glf_bn_stats over a [{rows_all}][{COUT}] slice of U (ld {4 * COUT})  #{i + 1}  {ms:7.3f} ms")
    print(f"  sum of medians {total:.3f} ms ({len(rows)} contraction launches, {len(per_call)} statistics reduces)")
    # per-update weight work of this head: every image a train step registers, recomputed (four launches)
    m(x).sum().backward()
    torch.cuda.synchronize()
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
