"""numpy restatement of the contour metrics: contours by shifted comparisons, directed squared distances by all-pairs
integer differences, ranks by np.sort, sums in float64.  Imports nothing from glfusion_amd: it is the yardstick of glf_contour_distances,
data.contour_metrics and the engine's contour report."""
import numpy as np


def pred_on(logits):
    """sigmoid(logit) > 0.5 in fp32, as the device decides it: 0.0, -0.0, -inf and NaN are off, +inf is on."""
    x = np.asarray(logits, dtype=np.float32)
    with np.errstate(over="ignore", invalid="ignore"):
        s = np.float32(1.0) / (np.float32(1.0) + np.exp(-x, dtype=np.float32))
        return s > np.float32(0.5)


def target_on(target):
    return np.asarray(target) != 0


def contour(mask):
    """[h, w] bool -> the on pixels with a 4-neighbour that is off or outside the image."""
    m = np.asarray(mask, dtype=bool)
    p = np.pad(m, 1, constant_values=False)
    inner = p[:-2, 1:-1] & p[2:, 1:-1] & p[1:-1, :-2] & p[1:-1, 2:]
    return m & ~inner


def directed_d2(edge_from, edge_to, chunk_bytes=1 << 27):
    """int64 [count_from]: per pixel of edge_from (row-major order) the least squared distance to a pixel of edge_to."""
    src = np.argwhere(edge_from).astype(np.int64)
    dst = np.argwhere(edge_to).astype(np.int64)
    assert len(dst) > 0
    out = np.empty(len(src), dtype=np.int64)
    step = max(1, chunk_bytes // (8 * len(dst)))                 # two [step, len(dst)] int64 temporaries at a time
    for i in range(0, len(src), step):
        dy = src[i:i + step, 0, None] - dst[None, :, 0]
        dx = src[i:i + step, 1, None] - dst[None, :, 1]
        dy *= dy
        dx *= dx
        dy += dx
        out[i:i + step] = dy.min(axis=1)
    return out


def ranks(count, pct):
    t = pct * (count - 1)
    lo = t // 100
    return lo, lo + (t % 100 != 0), (t % 100) / 100.0


def plane_stats(on_pred, on_target, pct=95):
    """One plane -> (stats int64 [2, 4] = (count, max_d2, d2_lo, d2_hi) per direction, sums float64 [2])."""
    edges = (contour(on_pred), contour(on_target))
    counts = [int(e.sum()) for e in edges]
    stats = np.empty((2, 4), dtype=np.int64)
    sums = np.zeros(2, dtype=np.float64)
    for d in range(2):
        stats[d, 0] = counts[d]
        if counts[0] == 0 or counts[1] == 0:
            stats[d, 1:] = -1
            continue
        d2 = np.sort(directed_d2(edges[d], edges[1 - d]))
        lo, hi, _ = ranks(counts[d], pct)
        stats[d, 1:] = (d2[-1], d2[lo], d2[hi])
        sums[d] = np.sqrt(d2.astype(np.float64)).sum()
    return stats, sums


def stats_ref(logits, target, pct=95):
    """[N, C, H, W] logits and targets -> (stats int64 [N, C, 2, 4], sums float64 [N, C, 2])."""
    p, t = pred_on(logits), target_on(target)
    n, c = p.shape[:2]
    stats = np.empty((n, c, 2, 4), dtype=np.int64)
    sums = np.empty((n, c, 2), dtype=np.float64)
    for i in range(n):
        for j in range(c):
            stats[i, j], sums[i, j] = plane_stats(p[i, j], t[i, j], pct)
    return stats, sums


def directed_percentile(stats, pct=95):
    """P per direction, [..., 2] float64, from stats [..., 2, 4] (only meaningful where both contours are non-empty)."""
    stats = np.asarray(stats)
    frac = ((pct * (stats[..., 0] - 1)) % 100) / 100.0
    lo, hi = np.sqrt(np.maximum(stats[..., 2], 0).astype(np.float64)), np.sqrt(np.maximum(stats[..., 3], 0).astype(np.float64))
    return lo + frac * (hi - lo)


def metrics_ref(stats, sums, pct=95):
    """stats [N, C, 2, 4], sums [N, C, 2] -> dict of [N, C] arrays: hd, hdp, assd (NaN where not scored) and the four bool masks."""
    stats, sums = np.asarray(stats), np.asarray(sums, dtype=np.float64)
    has_pred, has_target = stats[..., 0, 0] > 0, stats[..., 1, 0] > 0
    scored = has_pred & has_target
    with np.errstate(invalid="ignore", divide="ignore"):
        hd = np.sqrt(np.maximum(stats[..., 0, 1], stats[..., 1, 1]).astype(np.float64))
        hdp = directed_percentile(stats, pct).max(axis=-1)
        assd = sums.sum(axis=-1) / (stats[..., 0, 0] + stats[..., 1, 0])
    nan = np.float64("nan")
    return {"hd": np.where(scored, hd, nan), "hdp": np.where(scored, hdp, nan), "assd": np.where(scored, assd, nan),
            "scored": scored, "missed": has_target & ~has_pred, "spurious": has_pred & ~has_target, "absent": ~has_pred & ~has_target}


def report_ref(clips, pct=95):
    """clips: iterable of (logits, target) [N, C, H, W] of ONE view -> the engine's per-view report: per part the mean hd / hd95 / assd
    over the scored (frame, part) pairs (None without any) and the four pair counts, and 'mean' over all scored pairs of all parts."""
    acc = None
    for logits, target in clips:
        m = metrics_ref(*stats_ref(logits, target, pct), pct)
        rows = np.stack([np.where(m["scored"], m[k], 0.0).sum(axis=0) for k in ("hd", "hdp", "assd")]
                        + [m[k].sum(axis=0).astype(np.float64) for k in ("scored", "missed", "spurious", "absent")], axis=1)
        acc = rows if acc is None else acc + rows
    out = {}
    for i, key in enumerate(("hd", "hd95", "assd")):
        out[key] = [acc[c, i] / acc[c, 3] if acc[c, 3] > 0 else None for c in range(acc.shape[0])]
    for i, key in enumerate(("scored", "missed", "spurious", "absent")):
        out[key] = [int(acc[c, 3 + i]) for c in range(acc.shape[0])]
    total = acc[:, 3].sum()
    out["mean"] = tuple(acc[:, i].sum() / total for i in range(3)) if total > 0 else None
    return out
